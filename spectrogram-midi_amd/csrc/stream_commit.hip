// Streaming commit on gfx950 (MI355X / CDNA4, wave64): which frames of a stream already carry their final pYIN decode.
//
// The Viterbi of a push leaves, in device memory, the back-pointers of every step so far (ptr, uint16 [frame][state];
// ptr[q][s] = predecessor at frame q - 1 of state s at frame q) and the column of the newest frame t (vstate).  Let A_t
// be the states alive at t (finite value: the band kernel replaces the value of a dead voiced state by -inf and leaves
// its pointer unwritten, viterbi_band.inc "Dead voiced targets") and A_{q-1} = { ptr[q][s] : s in A_q }.  The path the
// final back-trace returns is a chain of these pointers that passes through a live state at t, so it passes through
// A_q at every q <= t.  The class of a state is its output (the bin of a voiced state, "unvoiced" for every s >= B):
// when all of A_q has one class, that class IS the final output of frame q, whatever audio follows.  Only pointers the
// Viterbi kernels have written are followed; no arithmetic is redone, so there is no rounding argument to make.
//
// One workgroup per launch.  The set starts as an S-bit mask in LDS (one lane per state, LDS atomic OR of the
// predecessor's bit, two barriers per frame; a lane that sets a bit first also counts it, so the class test of a frame
// is three LDS reads); the survivor paths merge within a few frames, and once the set has at
// most 64 members one wave carries one member per lane with no barrier at all: per frame one dependent 2-byte load
// (rows written microseconds to seconds earlier: L2 or Infinity Cache), a readfirstlane and a ballot.  The walk stops
// at the previous frontier, so a push pays for its lag, not for the length of the stream.
// Behind it, the two small kernels at the head and the tail of a push's captured graph (advance, gather).
#include "kernels.h"

namespace aegis {

constexpr int kCommitWords = 32;           // mask words: S = 2 B <= 2048 states
constexpr int16_t kUndecided = -2;

__global__ __launch_bounds__(1024) void stream_commit_kernel(const StreamCtl *ctl, int64_t frames_done, StreamCommitCtl *cc,
                                                             const uint16_t *__restrict__ ptr, const double *__restrict__ vstate,
                                                             int B, int16_t *bins, unsigned char *result) {
    __shared__ unsigned long long mask[2][kCommitWords];
    __shared__ int cnt[2][2];              // members of the set: [voiced, unvoiced]
    __shared__ int vany[2];                // a voiced member (THE voiced member when there is one)
    __shared__ int list[64];
    __shared__ int bad;                    // a walked pointer was >= S (unwritten row): the frontier stays where it is
    const int S = 2 * B, NW = (S + 63) >> 6;
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wid = tid >> 6;
    const int64_t t = (ctl ? ctl->frames_done : frames_done) - 1;      // newest frame: vstate is its column
    const int64_t f_old = cc->frontier, lo = f_old + 1;
    int64_t *res = reinterpret_cast<int64_t *>(result);
    int16_t *stage = reinterpret_cast<int16_t *>(result + 32);
    if (t < lo || t == cc->newest) {       // no frame yet, or no new frame since the last walk: nothing can change
        if (tid == 0) { res[0] = f_old; res[1] = f_old; res[2] = t; res[3] = 0; }
        return;
    }
    if (tid < 2 * kCommitWords) (&mask[0][0])[tid] = 0ull;
    if (tid < 4) (&cnt[0][0])[tid] = 0;
    if (tid == 0) bad = 0;
    __syncthreads();
    for (int s = tid; s < S; s += nthr) {                     // (a wave's 64 states are one mask word: nthr % 64 == 0)
        const bool alive = vstate[s] > -INFINITY;
        const unsigned long long bv = __ballot(alive && s < B), bu = __ballot(alive && s >= B);
        if (lane == 0) {
            mask[0][s >> 6] = bv | bu;
            if (bv != 0ull) { atomicAdd(&cnt[0][0], __popcll(bv)); vany[0] = s + __ffsll((long long)bv) - 1; }
            if (bu != 0ull) atomicAdd(&cnt[0][1], __popcll(bu));
        }
    }
    __syncthreads();

    int cur = 0, total = 0, wide = 0;      // wide: frames stepped with the whole workgroup
    int64_t q = t;
    bool few = false;
    // ---- the whole workgroup: the set as a bit mask ----------------------------------------------------------------
    for (;;) {
        const int nv = cnt[cur][0], nu = cnt[cur][1], first_v = vany[cur];
        total = nv + nu;
        const bool decided = total > 0 && (nv == 0 || (nv == 1 && nu == 0));
        if (tid == 0) {
            bins[q] = decided ? (int16_t)(nv ? first_v : -1) : kUndecided;
            if (total == 0) bad = 1;                          // (a column without a finite value: not a Viterbi column)
        }
        if (q == lo || total == 0) break;                     // (lo >= 0: row 0 of ptr is never read)
        if (total <= 64) { few = true; break; }
        if (tid < NW) mask[cur ^ 1][tid] = 0ull;
        if (tid < 2) cnt[cur ^ 1][tid] = 0;
        __syncthreads();
        for (int s = tid; s < S; s += nthr)
            if ((mask[cur][s >> 6] >> (s & 63)) & 1ull) {
                const unsigned pr = ptr[q * S + s];
                if (pr < (unsigned)S) {
                    const unsigned long long bit = 1ull << (pr & 63);
                    if ((atomicOr(&mask[cur ^ 1][pr >> 6], bit) & bit) == 0ull) {      // first to name this predecessor
                        atomicAdd(&cnt[cur ^ 1][pr < (unsigned)B ? 0 : 1], 1);
                        if (pr < (unsigned)B) vany[cur ^ 1] = (int)pr;
                    }
                } else {
                    bad = 1;
                }
            }
        __syncthreads();
        cur ^= 1;
        --q;
        ++wide;
    }
    // ---- at most 64 members: one per lane of wave 0, no barriers ---------------------------------------------------
    if (few) {
        for (int s = tid; s < S; s += nthr) {
            const int w = s >> 6;
            const unsigned long long m = mask[cur][w];
            if ((m >> (s & 63)) & 1ull) {
                int rank = __popcll(m & ((1ull << (s & 63)) - 1ull));
                for (int k = 0; k < w; ++k) rank += __popcll(mask[cur][k]);
                list[rank] = s;
            }
        }
        __syncthreads();
        if (wid == 0) {
            int s = list[lane < total ? lane : 0];
            while (q > lo) {
                unsigned pr = ptr[q * S + s];
                if (pr >= (unsigned)S) { bad = 1; pr = (unsigned)s; }
                s = (int)pr;
                --q;
                const int cls = s < B ? s : B;
                const int c0 = __builtin_amdgcn_readfirstlane(cls);
                const bool decided = __ballot(cls != c0) == 0ull;
                if (lane == 0) bins[q] = decided ? (int16_t)(c0 < B ? c0 : -1) : kUndecided;
            }
        }
    }
    __threadfence();
    __syncthreads();
    // ---- the new frontier: the decided prefix of the walked frames lo .. t ------------------------------------------
    if (wid != 0) return;
    int64_t f = f_old;
    for (int64_t base = lo; base <= t; base += 64) {
        const int64_t qq = base + lane;
        const bool ok = qq <= t && bins[qq] != kUndecided;
        const unsigned long long b = __ballot(ok);
        const int n = b == ~0ull ? 64 : __ffsll((long long)~b) - 1;
        f = base + n - 1;
        if (n < 64) break;
    }
    const int failed = bad;
    if (failed) f = f_old;
    for (int i = lane; i < kCommitStage; i += 64) stage[i] = lo + i <= f ? bins[lo + i] : (int16_t)0;
    if (lane == 0) {
        cc->frontier = f;
        cc->newest = t;
        res[0] = f_old; res[1] = f; res[2] = t; res[3] = failed ? -1 : ((int64_t)wide << 32) | (t - lo + 1);
    }
}

hipError_t launch_stream_commit(const StreamCtl *ctl, int64_t frames_done, StreamCommitCtl *cc, const uint16_t *ptr,
                                const double *vstate, int n_bins, int16_t *bins, void *result, hipStream_t s) {
    const int S = 2 * n_bins;
    if (n_bins < 1 || S > 64 * kCommitWords || n_bins > 32767) return hipErrorInvalidValue;
    const int nthr = S >= 1024 ? 1024 : (S + 63) & ~63;
    hipLaunchKernelGGL(stream_commit_kernel, dim3(1), dim3(nthr), 0, s, ctl, frames_done, cc, ptr, vstate, n_bins, bins,
                       static_cast<unsigned char *>(result));
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Streaming graph helpers.  stream_advance_kernel appends the pushed samples (already on the device in
// a fixed staging buffer) to the clip and derives the push's geometry exactly as the host path does:
// a frame is ready when its centred 2048-sample window is complete.  stream_gather_kernel packs the
// push's outputs into a fixed result block: [0] n_frames, then rms[8] f32, vprob[8] f64, live[8] i32.
// ------------------------------------------------------------------------------------------
__global__ void stream_advance_kernel(StreamCtl *ctl, const float *__restrict__ staging, int n_push,
                                      float *__restrict__ pcm, int hop) {
    const int64_t n0 = ctl->n_samples;
    for (int i = threadIdx.x; i < n_push; i += blockDim.x) pcm[n0 + i] = staging[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t n = n0 + n_push;
        const int64_t ready = n >= 1024 ? (n - 1024) / hop + 1 : 0;
        const int64_t lo = ctl->frames_done, hi = ready > lo ? ready : lo;
        ctl->n_samples = n;
        ctl->t_begin = lo; ctl->n_sel = hi - lo;
        ctl->vt_begin = lo; ctl->vt_end = hi;
        ctl->frames_done = hi;
        ctl->meta[kMetaSampleOff + 1] = n;
        ctl->meta[kMetaSelOff + 1] = hi - lo;
    }
}

__global__ void stream_gather_kernel(const StreamCtl *ctl, const float *__restrict__ rms, const double *__restrict__ vprob,
                                     const int32_t *__restrict__ live, unsigned char *__restrict__ result) {
    const int i = threadIdx.x;
    int64_t *cnt = reinterpret_cast<int64_t *>(result);
    float *r = reinterpret_cast<float *>(result + kGatherRms);
    double *v = reinterpret_cast<double *>(result + kGatherVprob);
    int32_t *l = reinterpret_cast<int32_t *>(result + kGatherLive);
    const int64_t n = ctl->n_sel, t0 = ctl->t_begin;
    if (i == 0) *cnt = n;
    if (i < 8 && i < n) { r[i] = rms[t0 + i]; v[i] = vprob[t0 + i]; l[i] = live[t0 + i]; }
}

void launch_stream_advance(StreamCtl *ctl, const float *staging, int n_push, float *pcm, int hop, hipStream_t s) {
    hipLaunchKernelGGL(stream_advance_kernel, dim3(1), dim3(256), 0, s, ctl, staging, n_push, pcm, hop);
}
void launch_stream_gather(const StreamCtl *ctl, const float *rms, const double *vprob, const int32_t *live, void *result,
                          hipStream_t s) {
    hipLaunchKernelGGL(stream_gather_kernel, dim3(1), dim3(64), 0, s, ctl, rms, vprob, live, static_cast<unsigned char *>(result));
}

}  // namespace aegis
