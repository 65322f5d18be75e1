// HIP kernels for the Aegis analyze path on gfx950 (MI355X / CDNA4, wave64).
//
// Reference behaviour being reproduced (the arithmetic lives in librosa, which
// /root/reference/aegis_engine.py:25-26,63,67,70 calls):
//   frame.hip (this file)  frame_yin_kernel: melspectrogram power + feature.rms + pyin's difference function
//                          (FFT autocorrelation + running energy; the serial walks are frame_walk.h)  
//   obs.hip                pyin_obs_kernel: CMND, troughs, threshold prior, pitch-bin observation (P4-P10)
//   viterbi.hip            882-state log-Viterbi with chunked back-tracking (P11, P12)
//   finalize.hip           power_to_db(ref=max), rake mask (vision.py:3-38), f0 decode, the finite check of the input
//   stream_commit.hip      the streaming graph's helpers and the streaming commit
// Each holds its kernels and their launchers (declared in kernels.h); wave_ops.h and pass_geometry.h are what they share.
// Built with -ffp-contract=off: every multiply/add below rounds exactly where
// NumPy rounds; fused operations are written as fma() where they are wanted.
#include "kernels.h"
#include "fft8.h"
#include "frame_walk.h"
#include "pass_geometry.h"
#include "wave_ops.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace aegis {

// ------------------------------------------------------------------------------------------
// Kernel 1: frame stage.  A 256-thread workgroup owns `frames_per_wg` consecutive selected frames (16 in batch
// launches, 2 for streaming pushes) and takes them two at a time; 81 KB of LDS, so two workgroups share a CU.
//
//   prologue  float32 running energy of pyin's difference function for ALL the workgroup's frames at once, one frame
//             per lane of wave 0: e = np.cumsum(frame**2) is strictly sequential, so the lanes walk their own frame
//             (samples straight from global memory, 16-byte loads, next block in flight) and leave
//             en[tau] = e[1024 + tau] - e[tau] in an LDS row per frame.  Same operations in the same order as NumPy.
//   per frame centred frame -> LDS (zero padded at the clip edges; the next frame's samples are already in flight),
//             feature.rms in NumPy's float32 pairwise order (bit-exact), ONE packed forward FFT
//             Z = FFT(x + i*b), b = reversed first half: A = FFT(x) and B = FFT(b) separate by symmetry, P = A*B is the
//             spectrum of pyin's autocorrelation, and the Hann-windowed spectrum librosa.stft needs is
//             XW[k] = A[k]/2 - (A[k-1] + A[k+1])/4 (periodic Hann in the frequency domain): the mel path costs no FFT.
//             |XW|^2 rounded through complex64 like librosa.stft -> sparse Slaney mel -> clip maximum.
//   per pair  ONE inverse FFT for both frames (Q = P0 + i*P1 by Hermitian extension) -> acf0 + i*acf1, then
//             d[tau] = (en[0] + en[tau]) - 2 acf[tau] with librosa's |.| < 1e-6 clamps, written to HBM (the only
//             pYIN intermediate this kernel materialises; the CMND cumsum and quotient open pyin_obs_kernel).
// FFT: csrc/fft8.h (radix 8 x 8 x 8 x 4 in registers, one in-place LDS buffer).  1.5 FFTs per frame.
// ------------------------------------------------------------------------------------------
constexpr int kFramesPerWg = 16;

constexpr size_t kFrameLdsFixed = (size_t)2048 * 16 + 2048 * 4 + 1040 * 4 + 128 * 4 + 16 * 4 + 256 * 4;

#if defined(AEGIS_ABLATE) && (AEGIS_ABLATE & 128)
__device__ long long g_frm_dbg[24];
#define FRM_TICK(k) { __builtin_amdgcn_s_waitcnt(0); const long long now__ = clock64(); facc[k] += now__ - flast; flast = now__; }
#else
#define FRM_TICK(k)
#endif
// INJECT (aegis_debug_set_difference, a test hook): the difference function is not stored but REPLACED, where it is stored,
// by the caller's row of the frame's output index (inj [out_total][max_period + 1]); everything else runs as always.  The
// shipping kernel is the INJECT = false instantiation, which holds no trace of the hook (inj is NULL and never read); the
// INJECT = true one is launched by an armed call only.
template <bool INJECT>
__global__ __launch_bounds__(256, 2) void frame_yin_kernel(PassParams p, DevTables tb, int frames_per_wg, int en_stride,
                                                           const double *__restrict__ inj) {
#if defined(AEGIS_ABLATE) && (AEGIS_ABLATE & 128)
    long long facc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, flast = clock64();
#endif
    extern __shared__ __align__(16) unsigned char fsm[];
    double2 *z = reinterpret_cast<double2 *>(fsm);               // [2048] FFT buffer (swizzled index, fft8.h)
    float *xs = reinterpret_cast<float *>(z + 2048);             // [2048] the frame
    float *pw = xs + 2048;                                       // [1040] windowed power spectrum (1025 bins, zero tail)
    float *red = pw + 1040;                                      // [128]  rms partial sums
    float *blk = red + 128;                                      // [16]
    float *part = blk + 16;                                      // [256]  mel partial sums, one per 16-bin chunk of a triangle
    float *en = part + 256;                                      // [frames_per_wg][en_stride] running energies
    int64_t *frow = reinterpret_cast<int64_t *>(en + (size_t)frames_per_wg * en_stride);   // [frames_per_wg] workspace row of each frame, -1: not live (epilogue)

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int64_t n_sel = geo_n_sel(p);
    const int64_t fs0 = (int64_t)blockIdx.x * frames_per_wg;
    if (fs0 >= n_sel) return;
    const int nfr = (int)min((int64_t)frames_per_wg, n_sel - fs0);
    const bool want_pyin = (p.stages & 0x4u) != 0, want_mel = (p.stages & 0x3u) != 0;
    const bool want_rms = (p.stages & 0x8u) && p.out_rms != nullptr;
    const bool want_fft = (p.stages & 0x7u) != 0;
    const int mp = p.max_period;

    struct Geo { bool live; int c; int64_t base, n, start, f, o; };
    auto locate = [&](int i) {
        Geo g{false, 0, 0, 0, 0, 0, 0};
        g.live = i < nfr;
        if (g.live) {
            int64_t t;
            map_frame(p, fs0 + i, g.c, t, g.f);
            g.o = out_index(p, g.c, t);
            g.base = p.sample_off[g.c];
            g.n = p.sample_len[g.c];
            g.start = t * p.hop - 1024;
        }
        return g;
    };
    auto fetch = [&](const Geo &g, float (&v)[8]) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int64_t idx = g.start + tid + r * 256;
            v[r] = (g.live && idx >= 0 && idx < g.n) ? p.pcm[g.base + idx] : 0.0f;
        }
    };
    // Frame i + 1 of the workgroup is normally the next frame of frame i's clip: one comparison against the end of the
    // clip's selection then replaces locate()'s binary search, a chain of dependent loads each frame had to wait for.
    auto locate_next = [&](const Geo &g, int i, int64_t sel_end) {
        if (i < nfr && g.live && fs0 + i < sel_end) {
            Geo n = g;
            n.start += p.hop; n.f += 1; n.o += 1;
            return n;
        }
        return locate(i);
    };
    Geo geo = locate(0);
    int64_t geo_sel_end = geo.live ? p.sel_off[geo.c + 1] : 0;
    float nx[8];
    fetch(geo, nx);
    Fft8Tw twr;

    // mel: thread t owns chunk t of the filterbank (<= 16 consecutive bins of one triangle) and, for t < n_mels, band t
    const bool has_chunk = want_mel && tid < tb.mel_chunks;
    const int mel_bin = has_chunk ? tb.mel_chunk_bin[tid] : 0;
    int band_c0 = 0, band_c1 = 0;             // band (tid mod 128): threads 0..127 sum it for the pair's first frame, 128..255 for the second
    if (want_mel && (tid & 127) < p.n_mels) { band_c0 = tb.mel_band_chunk[tid & 127]; band_c1 = tb.mel_band_chunk[(tid & 127) + 1]; }
    float *pw1 = xs;                          // the SECOND frame's power spectrum lives in the frame buffer, dead once that frame's FFT has read it
    float *part1 = xs + 1040;                 // ... and its chunk sums behind it
    if (tid < 15) pw[1025 + tid] = 0.0f;         // the last chunks read (zero-weighted) bins past 1024

    // ---- prologue: running energy of every frame of the workgroup, one frame per lane ------------------------
    if (want_pyin) {
        // The workgroup's frames are normally consecutive frames of one clip: their samples (one contiguous stretch,
        // <= 15 hops + 2048 samples) are staged with coalesced loads in the FFT buffer + frame area, which nothing
        // uses yet, so the serial walk reads LDS instead of waiting for a global load per eight samples.
        const Geo g0 = geo;
        Geo gl = g0;
        if (fs0 + nfr - 1 < geo_sel_end) { gl.start += (int64_t)(nfr - 1) * p.hop; } else gl = locate(nfr - 1);
        const int64_t span = (int64_t)(nfr - 1) * p.hop + 2048;
        const bool staged = g0.c == gl.c && p.hop == 512 && span + 4 * (span >> 9) <= 10240;
        float *stage = reinterpret_cast<float *>(z);
        if (staged) {                                // sample i sits at i + 4 (i / 512): the lanes' frames start one hop apart,
            // the skew puts their 16-byte reads on distinct bank groups.  Four samples per thread and request, all of a
            // thread's (<= 10) requests in flight together: one sample per request and iteration made the staging, not the
            // walk, two thirds of the prologue (a memory latency per iteration, 38 iterations).
            const float *__restrict__ x0 = p.pcm + g0.base;
            const int n4 = (int)(span >> 2);                 // span is a multiple of 4 (hop = 512)
            float4 sv[10];
#pragma unroll
            for (int u = 0; u < 10; ++u) {
                const int q = tid + 256 * u;
                const int64_t idx = g0.start + 4 * (int64_t)q;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (q < n4) {
                    if (idx >= 0 && idx + 3 < g0.n) {
                        // clip offsets are arbitrary, so the address is only 4-byte aligned: the vector type says so (the
                        // load is still one global_load_dwordx4, but nothing may assume 16-byte alignment)
                        typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
                        const f4u t = *reinterpret_cast<const f4u *>(x0 + idx);
                        v = make_float4(t.x, t.y, t.z, t.w);
                    } else {                                 // clip edge: librosa's centre padding is zeros
                        if (idx >= 0 && idx < g0.n) v.x = x0[idx];
                        if (idx + 1 >= 0 && idx + 1 < g0.n) v.y = x0[idx + 1];
                        if (idx + 2 >= 0 && idx + 2 < g0.n) v.z = x0[idx + 2];
                        if (idx + 3 >= 0 && idx + 3 < g0.n) v.w = x0[idx + 3];
                    }
                }
                sv[u] = v;
            }
#pragma unroll
            for (int u = 0; u < 10; ++u) {
                const int q = tid + 256 * u;
                if (q < n4) {                                // squared here, by all threads, not inside the serial walk
                    const int i = 4 * q;
                    *reinterpret_cast<float4 *>(stage + i + 4 * (i >> 9)) =
                        make_float4(sv[u].x * sv[u].x, sv[u].y * sv[u].y, sv[u].z * sv[u].z, sv[u].w * sv[u].w);
                }
            }
            __syncthreads();
        }
        // The walk is one dependent add after another: beside another workgroup's FFT waves on the same SIMD it would
        // get an issue slot only when they stall, while this workgroup's other three waves wait for it -- raise it.
        if (wid == 0) __builtin_amdgcn_s_setprio(3);
        if (wid == 0 && lane < nfr) {
            float *row = en + lane * en_stride;
            if (staged) {
                const float *srow = stage + lane * (512 + 4);
                energy_walk<true>([&](int j, float4 &a, float4 &b) {
                    const float *q = srow + j + 4 * (j >> 9);                // j + 8 <= 1024 + 8 nA + 8 < 2048: inside the frame
                    a = *reinterpret_cast<const float4 *>(q);
                    b = *reinterpret_cast<const float4 *>(q + 4);
                }, row, mp);
            } else {                                         // frames of two clips, or a hop the staging area cannot hold
                const Geo g = locate(lane);
                const float *__restrict__ x = p.pcm + g.base;
                energy_walk_plain([&](int j) {
                    const int64_t q = g.start + j;
                    return (q >= 0 && q < g.n) ? x[q] : 0.0f;
                }, row, mp);
            }
        }
        if (wid == 0) __builtin_amdgcn_s_setprio(0);
        if (staged) __syncthreads();                     // the staging area becomes the FFT buffer and the frame again
    }
    // (the first barrier of the frame loop publishes the rows)
    if (want_fft) fft8_load_twiddles(twr, tb.twiddle, tid);      // 40 registers: loaded after the walk, which wants its own
    FRM_TICK(0)
    // Loads and stores share ONE vector-memory counter, and the difference-function stores that end a pair are conditional,
    // so a wait for the prefetched samples at the top of the next pair can only be vmcnt(0): it also waited for those rows
    // (4.3 KB each, a few hundred cycles old) to be acknowledged, once per pair.  The samples are waited for explicitly
    // instead, where no fresh stores are outstanding: here, and behind the pair's second frame (below).  With nothing of
    // theirs pending on any path into the loop head, the frame buffer writes of a pair's first frame need no wait, and the
    // d rows are first waited for at the top of the pair's second frame, a forward transform later.
    // This rests on where the compiler's wait insertion puts its own waits: results never depend on it, the time does.
    // After a compiler upgrade, or an edit that leaves a sample load pending on some path into the loop head, look at the
    // ISA again (hipcc -O3 -ffp-contract=off --offload-arch=gfx950 --cuda-device-only -S): no `s_waitcnt vmcnt` may
    // stand in front of the first four `ds_write2st64_b32` of the pair loop (the first frame's buffer writes);
    // tools/isa_inflight.py prints what stands there and tests/test_frame_isa_inflight.py holds it.  Two pieces of work
    // below exist only to steer that wait insertion and compute nothing: the mel section's 32 power reads and its wait
    // stand outside `if (want_mel)` (a call without the mel stage reads 32 unused words per pair), and the quotient
    // loop's reads carry no condition (a small launch's dead frames read a live row's entries again).
    __builtin_amdgcn_s_waitcnt(kWaitVmcnt0);

    for (int pr = 0; pr < nfr; pr += 2) {
        double2 P[2][4], Pn[2];                // P = A B of the thread's four bins per frame; Pn: of the Nyquist bin (thread 255 only)
        int64_t fidx[2] = {0, 0};
        int64_t fout[2] = {0, 0};             // (INJECT only) output index of each frame: the caller's rows are in output order
        bool flive[2] = {false, false};
        int fclip[2] = {0, 0};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int r = 0; r < 4; ++r) P[h][r] = make_double2(0.0, 0.0);
            Pn[h] = make_double2(0.0, 0.0);
            if (pr + h >= nfr) continue;                      // odd tail: the pair's second frame does not exist (uniform)
            const bool live = geo.live;
            const int c = geo.c;
            const int64_t f = geo.f, fo = geo.o;
            fidx[h] = f; flive[h] = live; fclip[h] = c;
            if constexpr (INJECT) fout[h] = fo;
            if (tid == 0) frow[pr + h] = live ? f : -1;
#pragma unroll
            for (int r = 0; r < 8; ++r) xs[tid + r * 256] = nx[r];
            {
                const int cprev = geo.c;
                geo = locate_next(geo, pr + h + 1, geo_sel_end);
                if (geo.live && geo.c != cprev) geo_sel_end = p.sel_off[geo.c + 1];
            }
            fetch(geo, nx);                                   // in flight under everything below
            __syncthreads();
            FRM_TICK(1)

            // ---- feature.rms: np.mean(np.square(x), axis=-2) then sqrt, float32, NumPy's pairwise order -------
            if (want_rms && tid < 128) {
                const int bb = tid >> 3, a = tid & 7;
                const float *xb = xs + bb * 128 + a;
                // all sixteen reads requested before the first square: the adds chain in NumPy's order as before, behind
                // counted waits instead of an LDS round trip each (waves 2 and 3 wait for this at the transform's first barrier)
                float xv[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) xv[i] = xb[8 * i];
                __builtin_amdgcn_sched_barrier(0);
                float r = xv[0] * xv[0];
#pragma unroll
                for (int i = 1; i < 16; ++i) r = r + xv[i] * xv[i];
                red[tid] = r;
            }
            if (!want_fft) {
                __syncthreads();
                if (want_rms && tid < 16) {
                    const float *r = red + tid * 8;
                    blk[tid] = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
                }
                __syncthreads();
            } else {
                // ---- packed forward FFT of (frame, reversed first half); pass 1 straight from the frame ----
                double2 v[8];
                {
                    float xf[8], xr[4];                       // the thread's twelve samples in flight together
#pragma unroll
                    for (int q = 0; q < 8; ++q) xf[q] = xs[tid + 256 * q];
#pragma unroll
                    for (int q = 0; q < 4; ++q) xr[q] = xs[1024 - (tid + 256 * q)];
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int q = 0; q < 8; ++q) v[q] = make_double2((double)xf[q], q < 4 ? (double)xr[q] : 0.0);
                }
                fft8_pass1_write(z, tid, v);
                __syncthreads();
                if (want_rms && tid < 16) {
                    const float *r = red + tid * 8;
                    blk[tid] = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
                }
                fft8_read8(z, tid, v);
                __syncthreads();
                fft8_pass_write<8>(z, tid, v, twr.p2);
                __syncthreads();
                fft8_read8(z, tid, v);
                __syncthreads();
                fft8_pass_write<64>(z, tid, v, twr.p3);
                __syncthreads();
                fft8_pass4(z, tid, twr);
                __syncthreads();
            }
            FRM_TICK(2)
            if (want_rms && tid == 0 && live) {
                float b0 = (blk[0] + blk[1]) + (blk[2] + blk[3]);
                float b1 = (blk[4] + blk[5]) + (blk[6] + blk[7]);
                float b2 = (blk[8] + blk[9]) + (blk[10] + blk[11]);
                float b3 = (blk[12] + blk[13]) + (blk[14] + blk[15]);
                const float total = 0.0f + ((b0 + b1) + (b2 + b3));
                p.out_rms[fo] = sqrtf(total / 2048.0f);
            }
            if (!want_fft) continue;

            // ---- A[k] = FFT(x)[k], B[k] = FFT(b)[k] from Z by symmetry; P = A*B; windowed power from A ----------
            // A thread owns FOUR CONSECUTIVE bins k = 4 tid .. 4 tid + 3 (all 256 threads; 1025 bins are four per thread plus
            // the Nyquist bin, below): the windowed spectrum needs A[k - 1] and A[k + 1], which are then the thread's own
            // neighbours -- six (z[k], z[2048 - k]) pairs per thread and frame instead of fifteen with bins 256 apart, and an
            // instruction stream of four bins on every wave (five bins per thread ran the fifth on all four waves, the last
            // wave for 13 live lanes).  Lanes 64 bytes apart; with the zsw swizzle the 16 lanes of a ds_read_b128 group meet
            // on bank groups no more often than at 80 bytes.  k is taken modulo 2048: A[-1] = conj(A[1]).
            {
                auto zpair = [&](int k, double2 &zk, double2 &zn) { zk = z[zsw(k & 2047)]; zn = z[zsw((2048 - k) & 2047)]; };
                // A2 = 2 A and B2 = 2 B: the halves are folded into the powers of two applied later (P = A B arrives as 4 P in the
                // inverse transform, whose outputs are scaled by 1/8192 instead of 1/2048; the windowed spectrum is
                // A/2 - (A- + A+)/4 = (2 A2 - (A2- + A2+)) / 8) -- exact scalings, every value bit-identical
                auto Afrom = [](const double2 &zk, const double2 &zn) { return make_double2(zk.x + zn.x, zk.y - zn.y); };
                // one bin: its product P = A B and its windowed power
                auto bin = [&](int k, const double2 &Am, const double2 &A, const double2 &Ap, const double2 &zk, const double2 &zn,
                               double2 &Pk) {
                    if (want_pyin) {
                        const double2 Bv = make_double2(zk.y + zn.y, zn.x - zk.x);
                        Pk = c_mul(A, Bv);
                    }
                    if (want_mel) {
                        const float re = (float)(0.125 * (2.0 * A.x - (Am.x + Ap.x)));
                        const float im = (float)(0.125 * (2.0 * A.y - (Am.y + Ap.y)));
                        const float mag = (float)sqrt((double)re * (double)re + (double)im * (double)im);  // npy_hypotf
                        (h == 0 ? pw : pw1)[k] = mag * mag;
                    }
                };
                const int k0 = 4 * tid;
                double2 zk, zn, zk1, zn1;
                zpair(k0 - 1, zk, zn);
                double2 Am = Afrom(zk, zn);
                zpair(k0, zk, zn);
                double2 A = Afrom(zk, zn);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    zpair(k0 + r + 1, zk1, zn1);
                    const double2 Ap = Afrom(zk1, zn1);
                    bin(k0 + r, Am, A, Ap, zk, zn, P[h][r]);
                    Am = A; A = Ap; zk = zk1; zn = zn1;
                }
                // The Nyquist bin 1024 is the last thread's fifth: it holds A[1023], A[1024] and the pair of bin 1024 already,
                // and A[1025] = conj(A[1023]) -- the sum A[1023] + A[1025] the window takes is the same to the bit
                // (x the same two addends, y = a + (-a) = +0 as (a) + (b - c) with b - c = -a was).
                if (tid == 255) bin(1024, Am, A, make_double2(Am.x, -Am.y), zk, zn, Pn[h]);
            }
            if (want_mel && h == 1 && tid < 15) pw1[1025 + tid] = 0.0f;      // the last chunks read (zero-weighted) bins past 1024
            __syncthreads();
            FRM_TICK(3)
        }
        // ---- mel projection of BOTH frames of the pair: sparse Slaney triangles.  Every <= 16-bin chunk of a triangle is
        // one thread's float32 fma chain per frame (the 16 weights requested once per pair); a band then adds its
        // chunks' sums in order (the widest band has six), threads 0..127 for the first frame and 128..255 for the
        // second.  Clip maximum.  One section per pair instead of one per frame: half the barriers, half the weight
        // traffic, all four waves busy in the band phase.
        // The section is a few dozen fmas behind an L2 round trip (the weights) and the LDS round trips of 32 powers, so it
        // is laid out for those to overlap: the weights are requested FIRST; under them the input of the inverse transform
        // is written (below: z is dead since the barrier above, and the writes release the 40 registers of P for what
        // follows) and both frames' powers are requested, all 32 before the first fma; then ONE wait takes the weights
        // over.  That wait is also the wait for the next pair's first frame (requested a forward transform ago), see above
        // the loop: it stands outside every condition, and what is outstanding besides samples and weights is the
        // second frame's rms store, a power section old.
        float4 w0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), w1 = w0, w2 = w0, w3 = w0;
        if (has_chunk) {
            const float4 *wp = reinterpret_cast<const float4 *>(tb.mel_chunk_w) + tid * 4;
            w0 = wp[0]; w1 = wp[1]; w2 = wp[2]; w3 = wp[3];
        }
        // ---- input of the one inverse FFT for both frames: conj(Q), Q = Hermitian extension of P0 + i*P1 --------
        if (__builtin_expect(want_pyin, 1)) {    // the thread's own four consecutive bins (see above)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = 4 * tid + r;
                const double2 u = P[0][r], v = P[1][r];
                z[zsw(k)] = make_double2(u.x - v.y, -u.y - v.x);                          // conj(P0) - i conj(P1)
                if (k > 0) z[zsw(2048 - k)] = make_double2(u.x + v.y, u.y - v.x);         // P0 - i P1
            }
            if (tid == 255) z[zsw(1024)] = make_double2(Pn[0].x - Pn[1].y, -Pn[0].y - Pn[1].x);      // the Nyquist bin: no mirror
        }
        // The reads and the wait stand outside every condition (threads without a chunk, and calls without the mel stage,
        // read bins 0..15: in bounds, never used): a wait on one side of a branch leaves the compiler a path into the loop
        // head on which the samples count as pending, and it then waits in front of the first frame's buffer writes.
        float pa[16], pb[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) pa[k] = pw[mel_bin + k];
#pragma unroll
        for (int k = 0; k < 16; ++k) pb[k] = pw1[mel_bin + k];
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(kWaitVmcnt0);
        if (__builtin_expect(want_mel, 1)) {
            const float wv[16] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w, w3.x, w3.y, w3.z, w3.w};
            float acc0 = 0.0f, acc1 = 0.0f;
#pragma unroll
            for (int k = 0; k < 16; ++k) acc0 = fmaf(wv[k], pa[k], acc0);
#pragma unroll
            for (int k = 0; k < 16; ++k) acc1 = fmaf(wv[k], pb[k], acc1);
            if (has_chunk) { part[tid] = acc0; part1[tid] = acc1; }
            // this barrier publishes the chunk sums and, with them, the input of the inverse transform
            __syncthreads();
            {
                const int h = wid >> 1, bt = tid & 127;           // waves 0, 1: first frame; waves 2, 3: second
                const bool live = flive[h];
                const float *pt = h == 0 ? part : part1;
                float acc = 0.0f;
                if (bt < p.n_mels && live) {
                    // the band's chunk sums added in order; the first six (every band of the default bank has at most
                    // six) are requested together instead of one LDS round trip per chunk
                    const int c0 = band_c0, c1 = band_c1;
                    float pv[6];
#pragma unroll
                    for (int k = 0; k < 6; ++k) pv[k] = pt[min(c0 + k, 255)];
                    acc = c0 < c1 ? pv[0] : 0.0f;
#pragma unroll
                    for (int k = 1; k < 6; ++k) if (c0 + k < c1) acc = acc + pv[k];
                    for (int cidx = c0 + 6; cidx < c1; ++cidx) acc = acc + pt[cidx];
                    p.melpow[fidx[h] * p.n_mels + bt] = acc;
                }
                // powers are >= 0: float order == unsigned order of the bits
                const unsigned m = wave_umax(__float_as_uint(acc));
                if (lane == 0 && live) atomicMax(&p.clipmax[fclip[h]], m);
            }
            // pw, pw1 and the chunk sums are next written behind the barriers of the inverse FFT; without it the next pair's
            // first frame would land in the frame buffer while the second frame's chunk sums are still being read
            if (!want_pyin) __syncthreads();
        }
        FRM_TICK(4)
        if (!want_pyin) continue;

        // ---- one inverse FFT for both frames (its input was written in front of the mel section, whose barrier published it)
        if (!want_mel) __syncthreads();
        {
            double2 v[8];
            fft8_read8(z, tid, v);
            __syncthreads();
            fft8_pass1_write(z, tid, v);
            __syncthreads();
            fft8_read8(z, tid, v);
            __syncthreads();
            fft8_pass_write<8>(z, tid, v, twr.p2);
            __syncthreads();
            fft8_read8(z, tid, v);
            __syncthreads();
            fft8_pass_write<64>(z, tid, v, twr.p3);
            __syncthreads();
            fft8_pass4_lags(z, tid, twr, mp);          // only the lags the difference function reads
            __syncthreads();
        }
        FRM_TICK(5)
        // FFT(conj Q) = N * conj(acf0 + i acf1); difference function with librosa's clamps (pitch.py::_cumulative_mean_normalized_difference)
        // With the CMND formed in this kernel's epilogue, the FIRST frame's row stays in LDS: the pair's two energy rows are
        // dead once read, and together they are exactly one float64 row (8 (max_period + 1) <= 8 en_stride bytes).  Only the
        // second frame's row makes the trip through global memory and back.
        const bool keep_first = p.cmnd_in_frame != 0;
        if (keep_first) {
            float es[2][3];                  // en[0] + en[tau] of both frames (float32, librosa's clamps), read before the rows are overwritten
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float *row = en + (pr + h) * en_stride;
                float en0 = row[0];
                if (fabsf(en0) < 1e-6f) en0 = 0.0f;
#pragma unroll
                for (int u = 0; u < 3; ++u) {
                    float e = row[min(tid + 256 * u, mp)];
                    if (fabsf(e) < 1e-6f) e = 0.0f;
                    es[h][u] = en0 + e;
                }
            }
            __syncthreads();                 // every thread has read its energies: the two rows become the first frame's d row
            double *__restrict__ d0 = reinterpret_cast<double *>(en + pr * en_stride);
            double *__restrict__ d1 = p.dfn + fidx[1] * (int64_t)p.lag_stride;
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int tau = tid + 256 * u;
                if (tau <= mp) {
                    const double2 zz = z[zsw(1024 + tau)];
                    double a0 = zz.x * (1.0 / 8192.0), a1 = -zz.y * (1.0 / 8192.0);      // 1/2048 of the transform, 1/4 of P (see A2, B2)
                    if (fabs(a0) < 1e-6) a0 = 0.0;
                    if (fabs(a1) < 1e-6) a1 = 0.0;
                    if constexpr (INJECT) {
                        if (flive[0]) d0[tau] = inj[fout[0] * (int64_t)(mp + 1) + tau];
                        if (flive[1]) d1[tau] = inj[fout[1] * (int64_t)(mp + 1) + tau];
                    } else {
                        if (flive[0]) d0[tau] = (double)es[0][u] - 2.0 * a0;
                        if (flive[1]) d1[tau] = (double)es[1][u] - 2.0 * a1;
                    }
                }
            }
        } else {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (!flive[h]) continue;
            const float *row = en + (pr + h) * en_stride;
            float en0 = row[0];
            if (fabsf(en0) < 1e-6f) en0 = 0.0f;
            double *__restrict__ drow = p.dfn + fidx[h] * (int64_t)p.lag_stride;
            for (int tau = tid; tau <= mp; tau += 256) {
                const double2 zz = z[zsw(1024 + tau)];
                double a = (h == 0 ? zz.x : -zz.y) * (1.0 / 8192.0);
                if (fabs(a) < 1e-6) a = 0.0;
                float e = row[tau];
                if (fabsf(e) < 1e-6f) e = 0.0f;
                const float esum = en0 + e;
                if constexpr (INJECT) drow[tau] = inj[fout[h] * (int64_t)(mp + 1) + tau];
                else drow[tau] = (double)esum - 2.0 * a;
            }
        }
        }
        // the next pair's first write into z (pass 1) comes after that frame's first barrier
        FRM_TICK(6)
    }
    // ---- epilogue: cumulative-mean-normalised difference of ALL the workgroup's frames -------------------------------
    // yin[tau] = d[tau] / (cumsum(d[1:])[tau] / tau + tiny), pitch.py::_cumulative_mean_normalized_difference.  np.cumsum is
    // strictly sequential in float64: one lane per frame walks it, all frames of the workgroup in one wave's lanes at once
    // (pyin_obs_kernel spent a third of its time issuing whole-wave instructions for one lane's walk, frame after frame).
    // The rows of the even frames never left LDS (the pair loop wrote them over the pair's energy rows); those of the odd
    // frames come back from L2 / the fabric (this workgroup wrote them a moment ago) into the FFT buffer, which is dead by
    // now.  Every thread keeps its share of d in registers, the walk turns the LDS copy into the cumsum in place, the
    // quotients run on all threads and go out over d[min_period..]: pyin_obs_kernel reads the CMND directly.
    if (want_pyin && p.cmnd_in_frame) {
        const int RS = frame_cmnd_stride(mp), minp = p.min_period;
        // rows of the even frames: where the pair loop left them (over the pair's energy rows); rows of the odd frames: back
        // from global memory into the FFT buffer / frame / power area
        double *zrows = reinterpret_cast<double *>(fsm);
        auto row_of = [&](int i) { return (i & 1) ? zrows + (i >> 1) * RS : reinterpret_cast<double *>(en + i * en_stride); };
        __syncthreads();                         // the d rows are written (workgroup-scope release), the other LDS buffers are free
        double dv[kFramesPerWg][3];
        int64_t fr[kFramesPerWg];
#pragma unroll
        for (int i = 0; i < kFramesPerWg; ++i) fr[i] = i < nfr ? frow[i] : -1;
#pragma unroll
        for (int i = 0; i < kFramesPerWg; ++i) {
            const double *__restrict__ src = (i & 1) ? p.dfn + (fr[i] < 0 ? 0 : fr[i]) * (int64_t)p.lag_stride : row_of(i);
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int tau = tid + 256 * u;
                dv[i][u] = (fr[i] >= 0 && tau <= mp) ? src[tau] : 0.0;
            }
        }
#pragma unroll
        for (int i = 1; i < kFramesPerWg; i += 2) {
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int tau = tid + 256 * u;
                if (i < nfr && tau <= mp) zrows[(i >> 1) * RS + tau] = dv[i][u];
            }
        }
        __syncthreads();
        FRM_TICK(7)
        if (wid == 0) __builtin_amdgcn_s_setprio(3);
        if (wid == 0 && lane < nfr) cmnd_walk(row_of(lane), mp);
        if (wid == 0) __builtin_amdgcn_s_setprio(0);
        __syncthreads();
        FRM_TICK(8)
        const bool troughs = p.troughs != 0;
        // A frame's three cumsum entries are requested together, in front of its three divisions: one LDS round trip per
        // frame instead of one per quotient.  (Requesting the NEXT frame's entries under this frame's divisions as well was
        // measured and is not kept: profiles/frame_latency_quotient_prefetch_experiment.patch.)
        // The reads carry no condition (a choice of row by liveness became a branch per frame): frames past the workgroup's
        // last read the last even or odd row again, lags past max_period read entry max_period -- all in bounds, none of
        // these values used.  A clamped row is read at the thread's own lags, which only this thread writes; entry
        // max_period read by a thread whose lag lies past it belongs to another thread, which in troughs mode may be
        // writing its quotient over it in this same unsynchronised loop: a race on a value that is never used.
        auto q_live = [&](int i, int u) { const int tau = tid + 256 * u; return fr[i] >= 0 && tau >= minp && tau <= mp; };
        auto cs_read = [&](int i, double (&c)[3]) {
            const double *src = (i & 1) ? zrows + min(i >> 1, frames_per_wg / 2 - 1) * RS
                                        : reinterpret_cast<const double *>(en + min(i, frames_per_wg - 2) * en_stride);
#pragma unroll
            for (int u = 0; u < 3; ++u) c[u] = src[min(tid + 256 * u, mp)];
        };
#pragma unroll
        for (int i = 0; i < kFramesPerWg; ++i) {
            double *__restrict__ drow = p.dfn + (fr[i] < 0 ? 0 : fr[i]) * (int64_t)p.lag_stride;
            double *cs = row_of(i);
            double cv[3];
            cs_read(i, cv);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int tau = tid + 256 * u;
                if (q_live(i, u)) {
                    const double yv = dv[i][u] / (cv[u] / (double)tau + DBL_MIN);
                    if (troughs) cs[tau] = yv;          // the CMND stays in LDS, over the cumsum entry this thread has read (into cv)
                    else drow[tau] = yv;
                }
            }
        }
        FRM_TICK(9)
        // ---- troughs of the CMND, compacted (round 4).  pyin_obs_kernel used to load the 495-lag CMND row of every frame
        // from memory and spend a sixth of its time finding the local minima; here the row is in LDS anyway, so every wave
        // takes the frames wid, wid + 4, ... of the workgroup, finds the troughs exactly as pyin_obs_kernel does (util.localmin
        // plus the special first element) and writes, in ascending lag
        // order, each trough's CMND value, its parabolic shift (pitch.py::_parabolic_interpolation: a function of the three
        // CMND values around it) and its lag index: a few hundred bytes per frame instead of the 4 KB row, and the
        // observation kernel starts at the threshold prior.
        if (troughs) {
            __syncthreads();
            const int nl = p.n_lags, KM = trough_km(nl), NR = (nl + 63) >> 6;
            const unsigned long long below = (1ull << lane) - 1ull;
            for (int i = wid; i < nfr; i += 4) {
                if (fr[i] < 0) continue;                                  // (uniform)
                const double *__restrict__ y = row_of(i) + minp;
                double *__restrict__ trow = p.dfn + fr[i] * (int64_t)p.lag_stride;
                int16_t *__restrict__ tiv = reinterpret_cast<int16_t *>(trow + 8 + 2 * KM);
                // lag k = 64 r + lane: consecutive lanes read consecutive doubles (a contiguous chunk per lane, as
                // pyin_obs_kernel walks the row, puts 32 lanes on one pair of banks); ascending lag order = round after
                // round, lane after lane, so a round's ballot and a population count place its troughs
                int K = 0;
                for (int r = 0; r < NR; ++r) {
                    const int k = 64 * r + lane;
                    bool tr = false;
                    double ym = 0.0, y0 = 0.0, yp = 0.0;
                    if (k < nl) {
                        y0 = y[k];
                        if (k > 0) ym = y[k - 1];
                        if (k < nl - 1) yp = y[k + 1];
                        if (k == 0) tr = y0 < yp;
                        else if (k == nl - 1) tr = y0 < ym;
                        else tr = (y0 < ym) && (y0 <= yp);
                    }
                    const unsigned long long m = __ballot(tr);
                    if (tr) {
                        const int pos = K + __popcll(m & below);
                        double shift = 0.0;
                        if (k > 0 && k < nl - 1) {
                            const double a = yp + ym - 2.0 * y0;
                            const double b = (yp - ym) / 2.0;
                            if (fabs(b) < fabs(a)) shift = -b / a;
                        }
                        trow[8 + pos] = y0;
                        trow[8 + KM + pos] = shift;
                        tiv[pos] = (int16_t)k;
                    }
                    K += __popcll(m);
                }
                if (lane == 0) trow[0] = __longlong_as_double((long long)K);
            }
        }
    }
#if defined(AEGIS_ABLATE) && (AEGIS_ABLATE & 128)
    if (blockIdx.x == 1000 && (tid == 0 || tid == 64)) { for (int k = 0; k < 10; ++k) g_frm_dbg[(tid ? 12 : 0) + k] = facc[k]; }
#endif
}
#if defined(AEGIS_ABLATE) && (AEGIS_ABLATE & 128)
hipError_t frame_debug_fetch(long long *dst) { return hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_frm_dbg), sizeof(long long) * 24); }
#else
hipError_t frame_debug_fetch(long long *dst) { for (int i = 0; i < 24; ++i) dst[i] = 0; return hipSuccess; }
#endif
hipError_t frame_set_lds_limits() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(frame_yin_kernel<false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(frame_yin_kernel<true>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

// frames per workgroup of a batch launch: as many as keep two workgroups on a CU (16 at the reference's rates)
int frame_batch_fpw(int max_period) {
    const int stride = frame_en_stride(max_period);
    int fpw = kFramesPerWg;
    while (fpw > 2 && kFrameLdsFixed + (size_t)fpw * stride * 4 > 80 * 1024) fpw -= 2;
    return fpw;
}
int trough_row_doubles_host(int n_lags) { return trough_row_doubles(n_lags); }
bool frame_cmnd_supported(int max_period) {
    // the epilogue keeps three lags per thread and frame in registers and one row per frame in the LDS the loop has freed
    if (max_period + 1 > 3 * 256) return false;
    const int stride = frame_en_stride(max_period), rs = frame_cmnd_stride(max_period);
    if (stride < max_period + 1) return false;                   // a pair's two energy rows hold one float64 row
    for (int fpw : {2, frame_batch_fpw(max_period)})               // the odd frames' rows share the fixed buffers
        if ((size_t)(fpw / 2) * rs * 8 + 64 > kFrameLdsFixed) return false;
    return true;
}
void launch_frame(const PassParams &p, const DevTables &t, hipStream_t s, const double *inject_d) {
    if (p.n_sel == 0 || !(p.stages & 0xFu)) return;
    const int stride = frame_en_stride(p.max_period);
    // the running-energy prologue is one serial walk per workgroup, so small launches (streaming pushes) take a pair each
    const int fpw = p.n_sel >= 4096 ? frame_batch_fpw(p.max_period) : 2;
    size_t lds = kFrameLdsFixed + (size_t)fpw * stride * 4 + (size_t)fpw * 8;     // + the frames' workspace rows (epilogue)
    // AEGIS_FRAME_LDS_MIN=<bytes> (experiment knob): ask for at least that much LDS, e.g. 100000 keeps one workgroup per CU
    static const size_t lds_min = [] { const char *e = std::getenv("AEGIS_FRAME_LDS_MIN"); return e ? (size_t)std::atol(e) : (size_t)0; }();
    lds = std::max(lds, std::min<size_t>(lds_min, 160 * 1024));
    const dim3 grid((unsigned)((p.n_sel + fpw - 1) / fpw));
    if (inject_d) hipLaunchKernelGGL(frame_yin_kernel<true>, grid, dim3(256), lds, s, p, t, fpw, stride, inject_d);
    else hipLaunchKernelGGL(frame_yin_kernel<false>, grid, dim3(256), lds, s, p, t, fpw, stride, static_cast<const double *>(nullptr));
}

}  // namespace aegis
