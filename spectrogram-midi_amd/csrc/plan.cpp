// Pass planner (plan.h).  Everything here is a function of the call's clips, the handle's knobs and its adaptive state.
#include "plan.h"

#include <cmath>
#include <cstdlib>
#include <numeric>
#include <stdexcept>

namespace aegis {

namespace {

// ---- cost model ------------------------------------------------------------------------------------------------------
// The Viterbi recurrence keeps one compute unit per clip for (frames of the clip) x 3.1 us (7.3 us at the 22.05 kHz
// geometry, half width 50); the rest of the path costs ~43 ns per frame of the whole chip.  A split pass runs its frame
// stage first (3/4 of the work, not overlapped), then one segment + warm-up + a typical lock-on tail (600 steps), stitch
// and verification (2.5 ms).  Beside the frame stage the sequential kernel walks at 5.2 us per step (1.7 x, measured);
// the frame stage alone on the 192 CUs the partitioned pipeline leaves it takes 256 / 192 as long; a pass fed from host
// memory cannot outrun its copies (46.7 GB/s pageable, measured).  A hybrid pass pays 12 ms of lock-on runs,
// verification and exact walk behind its rounds of segments (each 1.1 x a segment + warm-up).
constexpr double kStepH25 = 3.1e-6, kStepH50 = 7.3e-6;   // s per Viterbi step, one compute unit per clip
constexpr double kFrame = 43e-9;                          // s per frame of the rest of the path, whole chip
constexpr double kSplitFront = 0.75, kHybridFront = 0.8;  // frame stage's share of the work in front of the segments
constexpr double kMaskedFrame = 256.0 / 192.0;            // the frame stage on 192 of 256 CUs
constexpr double kPageableBps = 46.7e9;                   // host -> device copy rate of pageable memory
constexpr double kSplitTail = 2.5e-3, kHybridTail = 12e-3;   // s behind a split pass's / a hybrid pass's segments
constexpr int kLockOnSteps = 600;                         // typical lock-on tail of a speculative run
constexpr double kStepBesideFrame = 1.7;                  // sequential step beside the frame stage, in steps alone
constexpr double kHybridRound = 1.1;                      // a round of hybrid segments, in segment + warm-up times
constexpr double kSplitPays = 0.8, kHybridPays = 0.9;     // planned: split / hybrid estimate below this share of sequential
constexpr double kClockPays = 0.92;                       // measured: frame stage + Viterbi below this share of sequential
constexpr double kRedoShare = 0.25;                       // redo of the flagged clips above this share of sequential: cool down

double step_time(int half_width) { return half_width == 25 ? kStepH25 : kStepH50; }

// fixed schedule shapes (were environment knobs; measured)
constexpr int64_t kChunkStart = 512;      // first time chunk of the growing ramp
constexpr int kChunkGrowthPct = 125;      // later ones grow by this percentage up to time_chunk
constexpr int kRampK = 4;                 // first chunks alternating over two frame streams
constexpr int64_t kBalancedEnds = 64;     // first chunk of a balanced single-launch pass, doubling up to the chunk size

long env_long(const char *name, bool &set) {
    const char *e = std::getenv(name);
    set = e != nullptr;
    return e ? std::strtol(e, nullptr, 10) : 0;
}

}  // namespace

void PlanKnobs::read_env() {
    bool set = false;
    long v = env_long("AEGIS_TIME_CHUNK", set);
    if (set && v >= 64 && v % kViterbiChunk == 0) time_chunk = v;
    v = env_long("AEGIS_TIME_SPLIT", set);
    if (set && v >= 0) split_seglen = v / kViterbiChunk * kViterbiChunk;
    if (const char *e = std::getenv("AEGIS_SPLIT_HYBRID")) split_hybrid = e[0] == '0' ? 0 : 1;
    v = env_long("AEGIS_HYBRID_ROUNDS", set);
    if (set && v >= 1 && v <= 8) hybrid_rounds = (int)v;
    v = env_long("AEGIS_HYBRID_MIN_SEG", set);
    if (set && v >= 64 && v <= 65536) hybrid_min_seg = (int)(v / kViterbiChunk * kViterbiChunk);
    v = env_long("AEGIS_HYBRID_PCT", set);
    if (set && v >= 5 && v <= 200) hybrid_pct = (int)v;
    v = env_long("AEGIS_SPLIT_SEGMENT_ROUNDS", set);
    if (set && v >= 1 && v <= 8) split_rounds_of_segments = (int)v;
    v = env_long("AEGIS_SPLIT_WARMUP", set);
    if (set && v >= 0) split_warmup = (int)(v / kViterbiChunk * kViterbiChunk);
    v = env_long("AEGIS_BALANCED_CHUNK", set);
    if (set && v >= 0 && v % kViterbiChunk == 0) balanced_chunk = v;
    if (const char *e = std::getenv("AEGIS_DENSE")) dense_mode = e[0] == '0' ? 0 : 1;
    if (const char *e = std::getenv("AEGIS_PROPORTIONAL_CHUNKS")) proportional_chunks = e[0] != '0';
    v = env_long("AEGIS_FEED_CHUNK", set);
    if (set && v >= kViterbiChunk && v % kViterbiChunk == 0) feed_chunk = v;
    v = env_long("AEGIS_BALANCED_MIN", set);
    if (set && v >= 1) balanced_min = (int)v;
    if (const char *e = std::getenv("AEGIS_VITERBI_PERSISTENT")) persistent_wanted = std::atoi(e) != 0;
    if (const char *e = std::getenv("AEGIS_CU_SPLIT")) split_limit = std::atoi(e);
}

bool split_allowed(const PlanInput &in) {
    return in.py && !in.caller_stream && in.sync && in.knobs.split_seglen != 0 && in.split_applies;
}

bool masked_streams_fit(const PlanKnobs &k, int n_cus, int n_clips) {
    // the masks are laid out for the 256 CUs of an un-partitioned MI355X; 65..128 clips: a 128 / 128 partition starves
    // the frame stage (170.8 vs 120.9 ms at 128 clips), only reachable through AEGIS_CU_SPLIT
    return n_clips <= k.split_limit && k.split_limit > 0 && n_cus == 256 && n_clips <= 128;
}

bool split_clock_pays(const CallPlan &c, double viterbi_ms) {
    return !(c.t_front + 1e-3 * viterbi_ms > kClockPays * c.t_seq);
}

bool split_redo_pays(const PassPlan &p, int64_t redo_frames, int half_width) {
    return !((double)redo_frames * step_time(half_width) > kRedoShare * p.t_seq);
}

namespace {

struct Planner {
    const PlanInput &in;
    const PlanKnobs &kn;
    std::vector<int64_t> frames;
    const double step;

    explicit Planner(const PlanInput &i) : in(i), kn(i.knobs), step(step_time(i.half_width)) {}

    int64_t clip_samples(int ci) const { return in.sample_offsets[ci + 1] - in.sample_offsets[ci]; }

    // ---- time-split planning (viterbi.hip "Time-split Viterbi") ------------------------------------------------------
    // A pass whose longest clip outlasts the work of the whole pass cuts its clips into segments that run concurrently
    // (blocking calls on the handle's own stream only: the clips that cannot be certified are redone after the pass).
    // The segment length for a set of clips, 0 = stay sequential.  want_hybrid: the pass pays only in the hybrid form (no
    // split pass if that cannot be set up).
    int64_t plan_split(const int *clips_of_pass, int nc, int64_t fp, int64_t maxF, bool &automatic, bool &want_hybrid) const {
        automatic = false; want_hybrid = false;
        if (!split_allowed(in) || nc >= 256) return 0;
        if (kn.split_seglen > 0) return kn.split_seglen;
        if (in.cooling) return 0;
        // automatic: when the estimate says so.  Sequential pass: the longest clip's recurrence, or the pass's whole work if
        // that is more (they overlap); split pass: the frame stage first, then one segment + warm-up + a typical lock-on
        // tail, stitch and verification.
        const double work = (double)fp * kFrame;
        const int seg_budget = std::max(1, in.n_cus) * kn.split_rounds_of_segments;
        int64_t sl = std::max<int64_t>(768, ((fp - nc) / seg_budget + kViterbiChunk - 1) / kViterbiChunk * kViterbiChunk);
        // whole rounds of workgroups: a 257th segment would run alone after the other 256
        for (int guard = 0; guard < 64; ++guard) {
            int64_t ns = 0;
            for (int i = 0; i < nc; ++i) ns += std::max<int64_t>(1, (frames[clips_of_pass[i]] - 1 + sl - 1) / sl);
            if (ns <= seg_budget) break;
            sl = (sl + sl / 32 + kViterbiChunk) / kViterbiChunk * kViterbiChunk;
        }
        const double t_seq = std::max((double)maxF * step, work);
        const double t_split = kSplitFront * work + (double)(sl + kn.split_warmup + kLockOnSteps) * step + kSplitTail;
        if (t_split < kSplitPays * t_seq) { automatic = true; return sl; }
        // Passes of 65 .. 255 clips that the rule above leaves alone: too much work for a frame stage IN FRONT of the segments
        // to pay, but their frame stage is through long before their longest clip (128 ragged clips, a rank of four: frame stage
        // 71 ms, last Viterbi launch 118 ms -- one in eight compute units busy in between).  The hybrid form costs no front:
        // the sequential launches run under the frame stage as they do today (5.2 us per step beside it, measured), and what the
        // longest clip has left when the frame stage ends is cut into segments.  Estimate: frame stage, then one segment +
        // warm-up per round and 12 ms of lock-on runs, verification and exact walk -- against the frame stage plus the steps
        // the longest clip still has to walk alone.
        if (kn.split_hybrid != 0 && nc > kn.split_limit && !in.feed) {
            const double front = kHybridFront * work, s_est = front / (kStepBesideFrame * step);
            const double t_seq2 = std::max(t_seq, front + std::max(0.0, (double)maxF - s_est) * step);
            const double t_hyb = front + (double)kn.hybrid_rounds * (double)(kn.hybrid_min_seg + kn.split_warmup) * kHybridRound * step + kHybridTail;
            if ((double)maxF > s_est + 4096 && t_hyb < kHybridPays * t_seq2) { automatic = true; want_hybrid = true; return kn.hybrid_min_seg; }
        }
        return 0;
    }

    void plan_pass(PassPlan &m, const int *pc, int nc, int64_t fp, const std::vector<int64_t> &out_first) const;
};

void Planner::plan_pass(PassPlan &m, const int *pc, int nc, int64_t fp, const std::vector<int64_t> &out_first) const {
    const bool py = in.py, feed = in.feed;
    m.clips.assign(pc, pc + nc);
    m.fp = fp;
    m.sample_off.resize(nc); m.sample_len.resize(nc); m.out_off.resize(nc);
    m.frame_off.resize(nc + 1); m.chunk_off.resize(nc + 1);
    m.frame_off[0] = 0; m.chunk_off[0] = 0;
    int64_t maxF = 0;
    for (int i = 0; i < nc; ++i) {
        const int ci = pc[i];
        m.sample_off[i] = in.sample_offsets[ci];
        m.sample_len[i] = clip_samples(ci);
        m.out_off[i] = out_first[ci];
        m.frame_off[i + 1] = m.frame_off[i] + frames[ci];
        m.chunk_off[i + 1] = m.chunk_off[i] + (frames[ci] - 1 + kViterbiChunk - 1) / kViterbiChunk;
        maxF = std::max(maxF, frames[ci]);
    }
    m.maxF = maxF;
    m.order.resize(nc);
    std::iota(m.order.begin(), m.order.end(), 0);     // already longest first
    m.t_seq = std::max((double)maxF * step, (double)fp * kFrame);

    // ---- time chunks of the pipeline ---------------------------------------------------------------
    // The Viterbi recurrence is sequential in time and occupies one compute unit per clip; the frame-stage kernels
    // are wide.  A pass is therefore cut into time chunks: chunk k's frame stage runs on the frame streams while
    // chunk k-1's Viterbi runs on the Viterbi stream, carrying its column of values exactly (vstate) across
    // launches.  Boundaries: frame 0, then 1 + (multiple of kViterbiChunk) so that every launch starts on a
    // back-pointer-map boundary.  Chunks start at a quarter of time_chunk and grow by 1.25x (the frame stage is
    // faster than the Viterbi per column, so the Viterbi stream never waits after the first chunk).
    //
    // Balanced passes: on the CU-partitioned streams (split_streams) a pass of 64 clips keeps the frame stage's 192
    // CUs as long per column as the Viterbi keeps its 64 (3.1 us each), so neither may wait for the other: chunks
    // of one small size (growing chunks make the Viterbi wait a quarter of each), alternating over the two frame
    // streams so that one chunk's FFT kernel overlaps the previous chunk's latency-bound observation kernel, and ONE
    // Viterbi launch that waits for a flag per chunk (64 clips x 180 s: 59.5 -> 50.8 ms).  With fewer clips the pass is
    // Viterbi-bound and the gain is the launches and the head (48 clips: 52.0 -> 50.2 ms, 16: 50.2 -> 50.0, 8: 49.5
    // -> 49.8), hence the lower limit; unpartitioned passes lose with small chunks.
    bool split_auto = false, want_hybrid = false;
    int64_t seglen = py ? plan_split(pc, nc, fp, maxF, split_auto, want_hybrid) : 0;
    bool tsplit = seglen > 0;
    // hybrid (see split_hybrid): S = the step the sequential kernel reaches while the frame stage runs, on a chunk boundary of
    // the schedule the pass would take anyway -- up to split_limit clips the balanced one on the CU-partitioned streams (ONE
    // launch of the sequential kernel), above it the ramp of growing chunks on the un-partitioned streams (a launch per
    // chunk, 5.2 us per step beside the frame stage); worth it when S is at least a couple of segments' worth of steps.
    // hyb_cb: the pass's chunk boundaries, S + 1 among them; behind S four large chunks (nothing waits for them one by one).
    int64_t hyb_S = 0, hyb_chunk = 0;
    bool hyb_part = false;
    std::vector<int64_t> hyb_cb;
    if (tsplit && kn.split_hybrid != 0 && (split_auto || kn.split_hybrid == 1) && in.n_cus == 256) {
        hyb_part = nc <= kn.split_limit && kn.split_limit > 0 && kn.balanced_chunk > 0 && in.masked_streams(nc);
        double front = hyb_part ? kSplitFront * (double)fp * kFrame * kMaskedFrame : kHybridFront * (double)fp * kFrame;
        if (feed) {       // a pass fed from host memory: its frame stage cannot outrun the copies
            int64_t samples = 0;
            for (int i = 0; i < nc; ++i) samples += clip_samples(pc[i]);
            front = std::max(front, (double)samples * 4.0 / kPageableBps);
        }
        const int64_t target = (int64_t)((double)kn.hybrid_pct / 100.0 * front / (hyb_part ? step : kStepBesideFrame * step));
        std::vector<int64_t> bs{0};
        if (hyb_part) {
            // (one launch of the sequential kernel waiting for a flag per chunk, as in balanced passes: half the chunk size)
            // (fed from host memory: the feed's chunk size and a launch per chunk, as balanced passes of that kind take)
            hyb_chunk = std::max<int64_t>(kViterbiChunk, (feed ? kn.feed_chunk : (in.persistent && in.sync ? kn.balanced_chunk / 2 : kn.balanced_chunk)) * 64 / nc / kViterbiChunk * kViterbiChunk);
            for (int64_t b = 1 + std::max<int64_t>(kViterbiChunk, hyb_chunk - kViterbiChunk); b < maxF; b += hyb_chunk) bs.push_back(b);
        } else {
            int64_t stp = std::max<int64_t>(kViterbiChunk, kChunkStart / kViterbiChunk * kViterbiChunk);
            for (int64_t b = 1 + stp; b < maxF;) {
                bs.push_back(b);
                stp = std::min<int64_t>(kn.time_chunk, (stp * kChunkGrowthPct / 100 + kViterbiChunk - 1) / kViterbiChunk * kViterbiChunk);
                b += stp;
            }
        }
        if (feed && !hyb_part) bs.resize(1);       // (host-fed passes: the partitioned form only)
        size_t best = 0;       // the boundary nearest the target
        for (size_t i = 1; i < bs.size(); ++i)
            if (std::llabs(bs[i] - 1 - target) < std::llabs(bs[best] - 1 - target)) best = i;
        const int64_t S0 = best > 0 ? bs[best] - 1 : 0;
        if (target >= 2048 && S0 >= 1024 && S0 + 4 * kViterbiChunk < maxF - 1) {
            hyb_S = S0;
            if (hyb_part) {
                hyb_cb.assign(bs.begin(), bs.begin() + (long)best + 1);
                const int64_t big = std::max<int64_t>(4 * kViterbiChunk, ((maxF - hyb_S - 1) / 4 + kViterbiChunk - 1) / kViterbiChunk * kViterbiChunk);
                for (int64_t b = hyb_S + 1 + big; b + big / 2 < maxF; b += big) hyb_cb.push_back(b);
            } else {
                // (un-partitioned: the sequential launches share the compute units with the frame stage, and four large chunks
                // queued in front of them held them back -- at step 7.8 k instead of 13.4 k when the frame stage was through)
                hyb_cb = bs;
                while (hyb_cb.size() > 1 && hyb_cb.back() + kn.time_chunk / 2 >= maxF && hyb_cb.back() > hyb_S + 1) hyb_cb.pop_back();
            }
        }
    }
    if (want_hybrid && hyb_S == 0) { seglen = 0; split_auto = false; tsplit = false; }      // (planned for the hybrid form only)
    const bool hybrid = hyb_S > 0;
    if (hybrid && split_auto) {       // the steps left behind S, one round of segments on the whole chip
        int64_t left = 0;
        for (int i = 0; i < nc; ++i) left += std::max<int64_t>(0, frames[pc[i]] - 1 - hyb_S);
        // (whole rounds of workgroups on the 192 compute units the frame stage leaves: the speculative runs start while the
        // sequential kernel still holds its 64)
        const int64_t budget = (int64_t)(hyb_part ? 192 : in.n_cus) * kn.hybrid_rounds;
        seglen = std::max<int64_t>(kn.hybrid_min_seg, (left / budget + kViterbiChunk) / kViterbiChunk * kViterbiChunk);
        for (int guard = 0; guard < 64; ++guard) {       // (ceil per clip: lengthen until the segments fit)
            int64_t ns = 0;
            for (int i = 0; i < nc; ++i) { const int64_t rest = frames[pc[i]] - 1 - hyb_S; if (rest > 0) ns += (rest + seglen - 1) / seglen; }
            if (ns <= budget) break;
            seglen = (seglen + seglen / 32 + kViterbiChunk) / kViterbiChunk * kViterbiChunk;
        }
    }
    int n_seg = 0, n_lock = 0;
    if (tsplit) {
        const int L = kn.split_warmup;
        std::vector<int64_t> sf0, sch0;
        std::vector<int32_t> sT, sst, sprev, sclip, cseg0(nc + 1, 0);
        for (int i = 0; i < nc; ++i) {
            const int64_t Fc = frames[pc[i]], steps = Fc - 1;
            if (hybrid) {
                // first segment = the sequential run to step S (a clip that ends by then: all of it, decoded by that kernel, and a
                // one-frame placeholder here), then ceil((steps - S) / seglen) segments of equal length behind S
                cseg0[i] = n_seg;
                const bool more = steps > hyb_S;
                sf0.push_back(m.frame_off[i]); sch0.push_back(m.chunk_off[i]);
                sT.push_back(more ? (int32_t)(hyb_S + 1) : 1); sst.push_back(0); sprev.push_back(-1); sclip.push_back(i);
                ++n_seg;
                if (!more) continue;
                const int64_t rest = steps - hyb_S;
                const int ns = (int)std::max<int64_t>(1, (rest + seglen - 1) / seglen);
                int64_t mprev = hyb_S;
                for (int k = 0; k < ns; ++k) {
                    const int64_t mk = k == 0 ? hyb_S : std::max<int64_t>(mprev + kViterbiChunk, hyb_S + (rest * k / ns) / kViterbiChunk * kViterbiChunk);
                    const int64_t mnext = k == ns - 1 ? Fc - 1 : std::max<int64_t>(mk + kViterbiChunk, hyb_S + (rest * (k + 1) / ns) / kViterbiChunk * kViterbiChunk);
                    const int64_t wk = std::max<int64_t>(0, mk - L);
                    sf0.push_back(m.frame_off[i] + wk);
                    sch0.push_back(m.chunk_off[i] + wk / kViterbiChunk);
                    sT.push_back((int32_t)(mnext - wk + 1));
                    sst.push_back((int32_t)(mk - wk));
                    sprev.push_back(n_seg - 1);
                    sclip.push_back(i);
                    mprev = mk;
                    ++n_seg;
                }
                continue;
            }
            // (ceil: no segment longer than seglen -- the launch lasts as long as its longest segment; with rounding a clip of
            // 1.49 segment lengths ran as ONE segment and set the pace of the whole launch)
            const int ns = (int)std::max<int64_t>(1, (steps + seglen - 1) / seglen);
            cseg0[i] = n_seg;
            int64_t mprev = 0;
            for (int k = 0; k < ns; ++k) {
                // boundaries on back-pointer chunk boundaries (multiples of 16); the last segment ends at the last frame
                const int64_t mk = k == 0 ? 0 : std::max<int64_t>(mprev + kViterbiChunk, (steps * k / ns) / kViterbiChunk * kViterbiChunk);
                const int64_t mnext = k == ns - 1 ? Fc - 1 : std::max<int64_t>(mk + kViterbiChunk, (steps * (k + 1) / ns) / kViterbiChunk * kViterbiChunk);
                const int64_t wk = k == 0 ? 0 : std::max<int64_t>(0, mk - L);
                sf0.push_back(m.frame_off[i] + wk);
                sch0.push_back(m.chunk_off[i] + wk / kViterbiChunk);
                sT.push_back((int32_t)(mnext - wk + 1));
                sst.push_back((int32_t)(mk - wk));
                sprev.push_back(k == 0 ? -1 : n_seg - 1);
                sclip.push_back(i);
                mprev = mk;
                ++n_seg;
            }
        }
        cseg0[nc] = n_seg;
        m.seg64 = sf0; m.seg64.insert(m.seg64.end(), sch0.begin(), sch0.end());
        // vf_off: the frames behind every split clip's first boundary (what the verification kernel's grid covers)
        {
            int64_t acc = 0;
            for (int i = 0; i <= nc; ++i) {
                m.seg64.push_back(acc);
                if (i < nc && cseg0[i + 1] - cseg0[i] >= 2) {
                    const int k1 = cseg0[i] + 1;
                    const int64_t fx = sf0[k1] + sst[k1];            // workspace frame of the first boundary
                    acc += m.frame_off[i] + frames[pc[i]] - 1 - fx;
                }
            }
        }
        m.seg32.clear();
        for (auto *v : {&sT, &sst, &sprev, &sclip, &cseg0}) m.seg32.insert(m.seg32.end(), v->begin(), v->end());
        // seg_order: the speculative runs (n_seg entries reserved; a hybrid pass lists only the segments behind the first ones)
        for (int k = 0; k < n_seg; ++k) if (!hybrid || sprev[k] >= 0) m.seg32.push_back(k);
        if (hybrid) for (int k = 0; k < n_seg; ++k) if (sprev[k] < 0) m.seg32.push_back(k);       // (padding: keeps the layout)
        for (int k = 0; k < n_seg; ++k) if (sprev[k] >= 0) { m.seg32.push_back(k); ++n_lock; }      // lock_order
        // what the executor sizes, clears and binds by: a table packed in another shape must never reach it (the entry's
        // frame turns this into an error code and a message, in every build)
        const SegLayout lay(n_seg, nc, n_lock);
        if (m.seg64.size() != lay.n64 || m.seg32.size() != lay.n32)
            throw std::logic_error("plan: the packed time-split tables (seg64, seg32) do not have SegLayout's totals");
        m.tube_cap = (int)std::max<int64_t>(4096, fp / 128);
    }
    const bool balanced = !tsplit && py && !in.caller_stream && kn.balanced_chunk > 0 && nc >= kn.balanced_min && in.n_cus == 256 &&
                          kn.split_limit > 0 && nc <= kn.split_limit && nc <= 128;
    // (a persistent Viterbi launch pays nothing per chunk: half the chunk size, 54.3 -> 52.0 ms).  The size is stated for
    // 64 clips and scaled so that a chunk's observation kernel is ONE full round of workgroups on the frame stage's
    // 192 CUs (2 x 192 workgroups of 32 frames = 12 288 frames = 192 steps x 64 clips) and its frame kernel two:
    // 224 steps instead of 192 leave a sixth of a second round behind (54.1 instead of 50.6 ms).
    // A pass fed from host memory (aegis_analyze_batch) copies each chunk's samples from the thread that launches its
    // kernels, and a pageable copy returns only when the bytes have left the caller's buffer: chunks of 192 steps are
    // 5 000 copies of 0.4 MB per 64 x 180 s, and the single launch spins on flags that thread is late to set (64 x
    // 180 s: 108 ms; a launch per chunk: 70).  Such a pass takes 1 024-step chunks (2 MB per clip and copy) and a launch
    // per chunk: 57 ms, against 63 on the unbalanced schedule it used before and 49.4 device-resident.
    const bool may_persist = balanced && !feed && in.persistent && in.sync && in.band_applies;
    int64_t kTimeChunk = kn.time_chunk;
    if (balanced) {
        const int64_t at64 = feed ? kn.feed_chunk : (may_persist ? kn.balanced_chunk / 2 : kn.balanced_chunk);
        kTimeChunk = std::max<int64_t>(kViterbiChunk, at64 * 64 / nc / kViterbiChunk * kViterbiChunk);
    }
    if (hybrid && hyb_part) kTimeChunk = hyb_chunk;
    std::vector<int64_t> &cb = m.cb;
    cb.assign(1, 0);
    if (hybrid) {
        // chunks of the schedule's own size while the sequential kernel follows (to step S: the Viterbi sets the pace), then the
        // rest of the frame stage in a few large ones: a chunk's two kernels take ~0.5 ms however few frames it holds, and
        // behind S nothing waits for them chunk by chunk (148 chunks of 192 steps: the frame stage alone took 66 ms)
        cb = hyb_cb;
    } else if (balanced && maxF > 2 * kTimeChunk) {
        // (chunk 0 holds frame 0 besides its steps: one back-pointer block less keeps it inside the round too)
        if (may_persist && kBalancedEnds > 0 && maxF > 8 * kTimeChunk) {
            // shorter chunks at both ends (the Viterbi starts behind chunk 0 and finishes a chunk after the frame
            // stage): ends, 2 ends, ... doubling up to the chunk size, mirrored at the end (50.8 -> 50.4 ms)
            std::vector<int64_t> ramp;
            for (int64_t sz = std::max<int64_t>(kViterbiChunk, kBalancedEnds / kViterbiChunk * kViterbiChunk); sz < kTimeChunk; sz *= 2) ramp.push_back(sz);
            int64_t ramp_sum = 0;
            for (int64_t v : ramp) ramp_sum += v;
            int64_t b = 1;
            for (int64_t v : ramp) { b += v; cb.push_back(b); }
            const int64_t mid_end = maxF - ramp_sum;
            for (b += kTimeChunk; b + kTimeChunk / 2 < mid_end; b += kTimeChunk) cb.push_back(b);
            b = cb.back() + ((mid_end - cb.back()) / kViterbiChunk * kViterbiChunk);
            if (b > cb.back()) cb.push_back(b);
            for (size_t i = ramp.size(); i-- > 1;) { b += ramp[i]; if (b < maxF) cb.push_back(b); }
        } else
        for (int64_t b = 1 + std::max<int64_t>(kViterbiChunk, kTimeChunk - kViterbiChunk); b + kTimeChunk / 2 < maxF; b += kTimeChunk) cb.push_back(b);
    } else if (py && tsplit && feed) {
        // a time-split pass fed from host memory: its segments need every frame's observations, but its frame stage need not
        // wait for the last sample -- chunks of the feed size, each chunk's copy under the frame stage of the chunk before
        // (64 x 180 s at 22 050 Hz: copy 20 ms + frame stage 12 ms + segments 22 ms in a row before)
        const int64_t fc = std::max<int64_t>(4 * kViterbiChunk, kn.feed_chunk * 64 / nc / kViterbiChunk * kViterbiChunk);
        for (int64_t b = 1 + fc - kViterbiChunk; b + fc / 2 < maxF; b += fc) cb.push_back(b);
    } else if (py && !tsplit && maxF > kTimeChunk + kTimeChunk / 2) {      // (a device-resident time-split pass: the whole frame stage, then all segments at once)
        int64_t step = std::max<int64_t>(kViterbiChunk, kChunkStart / kViterbiChunk * kViterbiChunk);
        cb.push_back(1 + step);
        while (cb.back() + kTimeChunk + kTimeChunk / 2 < maxF) {
            step = std::min<int64_t>(kTimeChunk, (step * kChunkGrowthPct / 100 + kViterbiChunk - 1) / kViterbiChunk * kViterbiChunk);
            cb.push_back(cb.back() + step);
        }
    }
    cb.push_back(maxF);
    const int nk = (int)cb.size() - 1;
    // Ragged passes: every clip is cut into the SAME nk chunks, each a share of the clip proportional to the chunk's
    // share of the longest clip (boundaries stay on 1 + multiples of kViterbiChunk).  With one time axis for all clips
    // the short clips are done after a few chunks and the last launches hold only the long clips' Viterbi workgroups
    // on an otherwise idle chip (512-clip folder: the last 36 of 363 ms); with proportional chunks every launch
    // carries every clip and all of them finish with the last chunk.  The results do not depend on the cut.
    // Throughput passes (a Viterbi workgroup for every CU and more): the register-capped Viterbi build and four-wave
    // observation workgroups (viterbi.hip); AEGIS_DENSE=0 turns it off, =1 forces it for every unbalanced pass (tests).
    const bool dense = py && !balanced && !tsplit && in.band_applies && in.half_width == 25 &&
                       (kn.dense_mode == 1 || (kn.dense_mode < 0 && nc >= 256));
    bool proportional = false;
    // (not for a pass fed from host memory: it is bound by the pageable copies, and a short clip's proportional chunk is a
    // copy of a few hundred KB -- 512-clip folder, host-inclusive: 496 ms against 466 on one time axis)
    if (py && !balanced && !feed && !tsplit && nk > 2 && kn.proportional_chunks) {
        int64_t minF = maxF;
        for (int i = 0; i < nc; ++i) minF = std::min(minF, frames[pc[i]]);
        proportional = 4 * minF < 3 * maxF;
    }
    // tb[k * nc + i]: first frame of chunk k of the pass's clip i (k = nk: its frame count)
    m.clip_tb.clear();
    if (proportional) {
        m.clip_tb.assign((size_t)(nk + 1) * nc, 0);
        for (int i = 0; i < nc; ++i) {
            const int64_t Fc = frames[pc[i]];
            int64_t prev = 0;
            for (int k = 1; k <= nk; ++k) {
                int64_t b = Fc;
                if (k < nk) {
                    const int64_t want = 1 + (int64_t)((double)(cb[k] - 1) * (double)Fc / (double)maxF) / kViterbiChunk * kViterbiChunk;
                    b = std::min(Fc, std::max(want, prev == 0 ? 1 + kViterbiChunk : prev + kViterbiChunk));
                }
                m.clip_tb[(size_t)k * nc + i] = b;
                prev = b;
            }
        }
    }
    m.proportional = proportional;
    m.sel_off.assign((size_t)nk * (nc + 1), 0);
    for (int k = 0; k < nk; ++k)
        for (int i = 0; i < nc; ++i) {
            const int64_t cnt = std::max<int64_t>(0, m.clip_hi(k, i) - m.clip_lo(k, i));
            m.sel_off[(size_t)k * (nc + 1) + i + 1] = m.sel_off[(size_t)k * (nc + 1) + i] + cnt;
        }

    // ---- streams -----------------------------------------------------------------------------------
    // CU-partitioned streams while the batch leaves compute units free (see split_streams); otherwise the caller's
    // stream carries the frame stage and the handle's second stream the Viterbi.
    const bool ss = (py && nk > 1 && !in.caller_stream && (!tsplit || (hybrid && hyb_part))) && in.masked_streams(nc);      // (segments want every CU)
    m.fa = ss ? Lane::masked_frame_a : Lane::main;
    m.fb = ss ? Lane::masked_frame_b : Lane::frame2;
    m.sv = ss ? Lane::masked_viterbi : ((py && (nk > 1 || tsplit)) ? Lane::viterbi2 : m.fa);      // (a split pass: the next pass's frame stage runs under its Viterbi kernels)
    // Large batches are frame-stage bound (every CU carries a Viterbi workgroup): alternating the chunks over two
    // streams lets chunk k+1's FFTs overlap chunk k's latency-bound observation kernel.  Small batches are
    // Viterbi-bound and want each chunk's frame stage finished as early as possible: one stream, except for the
    // first four (short) chunks, whose kernels are too small to fill the chip on their own.
    m.two_fs = py && nk > 2 && nc >= 128 && (!tsplit || hybrid);      // (a chunked split pass fed from host memory keeps one frame stream: its one Viterbi launch waits for the last chunk's event only)
    m.ramp_k = (py && nk > 2 && !m.two_fs && (!tsplit || hybrid)) ? ((balanced || (hybrid && hyb_part)) ? nk : kRampK) : 0;
    // a hybrid pass ends on an unmasked stream (its segments want every CU, the partitioned pipeline's Viterbi stream has 64);
    // its speculative runs go behind the frame stage, beside the sequential kernel's last chunks: a stream of their own on
    // the partitioned set, the frame stream itself otherwise
    m.sd = hybrid ? Lane::viterbi2 : Lane::none;
    m.sa = hybrid ? (hyb_part ? Lane::frame2 : m.fa) : Lane::none;
    m.use_fb = m.two_fs || m.ramp_k > 0;
    // Balanced passes launch the Viterbi ONCE: the kernel waits for a flag per time chunk, stored behind the chunk's
    // observation kernel, instead of being launched per chunk (40 launches of 45 us each at 64 clips x 180 s, and the
    // kernel's prologue each time).  It needs the frame stage to run beside it, which the CU partition guarantees.
    const bool persistent = (may_persist || (hybrid && !feed && in.persistent && in.sync)) && ss && nk > 1;
    if (persistent) m.chunk_lo.assign(cb.begin(), cb.end() - 1);

    m.tsplit = tsplit; m.split_auto = split_auto; m.want_hybrid = want_hybrid; m.hybrid = hybrid; m.hyb_part = hyb_part;
    m.hyb_S = hyb_S; m.seglen = seglen; m.n_seg = n_seg; m.n_lock = n_lock;
    m.balanced = balanced; m.may_persist = may_persist; m.persistent = persistent; m.dense = dense;
}

}  // namespace

CallPlan plan_call(const PlanInput &in) {
    Planner P(in);
    const int n_clips = (int)in.sample_offsets.size() - 1;
    CallPlan c;
    // per-clip frame counts and each clip's first frame in the output arrays (caller's clip order)
    P.frames.resize(n_clips);
    std::vector<int64_t> out_first(n_clips);
    for (int i = 0; i < n_clips; ++i) {
        P.frames[i] = 1 + P.clip_samples(i) / in.hop;
        out_first[i] = c.total_frames;
        c.total_frames += P.frames[i];
    }
    // Clips go through the passes LONGEST FIRST (outputs keep the caller's order through out_off): a pass lasts as long
    // as the Viterbi of its longest clip, so clips of similar length share a pass and no compute unit idles behind a
    // 330 s clip that happens to sit next to 30 s ones.  Passes alternate between two workspaces, so the frame stage of
    // pass k+1 runs under the Viterbi of pass k.
    std::vector<int> by_len(n_clips);
    std::iota(by_len.begin(), by_len.end(), 0);
    std::stable_sort(by_len.begin(), by_len.end(), [&](int a, int b) { return P.frames[a] > P.frames[b]; });
    if (n_clips == 0) return c;
    c.t_seq = std::max((double)P.frames[by_len[0]] * P.step, (double)c.total_frames * kFrame);
    bool split_started = false;
    for (int first = 0; first < n_clips;) {
        int last = first;
        int64_t fp = 0;
        while (last < n_clips && fp + P.frames[by_len[last]] <= in.max_frames_per_pass) { fp += P.frames[by_len[last]]; ++last; }
        c.passes.emplace_back();
        PassPlan &m = c.passes.back();
        P.plan_pass(m, by_len.data() + first, last - first, fp, out_first);
        if (m.tsplit && m.split_auto && !split_started) {
            // the clock check measures from this call's first automatic split pass's Viterbi kernels: what precedes them is
            // the frame stage (in front of the segments; on 192 CUs / beside 65 .. 255 Viterbi workgroups in a hybrid pass);
            // for a pass planned in the hybrid form only, the sequential estimate that rule used (frame stage + the
            // longest clip's rest)
            split_started = true;
            if (!m.hybrid) c.t_front = kSplitFront * (double)fp * kFrame;
            else {
                c.t_front = m.hyb_part ? (double)fp * kFrame : kHybridFront * (double)fp * kFrame;
                if (m.want_hybrid)
                    c.t_seq = std::max(c.t_seq, c.t_front + std::max(0.0, (double)m.maxF - c.t_front / (kStepBesideFrame * P.step)) * P.step);
            }
        }
        first = last;
    }
    return c;
}

}  // namespace aegis
