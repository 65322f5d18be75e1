// Pass planner of the batch entries (aegis_analyze_batch / _device): which clips share a pass, how each pass is cut into
// time chunks or time-split segments, which kernels run and on which stream.  Plain C++: no HIP, testable on the CPU
// (aegis_debug_plan, tests/test_plan.py).  aegis_exec.hip enqueues what it plans.
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <vector>

namespace aegis {

constexpr int kViterbiChunk = 16;   // steps per composed back-pointer map

// Scheduling knobs of a handle: defaults, and what the environment overrides when the handle is created (out-of-range
// values are ignored).
struct PlanKnobs {
    int64_t time_chunk = 2048;          // AEGIS_TIME_CHUNK: Viterbi steps per pipeline chunk (>= 64, multiple of 16)
    int64_t feed_chunk = 1024;          // AEGIS_FEED_CHUNK: chunk size of balanced passes fed from host memory
    int64_t balanced_chunk = 384;       // AEGIS_BALANCED_CHUNK: chunk size of balanced passes (0 = never balanced)
    int balanced_min = 16;              // AEGIS_BALANCED_MIN: fewest clips of a balanced pass
    int dense_mode = -1;                // AEGIS_DENSE: -1 (unset) = passes of >= 256 clips, 0 = never, 1 = every unbalanced pass
    bool proportional_chunks = true;    // AEGIS_PROPORTIONAL_CHUNKS=0: one time axis for the clips of a ragged pass
    int split_limit = 64;               // AEGIS_CU_SPLIT: passes of up to this many clips run partitioned (0 disables)
    bool persistent_wanted = true;      // AEGIS_VITERBI_PERSISTENT: one Viterbi launch per balanced pass (0: one per chunk)
    // time-split passes (viterbi.hip): AEGIS_TIME_SPLIT=<steps per segment> forces them, 0 turns them off, unset = when a
    // pass is bound by the recurrence of its longest clip
    int64_t split_seglen = -1;          // -1: automatic
    // AEGIS_SPLIT_SEGMENT_ROUNDS: segments per compute unit the automatic rule plans for (whole rounds of workgroups).  The
    // speculative runs take the same time in one round of long segments or two rounds of segments half as long (+ the second
    // warm-up), but a lock-on run that never meets its speculative run costs a whole segment and a round of second
    // speculation another: with two rounds of segments six of the folder's eight rank shards run in 77-79 ms instead of
    // 91-99 (and the other two in 68-71 instead of 66); with three the slowest shard takes 76.7 ms instead of 79.5, with
    // four 77.6.
    int split_rounds_of_segments = 3;
    int split_warmup = 256;             // AEGIS_SPLIT_WARMUP: frames a speculative run starts ahead of its boundary (128: lock-on after a median of 104 steps and one run in twenty never; 256: at the first check)
    // Hybrid split passes (AEGIS_SPLIT_HYBRID: unset = automatic split passes, 1 = forced ones as well, 0 = never).  A split
    // pass ran its whole frame stage in front of its segments (they need every frame's observations) with the Viterbi's
    // compute units idle; a hybrid pass runs the balanced pipeline instead -- frame stage
    // on 192 CUs, the SEQUENTIAL kernel chunk by chunk on 64 -- until the frame stage is through, and cuts only what the
    // sequential kernel has not reached by then (steps behind hybrid step S of every clip) into speculative segments: the
    // first segment of every clip is the sequential run itself, as before, only now thousands of steps long and free.
    // AEGIS_HYBRID_PCT: S as a percentage of (frame stage time on 192 CUs) / (time per step); AEGIS_HYBRID_ROUNDS: rounds
    // of speculative segments behind S; AEGIS_HYBRID_MIN_SEG: their shortest length.
    int split_hybrid = -1, hybrid_pct = 100, hybrid_rounds = 3, hybrid_min_seg = 768;

    void read_env();
};

// The streams a pass's kernels go on.  main: the caller's stream, or the handle's own; frame2 / viterbi2: the handle's
// second frame-stage and Viterbi streams; masked_*: the CU-masked set for the pass's clip count (split_streams).
enum class Lane : uint8_t { none, main, frame2, viterbi2, masked_frame_a, masked_frame_b, masked_viterbi };

struct PlanInput {
    std::vector<int64_t> sample_offsets;    // [n_clips + 1], the caller's clip order
    int64_t max_frames_per_pass = 0;
    int n_cus = 0, hop = 512, half_width = 25;
    bool py = true;                         // the pYIN stage runs
    bool feed = false;                      // host-fed entry (aegis_analyze_batch)
    bool caller_stream = false;             // the caller gave a stream
    int sync = 1;
    bool band_applies = false, split_applies = false;   // viterbi_band_applies / viterbi_split_applies
    std::function<bool(int)> masked_streams;            // a CU-masked stream set exists for n clips
    PlanKnobs knobs;
    // adaptive state of the handle
    bool cooling = false;                   // the split cool-down holds this call
    bool persistent = true;                 // single Viterbi launches allowed (false for a while after a give-up)
};

// The Viterbi launch that follows chunk k's observations (PassPlan::viterbi_behind).  The sequential kernel: none, the one
// persistent launch (behind chunk 0), one launch for this chunk.  segments: a plain split pass's one launch, behind its
// last chunk.
enum class ViterbiBehind : uint8_t { none, single_launch, per_chunk, segments };

struct PassPlan {
    std::vector<int> clips;                 // indices into the caller's arrays, longest first
    int64_t fp = 0, maxF = 0;               // frames of the pass, of its longest clip
    bool tsplit = false, split_auto = false, want_hybrid = false, hybrid = false, hyb_part = false;
    int64_t hyb_S = 0, seglen = 0;
    int n_seg = 0, n_lock = 0, tube_cap = 0;
    bool balanced = false, may_persist = false, persistent = false, dense = false, proportional = false;
    std::vector<int64_t> cb;                // chunk boundaries: cb[k] .. cb[k + 1] is chunk k, cb.back() = maxF
    bool two_fs = false, use_fb = false;
    int ramp_k = 0;
    Lane fa = Lane::none, fb = Lane::none, sv = Lane::none, sd = Lane::none, sa = Lane::none;
    double t_seq = 0.0;                     // the pass's sequential estimate (split_redo_pays)
    // host arrays uploaded to the workspace (kept alive until the stream has consumed them)
    std::vector<int64_t> sample_off, sample_len, out_off, frame_off, chunk_off, sel_off, chunk_lo, clip_tb;
    std::vector<int32_t> order;
    std::vector<int64_t> seg64;             // time-split pass: seg_f0 | seg_ch0 | vf_off
    std::vector<int32_t> seg32;             // seg_T | seg_store | seg_prev | seg_clip | clip_seg0 | seg_order | lock_order

    int nc() const { return (int)clips.size(); }
    int nk() const { return (int)cb.size() - 1; }
    int64_t frames(int i) const { return frame_off[i + 1] - frame_off[i]; }
    // first frame of chunk k of the pass's clip i, and one past its last
    int64_t clip_lo(int k, int i) const { return proportional ? clip_tb[(size_t)k * nc() + i] : std::min(frames(i), cb[k]); }
    int64_t clip_hi(int k, int i) const { return proportional ? clip_tb[(size_t)(k + 1) * nc() + i] : std::min(frames(i), cb[k + 1]); }
    // The chunks the sequential kernel runs: every one, or in a hybrid pass those that begin at or before step S (behind S
    // the segments take over).
    int sequential_chunks() const {
        if (!hybrid) return nk();
        int ks = 0;
        while (ks < nk() && cb[ks] <= hyb_S) ++ks;
        return ks;
    }
    ViterbiBehind viterbi_behind(int k) const {
        if (persistent) return k == 0 ? ViterbiBehind::single_launch : ViterbiBehind::none;      // its first column reads frame 0
        if (tsplit && !hybrid) return k == nk() - 1 ? ViterbiBehind::segments : ViterbiBehind::none;   // they need every frame's observations
        return (!hybrid || cb[k] <= hyb_S) ? ViterbiBehind::per_chunk : ViterbiBehind::none;   // (behind step S the segments take over)
    }
};

struct CallPlan {
    std::vector<PassPlan> passes;
    int64_t total_frames = 0;
    // the clock check of an automatic split call (split_clock_pays): its sequential estimate and the frame stage in front
    // of its first split pass's Viterbi kernels
    double t_seq = 0.0, t_front = 0.0;
};

// The packed tables of a time-split pass, in elements: where each array starts and how many there are.  plan.cpp packs
// seg64 and seg32 in this order, the executor sizes, clears and binds by it.
struct SegLayout {
    // seg64 (int64, from the plan): seg_f0 [n_seg] | seg_ch0 [n_seg] | vf_off [nc + 1]
    size_t f0, ch0, vf_off, n64;
    // seg32 (int32, from the plan): seg_T | seg_store | seg_prev | seg_clip [n_seg each] | clip_seg0 [nc + 1] | seg_order [n_seg] | lock_order [n_lock]
    size_t T, store, prev, clip, clip_seg0, seg_order, lock_order, n32;
    // seg_i32 (int32, device state): seg_kg | seg_lock | seg_end [n_seg each] | clip_first | clip_dirty [nc each]
    size_t kg, lock, end, clip_first, clip_dirty, n_i32;
    SegLayout(size_t n_seg, size_t nc, size_t n_lock)
        : f0(0), ch0(n_seg), vf_off(2 * n_seg), n64(2 * n_seg + nc + 1),
          T(0), store(n_seg), prev(2 * n_seg), clip(3 * n_seg), clip_seg0(4 * n_seg), seg_order(4 * n_seg + nc + 1),
          lock_order(5 * n_seg + nc + 1), n32(5 * n_seg + nc + 1 + n_lock),
          kg(0), lock(n_seg), end(2 * n_seg), clip_first(3 * n_seg), clip_dirty(3 * n_seg + nc), n_i32(3 * n_seg + 2 * nc) {}
};

// What sizes the workspace of one pass: a batch pass (ensure_pass) or a stream, which is one clip of its capacity.
struct PassGeometry {
    int64_t F = 0, S = 0;                   // frames, Viterbi states (2 n_bins)
    int64_t cmap_rows = 0, clips = 1;       // composed chunk maps (the pass's chunks + 1)
    int64_t lag_stride = 0, yin_stride = 0, obs_stride = 0, n_mels = 0;
    bool pyin = true, mel = true;           // the stages that run
    bool debug_stages = false, proportional = false, tsplit = false;
    int64_t nk = 1;                         // time chunks
    int64_t n_seg = 0, tube_cap = 0, tube_record_ints = 0, seg64_size = 0, seg32_size = 0;   // a time-split pass
};
// Bytes of every workspace buffer (0: the pass does not use it).  Growth goes by the request, so these ARE the requests.
struct PassBytes {
    size_t dfn = 0, logobs = 0, logunv = 0, obs_seg = 0, ptr = 0, cmap = 0, bnd = 0, states = 0, melpow = 0, clipmax = 0, rake_raw = 0, vstate = 0;
    size_t sample_off = 0, sample_len = 0, out_off = 0, frame_off = 0, order = 0, chunk_off = 0, sel_off = 0;   // batch geometry
    size_t yin = 0, chunk_lo = 0, chunk_flag = 0, clip_tb = 0;
    size_t seg64 = 0, seg32 = 0, seg_col = 0, seg_map = 0, seg_i32 = 0, colhist = 0, colG = 0, colkg = 0, clip_flag = 0, flag_order = 0,
           tube_buf = 0, tube_at = 0, tube_count = 0;
};
inline PassBytes pass_bytes(const PassGeometry &g) {
    const size_t F = (size_t)g.F, S = (size_t)g.S, nc = (size_t)g.clips, nk = (size_t)g.nk;
    PassBytes b;
    b.sample_off = nc * 8; b.sample_len = nc * 8; b.out_off = nc * 8; b.frame_off = (nc + 1) * 8;
    b.order = nc * 4; b.chunk_off = (nc + 1) * 8; b.sel_off = nk * (nc + 1) * 8;
    if (g.pyin) {
        b.dfn = F * g.lag_stride * 8; if (g.debug_stages) b.yin = F * g.yin_stride * 8;
        b.logobs = F * g.obs_stride * 8; b.logunv = F * 8; b.obs_seg = F * 4;
        b.ptr = F * S * 2; b.cmap = (size_t)g.cmap_rows * S * 2; b.bnd = (size_t)g.cmap_rows * 4;
        b.states = F * 4; b.vstate = nc * S * 8;
        b.chunk_lo = nk * 8; b.chunk_flag = nk * 4;
        if (g.proportional) b.clip_tb = (nk + 1) * nc * 8;
        if (g.tsplit) {
            const size_t n_seg = (size_t)g.n_seg;
            b.seg64 = (size_t)g.seg64_size * 8; b.seg32 = (size_t)g.seg32_size * 4;
            b.seg_col = 2 * n_seg * S * 8; b.seg_map = n_seg * S * 2; b.seg_i32 = SegLayout(n_seg, nc, 0).n_i32 * 4;
            b.colhist = F * S * 8; b.colG = F * 8; b.colkg = F * 4; b.clip_flag = nc * 4; b.flag_order = nc * 4;
            b.tube_buf = (size_t)g.tube_cap * g.tube_record_ints * 4; b.tube_at = F * 4; b.tube_count = 8;
        }
    }
    if (g.mel) { b.melpow = F * g.n_mels * 4; b.clipmax = nc * 4; b.rake_raw = F; }
    return b;
}

bool split_allowed(const PlanInput &in);              // time-split passes may be planned for this call at all
bool masked_streams_fit(const PlanKnobs &k, int n_cus, int n_clips);   // split_streams' conditions on the pass
CallPlan plan_call(const PlanInput &in);
// after an automatic split call: did frame stage + measured Viterbi time come clearly below the sequential estimate?
bool split_clock_pays(const CallPlan &c, double viterbi_ms);
// after a split pass: is the sequential redo of its longest flagged clip (redo_frames) cheap next to the pass?
bool split_redo_pays(const PassPlan &p, int64_t redo_frames, int half_width);

}  // namespace aegis
