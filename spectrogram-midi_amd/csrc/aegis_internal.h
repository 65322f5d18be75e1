// What the host-side files of libaegis_hip.so share: the handle, the stream, owned device buffers and events, the error
// macros, the call scope (StreamScope) that drains the stream on every way out of an entry.  Internal: not installed, not
// included by include/aegis_hip.h.
// An exported entry that locks its handle is ENTRY(h) ... ENTRY_END(h): the frame answers a null handle, takes the lock
// in front of the body's first write to h->err and maps an exception to a code.  A launch that is timed under a
// profiling name is TIMED(h, "name", s, launch): the event pair, the launch, the error check.  A host vector goes to
// its buffer with PUT, n elements come back with FETCH.  Clips of samples are walked by clip_samples and uploaded by
// upload_clips (aegis_onset.hip, next to the frame walks).  aegis_stream.hip follows the same rules: its entries are
// STREAM_ENTRY(st) ... STREAM_ENTRY_END(st), its plain push and its close hold a StreamScope, and the workspace it shares
// with a batch pass is PassBufs, sized by pass_bytes (plan.h) and bound by bind_core.
//   aegis_api.hip     the batch entries (plan input, the host and raw-byte feeds, recovery, the three analyze entries, PCM helpers)
//   aegis_exec.hip    the batch executor: analyze_device_locked runs the passes plan.cpp plans, step by step (check_call,
//                     open_pass, the pass workspace, the chunks, hybrid_segments, close_pass, join_call, the split verdicts)
//   aegis_handle.hip  create / destroy, profiling, the call scope's drain, tables, parameters, aegis_debug_plan / aegis_debug_fetch
//   aegis_stream.hip  aegis_stream_* (graph capture, commit delivery), aegis_debug_stream_set_observations / _stream_fetch
//   aegis_cqt.hip     CQT, chroma, the filter-bank cache, aegis_estimate_tuning, aegis_rake_patterns
//   aegis_trend.hip   aegis_trend, aegis_ghost_rsi
//   aegis_synth.hip   aegis_synth_* (the ADSR soft-synth, one envelope per clip or per note; kernels in adsr.hip, host
//                     preparation in adsr_host.h, the MIDI reader in synth_smf.cpp)
//   aegis_effects.hip aegis_reverb_ir, aegis_effects (the effect chain; kernels in effects.hip)
//   aegis_notefit.hip aegis_note_fit, aegis_compare_audio, aegis_synth_one_note (the per-note optimiser; kernels in
//                     notefit.hip and adsr.hip)
//   aegis_verify.hip  aegis_verify_techniques (the technique verifier; kernels in verify.hip, its renders through
//                     aegis_synth.hip's render_into)
//   aegis_salience.hip aegis_salience, aegis_cqt_salience (harmonic-sum salience and pitch candidates; kernel in
//                     salience.hip, the CQT in front of it through aegis_cqt.hip's cqt_host_locked)
//   aegis_onset.hip   aegis_onset_strength, aegis_onset_detect, aegis_analyze_onsets (onset envelope and onset picking;
//                     kernels in onset.hip, the mel stage in front of them through aegis_api.hip's mel_host_locked); the
//                     offsets walks every per-clip entry shares (frame_offsets, clip_frames, clip_samples) and upload_clips
//   aegis_beat.hip    aegis_tempo, aegis_beat_track, aegis_beat_tables, aegis_analyze_beats (tempogram mean, tempo, beat
//                     tracker; kernels in beat.hip, the mel stage and aegis_onset.hip's envelope stage in front of them)
//   aegis_hpss.hip    aegis_stft, aegis_istft, aegis_hpss (spectrogram, resynthesis, the whole separation), aegis_hpss_masks (running medians along time and bins and the soft masks of median-filter
//                     harmonic / percussive separation; kernels in hpss.hip, the pass planner that cuts long clips here)
//   aegis_dtw.hip     aegis_dtw, aegis_align_chroma (dynamic time warping of feature sequences, and of clips through the
//                     chroma of aegis_cqt.hip's cqt_host_locked; kernels in dtw.hip)
//   aegis_nnls.hip    aegis_activations, aegis_cqt_activations (the non-negative note-template fit of the CQT columns and
//                     the most active notes per frame; kernel in nnls.hip, the CQT in front of it through cqt_host_locked)
//   aegis_pvoc.hip    aegis_pvoc_steps, aegis_phase_vocoder, aegis_time_warp, aegis_resample, aegis_pitch_shift (phase vocoder
//                     along a time map, band-limited resampling; kernels in pvoc.hip, the STFT and the resynthesis
//                     around them hpss.hip's, the pass of whole clips clip_pass.h's, which aegis_hpss.hip shares)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <list>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/aegis_hip.h"
#include "kernels.h"
#include "plan.h"
#include "pcm.h"
#include "cqt.h"
#include "tables.h"
#include "tuning.h"

// A grow-only device block.  It is freed by whoever's list ensure() entered it in (aegis_handle::bufs, aegis_stream::bufs):
// a DevBuf member needs no other mention anywhere to be released.  PassParams and SplitCheck keep raw pointers into the
// blocks across calls, and the lists keep DevBuf addresses: a DevBuf stays a member of its owner and never moves.
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    bool listed = false;
    template <class T> T *as() const { return static_cast<T *>(p); }
};

// The pYIN / mel workspace of one pass, which a batch workspace (aegis_handle::Work) and a stream both own: sized from
// pass_bytes (plan.h), bound into PassParams by bind_core.
struct PassBufs {
    DevBuf dfn, logobs, logunv, obs_seg, ptr, cmap, bnd, states, melpow, clipmax, rake_raw, vstate;
};

// The slots of aegis_handle::sync_events as a batch call uses them: call start, pass done (by workspace parity), frame_b
// joined, frame_a final, pass metadata uploaded, then one per time chunk (reserve_chunk_events grows the list; EV_FIXED
// exist from aegis_create on).  Between batch calls aegis_trend.hip forks and joins its streams on the first four.
enum { EV_START = 0, EV_DONE0 = 1, EV_DONE1 = 2, EV_FB = 3, EV_FA = 4, EV_META = 5, EV_CHUNK0 = 6, EV_FIXED = 8 };

struct aegis_handle {
    aegis::Tables tab;
    aegis::DevTables dt{};
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;            // Viterbi stream of the time-chunked pipeline
    bool troughs_off = false;                 // AEGIS_TROUGHS_IN_FRAME=0 at create
    bool bin_table_off = false;               // AEGIS_OBS_BIN_TABLE=0 at create: pyin_obs_kernel evaluates the exact pitch-bin expression for every trough
    bool cmnd_off = false;                    // AEGIS_CMND_IN_FRAME=0 at create: pyin_obs_kernel walks the CMND cumsum (tests compare the two paths)
    bool debug_stages = false;                // AEGIS_DEBUG_STAGES=1 at create: pyin_obs also writes the CMND rows ("yin") for the stage tests
    hipStream_t stream4 = nullptr;            // second frame-stage stream: odd time chunks (their FFTs overlap the even chunks' YIN / observation kernels)
    hipStream_t stream3 = nullptr;            // host->device sample copies of aegis_analyze_batch, chunk by chunk
    // CU-partitioned stream sets of the pipeline (split_streams): [0] Viterbi on 64 CUs / frame stage on 192, [1] 128 / 128
    struct SplitSet { hipStream_t frame_a = nullptr, frame_b = nullptr, viterbi = nullptr; bool tried = false; } split[2];
    int n_cus = 0;                            // compute units of the device (CU masks are built for this count)
    // Events (all made by new_event, which enters them in owned_events: teardown destroys that list).  The fixed ones exist
    // from aegis_create on; sync_events grows by one per time chunk beyond its fixed slots.
    std::vector<hipEvent_t> owned_events;
    hipEvent_t copy_event = nullptr;
    std::vector<hipEvent_t> sync_events;      // cross-stream dependencies (no timing): the slots EV_* above
    hipEvent_t split_ev[2] = {nullptr, nullptr};   // around an automatic split call's Viterbi kernels: the planning rule checks its estimate against them
    hipEvent_t hyb_ev[3] = {nullptr, nullptr, nullptr};
    hipEvent_t fin_ev[2] = {nullptr, nullptr};       // fork / join of a split pass's two finishing streams (launch_viterbi_split)
    int64_t max_frames_per_pass = 0;
    int fail_allocs = 0;                             // test hook: workspace growths left to fail with AEGIS_ERR_NOMEM
    mutable std::string err;
    std::vector<void *> table_allocs;
    std::vector<DevBuf *> bufs;               // every DevBuf of the handle that holds memory (ensure)
    // workspaces (grow-only): passes alternate between the two, so that the frame stage of one pass runs under the
    // Viterbi of the previous one
    struct Work : PassBufs {
        DevBuf yin, chunk_off;
        DevBuf sample_off, sample_len, out_off, frame_off, order, sel_off, chunk_lo, chunk_flag, clip_tb;
        DevBuf seg64, seg32, seg_col, seg_map, seg_i32, colhist, colG, colkg, clip_flag, flag_order, tube_buf, tube_at, tube_count;    // time-split passes
    } work[2];
    DevBuf vstats, rk_raw, abort_flag, finite_flag, dbg_bins;
    // aegis_debug_set_observations: rows [F][n_bins] / [F] in the caller's clip order that the next analyze call feeds its
    // Viterbi in place of pyin_obs_kernel's (armed for that one call: the analyze entries disarm when they return)
    struct Inject { bool armed = false; int64_t F = 0; DevBuf obs, unv; } inject;
    // aegis_debug_set_difference: rows [F][max_period + 1] in the caller's clip order that the next analyze call's frame kernel
    // stores in place of its own difference function (armed for one call, like `inject`; never both)
    struct InjectD { bool armed = false; int64_t F = 0; DevBuf d; } inject_d;
    // aegis_debug_set_rake_columns: flags [F] in the caller's clip order that the next analyze call writes over each pass's
    // column flags, in front of the run-length filter (armed for one call, like the two above; one hook per call)
    struct InjectR { bool armed = false; int64_t F = 0; DevBuf flags; } inject_r;
    uint32_t chunk_gen = 0;                   // generation of the chunk flags of a persistent Viterbi launch
    int test_drop_signal = -1;
    // The single Viterbi launch of a balanced pass and its fall-back (run_with_recovery, aegis_api.hip)
    struct Persistent {
        bool on = true;                       // one Viterbi launch per balanced pass now (false for `cooldown` calls after a give-up)
        bool pending = false;                 // a persistent launch ran since the abort flag was last read
        bool gave_up = false;
        int cooldown = 0;                     // calls left on the one-launch-per-chunk schedule after a give-up; then the single launch is tried again
        int64_t fallbacks = 0;                // calls repeated with one launch per chunk (aegis_debug_fetch "persistent_fallbacks")
    } persist;
    // Time-split passes: the verdicts still to read, and the rule that stops planning them when they do not pay (split_verdict, aegis_exec.hip)
    struct SplitCheck { int pass; aegis::PassParams p; };
    struct TimeSplit {
        std::vector<SplitCheck> checks;       // split passes of the call in flight whose clip flags have not been read
        int bad = 0;                          // automatic split calls in a row that did not pay (two of them start the cool-down)
        int cooldown = 0;                     // automatic mode: calls left without time-split passes after one that did not pay (clips redone sequentially)
        int64_t stats[4] = {0, 0, 0, 0};      // since create: split passes, segments, clips flagged for the sequential kernel, lock-on runs that never locked
        double last_viterbi_ms = 0.0;         // measured Viterbi time of the call's last automatic split pass
        int64_t last_carried_steps = 0;       // rounds of second speculation (viterbi_band.inc, phases 3 / 4) that had work in the call's last split pass
        std::vector<int64_t> last_flags;      // per clip of the call's last split pass (pass order: longest first): the verification's verdict bits
    } tsplit;
    aegis::PlanKnobs knobs;                   // scheduling knobs (plan.h), read from the environment at create
    // Filter banks built and uploaded so far, most recently used first (aegis_cqt.hip::cqt_bank_locked): at most
    // cqt_bank_cap of them (8, or AEGIS_CQT_BANKS = 1..32 at create); the least recently used one is evicted.
    struct CachedBank { aegis::CqtBank bank; size_t bytes = 0; };
    std::list<CachedBank> cqt_banks;
    int cqt_bank_cap = 8;
    int64_t cqt_bank_builds = 0;              // banks built since create (aegis_get_param "cqt_bank_builds")
    int64_t cqt_bank_bytes = 0, cqt_bank_build_us = 0;   // of the last build: device bytes, host build + upload time
    DevBuf q_pcm, q_soff, q_foff, q_toff, q_out, q_chroma, q_cls;
    // aegis_estimate_tuning: the 101 histogram edges (host, and uploaded at create), geometry, peak lists, per-clip results
    std::vector<double> tuning_edges;
    const double *d_tuning_edges = nullptr;
    DevBuf tn_meta, tn_pitch, tn_mag, tn_count, tn_median, tn_cells, tn_tuning;
    std::vector<int64_t> tn_last_peak_off;    // [n_clips + 1] of the most recent call that ran (aegis_debug_fetch "tuning_*"); empty before one
    DevBuf t_x, t_off, t_a, t_b, t_c, t_d, t_e, t_i8, t_i64a, t_i64b;   // trend-filter staging
    DevBuf t_pa;                              // scratch of the fused pitch analysis: 12 rows of doubles + 1 of bytes
    DevBuf io_pcm, io_f0, io_voiced, io_vprob, io_rms, io_rake, io_sdb, io_bin, io_colmean;
    DevBuf pcm_raw, pcm_clips, pcm_ranges, pcm_taps;   // aegis_analyze_pcm: raw bytes, clip table, per-chunk range tables, filters
    DevBuf sy_oscs, sy_notes, sy_tiles, sy_tile_notes, sy_osc_peak, sy_clip_peak, sy_mix, sy_out;   // aegis_synth_adsr / aegis_synth_adsr_notes: records, peaks, float64 mix, int16 result
    DevBuf sy_bends, sy_segs;                 // aegis_synth_adsr_bend: per-oscillator slices and the segment tables of the bent notes
    // the layout of the most recent render_into that launched (aegis_debug_fetch "synth_*"); all empty before one, and after
    // one that failed: per clip its samples (back to back in sy_mix), per note of the mix its oscillator's index
    std::vector<int64_t> sy_last_total;
    std::vector<int32_t> sy_last_osc;
    DevBuf fx_a, fx_b, fx_recs, fx_tiles, fx_peak, fx_taps, fx_i16;   // aegis_effects: the two float64 batch buffers, records, clip maxima, taps, int16 in / out
    // aegis_note_fit / aegis_compare_audio / aegis_synth_one_note: slices, records, per-frame features, scores; stored note
    DevBuf nf_audio, nf_oscs, nf_cands, nf_notes, nf_boff, nf_peak, nf_cnum, nf_cden, nf_zc, nf_rms, nf_out, nf_best;
    DevBuf nf_sig, nf_sigoff, nf_cands2;
    // aegis_verify_techniques: segments, event records, mel power, signal maxima, results; the fmax-8000 mel bank of every
    // sample rate asked for so far (map nodes never move, so the DevBufs inside may be listed in bufs)
    DevBuf vf_audio, vf_events, vf_boff, vf_mel, vf_max, vf_sim, vf_keep;
    struct VerifyBank { aegis::MelBank host; int32_t n_used = 0; bool uploaded = false; DevBuf start, len, off, w; };
    std::map<int32_t, VerifyBank> vf_banks;
    DevBuf sl_mag, sl_foff, sl_img, sl_bin, sl_sal, sl_shift;   // aegis_salience / aegis_cqt_salience: caller magnitudes, frame offsets, image, candidates
    DevBuf on_img, on_foff, on_env, on_energy, on_x, on_mask, on_back, on_count;   // aegis_onset_* / aegis_analyze_onsets: caller images / envelopes, frame offsets, envelope, energy track, normalised envelope, results
    // aegis_tempo / aegis_beat_track / aegis_analyze_beats: caller envelopes, frame and tile offsets, window, tile sums, tempogram means,
    // moments, per-clip periods / table offsets / tables, local score, cumulative score, back links
    DevBuf bt_env, bt_foff, bt_toff, bt_win, bt_parts, bt_tg, bt_stats, bt_period, bt_taboff, bt_tabs, bt_ls, bt_cum, bt_back;
    // aegis_hpss_masks: one pass's magnitudes, the two medians, the two masks, its segment records, the first bad element
    // (aegis_stft: a pass's samples, its three offset tables, the complex spectrum; its magnitudes go to hp_in)
    DevBuf hp_in, hp_harm, hp_perc, hp_mh, hp_mp, hp_segs, hp_flag, hp_pcm, hp_off, hp_D;
    DevBuf hp_fa, hp_fb, hp_ya, hp_yb;        // aegis_istft / aegis_hpss: the float64 resynthesis frames of the two stems, their float32 audio
    // aegis_dtw / aegis_align_chroma: caller sequences, their unit columns, frame offsets, pair records, one pass's step codes
    // and boundary rows, the call's paths, path lengths and costs, the probe of D
    DevBuf dw_seq, dw_unit, dw_foff, dw_pairs, dw_codes, dw_bnd, dw_paths, dw_len, dw_cost, dw_probe;
    // aegis_activations / aegis_cqt_activations: caller magnitudes, frame offsets, the transposed dictionary, the Gram matrix,
    // the activation image, candidate rows and activations
    DevBuf nn_mag, nn_foff, nn_w, nn_g, nn_act, nn_row, nn_val;
    // aegis_phase_vocoder / aegis_time_warp / aegis_resample / aegis_pitch_shift: a pass's steps, clip records, the output
    // side's offset tables, the vocoder's spectrum D', the interpolation table, resampling records, resampled audio
    DevBuf pv_steps, pv_clips, pv_off, pv_D2, pv_win, pv_res, pv_y;
    int64_t dtw_pass_bytes =(int64_t)512 << 20;   // codes and boundary rows of one pass (AEGIS_DTW_PASS_BYTES at create; a pair that needs more runs alone)
    bool notefit_store = false;               // AEGIS_NOTEFIT_STORE=1 at create: every candidate rendered once into nf_sig and read by the frames instead of recomputed
    int32_t lag_stride = 0, yin_stride = 0, obs_stride = 0;
    aegis::CallPlan plan;                     // the last call's plan: its host arrays stay alive until the stream drained
    bool plan_in_flight = false;              // the stream may still read them
    // profiling
    bool profiling = false;
    std::vector<std::pair<std::string, std::pair<hipEvent_t, hipEvent_t>>> events;
    std::map<std::string, double> last_ms;
    std::map<std::string, int> last_count;
    std::mutex mu;                            // one analyze call at a time per handle (server.py shares an engine)
    // open aegis_stream objects keep the handle alive: aegis_destroy() with streams still open only marks the handle,
    // the last aegis_stream_free() tears it down (either order of the two calls is safe)
    int open_streams = 0;
    bool destroy_requested = false;
};

// One clip fed incrementally (aegis_stream_*): its own PCM buffer and workspace, so batch calls on
// the same handle may interleave.  Frames are analysed as soon as their 2048-sample window is
// complete; the Viterbi column is carried across pushes exactly as the offline pipeline carries it
// across time chunks, so aegis_stream_close() returns what aegis_analyze_batch() returns.
struct aegis_stream : PassBufs {
    aegis_handle *h = nullptr;
    int64_t cap_samples = 0, cap_frames = 0;
    int64_t n_samples = 0;      // samples received
    int64_t frames_done = 0;    // frames analysed (= Viterbi columns produced)
    bool closed = false;
    std::vector<DevBuf *> bufs; // every DevBuf of the stream that holds memory (sized through the handle's ensure, owned here)
    DevBuf pcm, live, meta;     // the stream's own: its samples, the arg-max state of every column, the one-clip geometry (kernels.h StreamMeta)
    DevBuf o_f0, o_voiced, o_vprob, o_rms, o_rake, o_sdb;
    std::vector<int64_t> host_meta;
    // captured hipGraph of one fixed-size push (built lazily for the first push size that is a multiple of hop)
    // ([0]: aegis_stream_push, [1]: aegis_stream_push_commit, the same chain with the commit kernel behind the Viterbi)
    DevBuf ctl, g_staging, g_result;
    float *pin_samples = nullptr;
    unsigned char *pin_result = nullptr;
    hipGraph_t graph[2] = {nullptr, nullptr};
    hipGraphExec_t graph_exec[2] = {nullptr, nullptr};
    int64_t graph_push[2] = {0, 0};
    bool graph_failed = false;
    // streaming commit (aegis_stream_push_commit): the device keeps the frontier in a StreamCommitCtl behind the StreamCtl
    // of `ctl` and the decided bins in c_bins [cap_frames]; the host mirrors the frontier and counts what it handed out
    DevBuf c_bins, c_result;
    unsigned char *pin_commit = nullptr;               // kCommitResultBytes, pinned (the graph's second D2H copy)
    unsigned char commit_host[aegis::kCommitResultBytes] = {};
    int64_t c_frontier = -1;    // last decided frame on the device
    int64_t c_newest = -1;      // newest frame the commit kernel has walked from
    int64_t c_delivered = 0;    // frames handed to the caller so far
    int64_t c_walked = 0, c_walked_wide = 0;    // frames the last commit launch walked, and how many of them as a bit mask
    // aegis_debug_stream_set_observations: rows [F][n_bins] / [F] in frame order that every launch of the observation kernel
    // of THIS stream is followed by a copy of (armed before the first sample, for the stream's whole life; the handle's
    // own arming neither sees nor disturbs it)
    struct Inject { bool armed = false; int64_t F = 0; DevBuf obs, unv; } inject;
};

#define HIPCHK(h, expr)                                                                         \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess) {                                                                \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e__);                      \
            return AEGIS_ERR_DEVICE;                                                            \
        }                                                                                       \
    } while (0)
// h->buf holds at least `bytes` afterwards, and at least 8 (an empty vector still gets a valid pointer), or the caller returns
// what ensure() answered
#define ENSURE(h, buf, bytes)                                                                               \
    do {                                                                                                    \
        const int rc__ = aegis::ensure(h, (h)->buf, std::max<size_t>((size_t)(bytes), 8));                 \
        if (rc__ != AEGIS_OK) return rc__;                                                                  \
    } while (0)
// the whole host vector v into h->buf (sized for it) on stream s; v outlives the caller's StreamScope
#define PUT(h, buf, v, s)                                                                                   \
    do {                                                                                                    \
        ENSURE(h, buf, (v).size() * sizeof((v)[0]));                                                        \
        HIPCHK(h, aegis::upload((h)->buf, (v).data(), (v).size() * sizeof((v)[0]), s));                     \
    } while (0)
// n elements of the device array src into the host array dst (whose element type counts the bytes) on stream s
#define FETCH(h, dst, src, n, s) HIPCHK(h, hipMemcpyAsync(dst, src, (size_t)(n) * sizeof(*(dst)), hipMemcpyDeviceToHost, s))
// A launch under a profiling name: the event pair around it on stream s, then the launch's error check.
#define TIMED(h, name, s, ...)                                                                              \
    do {                                                                                                    \
        aegis::begin_event(h, name, s);                                                                     \
        __VA_ARGS__;                                                                                        \
        aegis::end_event(h, s);                                                                             \
        HIPCHK(h, hipGetLastError());                                                                       \
    } while (0)
// what this header adds to the library without adding to its dynamic symbol table
#define AEGIS_LOCAL __attribute__((visibility("hidden")))
#define DEVICE_ONLY(h) \
    do { if ((h)->device < 0) { (h)->err = "handle was created with device=-1 (host tables only)"; return AEGIS_ERR_DEVICE; } } while (0)

namespace aegis {

// ---- owned buffers and events (aegis_handle.hip) ----
int grow_buf(aegis_handle *h, std::vector<DevBuf *> &owner, DevBuf &b, size_t bytes);
// b holds at least `bytes` afterwards (growth rule, the fail_allocs hook and the owner's list: grow_buf)
inline int ensure(aegis_handle *h, DevBuf &b, size_t bytes) { return bytes <= b.cap ? AEGIS_OK : grow_buf(h, h->bufs, b, bytes); }
inline int ensure(aegis_stream *st, DevBuf &b, size_t bytes) { return bytes <= b.cap ? AEGIS_OK : grow_buf(st->h, st->bufs, b, bytes); }
inline hipError_t upload(DevBuf &b, const void *src, size_t bytes, hipStream_t s) {
    return bytes ? hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
}
void free_bufs(std::vector<DevBuf *> &owner) noexcept;
int new_event(aegis_handle *h, hipEvent_t *e, unsigned flags);
void destroy_now(aegis_handle *h) noexcept;
// Nothing is thrown across the C boundary (include/aegis_hip.h): every exported entry runs its body inside
// try { ... } catch (...) { return abi_fail(h); }, which maps the in-flight exception to a return code.
int abi_fail(aegis_handle *h) noexcept;
// The frame of every exported entry that locks its handle, ENTRY(h) ... ENTRY_END(h) around its body: a null handle is
// AEGIS_ERR_INVALID, the body runs with h->mu held (a handle is shared between threads: nothing writes h->err in front
// of the lock) and what it throws becomes abi_fail's code.  Every path of the body returns.
#define ENTRY(h)                                                                                            \
    if (!(h)) return AEGIS_ERR_INVALID;                                                                     \
    try {                                                                                                   \
        std::lock_guard<std::mutex> entry_lock__((h)->mu);
#define ENTRY_END(h) } catch (...) { return aegis::abi_fail(h); }
// The same frame for an entry that takes a stream: a null stream, or one without a handle, is AEGIS_ERR_INVALID and
// nothing is written; the lock is the handle's; a stream whose handle aegis_destroy() has marked answers "handle was
// destroyed" before the body looks at an argument.
#define STREAM_ENTRY(st)                                                                                    \
    if (!(st) || !(st)->h) return AEGIS_ERR_INVALID;                                                        \
    try {                                                                                                   \
        std::lock_guard<std::mutex> entry_lock__((st)->h->mu);                                              \
        if ((st)->h->destroy_requested) { (st)->h->err = "handle was destroyed"; return AEGIS_ERR_INVALID; }
#define STREAM_ENTRY_END(st) } catch (...) { return aegis::abi_fail((st)->h); }
// The domain rules of injected observation rows (aegis_debug_set_observations and aegis_debug_stream_set_observations):
// AEGIS_OK, or AEGIS_ERR_INVALID with a message that names the frame.  Host arithmetic only.
AEGIS_LOCAL int check_observation_rows(aegis_handle *h, const double *logobs, const double *logunv, int64_t F);

// ---- profiling event pairs (aegis_handle.hip) ----
void begin_event(aegis_handle *h, const char *name, hipStream_t s);
void end_event(aegis_handle *h, hipStream_t s);
void drop_events(aegis_handle *h) noexcept;       // destroys the pairs not collected
void collect_events(aegis_handle *h);

// ---- the call scope (its drain: aegis_handle.hip) ----
// Waits for s, and for the feed stream (stream3) of a plan still in flight.  collect: a failed wait is AEGIS_ERR_DEVICE
// with a message, and the profiling pairs are collected; otherwise errors are ignored, the pairs dropped, nothing thrown.
AEGIS_LOCAL int drain_stream(aegis_handle *h, hipStream_t s, bool collect);
// Asynchronous copies read and write host arrays of an entry's frame, so no way out of the entry may leave that frame before
// the stream has drained.  THE RULE: declare every host array the stream will read or write, THEN the scope, at the point
// where the entry (or one run_halving group) starts enqueuing; the arrays then outlive the scope, and every later return
// (HIPCHK, ENSURE, a validation that fails half way) and every exception is safe.  The good path ends in
// `return scope.finish();`, the call's one final synchronisation; any other way out waits too and drops the call's
// profiling pairs.  Handle locked, device set.
class AEGIS_LOCAL StreamScope {
    aegis_handle *h;
    hipStream_t s;
    bool done = false;
public:
    explicit StreamScope(aegis_handle *h_, hipStream_t s_ = nullptr) : h(h_), s(s_ ? s_ : h_->stream) {}
    StreamScope(const StreamScope &) = delete;
    StreamScope &operator=(const StreamScope &) = delete;
    ~StreamScope() { if (!done) (void)drain_stream(h, s, false); }
    int finish() { done = true; return drain_stream(h, s, true); }
    void leave_enqueued() { done = true; }        // a caller's stream with sync == 0: no host array is in flight, nothing is waited for
};

// One device pass for the whole batch of n independent items (clips, notes, pairs): group(i0, i1) runs items [i0, i1)
// under a StreamScope of its own.  When its buffers cannot be allocated (AEGIS_ERR_NOMEM) the batch is cut into passes of
// half as many items and the rest is tried again: an item's result does not depend on the grouping.
template <class F>
int run_halving(aegis_handle *h, int32_t n, F &&group) {
    int32_t size = n;
    for (int32_t i0 = 0; i0 < n;) {
        const int32_t i1 = std::min(n, i0 + size);
        const int rc = group(i0, i1);
        if (rc == AEGIS_ERR_NOMEM && size > 1) {
            (void)hipDeviceSynchronize();
            (void)hipGetLastError();
            size = (size + 1) / 2;
            continue;
        }
        if (rc != AEGIS_OK) return rc;
        i0 = i1;
    }
    return AEGIS_OK;
}

// ---- the bent ADSR render as a stage of another entry (aegis_synth.hip; AdsrBatch: adsr_host.h) ----
struct AdsrBatch;
int check_bend_request(aegis_handle *h, int32_t sample_rate, int32_t n_clips, const aegis_synth_note *notes, const int64_t *note_off,
                       const double *length_seconds, const aegis_adsr_params *params, const int32_t *note_track,
                       const aegis_synth_wheel *wheel, const int64_t *wheel_off, const double *bend_range, int16_t *const *out,
                       const int64_t *out_cap);
int fill_bend_batch(aegis_handle *h, int32_t sr, int32_t c0, int32_t c1, const aegis_synth_note *notes, const int64_t *note_off,
                    const double *length_seconds, const aegis_adsr_params *params, const int32_t *note_track,
                    const aegis_synth_wheel *wheel, const int64_t *wheel_off, const double *bend_range, AdsrBatch &B);
int render_into(aegis_handle *h, const AdsrBatch &B, const char *const (&labels)[3]);

// ---- the CQT as a stage of another entry (aegis_cqt.hip) ----
// Handle locked, device set: the bank found or built, the clips validated, packed and uploaded, the CQT launched on the
// handle's stream into q_out (per clip [n_bins, F_c]) with the frame offsets in q_foff; n_bins comes back with its default
// filled in, *F_out is the frame total.  bin_class: the chroma fold's classes (uploaded to q_cls), or nullptr.
int cqt_host_locked(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips, int32_t &n_bins,
                    int32_t bins_per_octave, double fmin, double filter_scale, int32_t n_chroma, const int32_t *bin_class, int64_t *F_out);

// ---- the mel stage as a stage of another entry (aegis_api.hip) ----
// Handle locked, device set, clips validated (n_samples[i] >= 0, pcm[i] != NULL where there are samples): the samples fed
// as aegis_analyze_batch feeds them and the pipeline's AEGIS_STAGE_MEL pass enqueued on the handle's stream into io_sdb
// (per clip [n_mels, F_c], clip after clip, the caller's order; a clip without samples is one frame of silence).  Not
// synchronised: the caller enqueues behind it, and the caller's StreamScope drains the stream and the feed and clears
// plan_in_flight.  off / foff: sample and frame offsets [n_clips + 1], declared before that scope.
int mel_host_locked(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips, std::vector<int64_t> &off,
                    std::vector<int64_t> &foff);

// ---- the offsets walks and the onset stage as parts of another entry (aegis_onset.hip) ----
// n_frames[] -> foff [n_clips + 1] and the longest clip, or AEGIS_ERR_INVALID: clip_pre + "bad clip <c>", call_pre + "too
// many frames for one call".
AEGIS_LOCAL int frame_offsets(aegis_handle *h, const char *clip_pre, const char *call_pre, const int64_t *n_frames, int32_t n_clips,
                  std::vector<int64_t> &foff, int64_t &maxF);
// The same over clips of samples, a clip of n samples being 1 + n / hop frames (pcm[c] != NULL where there are samples);
// one prefix for both messages.
AEGIS_LOCAL int clip_frames(aegis_handle *h, const char *pre, const float *const *pcm, const int64_t *n_samples, int32_t n_clips,
                std::vector<int64_t> &foff, int64_t &maxF);
// The sample walk: clips [c0, c1) of pcm[] / n_samples[] -> soff [c1 - c0 + 1], or AEGIS_ERR_INVALID with pre + "bad clip
// <c>" (a negative length, samples without a pointer).
AEGIS_LOCAL int clip_samples(aegis_handle *h, const char *pre, const float *const *pcm, const int64_t *n_samples, int32_t c0, int32_t c1,
                 std::vector<int64_t> &soff);
// ... and the clips that have samples into b (sized here, for one sample at least) at those offsets, on stream s
AEGIS_LOCAL int upload_clips(aegis_handle *h, DevBuf &b, const float *const *pcm, int32_t c0, const std::vector<int64_t> &soff, hipStream_t s);
struct OnsetParams;
// the onset request with its defaults filled in, or AEGIS_ERR_INVALID with a message
AEGIS_LOCAL int onset_request(aegis_handle *h, const aegis_onset_params *p, OnsetParams &o);
// The envelope kernel over d_img / d_foff (device) into on_env (handle locked, device set); enqueued only.
AEGIS_LOCAL int onset_env_locked(aegis_handle *h, const float *d_img, const int64_t *d_foff, int32_t n_clips, int64_t F, int64_t maxF, int32_t n_mels,
                     const OnsetParams &o);

// ---- the batch executor and what feeds it (aegis_exec.hip, aegis_api.hip) ----
// Raw WAV bytes of aegis_analyze_pcm: per time chunk, the bytes of the input frames the chunk's new output samples read
// are copied on stream3 and one pcm_decode_resample_kernel writes those samples into the PCM buffer.
struct PcmFeed {
    const aegis_pcm_clip *src;            // [n_clips] the caller's clips
    std::vector<PcmClipDev> clips;        // host copy of the device clip table
    std::vector<int64_t> done_in;         // input frames of each clip already enqueued
    std::vector<std::vector<PcmRange>> tables;   // every launch's range table (host memory of in-flight copies)
    int64_t range_cap = 0, range_used = 0;       // entries of h->pcm_ranges
    float *y_out = nullptr;               // the decoded samples back to the host, pass after pass (optional)
};
// Host-resident input of aegis_analyze_batch: the samples each time chunk needs are copied on stream3 right
// before that chunk's frame stage is enqueued, so the transfer hides behind the pipeline instead of preceding it.
struct HostFeed {
    const float *const *pcm;      // [n_clips] host pointers
    float *dst;                   // packed device buffer (== d_pcm)
    std::vector<int64_t> copied;  // samples of each clip already enqueued (output samples for a raw-byte feed)
    PcmFeed *raw = nullptr;       // raw WAV bytes instead of float32 samples
    std::vector<int32_t> cis;
    std::vector<int64_t> need;    // (bring: samples of each clip the chunk at hand needs)
    // the samples chunk k of pass m reads, enqueued on stream3; frame stream fs waits for them (aegis_api.hip)
    int bring(aegis_handle *h, const PassPlan &m, int k, hipStream_t fs);
};
// sync: 0 = return with the work enqueued, 1 = synchronise and report (give-up of the single Viterbi launch, non-finite
// samples), 2 = the caller synchronises and makes those checks itself right away (aegis_analyze_batch: the single Viterbi
// launch is allowed, as with 1)
AEGIS_LOCAL int analyze_device_locked(aegis_handle *h, const float *d_pcm, const int64_t *sample_offsets, int32_t n_clips,
                                      double rake_sensitivity, uint32_t stages, aegis_outputs *dout, void *stream_v, int32_t sync,
                                      HostFeed *feed = nullptr);
// After a synchronisation: a persistent Viterbi launch that gave up waiting for its chunk flags says so here.
AEGIS_LOCAL int persistent_check(aegis_handle *h);
// After a synchronisation: the verdict of AEGIS_OPT_CHECK_FINITE (librosa.util.valid_audio's ParameterError).
AEGIS_LOCAL int finite_result(aegis_handle *h, uint32_t opts, const int64_t *sample_offsets, int32_t n_clips);

// ---- kernel parameters every entry fills the same way (aegis_api.hip) ----
struct RakeBounds { int min_frames, max_frames; };
RakeBounds rake_frame_bounds(const Tables &t);    // a rake lasts 10 .. 30 ms: in frames
PassParams base_params(const Tables &t);          // (rake_frame_bounds included)
int cmnd_in_frame(const aegis_handle *h);
int troughs_in_frame(const aegis_handle *h);
// The workspace half of PassParams, for a batch pass and a stream alike: the PassBufs pointers, the handle's three row
// strides, and which form of the frame / observation kernels the handle runs (cmnd_in_frame, troughs, bin_table).
AEGIS_LOCAL void bind_core(PassParams &p, const aegis_handle *h, const PassBufs &w);
DevTables rule_tables(const aegis_handle *h);     // h->dt as the Viterbi launch rules read it, also on a host-only handle
PlanInput plan_input(aegis_handle *h, const int64_t *sample_offsets, int32_t n_clips, uint32_t stages, bool feed,
                     bool caller_stream, int32_t sync, int n_cus, std::function<bool(int)> masked);

// The eight fields of aegis_outputs: which stage fills one, its bytes per frame (x n_mels for the dB image), where the pointer
// sits in the struct, the staging buffer of the host-fed entries and the stream's own buffer (nullptr: a stream has none).
struct OutField {
    uint32_t stage;
    int bytes;
    bool per_mel;
    size_t at;
    DevBuf aegis_handle::*io;
    DevBuf aegis_stream::*st;
    size_t size(int64_t F, int n_mels) const { return (size_t)F * bytes * (per_mel ? n_mels : 1); }
    void *get(const aegis_outputs *o) const { void *p; std::memcpy(&p, reinterpret_cast<const char *>(o) + at, sizeof p); return p; }
    void set(aegis_outputs *o, void *p) const { std::memcpy(reinterpret_cast<char *>(o) + at, &p, sizeof p); }
};
extern const OutField kOutFields[8];

}  // namespace aegis
