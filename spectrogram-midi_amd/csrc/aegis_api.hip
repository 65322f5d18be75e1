// C ABI of libaegis_hip.so (see include/aegis_hip.h).  Host-side orchestration:
// table upload, workspace management, kernel launches of the passes plan.cpp plans
// on one HIP stream per handle, optional hipEvent timing per kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <mutex>
#include <new>
#include <numeric>
#include <functional>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/aegis_hip.h"
#include "kernels.h"
#include "plan.h"
#include "cqt.h"
#include "pcm.h"
#include "tables.h"
#include "trend.h"

using namespace aegis;

namespace {

std::string g_create_error;

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

}  // namespace

struct aegis_handle {
    Tables tab;
    DevTables dt{};
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;            // Viterbi stream of the time-chunked pipeline
    bool troughs_off = false;                 // AEGIS_TROUGHS_IN_FRAME=0 at create
    bool cmnd_off = false;                    // AEGIS_CMND_IN_FRAME=0 at create: pyin_obs_kernel walks the CMND cumsum (tests compare the two paths)
    bool debug_stages = false;                // AEGIS_DEBUG_STAGES=1 at create: pyin_obs also writes the CMND rows ("yin") for the stage tests
    hipStream_t stream4 = nullptr;            // second frame-stage stream: odd time chunks (their FFTs overlap the even chunks' YIN / observation kernels)
    hipStream_t stream3 = nullptr;            // host->device sample copies of aegis_analyze_batch, chunk by chunk
    // CU-partitioned stream sets of the pipeline (split_streams): [0] Viterbi on 64 CUs / frame stage on 192, [1] 128 / 128
    struct SplitSet { hipStream_t frame_a = nullptr, frame_b = nullptr, viterbi = nullptr; bool tried = false; } split[2];
    int n_cus = 0;                            // compute units of the device (CU masks are built for this count)
    hipEvent_t copy_event = nullptr;
    std::vector<hipEvent_t> sync_events;      // cross-stream dependencies (no timing)
    int64_t max_frames_per_pass = 0;
    int fail_allocs = 0;                             // test hook: workspace growths left to fail with AEGIS_ERR_NOMEM
    mutable std::string err;
    std::vector<void *> table_allocs;
    // workspaces (grow-only): passes alternate between the two, so that the frame stage of one pass runs under the
    // Viterbi of the previous one
    struct Work {
        DevBuf dfn, yin, logobs, logunv, obs_seg, ptr, cmap, chunk_off, bnd, states, melpow, clipmax, rake_raw;
        DevBuf sample_off, sample_len, out_off, frame_off, order, sel_off, vstate, chunk_lo, chunk_flag, clip_tb;
        DevBuf seg64, seg32, seg_col, seg_map, seg_i32, colhist, colG, colkg, clip_flag, flag_order, tube_buf, tube_at, tube_count;    // time-split passes
    } work[2];
    DevBuf vstats, rk_raw, abort_flag, finite_flag;
    uint32_t chunk_gen = 0;                   // generation of the chunk flags of a persistent Viterbi launch
    int test_drop_signal = -1;
    bool persist_gave_up = false;
    int persist_cooldown = 0;                 // calls left on the one-launch-per-chunk schedule after a give-up; then the single launch is tried again
    int64_t persistent_fallbacks = 0;         // calls repeated with one launch per chunk (aegis_debug_fetch "persistent_fallbacks")
    bool persist_pending = false;             // a persistent launch ran since the abort flag was last read
    bool persistent = true;                   // one Viterbi launch per balanced pass now (false for persist_cooldown calls after a give-up)
    PlanKnobs knobs;                          // scheduling knobs (plan.h), read from the environment at create
    CqtBank cqt_bank;
    DevBuf q_pcm, q_soff, q_foff, q_toff, q_out, q_chroma, q_cls;
    DevBuf t_x, t_off, t_a, t_b, t_c, t_d, t_e, t_i8, t_i64a, t_i64b;   // trend-filter staging
    DevBuf t_pa;                              // scratch of the fused pitch analysis: 12 rows of doubles + 1 of bytes
    DevBuf io_pcm, io_f0, io_voiced, io_vprob, io_rms, io_rake, io_sdb, io_bin, io_colmean;
    DevBuf pcm_raw, pcm_clips, pcm_ranges, pcm_taps;   // aegis_analyze_pcm: raw bytes, clip table, per-chunk range tables, filters
    int32_t lag_stride = 0, yin_stride = 0, obs_stride = 0;
    CallPlan plan;                            // the last call's plan: its host arrays stay alive until the stream drained
    bool plan_in_flight = false;              // the stream may still read them
    struct SplitCheck { int pass; PassParams p; };
    hipEvent_t split_ev[2] = {nullptr, nullptr};   // around an automatic split call's Viterbi kernels: the planning rule checks its estimate against them
    hipEvent_t hyb_ev[3] = {nullptr, nullptr, nullptr};
    hipEvent_t fin_ev[2] = {nullptr, nullptr};       // fork / join of a split pass's two finishing streams (launch_viterbi_split)
    int split_bad = 0;                        // automatic split calls in a row that did not pay (two of them start the cool-down)
    int split_cooldown = 0;                   // automatic mode: calls left without time-split passes after one that did not pay (clips redone sequentially)
    std::vector<SplitCheck> split_checks;     // split passes of the call in flight whose clip flags have not been read
    int64_t split_stats[4] = {0, 0, 0, 0};    // since create: split passes, segments, clips flagged for the sequential kernel, lock-on runs that never locked
    double last_split_viterbi_ms = 0.0;      // measured Viterbi time of the call's last automatic split pass
    int64_t last_carried_steps = 0;          // rounds of second speculation (viterbi_band.inc, phases 3 / 4) that had work in the call's last split pass
    std::vector<int64_t> last_split_flags;   // per clip of the call's last split pass (pass order: longest first): the verification's verdict bits
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
struct aegis_stream {
    aegis_handle *h = nullptr;
    int64_t cap_samples = 0, cap_frames = 0;
    int64_t n_samples = 0;      // samples received
    int64_t frames_done = 0;    // frames analysed (= Viterbi columns produced)
    bool closed = false;
    DevBuf pcm, dfn, logobs, logunv, obs_seg, ptr, cmap, bnd, states, live, melpow, clipmax, rake_raw, vstate, meta;
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
    unsigned char commit_host[kCommitResultBytes] = {};
    int64_t c_frontier = -1;    // last decided frame on the device
    int64_t c_newest = -1;      // newest frame the commit kernel has walked from
    int64_t c_delivered = 0;    // frames handed to the caller so far
    int64_t c_walked = 0, c_walked_wide = 0;    // frames the last commit launch walked, and how many of them as a bit mask
};

namespace {

#define HIPCHK(h, expr)                                                                         \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess) {                                                                \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e__);                      \
            return AEGIS_ERR_DEVICE;                                                            \
        }                                                                                       \
    } while (0)

int ensure(aegis_handle *h, DevBuf &b, size_t bytes) {
    if (bytes <= b.cap) return AEGIS_OK;
    if (h->fail_allocs > 0) {                        // test hook (aegis_debug_fetch "fail_allocs"): the next growths fail as hipMalloc would
        --h->fail_allocs;
        h->err = "hipMalloc(" + std::to_string(bytes) + " bytes): out of memory (test hook)";
        return AEGIS_ERR_NOMEM;
    }
    if (b.p) {
        HIPCHK(h, hipDeviceSynchronize());          // kernels on any of the pipeline's streams may still use the old block
        HIPCHK(h, hipFree(b.p));
        b.p = nullptr; b.cap = 0;
    }
    const size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        b.p = nullptr;
        h->err = "hipMalloc(" + std::to_string(want) + " bytes): " + hipGetErrorString(e);
        return AEGIS_ERR_NOMEM;
    }
    b.cap = want;
    return AEGIS_OK;
}

template <typename T>
int upload_table(aegis_handle *h, const std::vector<T> &v, const T **dst) {
    void *d = nullptr;
    const size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
    HIPCHK(h, hipMalloc(&d, bytes));
    h->table_allocs.push_back(d);
    if (!v.empty()) HIPCHK(h, hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *dst = static_cast<const T *>(d);
    return AEGIS_OK;
}

PassParams base_params(const Tables &t) {
    PassParams p{};
    p.sr = t.sr; p.hop = t.hop; p.n_mels = t.n_mels;
    p.min_period = t.min_period; p.max_period = t.max_period; p.n_lags = t.n_lags;
    p.n_bins = t.n_bins; p.half_width = t.half_width; p.width = t.width; p.n_cls = t.n_cls;
    p.f0_unvoiced = NAN;
    p.fmin = t.fmin; p.log_tiny = t.log_tiny; p.log_pinit_v = t.log_pinit[0]; p.log_pinit_u = t.log_pinit[1];
    return p;
}

// The frame kernel's epilogue forms the CMND unless the stage tests want the difference function and the CMND as separate
// buffers (AEGIS_DEBUG_STAGES=1), AEGIS_CMND_IN_FRAME=0 was set when the handle was created, or the lag range does not fit
// its LDS.
int cmnd_in_frame(const aegis_handle *h) {
    return (!h->cmnd_off && !h->debug_stages && frame_cmnd_supported(h->tab.max_period)) ? 1 : 0;
}
// ... and finds the CMND's troughs there as well (AEGIS_TROUGHS_IN_FRAME=0 at create: pyin_obs_kernel loads the CMND row and
// finds them, the round-3 path; tests compare the two)
int troughs_in_frame(const aegis_handle *h) { return (cmnd_in_frame(h) && !h->troughs_off) ? 1 : 0; }

void free_buf(DevBuf &b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
}

void begin_event(aegis_handle *h, const char *name, hipStream_t s) {
    if (!h->profiling) return;
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
    (void)hipEventRecord(a, s);
    h->events.push_back({name, {a, b}});
}
void end_event(aegis_handle *h, hipStream_t s) {
    if (!h->profiling || h->events.empty()) return;
    (void)hipEventRecord(h->events.back().second.second, s);
}
void collect_events(aegis_handle *h) {
    h->last_ms.clear();
    h->last_count.clear();
    double total = 0;
    for (auto &ev : h->events) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.second.first, ev.second.second) == hipSuccess) {
            h->last_ms[ev.first] += ms;
            h->last_count[ev.first] += 1;
            total += ms;
        }
        (void)hipEventDestroy(ev.second.first);
        (void)hipEventDestroy(ev.second.second);
    }
    h->events.clear();
    h->last_ms["total"] = total;
}

// Nothing is thrown across the C boundary (include/aegis_hip.h): every exported entry runs its body inside
// try { ... } catch (...) { return abi_fail(h); }, which maps the in-flight exception to a return code.
int abi_fail(aegis_handle *h) noexcept {
    int code = AEGIS_ERR_DEVICE;
    const char *msg = "unknown C++ exception";
    std::string what;
    try { throw; }
    catch (const std::bad_alloc &) { code = AEGIS_ERR_NOMEM; msg = "out of host memory"; }
    catch (const std::length_error &) { code = AEGIS_ERR_NOMEM; msg = "request too large for a host container"; }
    catch (const std::exception &e) { try { what = e.what(); msg = what.c_str(); } catch (...) {} }
    catch (...) {}
    try { (h ? h->err : g_create_error) = msg; } catch (...) {}
    return code;
}

}  // namespace

extern "C" {

int aegis_abi_version(void) { return AEGIS_ABI_VERSION; }

const char *aegis_last_error(const aegis_handle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int aegis_create(const aegis_config *cfg, aegis_handle **out) {
    aegis_handle *h = nullptr;
    try {
    if (!out) { g_create_error = "out == NULL"; return AEGIS_ERR_INVALID; }
    *out = nullptr;
    aegis_config c{};
    if (cfg) c = *cfg;
    if (c.sample_rate == 0) c.sample_rate = 44100;
    if (c.hop_length == 0) c.hop_length = 512;
    if (c.n_fft == 0) c.n_fft = 2048;
    if (c.n_mels == 0) c.n_mels = 128;
    if (!(c.fmin > 0)) c.fmin = 82.4068892282175;      // note_to_hz('E2'), aegis_engine.py:63
    if (!(c.fmax > 0)) c.fmax = 1046.5022612023945;    // note_to_hz('C6')
    const bool auto_pass = c.max_frames_per_pass <= 0;
    if (auto_pass) c.max_frames_per_pass = (int64_t)1 << 21;

    h = new (std::nothrow) aegis_handle();
    if (!h) { g_create_error = "out of host memory"; return AEGIS_ERR_NOMEM; }
    const std::string terr = h->tab.build(c.sample_rate, c.hop_length, c.n_fft, c.n_mels, c.fmin, c.fmax);
    if (!terr.empty()) { g_create_error = terr; delete h; return AEGIS_ERR_INVALID; }
    if (!h->tab.set_pyin_init(c.pyin_init)) { g_create_error = "pyin_init must be AEGIS_PYIN_INIT_UNVOICED (0) or AEGIS_PYIN_INIT_UNIFORM (1)"; delete h; return AEGIS_ERR_INVALID; }
    h->device = c.device;
    h->max_frames_per_pass = c.max_frames_per_pass;
    h->knobs.read_env();                       // (a host-only handle plans with the knobs a device handle would)
    h->persistent = h->knobs.persistent_wanted;

    h->lag_stride = (h->tab.max_period + 1 + 7) & ~7;
    // a dfn row also holds the frame's trough list when the frame kernel finds the troughs (PassParams::troughs)
    h->lag_stride = std::max<int32_t>(h->lag_stride, (trough_row_doubles_host(h->tab.n_lags) + 7) & ~7);
    h->yin_stride = (h->tab.n_lags + 7) & ~7;
    h->obs_stride = (h->tab.n_bins + 7) & ~7;
    if (c.device == -1) { *out = h; return AEGIS_OK; }   // host tables only

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_create_error = std::string("no HIP device available: ") + hipGetErrorString(e);
        delete h; return AEGIS_ERR_DEVICE;
    }
    if (c.device < 0 || c.device >= ndev) { g_create_error = "device ordinal out of range"; delete h; return AEGIS_ERR_INVALID; }
    auto fail = [&](int code) { g_create_error = h->err; aegis_destroy(h); return code; };
#define CRT(expr) do { int rc__ = (expr); if (rc__ != AEGIS_OK) return fail(rc__); } while (0)
#define CRTHIP(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) { h->err = std::string(#expr) + ": " + hipGetErrorString(e__); return fail(AEGIS_ERR_DEVICE); } } while (0)
    CRTHIP(hipSetDevice(c.device));
    CRTHIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    CRTHIP(hipStreamCreateWithFlags(&h->stream4, hipStreamNonBlocking));
    CRTHIP(hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
    CRTHIP(hipStreamCreateWithFlags(&h->stream3, hipStreamNonBlocking));
    if (const char *e = std::getenv("AEGIS_DEBUG_STAGES")) h->debug_stages = (e[0] == '1');
    if (const char *e = std::getenv("AEGIS_CMND_IN_FRAME")) h->cmnd_off = (e[0] == '0');
    if (const char *e = std::getenv("AEGIS_TROUGHS_IN_FRAME")) h->troughs_off = (e[0] == '0');
    if (const char *e = std::getenv("AEGIS_TEST_DROP_CHUNK_SIGNAL")) h->test_drop_signal = std::atoi(e);
    CRTHIP(hipDeviceGetAttribute(&h->n_cus, hipDeviceAttributeMultiprocessorCount, c.device));
    if (auto_pass) {
        // Default workspace bound: as many frames per pass as a third of the free device memory holds (a pass needs
        // ~10.3 KB per frame at the reference's rates, and two workspaces alternate when a call needs several passes), between
        // 2^21 and 2^24 frames.  On a 288 GB MI355X the 512-clip folder of BASELINE.json configs[3] (8.36 M frames) is then ONE
        // pass: every clip's Viterbi starts at once and the frame stage of the whole folder runs beside it (411 -> 385 ms).
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const int64_t per_frame = (int64_t)h->lag_stride * 8 + (int64_t)h->obs_stride * 8 + 8 + 2 * h->tab.n_bins * 2 +
                                      2 * h->tab.n_bins * 2 / kViterbiChunk + h->tab.n_mels * 4 + 16;
            const int64_t fit = (int64_t)(free_b / 3) / per_frame;
            h->max_frames_per_pass = std::min<int64_t>((int64_t)1 << 24, std::max<int64_t>((int64_t)1 << 21, fit));
        }
    }
    CRTHIP(hipEventCreateWithFlags(&h->copy_event, hipEventDisableTiming));
    CRTHIP(viterbi_configure());
    CRT(ensure(h, h->vstats, 32));
    CRTHIP(hipMemset(h->vstats.p, 0, 32));
    CRTHIP(cqt_configure());

    const Tables &t = h->tab;
    CRT(upload_table(h, t.hann, &h->dt.hann));
    CRT(upload_table(h, t.mel_start, &h->dt.mel_start));
    CRT(upload_table(h, t.mel_len, &h->dt.mel_len));
    CRT(upload_table(h, t.mel_off, &h->dt.mel_off));
    CRT(upload_table(h, t.mel_w, &h->dt.mel_w));
    CRT(upload_table(h, t.mel_chunk_bin, &h->dt.mel_chunk_bin));
    CRT(upload_table(h, t.mel_chunk_w, &h->dt.mel_chunk_w));
    CRT(upload_table(h, t.mel_band_chunk, &h->dt.mel_band_chunk));
    h->dt.mel_chunks = (int32_t)t.mel_chunk_bin.size();
    CRT(upload_table(h, t.thresholds, &h->dt.thresholds));
    CRT(upload_table(h, t.beta_probs, &h->dt.beta_probs));
    CRT(upload_table(h, t.beta_cumsum, &h->dt.beta_cumsum));
    CRT(upload_table(h, t.beta_suffix, &h->dt.beta_suffix));
    CRT(upload_table(h, t.boltz_fact, &h->dt.boltz_fact));
    CRT(upload_table(h, t.boltz_exp, &h->dt.boltz_exp));
    CRT(upload_table(h, t.log_trans_band, &h->dt.lt_band));
    if (!t.log_trans_pack.empty()) CRT(upload_table(h, t.log_trans_pack, &h->dt.lt_pack));
    CRT(upload_table(h, t.freqs, &h->dt.freqs));
    {
        const double *tw = nullptr;
        CRT(upload_table(h, t.twiddle, &tw));
        h->dt.twiddle = reinterpret_cast<const double2 *>(tw);
    }
#undef CRT
#undef CRTHIP
    *out = h;
    return AEGIS_OK;
    } catch (...) {
        const int code = abi_fail(nullptr);
        if (h) { if (out) *out = nullptr; aegis_destroy(h); }
        return code;
    }
}

static void destroy_now(aegis_handle *h) noexcept;

void aegis_destroy(aegis_handle *h) {
    if (!h) return;
    {
        std::lock_guard<std::mutex> lock(h->mu);
        if (h->open_streams > 0) { h->destroy_requested = true; return; }   // the last aegis_stream_free() finishes the job
    }
    destroy_now(h);
}

static void destroy_now(aegis_handle *h) noexcept {
    if (h->device < 0) { delete h; return; }
    // AEGIS_TRACE_DESTROY=1: one line on stderr before every step that can block (which call a teardown sat in)
    const bool trace = std::getenv("AEGIS_TRACE_DESTROY") != nullptr;
    auto T = [&](const char *what) { if (trace) { std::fprintf(stderr, "[aegis destroy] %s\n", what); std::fflush(stderr); } };
    T("hipSetDevice");
    (void)hipSetDevice(h->device);
    // Bounded wait first: the handle's streams normally are idle here (every blocking entry synchronises before it returns).
    // If something is still running after ten seconds -- a caller that enqueued with sync = 0 and never waited, a wedged
    // device -- the GPU objects are leaked rather than waited for: a teardown (Handle.__del__ runs it from the garbage
    // collector, possibly while an exception unwinds) must never be the call that hangs a process.
    {
        std::vector<hipStream_t> all{h->stream, h->stream2, h->stream3, h->stream4};
        for (auto &ss : h->split) for (hipStream_t q : {ss.frame_a, ss.frame_b, ss.viterbi}) all.push_back(q);
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            bool busy = false;
            for (hipStream_t q : all) if (q && hipStreamQuery(q) == hipErrorNotReady) busy = true;
            if (!busy) break;
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10)) {
                std::fprintf(stderr, "libaegis_hip: aegis_destroy: work still running on the handle's streams after 10 s; its device memory and streams are leaked\n");
                (void)hipGetLastError();
                delete h;
                return;
            }
            std::this_thread::sleep_for(std::chrono::milliseconds(1));
        }
        (void)hipGetLastError();
    }
    // The CU-masked streams own their hardware queues (plain streams draw from the runtime's pool), so destroying one really
    // tears a queue down -- and hipStreamDestroy sat in that for ever (gpurun_out/call53.log) after
    // a pass whose streams had waited on each other's events with timing events recorded between them (profiling on, the
    // host-buffer entry's schedule), although every stream of the handle had been synchronised one by one.  A device-wide
    // synchronisation first makes the runtime retire what it still tracks across streams; with it the same teardown
    // returns (tools/exit_hang_probe.py, matrix in profiles/r4_exit_hang_probe.txt).
    T("device sync");
    (void)hipDeviceSynchronize();
    for (auto &ss : h->split)
        for (hipStream_t q : {ss.frame_a, ss.frame_b, ss.viterbi})
            if (q) { T("destroy masked stream"); (void)hipStreamDestroy(q); }
    T("sync stream"); if (h->stream) (void)hipStreamSynchronize(h->stream);
    T("sync stream2"); if (h->stream2) (void)hipStreamSynchronize(h->stream2);
    T("sync stream3"); if (h->stream3) (void)hipStreamSynchronize(h->stream3);
    T("sync stream4"); if (h->stream4) (void)hipStreamSynchronize(h->stream4);
    T("events");
    for (auto &ev : h->events) { (void)hipEventDestroy(ev.second.first); (void)hipEventDestroy(ev.second.second); }
    h->events.clear();
    for (hipEvent_t e : h->sync_events) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->split_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->hyb_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->fin_ev) if (e) (void)hipEventDestroy(e);
    T("free tables");
    for (void *p : h->table_allocs) (void)hipFree(p);
    if (h->cqt_bank.dev) (void)hipFree(h->cqt_bank.dev);
    T("free workspaces");
    for (auto &w : h->work)
        for (DevBuf *b : {&w.dfn, &w.yin, &w.logobs, &w.logunv, &w.obs_seg, &w.ptr, &w.cmap, &w.chunk_off, &w.bnd, &w.states, &w.melpow,
                          &w.clipmax, &w.rake_raw, &w.sample_off, &w.sample_len, &w.out_off, &w.frame_off, &w.order, &w.sel_off,
                          &w.vstate, &w.chunk_lo, &w.chunk_flag, &w.clip_tb, &w.seg64, &w.seg32, &w.seg_col, &w.seg_map, &w.seg_i32,
                          &w.colhist, &w.colG, &w.colkg, &w.clip_flag, &w.flag_order, &w.tube_buf, &w.tube_at, &w.tube_count})
            free_buf(*b);
    T("free staging");
    for (DevBuf *b : {&h->vstats, &h->rk_raw, &h->abort_flag, &h->finite_flag, &h->t_x, &h->t_off, &h->t_a, &h->t_b, &h->t_c, &h->t_d, &h->t_e,
                      &h->t_i8, &h->t_i64a, &h->t_i64b, &h->t_pa, &h->q_pcm, &h->q_soff, &h->q_foff, &h->q_toff, &h->q_out, &h->q_chroma, &h->q_cls, &h->io_pcm, &h->io_f0, &h->io_voiced, &h->io_vprob, &h->io_rms, &h->io_rake,
                      &h->io_sdb, &h->io_bin, &h->io_colmean, &h->pcm_raw, &h->pcm_clips, &h->pcm_ranges, &h->pcm_taps})
        free_buf(*b);
    T("destroy streams");
    if (h->stream) (void)hipStreamDestroy(h->stream);
    if (h->stream2) (void)hipStreamDestroy(h->stream2);
    if (h->stream3) (void)hipStreamDestroy(h->stream3);
    if (h->stream4) (void)hipStreamDestroy(h->stream4);
    if (h->copy_event) (void)hipEventDestroy(h->copy_event);
    T("done");
    delete h;
}

int64_t aegis_frames_for(const aegis_handle *h, int64_t n_samples) {
    try {
    if (!h || n_samples < 0) return AEGIS_ERR_INVALID;
    return 1 + n_samples / h->tab.hop;
    } catch (...) { return abi_fail(const_cast<aegis_handle *>(h)); }
}

int aegis_set_profiling(aegis_handle *h, int32_t on) {
    try {
    if (!h) return AEGIS_ERR_INVALID;
    h->profiling = on != 0;
    return AEGIS_OK;
    } catch (...) { return abi_fail(h); }
}

int aegis_last_kernel_launches(const aegis_handle *h, const char *name) {
    if (!h || !name) return -1;
    auto it = h->last_count.find(name);
    return it == h->last_count.end() ? 0 : it->second;
}

double aegis_last_kernel_ms(const aegis_handle *h, const char *name) {
    if (!h || !name) return -1.0;
    auto it = h->last_ms.find(name);
    return it == h->last_ms.end() ? -1.0 : it->second;
}

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
};

// Enqueues on stream3 the raw bytes and the decode of output samples [copied[ci], need[i]) of the pass's clips i.
static int pcm_feed(aegis_handle *h, HostFeed &feed, const std::vector<int32_t> &cis, const std::vector<int64_t> &need) {
    PcmFeed &pf = *feed.raw;
    std::vector<PcmRange> tab;
    int64_t tiles = 0;
    for (size_t i = 0; i < cis.size(); ++i) {
        const int ci = cis[i];
        int64_t &done = feed.copied[(size_t)ci];
        if (need[i] <= done) continue;
        const PcmClipDev &c = pf.clips[(size_t)ci];
        const int64_t fb = (int64_t)c.ch * (c.fmt == AEGIS_PCM_U8 ? 1 : c.fmt == AEGIS_PCM_S16 ? 2 : c.fmt == AEGIS_PCM_S24 ? 3 : 4);
        const int64_t in_hi = pcm_inputs_needed(c, need[i]);
        int64_t &din = pf.done_in[(size_t)ci];
        if (in_hi > din) {
            HIPCHK(h, hipMemcpyAsync(static_cast<uint8_t *>(h->pcm_raw.p) + c.byte_off + din * fb,
                                     static_cast<const uint8_t *>(pf.src[ci].data) + din * fb, (size_t)((in_hi - din) * fb),
                                     hipMemcpyHostToDevice, h->stream3));
            din = in_hi;
        }
        tab.push_back(PcmRange{done, need[i], tiles, ci, 0});
        tiles += (need[i] - done + c.tile - 1) / c.tile;
        done = need[i];
    }
    if (tab.empty()) return AEGIS_OK;
    if (pf.range_used + (int64_t)tab.size() > pf.range_cap) {      // the slots are reused once the launches reading them are done
        HIPCHK(h, hipStreamSynchronize(h->stream3));
        pf.range_used = 0;
    }
    PcmRange *d_tab = static_cast<PcmRange *>(h->pcm_ranges.p) + pf.range_used;
    pf.range_used += (int64_t)tab.size();
    pf.tables.push_back(std::move(tab));
    const std::vector<PcmRange> &t = pf.tables.back();
    HIPCHK(h, hipMemcpyAsync(d_tab, t.data(), t.size() * sizeof(PcmRange), hipMemcpyHostToDevice, h->stream3));
    launch_pcm_decode(static_cast<const uint8_t *>(h->pcm_raw.p), static_cast<const PcmClipDev *>(h->pcm_clips.p), d_tab,
                      (int)t.size(), tiles, static_cast<const float *>(h->pcm_taps.p), feed.dst, h->stream3);
    HIPCHK(h, hipGetLastError());
    return AEGIS_OK;
}

// sync: 0 = return with the work enqueued, 1 = synchronise and report (give-up of the single Viterbi launch, non-finite
// samples), 2 = the caller synchronises and makes those checks itself right away (aegis_analyze_batch: the single Viterbi
// launch is allowed, as with 1)
static int analyze_device_locked(aegis_handle *h, const float *d_pcm, const int64_t *sample_offsets,
                                 int32_t n_clips, double rake_sensitivity, uint32_t stages,
                                 aegis_outputs *dout, void *stream_v, int32_t sync, HostFeed *feed = nullptr);

int aegis_analyze_batch_device(aegis_handle *h, const float *d_pcm, const int64_t *sample_offsets,
                               int32_t n_clips, double rake_sensitivity, uint32_t stages,
                               aegis_outputs *dout, void *stream_v, int32_t sync) {
    try {
    if (!h) return AEGIS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(h->mu);
    if (!h->persistent && h->knobs.persistent_wanted && h->persist_cooldown > 0 && --h->persist_cooldown == 0)
        h->persistent = true;                 // the give-up is not for good: whatever serialised the kernels may be gone
    int rc = analyze_device_locked(h, d_pcm, sample_offsets, n_clips, rake_sensitivity, stages, dout, stream_v, sync);
    // The default pass size was taken from the device memory free when the handle was created; other handles, the caller's
    // own buffers or a second workspace may have taken it since: on an allocation failure the passes are halved (down to
    // 2^21 frames) and the call planned again.
    while (rc == AEGIS_ERR_NOMEM && h->max_frames_per_pass > ((int64_t)1 << 21)) {
        (void)hipDeviceSynchronize();
        (void)hipGetLastError();
        h->max_frames_per_pass = std::max<int64_t>((int64_t)1 << 21, h->max_frames_per_pass / 2);
        rc = analyze_device_locked(h, d_pcm, sample_offsets, n_clips, rake_sensitivity, stages, dout, stream_v, sync);
    }
    if (rc != AEGIS_OK && h->persist_gave_up) {
        // The single Viterbi launch of a balanced pass found the frame stage not running beside it (a profiler collecting
        // counters serialises kernels, for one): this handle goes back to one launch per chunk for the next 16 calls and
        // the call is repeated.
        h->persist_gave_up = false;
        h->persistent = false;
        h->persist_cooldown = 16;
        ++h->persistent_fallbacks;
        rc = analyze_device_locked(h, d_pcm, sample_offsets, n_clips, rake_sensitivity, stages, dout, stream_v, sync);
    }
    return rc;
    } catch (...) { return abi_fail(h); }
}

// the last call's plan: its last pass, and the workspace that pass used
static const PassPlan *last_pass(const aegis_handle *h) { return h->plan.passes.empty() ? nullptr : &h->plan.passes.back(); }
static int last_work(const aegis_handle *h) { return h->plan.passes.empty() ? 0 : (int)((h->plan.passes.size() - 1) & 1); }

// After a synchronisation: a persistent Viterbi launch that gave up waiting for its chunk flags says so here.
static int persistent_check(aegis_handle *h) {
    if (!h->persist_pending) return AEGIS_OK;
    h->persist_pending = false;
    uint32_t aborted = 0;
    HIPCHK(h, hipMemcpy(&aborted, h->abort_flag.p, 4, hipMemcpyDeviceToHost));
    if (aborted) {
        HIPCHK(h, hipMemset(h->abort_flag.p, 0, 4));
        h->err = "the Viterbi kernel gave up waiting for the frame stage (AEGIS_VITERBI_PERSISTENT=0 launches it per chunk)";
        h->persist_gave_up = true;
        return AEGIS_ERR_DEVICE;
    }
    return AEGIS_OK;
}

// After a synchronisation: the verdict of AEGIS_OPT_CHECK_FINITE (librosa.util.valid_audio's ParameterError).
static int finite_result(aegis_handle *h, uint32_t opts, const int64_t *sample_offsets, int32_t n_clips) {
    if (!(opts & AEGIS_OPT_CHECK_FINITE) || !h->finite_flag.p) return AEGIS_OK;
    unsigned long long bad = ~0ull;
    HIPCHK(h, hipMemcpy(&bad, h->finite_flag.p, 8, hipMemcpyDeviceToHost));
    if (bad == ~0ull) return AEGIS_OK;
    const int64_t idx = sample_offsets[0] + (int64_t)bad;
    int clip = 0;
    while (clip + 1 < n_clips && sample_offsets[clip + 1] <= idx) ++clip;
    h->err = "Audio buffer is not finite everywhere (clip " + std::to_string(clip) + ", sample " + std::to_string(idx - sample_offsets[clip]) + ")";
    return AEGIS_ERR_INVALID;
}

// After a time-split pass has finished (its done event, or the call's synchronisation): the clips whose decode the
// verification kernel could not certify (or whose lock-on run never met the speculative run) are decoded again by the
// sequential kernel, and the pass is decoded into the outputs once more.  Rare (a near-tie on the decoded path that
// involves a voiced state; a boundary inside a long stretch without a voiced note).
static int split_check(aegis_handle *h, const aegis_handle::SplitCheck &sc, hipStream_t s) {
    const Tables &t = h->tab;
    const PassPlan &m = h->plan.passes[sc.pass];
    const int nc = m.nc();
    std::vector<uint32_t> flags((size_t)nc);
    HIPCHK(h, hipMemcpy(flags.data(), sc.p.clip_flag, (size_t)nc * 4, hipMemcpyDeviceToHost));
    std::vector<int32_t> redo;
    h->last_split_flags.assign(flags.begin(), flags.end());
    for (int i = 0; i < nc; ++i)
        if (flags[i]) { redo.push_back(i); if (flags[i] & 1u) ++h->split_stats[3]; }
    uint32_t counts[2] = {0, 0};
    HIPCHK(h, hipMemcpy(counts, sc.p.tube_count, 8, hipMemcpyDeviceToHost));
    h->last_carried_steps = counts[1];
    // The planning rule's estimate against the clock.  A split pass's Viterbi kernels come behind its frame stage, and their
    // time depends on the material: a lock-on run that never meets the speculative one runs its whole segment, and the
    // segments behind it speculate again (one more segment time per round).  When frame stage + measured Viterbi time is
    // not clearly below what the pass would have taken sequentially twice in a row, the next 32 calls of this handle plan
    // their passes sequentially.  Once per call, at its last split pass: from its first split pass's Viterbi kernels to its
    // last's.
    bool last_split = true;
    for (size_t j = (size_t)sc.pass + 1; j < h->plan.passes.size(); ++j) last_split = last_split && !h->plan.passes[j].tsplit;
    if (m.split_auto && h->split_ev[1] && last_split) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, h->split_ev[0], h->split_ev[1]) == hipSuccess) {
            h->last_split_viterbi_ms = ms;
            if (!split_clock_pays(h->plan, ms)) { if (++h->split_bad >= 2) { h->split_cooldown = 32; h->split_bad = 0; } }
            else h->split_bad = 0;
        }
    }
    if (redo.empty()) return AEGIS_OK;
    h->split_stats[2] += (int64_t)redo.size();
    if (m.split_auto) {
        // the redo is sequential and comes on top of the split pass: when it costs too much of what the pass would have
        // taken sequentially (material without voiced notes never locks on and keeps its tubes open: noise, silence), the
        // next 32 calls of this handle plan their passes sequentially
        int64_t redoF = 0;
        for (int i : redo) redoF = std::max(redoF, m.frames(i));
        if (!split_redo_pays(m, redoF, t.half_width)) h->split_cooldown = 32;
    }
    aegis_handle::Work &w = h->work[sc.pass & 1];
    HIPCHK(h, hipMemcpy(w.flag_order.p, redo.data(), redo.size() * 4, hipMemcpyHostToDevice));
    PassParams q = sc.p;
    q.order = static_cast<const int32_t *>(w.flag_order.p);
    q.n_clips = (int32_t)redo.size();
    q.vt_begin = 0; q.vt_end = INT64_MAX; q.clip_t0 = nullptr; q.clip_t1 = nullptr; q.chunk_flag = nullptr; q.dense = 0;
    hipError_t ve = launch_viterbi(q, h->dt, t.log_trans_band.data(), s);
    if (ve != hipSuccess) { h->err = std::string("viterbi launch: ") + hipGetErrorString(ve); return AEGIS_ERR_DEVICE; }
    launch_decode(sc.p, h->dt, s);
    HIPCHK(h, hipStreamSynchronize(s));
    return AEGIS_OK;
}

// The Viterbi workgroups (one CU per clip, latency-bound) lose a fifth of their speed when frame-stage workgroups run on
// NEIGHBOURING compute units: the kernels' code (19 + 31 + 48 KB) does not fit the instruction cache a CU shares with
// its neighbour (measured: Viterbi 77.5 ms beside the frame stage, 67.9 ms with the frame stage confined to 192 CUs;
// keeping frame workgroups off the Viterbi's own CU alone changed nothing).  While a batch leaves CUs free the pipeline
// therefore runs on CU-masked streams: the Viterbi on the last V CUs of the mask, the frame stage on the others.
static aegis_handle::SplitSet *split_streams(aegis_handle *h, int n_clips) {
    if (!masked_streams_fit(h->knobs, h->n_cus, n_clips)) return nullptr;
    const int idx = n_clips <= 64 ? 0 : 1;
    aegis_handle::SplitSet &ss = h->split[idx];
    if (!ss.tried) {
        ss.tried = true;
        const int v = idx == 0 ? 64 : 128;
        uint32_t fm[8], vm[8];
        for (int w = 0; w < 8; ++w) { fm[w] = 0; vm[w] = 0; }
        for (int i = 0; i < 256; ++i) {
            if (i < 256 - v) fm[i >> 5] |= 1u << (i & 31);
            if (i >= 256 - v) vm[i >> 5] |= 1u << (i & 31);
        }
        if (hipExtStreamCreateWithCUMask(&ss.frame_a, 8, fm) != hipSuccess || hipExtStreamCreateWithCUMask(&ss.frame_b, 8, fm) != hipSuccess ||
            hipExtStreamCreateWithCUMask(&ss.viterbi, 8, vm) != hipSuccess) {
            (void)hipGetLastError();
            for (hipStream_t *q : {&ss.frame_a, &ss.frame_b, &ss.viterbi}) { if (*q) (void)hipStreamDestroy(*q); *q = nullptr; }
        }
    }
    return ss.viterbi ? &ss : nullptr;
}

// What the planner needs to know about a call.  masked: whether a CU-masked stream set exists for n clips (the executor
// creates them through split_streams; aegis_debug_plan only asks whether they would be laid out).
static PlanInput plan_input(aegis_handle *h, const int64_t *sample_offsets, int32_t n_clips, uint32_t stages, bool feed,
                            bool caller_stream, int32_t sync, int n_cus, std::function<bool(int)> masked) {
    const Tables &t = h->tab;
    PlanInput in;
    in.sample_offsets.assign(sample_offsets, sample_offsets + n_clips + 1);
    in.max_frames_per_pass = h->max_frames_per_pass;
    in.n_cus = n_cus; in.hop = t.hop; in.half_width = t.half_width;
    in.py = stages & AEGIS_STAGE_PYIN;
    in.feed = feed; in.caller_stream = caller_stream; in.sync = sync;
    DevTables dt = h->dt;      // (a host-only handle: the packed table the device would hold)
    if (h->device < 0 && !t.log_trans_pack.empty()) dt.lt_pack = t.log_trans_pack.data();
    in.band_applies = viterbi_band_applies(base_params(t), dt);
    in.split_applies = viterbi_split_applies(base_params(t), dt);
    in.masked_streams = std::move(masked);
    in.knobs = h->knobs;
    in.persistent = h->persistent;
    if (split_allowed(in) && in.knobs.split_seglen < 0 && h->split_cooldown > 0) in.cooling = true;
    return in;
}

static int ensure_pass(aegis_handle *h, aegis_handle::Work &w, const PassPlan &m, uint32_t stages) {
    const int64_t nc = m.nc(), nk = m.nk(), fp = m.fp, S = 2 * h->tab.n_bins, nchunks = m.chunk_off[nc];
    int rc;
#define ENS(buf, bytes) if ((rc = ensure(h, w.buf, (size_t)(bytes))) != AEGIS_OK) return rc
    ENS(sample_off, nc * 8); ENS(sample_len, nc * 8); ENS(out_off, nc * 8); ENS(frame_off, (nc + 1) * 8);
    ENS(order, nc * 4); ENS(chunk_off, (nc + 1) * 8); ENS(sel_off, (size_t)nk * (nc + 1) * 8);
    if (stages & AEGIS_STAGE_PYIN) {
        ENS(dfn, fp * h->lag_stride * 8); if (h->debug_stages) ENS(yin, fp * h->yin_stride * 8);
        ENS(logobs, fp * h->obs_stride * 8); ENS(logunv, fp * 8); ENS(obs_seg, fp * 4);
        ENS(ptr, fp * S * 2); ENS(cmap, (nchunks + 1) * S * 2); ENS(bnd, (nchunks + 1) * 4);
        ENS(states, fp * 4); ENS(vstate, (size_t)nc * S * 8);
        ENS(chunk_lo, (size_t)nk * 8); ENS(chunk_flag, (size_t)nk * 4);
        if (m.proportional) ENS(clip_tb, (size_t)(nk + 1) * nc * 8);
        if (m.tsplit) {
            const int64_t n_seg = m.n_seg;
            ENS(seg64, m.seg64.size() * 8); ENS(seg32, m.seg32.size() * 4);
            ENS(seg_col, (size_t)2 * n_seg * S * 8); ENS(seg_map, (size_t)n_seg * S * 2); ENS(seg_i32, ((size_t)n_seg * 3 + 2 * nc) * 4);
            ENS(colhist, (size_t)fp * S * 8); ENS(colG, (size_t)fp * 8); ENS(colkg, (size_t)fp * 4); ENS(clip_flag, (size_t)nc * 4);
            ENS(flag_order, (size_t)nc * 4);
            ENS(tube_buf, (size_t)m.tube_cap * viterbi_tube_record_ints() * 4); ENS(tube_at, (size_t)fp * 4); ENS(tube_count, 8);
        }
    }
    if (stages & AEGIS_STAGE_MEL) { ENS(melpow, fp * h->tab.n_mels * 4); ENS(clipmax, nc * 4); ENS(rake_raw, fp); }
#undef ENS
    return AEGIS_OK;
}

// the plan's host arrays into the workspace, and the device state a pass starts from (on stream fa)
static int upload_pass(aegis_handle *h, aegis_handle::Work &w, const PassPlan &m, uint32_t stages, hipStream_t fa) {
    const size_t nc = m.nc(), nk = m.nk();
    auto up = [&](DevBuf &b, const auto &v) { return hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice, fa); };
    HIPCHK(h, up(w.sample_off, m.sample_off)); HIPCHK(h, up(w.sample_len, m.sample_len)); HIPCHK(h, up(w.out_off, m.out_off));
    HIPCHK(h, up(w.frame_off, m.frame_off)); HIPCHK(h, up(w.chunk_off, m.chunk_off)); HIPCHK(h, up(w.order, m.order));
    HIPCHK(h, up(w.sel_off, m.sel_off));
    if (m.proportional) HIPCHK(h, up(w.clip_tb, m.clip_tb));
    if (stages & AEGIS_STAGE_MEL) HIPCHK(h, hipMemsetAsync(w.clipmax.p, 0, nc * 4, fa));
    if (m.tsplit) {
        HIPCHK(h, up(w.seg64, m.seg64)); HIPCHK(h, up(w.seg32, m.seg32));
        HIPCHK(h, hipMemsetAsync(w.seg_i32.p, 0, ((size_t)m.n_seg * 3 + 2 * nc) * 4, fa));       // seg_lock = 0 for the segments without a lock-on run
        HIPCHK(h, hipMemsetAsync(w.clip_flag.p, 0, nc * 4, fa));
        HIPCHK(h, hipMemsetAsync(w.tube_at.p, 0, (size_t)m.fp * 4, fa));
        HIPCHK(h, hipMemsetAsync(w.tube_count.p, 0, 8, fa));       // tubes recorded, rounds of second speculation that had work
    }
    if (m.persistent) {
        if (!h->abort_flag.p) {
            int rc;
            if ((rc = ensure(h, h->abort_flag, 4)) != AEGIS_OK) return rc;
            HIPCHK(h, hipMemsetAsync(h->abort_flag.p, 0, 4, fa));
        }
        HIPCHK(h, up(w.chunk_lo, m.chunk_lo));
        HIPCHK(h, hipMemsetAsync(w.chunk_flag.p, 0, nk * 4, fa));       // generations start at 1
    }
    return AEGIS_OK;
}

// The kernels' view of a pass: the workspace's buffers, the call's outputs, the plan's geometry.
static PassParams bind_pass(const aegis_handle *h, const PassPlan &m, const aegis_handle::Work &w, const float *d_pcm,
                            uint32_t stages, uint32_t opts, const aegis_outputs *dout, double rake_sensitivity) {
    const Tables &t = h->tab;
    const bool py = stages & AEGIS_STAGE_PYIN, mel = stages & AEGIS_STAGE_MEL;
    const int nc = m.nc(), n_seg = m.n_seg, S = 2 * t.n_bins;
    PassParams p = base_params(t);
    p.stages = stages;
    p.pcm = d_pcm;
    p.sample_off = static_cast<const int64_t *>(w.sample_off.p);
    p.sample_len = static_cast<const int64_t *>(w.sample_len.p);
    p.frame_off = static_cast<const int64_t *>(w.frame_off.p);
    p.out_off = static_cast<const int64_t *>(w.out_off.p);
    p.order = static_cast<const int32_t *>(w.order.p);
    p.n_clips = nc; p.n_frames = m.fp;
    p.dfn = static_cast<double *>(w.dfn.p); p.lag_stride = h->lag_stride;
    p.yin = (py && h->debug_stages) ? static_cast<double *>(w.yin.p) : nullptr; p.yin_stride = h->yin_stride;
    p.cmnd_in_frame = cmnd_in_frame(h); p.troughs = troughs_in_frame(h);
    p.logobs = static_cast<double *>(w.logobs.p); p.obs_stride = h->obs_stride;
    p.logunv = static_cast<double *>(w.logunv.p);
    p.obs_seg = static_cast<int32_t *>(w.obs_seg.p);
    p.ptr = static_cast<uint16_t *>(w.ptr.p);
    p.cmap = static_cast<uint16_t *>(w.cmap.p);
    p.chunk_off = static_cast<int64_t *>(w.chunk_off.p);
    p.bnd = static_cast<int32_t *>(w.bnd.p);
    p.states = static_cast<int32_t *>(w.states.p);
    p.melpow = static_cast<float *>(w.melpow.p);
    p.clipmax = static_cast<uint32_t *>(w.clipmax.p);
    p.rake_raw = static_cast<uint8_t *>(w.rake_raw.p);
    p.vstate = static_cast<double *>(w.vstate.p);
    p.vstats = static_cast<unsigned long long *>(h->vstats.p);
    p.out_f0 = py ? dout->f0 : nullptr;
    p.out_voiced = py ? dout->voiced_flag : nullptr;
    p.out_vprob = py ? dout->voiced_prob : nullptr;
    p.out_bin = py ? dout->pitch_bin : nullptr;
    p.out_rms = (stages & AEGIS_STAGE_RMS) ? dout->rms : nullptr;
    p.out_rake = (stages & AEGIS_STAGE_RAKE) ? dout->rake_mask : nullptr;
    p.out_sdb = mel ? dout->S_dB : nullptr;
    p.out_colmean = mel ? dout->sdb_col_means : nullptr;
    p.out_total = h->plan.total_frames;
    p.rake_ratio = rake_sensitivity;
    const double ms_per_frame = ((double)t.hop / (double)t.sr) * 1000;      // vision.py:23-25
    p.rake_min_frames = (int)(10 / ms_per_frame); p.rake_max_frames = (int)(30 / ms_per_frame);
    if (opts & AEGIS_OPT_F0_ZERO) p.f0_unvoiced = 0.0;
    p.dense = m.dense ? 1 : 0;
    if (m.tsplit) {
        const int64_t *g64 = static_cast<const int64_t *>(w.seg64.p);
        const int32_t *g32 = static_cast<const int32_t *>(w.seg32.p);
        p.seg_f0 = g64; p.seg_ch0 = g64 + n_seg;
        p.vf_off = g64 + 2 * n_seg; p.vf_total = m.seg64.back();
        p.seg_T = g32; p.seg_store = g32 + n_seg; p.seg_prev = g32 + 2 * n_seg; p.seg_clip = g32 + 3 * n_seg;
        p.clip_seg0 = g32 + 4 * n_seg;
        p.seg_col = static_cast<double *>(w.seg_col.p); p.seg_col2 = p.seg_col + (size_t)n_seg * S;
        p.seg_map = static_cast<uint16_t *>(w.seg_map.p);
        p.seg_kg = static_cast<int32_t *>(w.seg_i32.p); p.seg_lock = p.seg_kg + n_seg; p.seg_end = p.seg_kg + 2 * n_seg; p.clip_first = p.seg_kg + 3 * n_seg; p.clip_dirty = p.clip_first + nc;
        p.colhist = static_cast<double *>(w.colhist.p); p.colG = static_cast<double *>(w.colG.p); p.colkg = static_cast<int32_t *>(w.colkg.p);
        p.clip_flag = static_cast<uint32_t *>(w.clip_flag.p);
        p.tube_buf = static_cast<int32_t *>(w.tube_buf.p); p.tube_cap = m.tube_cap; p.tube_count = static_cast<uint32_t *>(w.tube_count.p);
        p.tube_at = static_cast<int32_t *>(w.tube_at.p);
        p.n_seg = n_seg;
    }
    if (m.persistent) {
        p.chunk_flag = static_cast<const uint32_t *>(w.chunk_flag.p);
        p.chunk_lo = static_cast<const int64_t *>(w.chunk_lo.p);
        p.n_chunks = m.nk();
        if (m.hybrid) { int ks = 0; while (ks < m.nk() && m.cb[ks] <= m.hyb_S) ++ks; p.n_chunks = ks; }      // (the launch ends at step S: chunks 0 .. ks - 1)
        p.abort_flag = static_cast<uint32_t *>(h->abort_flag.p);
        // bound of one chunk wait: a chunk's frame stage takes well under a millisecond per 10 k frames, so 0.1 s plus
        // 0.1 s per million frames of the pass is two orders of magnitude of slack, and a pass that cannot overlap
        // (kernels serialised) costs that much once instead of 1.5 s
        p.wait_ticks = (uint64_t)std::min<int64_t>(150000000, 10000000 + m.fp * 10);
    }
    return p;
}

static hipStream_t lane_stream(const aegis_handle *h, Lane l, hipStream_t s, const aegis_handle::SplitSet *ss) {
    switch (l) {
    case Lane::main: return s;
    case Lane::frame2: return h->stream4;
    case Lane::viterbi2: return h->stream2;
    case Lane::masked_frame_a: return ss->frame_a;
    case Lane::masked_frame_b: return ss->frame_b;
    case Lane::masked_viterbi: return ss->viterbi;
    default: return nullptr;
    }
}

#define VCHK(expr) do { hipError_t ve__ = (expr); if (ve__ != hipSuccess) { h->err = std::string("viterbi launch: ") + hipGetErrorString(ve__); return AEGIS_ERR_DEVICE; } } while (0)

static int analyze_device_locked(aegis_handle *h, const float *d_pcm, const int64_t *sample_offsets,
                                 int32_t n_clips, double rake_sensitivity, uint32_t stages,
                                 aegis_outputs *dout, void *stream_v, int32_t sync, HostFeed *feed) {
    // ---- validate -----------------------------------------------------------------------------------------------------
    if (!h) return AEGIS_ERR_INVALID;
    if (n_clips < 0 || (n_clips > 0 && (!sample_offsets || !dout))) { h->err = "null argument"; return AEGIS_ERR_INVALID; }
    if (n_clips == 0) return AEGIS_OK;
    if (stages & AEGIS_STAGE_RAKE) stages |= AEGIS_STAGE_MEL;
    const uint32_t opts = stages & (AEGIS_OPT_CHECK_FINITE | AEGIS_OPT_F0_ZERO);
    stages &= AEGIS_STAGE_ALL;
    if ((opts & AEGIS_OPT_CHECK_FINITE) && sync == 0) {      // the verdict is read after a synchronisation: nobody would read it
        h->err = "AEGIS_OPT_CHECK_FINITE needs sync != 0 (the verdict is reported by the call that synchronises)";
        return AEGIS_ERR_INVALID;
    }
    const Tables &t = h->tab;
    if (h->device < 0) { h->err = "handle was created with device=-1 (host tables only)"; return AEGIS_ERR_DEVICE; }
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = stream_v ? static_cast<hipStream_t>(stream_v) : h->stream;
    for (int i = 0; i < n_clips; ++i) {
        const int64_t n = sample_offsets[i + 1] - sample_offsets[i];
        if (n < 0) { h->err = "sample_offsets must be non-decreasing"; return AEGIS_ERR_INVALID; }
        if (n > 0 && !d_pcm) { h->err = "d_pcm == NULL"; return AEGIS_ERR_INVALID; }
        if (1 + n / t.hop > h->max_frames_per_pass) {
            h->err = "clip of " + std::to_string(1 + n / t.hop) + " frames exceeds max_frames_per_pass=" +
                     std::to_string(h->max_frames_per_pass);
            return AEGIS_ERR_INVALID;
        }
    }
    // host arrays of the previous call's plan are no longer referenced once the stream drained
    if (h->plan_in_flight) { HIPCHK(h, hipStreamSynchronize(s)); h->plan_in_flight = false; }
    h->split_checks.clear();
    if (h->profiling) { for (auto &ev : h->events) { (void)hipEventDestroy(ev.second.first); (void)hipEventDestroy(ev.second.second); } h->events.clear(); }

    // ---- plan ---------------------------------------------------------------------------------------------------------
    const PlanInput in = plan_input(h, sample_offsets, n_clips, stages, feed != nullptr, stream_v != nullptr, sync, h->n_cus,
                                    [h](int n) { return split_streams(h, n) != nullptr; });
    if (in.cooling) --h->split_cooldown;
    h->plan = plan_call(in);
    h->plan_in_flight = true;
    const bool py = in.py;

    while (h->sync_events.size() < 8) {
        hipEvent_t e;
        HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->sync_events.push_back(e);
    }
    // fixed slots of sync_events: 0 call start, 1/2 pass done (workspace parity), 3 frame_b joined, 4 frame_a final, 5.. per chunk
    enum { EV_START = 0, EV_DONE0 = 1, EV_DONE1 = 2, EV_FB = 3, EV_FA = 4, EV_META = 5, EV_CHUNK0 = 6 };
    bool done_recorded[2] = {false, false}, split_started = false;
    std::vector<hipStream_t> joined;          // streams whose work s must wait for before the call returns
    for (int pi = 0; pi < (int)h->plan.passes.size(); ++pi) {
        const PassPlan &m = h->plan.passes[pi];
        const int nc = m.nc(), nk = m.nk();
        aegis_handle::Work &w = h->work[pi & 1];
        int rc;
        // ---- wait for the workspace: a split verdict of the pass two back is read (and acted on) before anything
        // overwrites it or ensure() moves its buffers
        if (!h->split_checks.empty() && h->split_checks.front().pass == pi - 2) {
            HIPCHK(h, hipEventSynchronize(h->sync_events[EV_DONE0 + (pi & 1)]));
            const aegis_handle::SplitCheck sc = h->split_checks.front();
            h->split_checks.erase(h->split_checks.begin());
            if ((rc = split_check(h, sc, s)) != AEGIS_OK) return rc;
        }
        const aegis_handle::SplitSet *ss = m.fa == Lane::masked_frame_a ? split_streams(h, nc) : nullptr;
        hipStream_t fa = lane_stream(h, m.fa, s, ss), fb = lane_stream(h, m.fb, s, ss), sv = lane_stream(h, m.sv, s, ss);
        hipStream_t sd = lane_stream(h, m.sd, s, ss), sa = lane_stream(h, m.sa, s, ss);
        while ((int)h->sync_events.size() < EV_CHUNK0 + nk) {
            hipEvent_t e;
            HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
            h->sync_events.push_back(e);
        }
        auto join_later = [&](hipStream_t q) { if (q != s && std::find(joined.begin(), joined.end(), q) == joined.end()) joined.push_back(q); };
        if (pi == 0) HIPCHK(h, hipEventRecord(h->sync_events[EV_START], s));
        for (hipStream_t q : {fa, fb, sv, sd, sa}) {
            if (q == s || q == nullptr) continue;
            if (std::find(joined.begin(), joined.end(), q) == joined.end())
                HIPCHK(h, hipStreamWaitEvent(q, h->sync_events[EV_START], 0));      // the caller's earlier work on s comes first
            // this workspace was last used two passes ago: everything of that pass must have finished
            if (done_recorded[pi & 1]) HIPCHK(h, hipStreamWaitEvent(q, h->sync_events[EV_DONE0 + (pi & 1)], 0));
        }
        if (fa == s && done_recorded[pi & 1]) HIPCHK(h, hipStreamWaitEvent(s, h->sync_events[EV_DONE0 + (pi & 1)], 0));
        join_later(fa); join_later(sv); if (m.use_fb) join_later(fb); if (sd) { join_later(sd); join_later(sa); }

        // ---- workspace ----------------------------------------------------------------------------------------------
        if ((rc = ensure_pass(h, w, m, stages)) != AEGIS_OK) return rc;
        if ((rc = upload_pass(h, w, m, stages, fa)) != AEGIS_OK) return rc;
        if (m.use_fb || m.persistent) {      // the metadata precedes the second frame stream's kernels and the Viterbi
            HIPCHK(h, hipEventRecord(h->sync_events[EV_META], fa));
            if (m.use_fb) HIPCHK(h, hipStreamWaitEvent(fb, h->sync_events[EV_META], 0));
            if (m.persistent) HIPCHK(h, hipStreamWaitEvent(sv, h->sync_events[EV_META], 0));
        }
        PassParams p = bind_pass(h, m, w, d_pcm, stages, opts, dout, rake_sensitivity);
        const int32_t *d_seg_order = m.tsplit ? p.clip_seg0 + nc + 1 : nullptr, *d_lock_order = d_seg_order ? d_seg_order + m.n_seg : nullptr;
        if (m.persistent) {
            p.chunk_gen = ++h->chunk_gen;
            if (p.chunk_gen == 0) p.chunk_gen = ++h->chunk_gen;
            h->persist_pending = true;
        }

        // ---- time chunks: frame stage, then the Viterbi behind it -----------------------------------------------------
        for (int k = 0; k < nk; ++k) {
            hipStream_t fs = ((m.two_fs || k < m.ramp_k) && (k & 1)) ? fb : fa;
            p.sel_off = static_cast<const int64_t *>(w.sel_off.p) + (size_t)k * (nc + 1);
            p.t_begin = m.cb[k];
            p.n_sel = m.sel_off[(size_t)k * (nc + 1) + nc];
            p.vt_begin = m.cb[k];
            p.vt_end = (k == nk - 1) ? INT64_MAX : m.cb[k + 1];
            p.clip_t0 = m.proportional ? static_cast<const int64_t *>(w.clip_tb.p) + (size_t)k * nc : nullptr;
            p.clip_t1 = m.proportional ? static_cast<const int64_t *>(w.clip_tb.p) + (size_t)(k + 1) * nc : nullptr;
            if (feed && feed->raw) {      // the same samples, decoded on the device from the raw bytes
                std::vector<int32_t> cis((size_t)nc);
                std::vector<int64_t> need((size_t)nc);
                bool any = false;
                for (int i = 0; i < nc; ++i) {
                    const int64_t n = m.sample_len[i];
                    cis[(size_t)i] = m.clips[i];
                    need[(size_t)i] = (k == nk - 1) ? n : std::min(n, (m.clip_hi(k, i) - 1) * (int64_t)t.hop + t.n_fft / 2);
                    any = any || need[(size_t)i] > feed->copied[(size_t)m.clips[i]];
                }
                if (any) {
                    if ((rc = pcm_feed(h, *feed, cis, need)) != AEGIS_OK) return rc;
                    HIPCHK(h, hipEventRecord(h->copy_event, h->stream3));
                    HIPCHK(h, hipStreamWaitEvent(fs, h->copy_event, 0));
                }
            } else if (feed) {      // frame t reads samples [t*hop - 1024, t*hop + 1024)
                bool any = false;
                for (int i = 0; i < nc; ++i) {
                    const int ci = m.clips[i];
                    const int64_t n = m.sample_len[i];
                    const int64_t need = (k == nk - 1) ? n : std::min(n, (m.clip_hi(k, i) - 1) * (int64_t)t.hop + t.n_fft / 2);
                    int64_t &done = feed->copied[ci];
                    if (need > done) {
                        HIPCHK(h, hipMemcpyAsync(feed->dst + m.sample_off[i] + done, feed->pcm[ci] + done,
                                                 (size_t)(need - done) * 4, hipMemcpyHostToDevice, h->stream3));
                        done = need;
                        any = true;
                    }
                }
                if (any) {
                    HIPCHK(h, hipEventRecord(h->copy_event, h->stream3));
                    HIPCHK(h, hipStreamWaitEvent(fs, h->copy_event, 0));
                }
            }
            begin_event(h, "frame", fs); launch_frame(p, h->dt, fs); end_event(h, fs);
            if (!py) continue;
            begin_event(h, "pyin_obs", fs); launch_pyin_obs(p, h->dt, fs); end_event(h, fs);
            if (m.persistent) {
                if (k != h->test_drop_signal)      // AEGIS_TEST_DROP_CHUNK_SIGNAL=k: the kernel's bounded wait is tested with it
                    launch_chunk_signal(static_cast<uint32_t *>(w.chunk_flag.p) + k, p.chunk_gen, fs);
                if (k == 0) {        // the one launch, ordered behind chunk 0 (its first column reads frame 0)
                    HIPCHK(h, hipEventRecord(h->sync_events[EV_CHUNK0], fs));
                    HIPCHK(h, hipStreamWaitEvent(sv, h->sync_events[EV_CHUNK0], 0));
                    PassParams pv = p;
                    pv.vt_begin = 0; pv.vt_end = m.hybrid ? m.hyb_S + 1 : INT64_MAX;
                    begin_event(h, "viterbi", sv);
                    hipError_t ve = launch_viterbi(pv, h->dt, t.log_trans_band.data(), sv);
                    end_event(h, sv);
                    VCHK(ve);
                }
                continue;
            }
            if (m.tsplit && !m.hybrid && k < nk - 1) continue;      // the segments are launched once, behind the last chunk's observations
            if (m.hybrid && m.cb[k] > m.hyb_S) continue;            // (hybrid: behind step S the segments take over, launched after the loop)
            if (sv != fs) {
                HIPCHK(h, hipEventRecord(h->sync_events[EV_CHUNK0 + k], fs));
                HIPCHK(h, hipStreamWaitEvent(sv, h->sync_events[EV_CHUNK0 + k], 0));
            }
            begin_event(h, "viterbi", sv);
            const bool split_now = m.tsplit && !m.hybrid;
            if (split_now && m.split_auto) {
                for (auto &e : h->split_ev) if (!e) HIPCHK(h, hipEventCreate(&e));
                if (!split_started) { HIPCHK(h, hipEventRecord(h->split_ev[0], sv)); split_started = true; }
            }
            if (split_now) for (auto &e : h->fin_ev) if (!e) HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
            hipError_t ve = split_now ? launch_viterbi_split(p, h->dt, t.log_trans_band.data(), d_seg_order, m.n_seg, d_lock_order, m.n_lock, sv,
                                                             h->stream4 != sv ? h->stream4 : nullptr, h->fin_ev)
                                      : launch_viterbi(p, h->dt, t.log_trans_band.data(), sv);
            if (split_now && m.split_auto) HIPCHK(h, hipEventRecord(h->split_ev[1], sv));
            end_event(h, sv);
            VCHK(ve);
            if (split_now) { h->split_checks.push_back({pi, p}); ++h->split_stats[0]; h->split_stats[1] += m.n_seg; }
        }
        if (m.use_fb) {                    // the dB / rake finalisation needs every chunk's mel rows and clip maxima
            HIPCHK(h, hipEventRecord(h->sync_events[EV_FB], fb));
            HIPCHK(h, hipStreamWaitEvent(fa, h->sync_events[EV_FB], 0));
        }
        if (m.hybrid) {
            // the segments behind step S: after the last chunk's observations (fa; fb has joined it above) and the sequential
            // kernel's last launch (sv), on the unmasked stream
            for (auto &e : h->hyb_ev) if (!e) HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
            PassParams ph = p;
            ph.split_hybrid = 1; ph.hybrid_step = (int32_t)m.hyb_S;
            ph.vt_begin = 0; ph.vt_end = INT64_MAX;
            // the speculative runs need the observations only: they start behind the frame stage, on the compute units it has
            // left, while the sequential kernel walks its last chunks; lock-on runs and everything after wait for both
            if (sa != fa) {
                HIPCHK(h, hipEventRecord(h->hyb_ev[0], fa));
                HIPCHK(h, hipStreamWaitEvent(sa, h->hyb_ev[0], 0));
            }
            VCHK(launch_viterbi_split_spec(ph, h->dt, t.log_trans_band.data(), d_seg_order, m.n_lock, sa));
            HIPCHK(h, hipEventRecord(h->hyb_ev[2], sa));
            if (sd != sv) {
                HIPCHK(h, hipEventRecord(h->hyb_ev[1], sv));
                HIPCHK(h, hipStreamWaitEvent(sd, h->hyb_ev[1], 0));
            }
            HIPCHK(h, hipStreamWaitEvent(sd, h->hyb_ev[2], 0));
            begin_event(h, "viterbi", sd);
            if (m.split_auto) {
                for (auto &e : h->split_ev) if (!e) HIPCHK(h, hipEventCreate(&e));
                if (!split_started) { HIPCHK(h, hipEventRecord(h->split_ev[0], sd)); split_started = true; }
            }
            for (auto &e : h->fin_ev) if (!e) HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
            hipError_t ve = launch_viterbi_split(ph, h->dt, t.log_trans_band.data(), d_seg_order, 0, d_lock_order, m.n_lock, sd, h->stream4, h->fin_ev);
            if (m.split_auto) HIPCHK(h, hipEventRecord(h->split_ev[1], sd));
            end_event(h, sd);
            VCHK(ve);
            h->split_checks.push_back({pi, ph});
            ++h->split_stats[0]; h->split_stats[1] += m.n_seg;
        }
        // ---- finalize ---------------------------------------------------------------------------------------------------
        hipStream_t se = m.hybrid ? sd : sv;       // the stream the pass ends on
        begin_event(h, "finalize", fa); launch_finalize_mel(p, h->dt, fa); end_event(h, fa);
        if (py) { begin_event(h, "finalize", se); launch_decode(p, h->dt, se); end_event(h, se); }
        // pass done = its last kernels on the frame stream and on the Viterbi stream
        if (se != fa) {
            HIPCHK(h, hipEventRecord(h->sync_events[EV_FA], fa));
            HIPCHK(h, hipStreamWaitEvent(se, h->sync_events[EV_FA], 0));
        }
        HIPCHK(h, hipEventRecord(h->sync_events[EV_DONE0 + (pi & 1)], se));
        done_recorded[pi & 1] = true;
        HIPCHK(h, hipGetLastError());
        if (feed && feed->raw && feed->raw->y_out) {      // the pass's samples back to the host, behind its last decode
            for (int i = 0; i < nc; ++i)
                if (m.sample_len[i] > 0)
                    HIPCHK(h, hipMemcpyAsync(feed->raw->y_out + m.sample_off[i], feed->dst + m.sample_off[i], (size_t)m.sample_len[i] * 4,
                                             hipMemcpyDeviceToHost, h->stream3));
        }
    }
    // ---- join: the caller's stream continues after everything enqueued above --------------------------------------------
    for (int q = 0; q < 2; ++q)
        if (done_recorded[q]) HIPCHK(h, hipStreamWaitEvent(s, h->sync_events[EV_DONE0 + q], 0));
    if (opts & AEGIS_OPT_CHECK_FINITE) {       // behind the last sample copy of a host feed: every sample is on the device by now
        int rc;
        if ((rc = ensure(h, h->finite_flag, 8)) != AEGIS_OK) return rc;
        HIPCHK(h, hipMemsetAsync(h->finite_flag.p, 0xff, 8, s));
        const int64_t lo = sample_offsets[0], hi = sample_offsets[n_clips];
        launch_finite_check(d_pcm + lo, hi - lo, static_cast<unsigned long long *>(h->finite_flag.p), s);
    }
    if (!h->split_checks.empty()) {         // (sync != 0: time-split passes are planned for blocking calls only)
        HIPCHK(h, hipStreamSynchronize(s));
        for (const auto &sc : h->split_checks) {
            const int rc = split_check(h, sc, s);
            if (rc != AEGIS_OK) return rc;
        }
        h->split_checks.clear();
    }
    if (sync == 1) {
        HIPCHK(h, hipStreamSynchronize(s));
        h->plan_in_flight = false;
        if (h->profiling) collect_events(h);
        int rc = persistent_check(h);
        if (rc != AEGIS_OK) return rc;
        return finite_result(h, opts, sample_offsets, n_clips);
    }
    return AEGIS_OK;
}
#undef VCHK

static int host_fed_locked(aegis_handle *h, const std::vector<int64_t> &off, int64_t F, int32_t n_clips, double rake_sensitivity,
                           uint32_t stages, aegis_outputs *out, const std::function<HostFeed()> &make_feed);

int aegis_analyze_batch(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips,
                        double rake_sensitivity, uint32_t stages, aegis_outputs *out) {
    try {
    if (!h) return AEGIS_ERR_INVALID;
    if (n_clips < 0 || (n_clips > 0 && (!pcm || !n_samples || !out))) { h->err = "null argument"; return AEGIS_ERR_INVALID; }
    if (n_clips == 0) return AEGIS_OK;
    if (stages & AEGIS_STAGE_RAKE) stages |= AEGIS_STAGE_MEL;
    if (h->device < 0) { h->err = "handle was created with device=-1 (host tables only)"; return AEGIS_ERR_DEVICE; }
    std::lock_guard<std::mutex> lock(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    std::vector<int64_t> off(n_clips + 1, 0);
    int64_t F = 0;
    for (int i = 0; i < n_clips; ++i) {
        if (n_samples[i] < 0 || (n_samples[i] > 0 && !pcm[i])) { h->err = "bad clip " + std::to_string(i); return AEGIS_ERR_INVALID; }
        // keep every clip 16-byte aligned in the packed device buffer
        off[i + 1] = off[i] + n_samples[i];
        F += 1 + n_samples[i] / h->tab.hop;
    }
    int rc;
    if ((rc = ensure(h, h->io_pcm, (size_t)std::max<int64_t>(off[n_clips], 1) * 4)) != AEGIS_OK) return rc;
    return host_fed_locked(h, off, F, n_clips, rake_sensitivity, stages, out, [&]() {
        return HostFeed{pcm, static_cast<float *>(h->io_pcm.p), std::vector<int64_t>((size_t)n_clips, 0)};
    });
    } catch (...) { return abi_fail(h); }
}

// The blocking host-fed analysis of aegis_analyze_batch and aegis_analyze_pcm (handle locked, io_pcm sized): the device
// outputs, the pipeline fed by make_feed() (a fresh feed for every attempt), the outputs back to the host.
static int host_fed_locked(aegis_handle *h, const std::vector<int64_t> &off, int64_t F, int32_t n_clips, double rake_sensitivity,
                           uint32_t stages, aegis_outputs *out, const std::function<HostFeed()> &make_feed) {
    int rc;
    hipStream_t s = h->stream;
    // the previous call's kernels may still read io_pcm only if it returned without a sync -- it never does
    if (!h->persistent && h->knobs.persistent_wanted && h->persist_cooldown > 0 && --h->persist_cooldown == 0)
        h->persistent = true;                 // as in aegis_analyze_batch_device: a give-up is not for good
    aegis_outputs d{};
    const int nm = h->tab.n_mels;
    if ((stages & AEGIS_STAGE_PYIN) && out->f0) { if ((rc = ensure(h, h->io_f0, F * 8))) return rc; d.f0 = static_cast<double *>(h->io_f0.p); }
    if ((stages & AEGIS_STAGE_PYIN) && out->voiced_flag) { if ((rc = ensure(h, h->io_voiced, F))) return rc; d.voiced_flag = static_cast<uint8_t *>(h->io_voiced.p); }
    if ((stages & AEGIS_STAGE_MEL) && out->sdb_col_means) { if ((rc = ensure(h, h->io_colmean, F * 12))) return rc; d.sdb_col_means = static_cast<float *>(h->io_colmean.p); }
    if ((stages & AEGIS_STAGE_PYIN) && out->pitch_bin) { if ((rc = ensure(h, h->io_bin, F * 2))) return rc; d.pitch_bin = static_cast<int16_t *>(h->io_bin.p); }
    if ((stages & AEGIS_STAGE_PYIN) && out->voiced_prob) { if ((rc = ensure(h, h->io_vprob, F * 8))) return rc; d.voiced_prob = static_cast<double *>(h->io_vprob.p); }
    if ((stages & AEGIS_STAGE_RMS) && out->rms) { if ((rc = ensure(h, h->io_rms, F * 4))) return rc; d.rms = static_cast<float *>(h->io_rms.p); }
    if ((stages & AEGIS_STAGE_RAKE) && out->rake_mask) { if ((rc = ensure(h, h->io_rake, F))) return rc; d.rake_mask = static_cast<uint8_t *>(h->io_rake.p); }
    if ((stages & AEGIS_STAGE_MEL) && out->S_dB) { if ((rc = ensure(h, h->io_sdb, F * nm * 4))) return rc; d.S_dB = static_cast<float *>(h->io_sdb.p); }
    for (int attempt = 0;; ++attempt) {
        // stream_v = NULL (the handle's own stream) and sync = 2: the schedule the device-pointer entry takes with
        // sync = 1, single Viterbi launch included -- this function synchronises below
        HostFeed feed = make_feed();
        rc = analyze_device_locked(h, static_cast<const float *>(h->io_pcm.p), off.data(), n_clips,
                                   rake_sensitivity, stages, &d, nullptr, 2, &feed);
        if (rc == AEGIS_ERR_NOMEM && h->max_frames_per_pass > ((int64_t)1 << 21)) {      // as in aegis_analyze_batch_device
            (void)hipDeviceSynchronize();
            (void)hipGetLastError();
            h->max_frames_per_pass = std::max<int64_t>((int64_t)1 << 21, h->max_frames_per_pass / 2);
            --attempt;
            continue;
        }
        if (rc != AEGIS_OK) return rc;
        if (!h->persist_pending) break;
        HIPCHK(h, hipStreamSynchronize(s));
        if ((rc = persistent_check(h)) == AEGIS_OK) break;
        if (!h->persist_gave_up || attempt > 0) return rc;
        h->persist_gave_up = false;           // one launch per chunk for the next 16 calls, and this call again
        h->persistent = false;
        h->persist_cooldown = 16;
        ++h->persistent_fallbacks;
    }
    if (d.f0) HIPCHK(h, hipMemcpyAsync(out->f0, d.f0, F * 8, hipMemcpyDeviceToHost, s));
    if (d.voiced_flag) HIPCHK(h, hipMemcpyAsync(out->voiced_flag, d.voiced_flag, F, hipMemcpyDeviceToHost, s));
    if (d.sdb_col_means) HIPCHK(h, hipMemcpyAsync(out->sdb_col_means, d.sdb_col_means, F * 12, hipMemcpyDeviceToHost, s));
    if (d.pitch_bin) HIPCHK(h, hipMemcpyAsync(out->pitch_bin, d.pitch_bin, F * 2, hipMemcpyDeviceToHost, s));
    if (d.voiced_prob) HIPCHK(h, hipMemcpyAsync(out->voiced_prob, d.voiced_prob, F * 8, hipMemcpyDeviceToHost, s));
    if (d.rms) HIPCHK(h, hipMemcpyAsync(out->rms, d.rms, F * 4, hipMemcpyDeviceToHost, s));
    if (d.rake_mask) HIPCHK(h, hipMemcpyAsync(out->rake_mask, d.rake_mask, F, hipMemcpyDeviceToHost, s));
    if (d.S_dB) HIPCHK(h, hipMemcpyAsync(out->S_dB, d.S_dB, (size_t)F * nm * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipStreamSynchronize(h->stream3));      // (a raw-byte feed's decoded samples back to the host)
    h->plan_in_flight = false;
    if ((rc = persistent_check(h)) != AEGIS_OK) return rc;
    if (h->profiling) collect_events(h);
    return finite_result(h, stages, off.data(), n_clips);
}

static int64_t pcm_width(int32_t fmt) {
    return fmt == AEGIS_PCM_U8 ? 1 : fmt == AEGIS_PCM_S16 ? 2 : fmt == AEGIS_PCM_S24 ? 3 : fmt == AEGIS_PCM_S32 || fmt == AEGIS_PCM_F32 ? 4 : 0;
}

// samples of a clip at rate sr (audio_io.resampled_length); negative with a message for an invalid clip
static int64_t pcm_samples(int32_t sr, const aegis_pcm_clip &c, std::string *why) {
    const char *bad = nullptr;
    if (!pcm_width(c.format)) bad = "unsupported sample format (AEGIS_PCM_U8 .. AEGIS_PCM_F32)";
    else if (c.channels < 1 || c.channels > 8) bad = "channels must be 1..8";
    else if (c.sample_rate <= 0) bad = "sample_rate must be positive";
    else if (c.n_frames < 0) bad = "n_frames < 0";
    else if (c.n_frames > 0 && !c.data) bad = "data == NULL";
    else if (c.taps && (c.n_taps <= 0 || !(c.n_taps & 1))) bad = "n_taps must be odd and positive";
    if (bad) { if (why) *why = bad; return AEGIS_ERR_INVALID; }
    if (c.sample_rate == sr) return c.n_frames;
    return (int64_t)std::ceil((double)c.n_frames * (double)sr / (double)c.sample_rate);
}

int64_t aegis_pcm_samples_for(const aegis_handle *h, const aegis_pcm_clip *clip) {
    if (!h || !clip) return AEGIS_ERR_INVALID;
    return pcm_samples(h->tab.sr, *clip, nullptr);
}

int64_t aegis_resample_taps(int32_t up, int32_t down, float *dst, int64_t cap) {
    try {
    if (up < 1 || down < 1) return AEGIS_ERR_INVALID;
    const int32_t g = std::gcd(up, down);
    const std::vector<float> t = pcm_builtin_taps(up / g, down / g);
    if (dst && cap > 0) std::memcpy(dst, t.data(), (size_t)std::min<int64_t>(cap, (int64_t)t.size()) * 4);
    return (int64_t)t.size();
    } catch (...) { return AEGIS_ERR_NOMEM; }
}

int aegis_analyze_pcm(aegis_handle *h, const aegis_pcm_clip *clips, int32_t n_clips, double rake_sensitivity, uint32_t stages,
                      aegis_outputs *out, float *y_out) {
    try {
    if (!h) return AEGIS_ERR_INVALID;
    if (stages & AEGIS_STAGE_RAKE) stages |= AEGIS_STAGE_MEL;
    const bool analyse = (stages & AEGIS_STAGE_ALL) != 0;
    if (n_clips < 0 || (n_clips > 0 && (!clips || (analyse && !out)))) { h->err = "null argument"; return AEGIS_ERR_INVALID; }
    if (!analyse && !y_out) { h->err = "stages == 0 decodes only and needs y_out"; return AEGIS_ERR_INVALID; }
    if (n_clips == 0) return AEGIS_OK;
    if (h->device < 0) { h->err = "handle was created with device=-1 (host tables only)"; return AEGIS_ERR_DEVICE; }
    std::lock_guard<std::mutex> lock(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    const int32_t sr = h->tab.sr;
    PcmFeed pf;
    pf.src = clips;
    pf.y_out = y_out;
    pf.clips.resize((size_t)n_clips);
    std::vector<int64_t> off((size_t)n_clips + 1, 0);
    std::vector<float> taps;
    std::map<std::pair<std::pair<int32_t, int32_t>, const float *>, size_t> filters;   // (up, down, caller's taps) -> first clip using it
    int64_t F = 0, raw_bytes = 0;
    for (int i = 0; i < n_clips; ++i) {
        const aegis_pcm_clip &a = clips[i];
        std::string why;
        const int64_t n_out = pcm_samples(sr, a, &why);
        if (n_out < 0) { h->err = "clip " + std::to_string(i) + ": " + why; return AEGIS_ERR_INVALID; }
        PcmClipDev &c = pf.clips[(size_t)i];
        c.byte_off = raw_bytes;
        raw_bytes += (a.n_frames * pcm_width(a.format) * a.channels + 15) & ~(int64_t)15;
        c.n_in = a.n_frames; c.out_off = off[(size_t)i];
        c.fmt = a.format; c.ch = a.channels;
        c.up = 1; c.down = 1; c.P = 1; c.rm = 0; c.taps_off = 0; c.n_res = a.n_frames;
        if (a.sample_rate != sr) {
            const int32_t g = std::gcd(a.sample_rate, sr);
            c.up = sr / g; c.down = a.sample_rate / g;
            c.n_res = (a.n_frames * c.up + c.down - 1) / c.down;
            const auto key = std::make_pair(std::make_pair(c.up, c.down), a.taps);
            auto it = filters.find(key);
            if (it != filters.end()) {
                const PcmClipDev &o = pf.clips[it->second];
                c.P = o.P; c.rm = o.rm; c.taps_off = o.taps_off;
            } else {
                const std::vector<float> own = a.taps ? std::vector<float>(a.taps, a.taps + a.n_taps) : pcm_builtin_taps(c.up, c.down);
                std::vector<float> htf;
                c.P = pcm_filter_layout(own.data(), (int)own.size(), c.up, c.down, htf, &c.rm);
                c.taps_off = (int64_t)taps.size();
                taps.insert(taps.end(), htf.begin(), htf.end());
                filters[key] = (size_t)i;
            }
        }
        c.tile = pcm_tile(c);
        off[(size_t)i + 1] = off[(size_t)i] + n_out;
        F += 1 + n_out / h->tab.hop;
    }
    int rc;
    if ((rc = ensure(h, h->io_pcm, (size_t)std::max<int64_t>(off[(size_t)n_clips], 1) * 4)) != AEGIS_OK) return rc;
    if ((rc = ensure(h, h->pcm_raw, (size_t)raw_bytes + 16)) != AEGIS_OK) return rc;
    if ((rc = ensure(h, h->pcm_clips, (size_t)n_clips * sizeof(PcmClipDev))) != AEGIS_OK) return rc;
    if ((rc = ensure(h, h->pcm_taps, std::max<size_t>(taps.size(), 1) * 4)) != AEGIS_OK) return rc;
    pf.range_cap = (int64_t)n_clips * 32;
    if ((rc = ensure(h, h->pcm_ranges, (size_t)pf.range_cap * sizeof(PcmRange))) != AEGIS_OK) return rc;
    pf.range_cap = (int64_t)(h->pcm_ranges.cap / sizeof(PcmRange));
    HIPCHK(h, hipMemcpyAsync(h->pcm_clips.p, pf.clips.data(), (size_t)n_clips * sizeof(PcmClipDev), hipMemcpyHostToDevice, h->stream3));
    if (!taps.empty()) HIPCHK(h, hipMemcpyAsync(h->pcm_taps.p, taps.data(), taps.size() * 4, hipMemcpyHostToDevice, h->stream3));
    float *d_pcm = static_cast<float *>(h->io_pcm.p);
    if (!analyse) {      // decode only: every clip at once
        HostFeed feed{nullptr, d_pcm, std::vector<int64_t>((size_t)n_clips, 0), &pf};
        pf.done_in.assign((size_t)n_clips, 0);
        std::vector<int32_t> cis((size_t)n_clips);
        std::vector<int64_t> need((size_t)n_clips);
        for (int i = 0; i < n_clips; ++i) { cis[(size_t)i] = i; need[(size_t)i] = off[(size_t)i + 1] - off[(size_t)i]; }
        if ((rc = pcm_feed(h, feed, cis, need)) != AEGIS_OK) return rc;
        if (stages & AEGIS_OPT_CHECK_FINITE) {
            if ((rc = ensure(h, h->finite_flag, 8)) != AEGIS_OK) return rc;
            HIPCHK(h, hipMemsetAsync(h->finite_flag.p, 0xff, 8, h->stream3));
            launch_finite_check(d_pcm, off[(size_t)n_clips], static_cast<unsigned long long *>(h->finite_flag.p), h->stream3);
        }
        for (int i = 0; i < n_clips; ++i)
            if (off[(size_t)i + 1] > off[(size_t)i])
                HIPCHK(h, hipMemcpyAsync(y_out + off[(size_t)i], d_pcm + off[(size_t)i], (size_t)(off[(size_t)i + 1] - off[(size_t)i]) * 4,
                                         hipMemcpyDeviceToHost, h->stream3));
        HIPCHK(h, hipStreamSynchronize(h->stream3));
        return finite_result(h, stages, off.data(), n_clips);
    }
    return host_fed_locked(h, off, F, n_clips, rake_sensitivity, stages, out, [&]() {
        pf.done_in.assign((size_t)n_clips, 0);
        pf.tables.clear();
        pf.range_used = 0;
        return HostFeed{nullptr, d_pcm, std::vector<int64_t>((size_t)n_clips, 0), &pf};
    });
    } catch (...) { return abi_fail(h); }
}

int aegis_rake_patterns(aegis_handle *h, const float *S_dB, int32_t n_mels, int64_t n_frames,
                        double broadband_threshold_ratio, uint8_t *mask_out) {
    try {
    if (!h) return AEGIS_ERR_INVALID;
    if (n_mels <= 0 || n_frames < 0 || (n_frames > 0 && (!S_dB || !mask_out))) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    if (n_frames == 0) return AEGIS_OK;
    if (h->device < 0) { h->err = "handle was created with device=-1 (host tables only)"; return AEGIS_ERR_DEVICE; }
    std::lock_guard<std::mutex> lock(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    const size_t img = (size_t)n_mels * n_frames * 4;
    if ((rc = ensure(h, h->io_sdb, img)) != AEGIS_OK) return rc;
    if ((rc = ensure(h, h->rk_raw, n_frames)) != AEGIS_OK) return rc;
    if ((rc = ensure(h, h->io_rake, n_frames)) != AEGIS_OK) return rc;
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemcpyAsync(h->io_sdb.p, S_dB, img, hipMemcpyHostToDevice, s));
    const double ms_per_frame = ((double)h->tab.hop / (double)h->tab.sr) * 1000;   // vision.py:23-25
    launch_rake_from_db(static_cast<const float *>(h->io_sdb.p), n_mels, n_frames, broadband_threshold_ratio,
                        (int)(10 / ms_per_frame), (int)(30 / ms_per_frame), static_cast<uint8_t *>(h->rk_raw.p),
                        static_cast<uint8_t *>(h->io_rake.p), s);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(mask_out, h->io_rake.p, n_frames, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return AEGIS_OK;
    } catch (...) { return abi_fail(h); }
}

// the bank of (n_bins, bins_per_octave, fmin, filter_scale), built and uploaded on first use
static int cqt_bank_locked(aegis_handle *h, int32_t &n_bins, int32_t &bins_per_octave, double &fmin, double &filter_scale, hipStream_t s) {
    if (n_bins == 0) n_bins = 84;
    if (bins_per_octave == 0) bins_per_octave = 12;
    if (!(fmin > 0)) fmin = 32.70319566257483;            // note_to_hz('C1')
    if (!(filter_scale > 0)) filter_scale = 1.0;
    CqtBank &b = h->cqt_bank;
    if (b.n_bins != n_bins || b.bins_per_octave != bins_per_octave || b.fmin != fmin || b.filter_scale != filter_scale || !b.dev) {
        HIPCHK(h, hipStreamSynchronize(s));
        if (b.dev) { (void)hipFree(b.dev); b.dev = nullptr; }
        const char *msg = build_cqt_bank(b, h->tab.sr, n_bins, fmin, bins_per_octave, filter_scale);
        if (msg[0]) { h->err = msg; b.n_bins = 0; return AEGIS_ERR_INVALID; }
        // + 64 KiB: the slide kernel refills a tile's register queue unconditionally, so a wave's last groups request up to
        // kSlotDepth KiB past its stream (never used)
        HIPCHK(h, hipMalloc(reinterpret_cast<void **>(&b.dev), b.data.size() * 4 + 65536));
        HIPCHK(h, hipMemset(reinterpret_cast<char *>(b.dev) + b.data.size() * 4, 0, 65536));
        HIPCHK(h, hipMemcpy(b.dev, b.data.data(), b.data.size() * 4, hipMemcpyHostToDevice));
    }
    return AEGIS_OK;
}

// clip geometry on the device + the launch; d_pcm and d_out are device pointers
static int cqt_launch_locked(aegis_handle *h, const float *d_pcm, const int64_t *soff, int32_t n_clips, float *d_out, hipStream_t s,
                             int64_t *total_frames) {
    std::vector<int64_t> foff(n_clips + 1, 0), toff(n_clips + 1, 0);
    for (int i = 0; i < n_clips; ++i) {
        const int64_t n = soff[i + 1] - soff[i];
        if (n < 0) { h->err = "sample_offsets must be non-decreasing"; return AEGIS_ERR_INVALID; }
        foff[i + 1] = foff[i] + 1 + n / h->tab.hop;
        toff[i + 1] = toff[i] + (1 + n / h->tab.hop + kCqtSlideFrames - 1) / kCqtSlideFrames;
    }
    int rc;
    if ((rc = ensure(h, h->q_soff, (n_clips + 1) * 8)) != AEGIS_OK) return rc;
    if ((rc = ensure(h, h->q_foff, (n_clips + 1) * 8)) != AEGIS_OK) return rc;
    if ((rc = ensure(h, h->q_toff, (n_clips + 1) * 8)) != AEGIS_OK) return rc;
    // (pageable host vectors: the copies complete before hipMemcpyAsync returns)
    HIPCHK(h, hipMemcpyAsync(h->q_soff.p, soff, (n_clips + 1) * 8, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(h->q_foff.p, foff.data(), (n_clips + 1) * 8, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(h->q_toff.p, toff.data(), (n_clips + 1) * 8, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));         // ... but the vectors die with this frame: make it certain
    CqtArgs a{d_pcm, static_cast<const int64_t *>(h->q_soff.p), static_cast<const int64_t *>(h->q_foff.p), n_clips,
              foff[n_clips], h->tab.hop, d_out};
    if (h->profiling) { for (auto &ev : h->events) { (void)hipEventDestroy(ev.second.first); (void)hipEventDestroy(ev.second.second); } h->events.clear(); }
    begin_event(h, "cqt", s); launch_cqt(a, h->cqt_bank, static_cast<const int64_t *>(h->q_toff.p), toff[n_clips], s); end_event(h, s);
    HIPCHK(h, hipGetLastError());
    *total_frames = foff[n_clips];
    return AEGIS_OK;
}

int aegis_cqt(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips,
              int32_t n_bins, int32_t bins_per_octave, double fmin, double filter_scale, float *mag_out) {
    try {
    if (!h) return AEGIS_ERR_INVALID;
    if (n_clips < 0 || (n_clips > 0 && (!pcm || !n_samples || !mag_out))) { h->err = "null argument"; return AEGIS_ERR_INVALID; }
    if (n_clips == 0) return AEGIS_OK;
    if (h->device < 0) { h->err = "handle was created with device=-1 (host tables only)"; return AEGIS_ERR_DEVICE; }
    std::lock_guard<std::mutex> lock(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    int rc;
    if ((rc = cqt_bank_locked(h, n_bins, bins_per_octave, fmin, filter_scale, s)) != AEGIS_OK) return rc;
    std::vector<int64_t> soff(n_clips + 1, 0);
    int64_t F = 0;
    for (int i = 0; i < n_clips; ++i) {
        if (n_samples[i] < 0 || (n_samples[i] > 0 && !pcm[i])) { h->err = "bad clip " + std::to_string(i); return AEGIS_ERR_INVALID; }
        soff[i + 1] = soff[i] + n_samples[i];
        F += 1 + n_samples[i] / h->tab.hop;
    }
    if ((rc = ensure(h, h->q_pcm, (size_t)std::max<int64_t>(soff[n_clips], 1) * 4)) != AEGIS_OK) return rc;
    if ((rc = ensure(h, h->q_out, (size_t)F * n_bins * 4)) != AEGIS_OK) return rc;
    for (int i = 0; i < n_clips; ++i)
        if (n_samples[i] > 0)
            HIPCHK(h, hipMemcpyAsync(static_cast<float *>(h->q_pcm.p) + soff[i], pcm[i], n_samples[i] * 4, hipMemcpyHostToDevice, s));
    int64_t Fd = 0;
    if ((rc = cqt_launch_locked(h, static_cast<const float *>(h->q_pcm.p), soff.data(), n_clips, static_cast<float *>(h->q_out.p), s, &Fd)) != AEGIS_OK) return rc;
    HIPCHK(h, hipMemcpyAsync(mag_out, h->q_out.p, (size_t)F * n_bins * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (h->profiling) collect_events(h);
    return AEGIS_OK;
    } catch (...) { return abi_fail(h); }
}

int aegis_chroma_cqt(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips,
                     int32_t n_bins, int32_t bins_per_octave, double fmin, double filter_scale, int32_t n_chroma,
                     const int32_t *bin_class, float *chroma_out) {
    try {
    if (!h) return AEGIS_ERR_INVALID;
    if (n_clips < 0 || (n_clips > 0 && (!pcm || !n_samples || !chroma_out)) || !bin_class) { h->err = "null argument"; return AEGIS_ERR_INVALID; }
    if (n_clips == 0) return AEGIS_OK;
    if (n_chroma < 1 || n_chroma > 24) { h->err = "n_chroma must be 1..24"; return AEGIS_ERR_INVALID; }
    if (h->device < 0) { h->err = "handle was created with device=-1 (host tables only)"; return AEGIS_ERR_DEVICE; }
    std::lock_guard<std::mutex> lock(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    int rc;
    if ((rc = cqt_bank_locked(h, n_bins, bins_per_octave, fmin, filter_scale, s)) != AEGIS_OK) return rc;
    for (int b = 0; b < n_bins; ++b)
        if (bin_class[b] < 0 || bin_class[b] >= n_chroma) { h->err = "bin_class entries must lie in [0, n_chroma)"; return AEGIS_ERR_INVALID; }
    std::vector<int64_t> soff(n_clips + 1, 0);
    int64_t F = 0;
    for (int i = 0; i < n_clips; ++i) {
        if (n_samples[i] < 0 || (n_samples[i] > 0 && !pcm[i])) { h->err = "bad clip " + std::to_string(i); return AEGIS_ERR_INVALID; }
        soff[i + 1] = soff[i] + n_samples[i];
        F += 1 + n_samples[i] / h->tab.hop;
    }
    if ((rc = ensure(h, h->q_pcm, (size_t)std::max<int64_t>(soff[n_clips], 1) * 4)) != AEGIS_OK) return rc;
    if ((rc = ensure(h, h->q_out, (size_t)F * n_bins * 4)) != AEGIS_OK) return rc;
    if ((rc = ensure(h, h->q_chroma, (size_t)F * n_chroma * 4)) != AEGIS_OK) return rc;
    if ((rc = ensure(h, h->q_cls, (size_t)n_bins * 4)) != AEGIS_OK) return rc;
    HIPCHK(h, hipMemcpyAsync(h->q_cls.p, bin_class, (size_t)n_bins * 4, hipMemcpyHostToDevice, s));
    for (int i = 0; i < n_clips; ++i)
        if (n_samples[i] > 0)
            HIPCHK(h, hipMemcpyAsync(static_cast<float *>(h->q_pcm.p) + soff[i], pcm[i], n_samples[i] * 4, hipMemcpyHostToDevice, s));
    int64_t Fd = 0;
    if ((rc = cqt_launch_locked(h, static_cast<const float *>(h->q_pcm.p), soff.data(), n_clips, static_cast<float *>(h->q_out.p), s, &Fd)) != AEGIS_OK) return rc;
    begin_event(h, "chroma", s);
    launch_chroma_fold(static_cast<const float *>(h->q_out.p), static_cast<const int64_t *>(h->q_foff.p), n_clips, F, n_bins, n_chroma,
                       static_cast<const int32_t *>(h->q_cls.p), static_cast<float *>(h->q_chroma.p), s);
    end_event(h, s);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(chroma_out, h->q_chroma.p, (size_t)F * n_chroma * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (h->profiling) collect_events(h);
    return AEGIS_OK;
    } catch (...) { return abi_fail(h); }
}

int aegis_cqt_device(aegis_handle *h, const float *d_pcm, const int64_t *sample_offsets, int32_t n_clips,
                     int32_t n_bins, int32_t bins_per_octave, double fmin, double filter_scale, float *d_mag_out,
                     void *stream, int32_t sync) {
    try {
    if (!h) return AEGIS_ERR_INVALID;
    if (n_clips < 0 || (n_clips > 0 && (!sample_offsets || !d_mag_out))) { h->err = "null argument"; return AEGIS_ERR_INVALID; }
    if (n_clips == 0) return AEGIS_OK;
    if (h->device < 0) { h->err = "handle was created with device=-1 (host tables only)"; return AEGIS_ERR_DEVICE; }
    if (sample_offsets[n_clips] > sample_offsets[0] && !d_pcm) { h->err = "d_pcm == NULL"; return AEGIS_ERR_INVALID; }
    std::lock_guard<std::mutex> lock(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
    int rc;
    if ((rc = cqt_bank_locked(h, n_bins, bins_per_octave, fmin, filter_scale, s)) != AEGIS_OK) return rc;
    int64_t F = 0;
    if ((rc = cqt_launch_locked(h, d_pcm, sample_offsets, n_clips, d_mag_out, s, &F)) != AEGIS_OK) return rc;
    if (sync) {
        HIPCHK(h, hipStreamSynchronize(s));
        if (h->profiling) collect_events(h);
    }
    return AEGIS_OK;
    } catch (...) { return abi_fail(h); }
}

// ---- streaming -------------------------------------------------------------------------------
static PassParams stream_params(aegis_stream *st, const int64_t *dm) {
    aegis_handle *h = st->h;
    const Tables &t = h->tab;
    PassParams p = base_params(t);
    p.stages = AEGIS_STAGE_ALL;
    p.pcm = static_cast<const float *>(st->pcm.p);
    p.sample_off = dm; p.sample_len = dm + 1; p.frame_off = dm + 2; p.out_off = dm + 2; p.sel_off = dm + 4;
    p.chunk_off = const_cast<int64_t *>(dm + 6);
    p.order = reinterpret_cast<const int32_t *>(dm + 8);
    p.n_clips = 1;
    p.dfn = static_cast<double *>(st->dfn.p); p.lag_stride = h->lag_stride;
    p.yin = nullptr; p.yin_stride = h->yin_stride;
    p.cmnd_in_frame = cmnd_in_frame(h); p.troughs = troughs_in_frame(h);
    p.logobs = static_cast<double *>(st->logobs.p); p.obs_stride = h->obs_stride;
    p.logunv = static_cast<double *>(st->logunv.p);
    p.obs_seg = static_cast<int32_t *>(st->obs_seg.p);
    p.ptr = static_cast<uint16_t *>(st->ptr.p); p.cmap = static_cast<uint16_t *>(st->cmap.p);
    p.bnd = static_cast<int32_t *>(st->bnd.p); p.states = static_cast<int32_t *>(st->states.p);
    p.live_states = static_cast<int32_t *>(st->live.p);
    p.melpow = static_cast<float *>(st->melpow.p); p.clipmax = static_cast<uint32_t *>(st->clipmax.p);
    p.rake_raw = static_cast<uint8_t *>(st->rake_raw.p);
    p.vstate = static_cast<double *>(st->vstate.p);
    p.out_vprob = static_cast<double *>(st->o_vprob.p);
    p.out_rms = static_cast<float *>(st->o_rms.p);
    p.out_f0 = static_cast<double *>(st->o_f0.p); p.out_voiced = static_cast<uint8_t *>(st->o_voiced.p);
    p.out_rake = static_cast<uint8_t *>(st->o_rake.p); p.out_sdb = static_cast<float *>(st->o_sdb.p);
    p.rake_ratio = 0.6;
    const double ms_per_frame = ((double)t.hop / (double)t.sr) * 1000;
    p.rake_min_frames = (int)(10 / ms_per_frame); p.rake_max_frames = (int)(30 / ms_per_frame);
    return p;
}

// Captures one fixed-size push as a hipGraph: H2D of the samples, advance (append + geometry), the four
// analysis kernels reading their geometry from the device control block, result gather, D2H.
static StreamCommitCtl *stream_commit_ctl(aegis_stream *st) {
    return reinterpret_cast<StreamCommitCtl *>(static_cast<unsigned char *>(st->ctl.p) + sizeof(StreamCtl));
}

static bool stream_build_graph(aegis_stream *st, int64_t n_push, hipStream_t s, int commit) {
    aegis_handle *h = st->h;
    const Tables &t = h->tab;
    if (!st->pin_samples || !st->pin_result || (commit && !st->pin_commit) || n_push > 8192 || n_push % t.hop != 0 || n_push / t.hop + 1 > 8) return false;
    StreamCtl *ctl = static_cast<StreamCtl *>(st->ctl.p);
    PassParams p = stream_params(st, ctl->meta);      // device address arithmetic only
    p.ctl = ctl;
    p.n_frames = st->cap_frames;
    p.n_sel = n_push / t.hop + 1;                       // launch sizes; the kernels clamp to ctl->n_sel
    if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) return false;
    bool ok = true;
    ok &= hipMemcpyAsync(st->g_staging.p, st->pin_samples, n_push * 4, hipMemcpyHostToDevice, s) == hipSuccess;
    launch_stream_advance(ctl, static_cast<const float *>(st->g_staging.p), (int)n_push, static_cast<float *>(st->pcm.p), t.hop, s);
    launch_frame(p, h->dt, s);
    launch_pyin_obs(p, h->dt, s);
    ok &= launch_viterbi(p, h->dt, t.log_trans_band.data(), s) == hipSuccess;
    if (commit)
        ok &= launch_stream_commit(ctl, 0, stream_commit_ctl(st), p.ptr, p.vstate, t.n_bins, static_cast<int16_t *>(st->c_bins.p),
                                   st->c_result.p, s) == hipSuccess;
    launch_stream_gather(ctl, p.out_rms, p.out_vprob, p.live_states, st->g_result.p, s);
    ok &= hipMemcpyAsync(st->pin_result, st->g_result.p, 256, hipMemcpyDeviceToHost, s) == hipSuccess;
    if (commit) ok &= hipMemcpyAsync(st->pin_commit, st->c_result.p, kCommitResultBytes, hipMemcpyDeviceToHost, s) == hipSuccess;
    hipGraph_t g = nullptr;
    ok &= hipStreamEndCapture(s, &g) == hipSuccess && g != nullptr;
    if (!ok) { if (g) (void)hipGraphDestroy(g); (void)hipGetLastError(); return false; }
    hipGraphExec_t ex = nullptr;
    if (hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) != hipSuccess) { (void)hipGraphDestroy(g); (void)hipGetLastError(); return false; }
    st->graph[commit] = g; st->graph_exec[commit] = ex; st->graph_push[commit] = n_push;
    return true;
}

static int stream_run(aegis_stream *st, int64_t f_lo, int64_t f_hi, bool final_pass, hipStream_t s) {
    // analyses frames [f_lo, f_hi) and advances the Viterbi over them; final_pass also finishes the
    // back-trace and the clip-global stages
    aegis_handle *h = st->h;
    const Tables &t = h->tab;
    const int S = 2 * t.n_bins;
    const int64_t Ftot = final_pass ? f_hi : st->cap_frames;     // clip length as far as the kernels know
    // meta layout (int64): sample_off[2] | frame_off[2] | sel_off[2] | chunk_off[2] | order (int32 in one slot)
    st->host_meta.assign(9, 0);
    st->host_meta[1] = st->n_samples;
    st->host_meta[3] = Ftot;
    st->host_meta[5] = f_hi - f_lo;
    st->host_meta[7] = (Ftot - 1 + kViterbiChunk - 1) / kViterbiChunk;
    HIPCHK(h, hipMemcpyAsync(st->meta.p, st->host_meta.data(), 9 * 8, hipMemcpyHostToDevice, s));
    const int64_t *dm = static_cast<const int64_t *>(st->meta.p);
    PassParams p = stream_params(st, dm);
    p.n_frames = Ftot;
    p.t_begin = f_lo; p.n_sel = f_hi - f_lo;
    p.vt_begin = f_lo; p.vt_end = final_pass ? INT64_MAX : f_hi;
    (void)S;
    if (p.n_sel > 0) {
        launch_frame(p, h->dt, s);
        launch_pyin_obs(p, h->dt, s);
    }
    if (p.n_sel > 0 || final_pass) {
        hipError_t ve = launch_viterbi(p, h->dt, t.log_trans_band.data(), s);
        if (ve != hipSuccess) { h->err = std::string("viterbi launch: ") + hipGetErrorString(ve); return AEGIS_ERR_DEVICE; }
    }
    HIPCHK(h, hipGetLastError());
    return AEGIS_OK;
}

// Releases everything a stream owns.  The caller holds h->mu, or the stream was never handed out.
static void stream_release(aegis_stream *st) noexcept {
    if (st->h && st->h->device >= 0) { (void)hipSetDevice(st->h->device); (void)hipStreamSynchronize(st->h->stream); }
    for (int k = 0; k < 2; ++k) {
        if (st->graph_exec[k]) (void)hipGraphExecDestroy(st->graph_exec[k]);
        if (st->graph[k]) (void)hipGraphDestroy(st->graph[k]);
    }
    if (st->pin_samples) (void)hipHostFree(st->pin_samples);
    if (st->pin_result) (void)hipHostFree(st->pin_result);
    if (st->pin_commit) (void)hipHostFree(st->pin_commit);
    for (DevBuf *b : {&st->c_bins, &st->c_result, &st->ctl, &st->g_staging, &st->g_result, &st->pcm, &st->dfn, &st->logobs, &st->logunv, &st->obs_seg, &st->ptr, &st->cmap, &st->bnd, &st->states,
                      &st->live, &st->melpow, &st->clipmax, &st->rake_raw, &st->vstate, &st->meta, &st->o_f0, &st->o_voiced,
                      &st->o_vprob, &st->o_rms, &st->o_rake, &st->o_sdb})
        free_buf(*b);
    delete st;
}

static int stream_open_locked(aegis_handle *h, int64_t max_samples, aegis_stream *st) {
    HIPCHK(h, hipSetDevice(h->device));
    st->h = h;
    const Tables &t = h->tab;
    st->cap_samples = max_samples;
    st->cap_frames = 1 + max_samples / t.hop;
    const int64_t F = st->cap_frames, S = 2 * t.n_bins;
    const int64_t nch = (F - 1 + kViterbiChunk - 1) / kViterbiChunk + 1;
    int rc = AEGIS_OK;
    auto need = [&](DevBuf &b, size_t bytes) { if (rc == AEGIS_OK) rc = ensure(h, b, bytes); };
    need(st->pcm, max_samples * 4); need(st->dfn, F * h->lag_stride * 8);
    need(st->logobs, F * h->obs_stride * 8); need(st->logunv, F * 8); need(st->obs_seg, F * 4); need(st->ptr, F * S * 2);
    need(st->cmap, nch * S * 2); need(st->bnd, nch * 4); need(st->states, F * 4); need(st->live, F * 4);
    need(st->melpow, F * t.n_mels * 4); need(st->clipmax, 16); need(st->rake_raw, F); need(st->vstate, S * 8);
    need(st->meta, 9 * 8); need(st->ctl, sizeof(StreamCtl) + sizeof(StreamCommitCtl)); need(st->g_staging, 8192 * 4); need(st->g_result, 256);
    need(st->c_bins, F * 2); need(st->c_result, kCommitResultBytes);
    need(st->o_f0, F * 8); need(st->o_voiced, F); need(st->o_vprob, F * 8); need(st->o_rms, F * 4); need(st->o_rake, F);
    need(st->o_sdb, F * t.n_mels * 4);
    if (rc != AEGIS_OK) return rc;
    HIPCHK(h, hipMemsetAsync(st->clipmax.p, 0, 16, h->stream));
    // The band Viterbi leaves the back-pointer of a dead voiced state unwritten, and a launch that starts inside a 16-step
    // chunk (any push that is not a whole number of chunks) walks the rows of the chunk's earlier steps for EVERY state to
    // rebuild its chunk map (viterbi_band.inc, "rebuilds org from the HBM pointers").  What it reads for a dead state is
    // never used, but it is used as the next index: with recycled memory behind the rows an index up to 65535 reaches
    // 128 KB past a short stream's last row (an illegal access on a 0.5 s stream, met in the test suite).  Zeroed rows keep
    // every such index at state 0.
    HIPCHK(h, hipMemsetAsync(st->ptr.p, 0, (size_t)F * S * 2, h->stream));
    {
        struct { StreamCtl ctl; StreamCommitCtl commit; } c0{};
        static_assert(sizeof(c0) == sizeof(StreamCtl) + sizeof(StreamCommitCtl), "the commit block sits right behind the control block");
        c0.ctl.meta[3] = st->cap_frames;
        c0.ctl.meta[7] = (st->cap_frames - 1 + kViterbiChunk - 1) / kViterbiChunk;
        c0.commit.frontier = -1; c0.commit.newest = -1;
        HIPCHK(h, hipMemcpyAsync(st->ctl.p, &c0, sizeof(c0), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (hipHostMalloc(reinterpret_cast<void **>(&st->pin_samples), 8192 * 4, hipHostMallocDefault) != hipSuccess) st->pin_samples = nullptr;
    if (hipHostMalloc(reinterpret_cast<void **>(&st->pin_result), 256, hipHostMallocDefault) != hipSuccess) st->pin_result = nullptr;
    if (hipHostMalloc(reinterpret_cast<void **>(&st->pin_commit), kCommitResultBytes, hipHostMallocDefault) != hipSuccess) st->pin_commit = nullptr;
    // AEGIS_STREAM_GRAPH=0 keeps every push on the plain-launch path, =1 allows the hipGraph replay.  Unset: the replay,
    // except under an injected rocprofiler tool -- round 1's SIGSEGV in aegis_stream_push (profiles/
    // r1_stream_push_sigsegv_symbolised.txt) was the profiler-side packet copy of an INTERCEPTED queue running off the end
    // of a 1 MiB AQL ring when the HIP runtime rang the doorbell for a graph launch: not this library's memory, and not
    // something this library can fix, so profiled runs take the plain launches unless told otherwise.
    if (const char *e = std::getenv("AEGIS_STREAM_GRAPH")) st->graph_failed = (e[0] == '0');
    else {
        const char *tool = std::getenv("ROCP_TOOL_LIBRARIES"), *pre = std::getenv("LD_PRELOAD");
        if ((tool && tool[0]) || (pre && std::strstr(pre, "rocprofiler"))) st->graph_failed = true;
    }
    return AEGIS_OK;
}

int aegis_stream_open(aegis_handle *h, int64_t max_samples, aegis_stream **out) {
    aegis_stream *st = nullptr;
    try {
    if (!h || !out || max_samples <= 0) { if (h) h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    *out = nullptr;
    if (h->device < 0) { h->err = "handle was created with device=-1 (host tables only)"; return AEGIS_ERR_DEVICE; }
    std::lock_guard<std::mutex> lock(h->mu);
    if (h->destroy_requested) { h->err = "handle was destroyed"; return AEGIS_ERR_INVALID; }
    st = new (std::nothrow) aegis_stream();
    if (!st) { h->err = "out of host memory"; return AEGIS_ERR_NOMEM; }
    const int rc = stream_open_locked(h, max_samples, st);
    if (rc != AEGIS_OK) { stream_release(st); st = nullptr; return rc; }     // nothing leaks on a failed open
    ++h->open_streams;
    *out = st;
    return AEGIS_OK;
    } catch (...) {
        const int code = abi_fail(h);
        if (st) stream_release(st);
        return code;
    }
}

void aegis_stream_free(aegis_stream *st) {
    if (!st) return;
    aegis_handle *h = st->h;
    if (!h) { stream_release(st); return; }
    bool last;
    {
        std::lock_guard<std::mutex> lock(h->mu);
        stream_release(st);
        --h->open_streams;
        last = h->destroy_requested && h->open_streams == 0;
    }
    if (last) destroy_now(h);     // aegis_destroy() was called while this stream was still open
}

// The host's half of a commit push, after the stream has drained: `res` is the commit kernel's result block (nullptr: no
// launch was needed, the device frontier is where it was).  Hands out the next decided frames, `cap` at most.
static int stream_deliver(aegis_stream *st, const unsigned char *res, aegis_stream_commit *commit) {
    aegis_handle *h = st->h;
    int64_t staged_lo = -1;
    if (res) {
        int64_t r[4];
        std::memcpy(r, res, 32);
        if (r[3] < 0) { h->err = "stream commit: the walk met a back-pointer the Viterbi never wrote"; return AEGIS_ERR_DEVICE; }
        if (r[0] != st->c_frontier || r[1] < r[0] || r[1] >= st->frames_done) {
            h->err = "stream commit: device and host disagree on the frontier"; return AEGIS_ERR_DEVICE;
        }
        staged_lo = r[0] + 1;
        st->c_frontier = r[1];
        st->c_walked = r[3] & 0xffffffff;
        st->c_walked_wide = r[3] >> 32;
        st->c_newest = st->frames_done - 1;
    } else {
        st->c_walked = st->c_walked_wide = 0;
    }
    const int64_t first = st->c_delivered;
    const int64_t k = std::min<int64_t>(st->c_frontier + 1 - first, commit->cap);
    if (k > 0) {
        if (staged_lo >= 0 && first >= staged_lo && first + k <= staged_lo + kCommitStage)
            std::memcpy(commit->pitch_bin, res + 32 + 2 * (first - staged_lo), (size_t)k * 2);
        else
            HIPCHK(h, hipMemcpy(commit->pitch_bin, static_cast<int16_t *>(st->c_bins.p) + first, (size_t)k * 2, hipMemcpyDeviceToHost));
        st->c_delivered += k;
    }
    commit->first = first;
    commit->count = k > 0 ? k : 0;
    commit->frontier = st->c_delivered - 1;
    commit->walked = st->c_walked;
    commit->walked_wide = st->c_walked_wide;
    return AEGIS_OK;
}

// aegis_stream_push (commit == nullptr: exactly the launches of a stream without the commit) and aegis_stream_push_commit.
// The caller holds h->mu.
static int stream_push_locked(aegis_stream *st, const float *samples, int64_t n, aegis_stream_frames *out, int64_t *n_frames,
                              aegis_stream_commit *commit) {
    aegis_handle *h = st->h;
    if (h->destroy_requested) { h->err = "handle was destroyed"; return AEGIS_ERR_INVALID; }
    if (n < 0 || (n > 0 && !samples) || !n_frames) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    if (commit && (commit->cap < 0 || (commit->cap > 0 && !commit->pitch_bin))) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    if (st->closed) { h->err = "stream is closed"; return AEGIS_ERR_INVALID; }
    if (st->n_samples + n > st->cap_samples) { h->err = "stream capacity exceeded"; return AEGIS_ERR_INVALID; }
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const int ci = commit ? 1 : 0;
    // ---- fixed-size pushes replay a captured hipGraph ---------------------------------------------
    const bool eligible = n > 0 && n <= 8192 && n % h->tab.hop == 0 && n / h->tab.hop + 1 <= 8;
    if (eligible && !st->graph_failed && (st->graph_exec[ci] == nullptr || st->graph_push[ci] == n)) {
        if (st->graph_exec[ci] == nullptr && !stream_build_graph(st, n, s, ci)) st->graph_failed = true;
        if (st->graph_exec[ci] != nullptr && st->graph_push[ci] == n) {
            std::memcpy(st->pin_samples, samples, (size_t)n * 4);
            HIPCHK(h, hipGraphLaunch(st->graph_exec[ci], s));
            HIPCHK(h, hipStreamSynchronize(s));
            st->n_samples += n;
            const int64_t ready = st->n_samples >= kFrameLength / 2 ? (st->n_samples - kFrameLength / 2) / h->tab.hop + 1 : 0;
            const int64_t lo = st->frames_done, hi = std::max(lo, ready);
            int64_t got = 0;
            std::memcpy(&got, st->pin_result, 8);
            if (got != hi - lo) { h->err = "stream graph and host disagree on the frame count"; return AEGIS_ERR_DEVICE; }
            st->frames_done = hi;
            *n_frames = got;
            if (out) {
                if (out->rms) std::memcpy(out->rms, st->pin_result + 8, (size_t)got * 4);
                if (out->voiced_prob) std::memcpy(out->voiced_prob, st->pin_result + 8 + 32, (size_t)got * 8);
                if (out->live_state) std::memcpy(out->live_state, st->pin_result + 8 + 32 + 64, (size_t)got * 4);
            }
            return commit ? stream_deliver(st, st->pin_commit, commit) : AEGIS_OK;
        }
    }
    if (n > 0)
        HIPCHK(h, hipMemcpyAsync(static_cast<float *>(st->pcm.p) + st->n_samples, samples, n * 4, hipMemcpyHostToDevice, s));
    st->n_samples += n;
    // frames whose centred window [t*hop - 1024, t*hop + 1024) is complete
    const int hop = h->tab.hop;
    const int64_t ready = st->n_samples >= kFrameLength / 2 ? (st->n_samples - kFrameLength / 2) / hop + 1 : 0;
    const int64_t lo = st->frames_done, hi = std::max(lo, ready);
    *n_frames = hi - lo;
    if (hi > lo) {
        int rc = stream_run(st, lo, hi, false, s);
        if (rc != AEGIS_OK) return rc;
        st->frames_done = hi;
        if (out) {
            const int64_t k = hi - lo;
            if (out->rms) HIPCHK(h, hipMemcpyAsync(out->rms, static_cast<float *>(st->o_rms.p) + lo, k * 4, hipMemcpyDeviceToHost, s));
            if (out->voiced_prob) HIPCHK(h, hipMemcpyAsync(out->voiced_prob, static_cast<double *>(st->o_vprob.p) + lo, k * 8, hipMemcpyDeviceToHost, s));
            if (out->live_state) HIPCHK(h, hipMemcpyAsync(out->live_state, static_cast<int32_t *>(st->live.p) + lo, k * 4, hipMemcpyDeviceToHost, s));
        }
    }
    {   // the device control block of the graph path mirrors the host counters
        const int64_t counters[2] = {st->n_samples, st->frames_done};
        HIPCHK(h, hipMemcpyAsync(st->ctl.p, counters, 16, hipMemcpyHostToDevice, s));
    }
    // commit: one more launch behind the Viterbi, when there is a frame the last walk has not seen (also the frames of
    // earlier plain pushes: the walk goes from the newest frame back to the frontier, however far that is)
    unsigned char *cres = nullptr;
    if (commit && st->frames_done > 0 && st->frames_done - 1 != st->c_newest) {
        cres = st->pin_commit ? st->pin_commit : st->commit_host;
        hipError_t ce = launch_stream_commit(nullptr, st->frames_done, stream_commit_ctl(st), static_cast<const uint16_t *>(st->ptr.p),
                                             static_cast<const double *>(st->vstate.p), h->tab.n_bins, static_cast<int16_t *>(st->c_bins.p),
                                             st->c_result.p, s);
        if (ce != hipSuccess) { h->err = std::string("stream commit launch: ") + hipGetErrorString(ce); return AEGIS_ERR_DEVICE; }
        HIPCHK(h, hipMemcpyAsync(cres, st->c_result.p, kCommitResultBytes, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(h, hipStreamSynchronize(s));
    return commit ? stream_deliver(st, cres, commit) : AEGIS_OK;
}

int aegis_stream_push(aegis_stream *st, const float *samples, int64_t n, aegis_stream_frames *out, int64_t *n_frames) {
    try {
    if (!st || !st->h) return AEGIS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(st->h->mu);
    return stream_push_locked(st, samples, n, out, n_frames, nullptr);
    } catch (...) { return abi_fail((st ? st->h : nullptr)); }
}

int aegis_stream_push_commit(aegis_stream *st, const float *samples, int64_t n, aegis_stream_frames *out, int64_t *n_frames,
                             aegis_stream_commit *commit) {
    try {
    if (!st || !st->h) return AEGIS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(st->h->mu);
    return stream_push_locked(st, samples, n, out, n_frames, commit);
    } catch (...) { return abi_fail((st ? st->h : nullptr)); }
}

int aegis_stream_close(aegis_stream *st, double rake_sensitivity, aegis_outputs *out, int64_t *n_frames) {
    try {
    if (!st || !st->h) return AEGIS_ERR_INVALID;
    aegis_handle *h = st->h;
    std::lock_guard<std::mutex> lock(h->mu);
    if (h->destroy_requested) { h->err = "handle was destroyed"; return AEGIS_ERR_INVALID; }
    if (!n_frames) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    if (st->closed) { h->err = "stream is closed"; return AEGIS_ERR_INVALID; }
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const Tables &t = h->tab;
    const int64_t F = 1 + st->n_samples / t.hop;
    int rc = stream_run(st, st->frames_done, F, true, s);       // zero-padded tail frames + back-trace
    if (rc != AEGIS_OK) return rc;
    // clip-global stages over all F frames
    st->host_meta[5] = F;
    PassParams p = base_params(t);
    p.stages = AEGIS_STAGE_ALL;
    const int64_t *dm = static_cast<const int64_t *>(st->meta.p);
    p.sample_off = dm; p.sample_len = dm + 1; p.frame_off = dm + 2; p.out_off = dm + 2; p.sel_off = dm + 2; p.n_clips = 1; p.n_frames = F; p.n_sel = F;
    p.states = static_cast<int32_t *>(st->states.p);
    p.melpow = static_cast<float *>(st->melpow.p); p.clipmax = static_cast<uint32_t *>(st->clipmax.p);
    p.rake_raw = static_cast<uint8_t *>(st->rake_raw.p);
    p.out_f0 = static_cast<double *>(st->o_f0.p); p.out_voiced = static_cast<uint8_t *>(st->o_voiced.p);
    p.out_rake = static_cast<uint8_t *>(st->o_rake.p); p.out_sdb = static_cast<float *>(st->o_sdb.p);
    p.rake_ratio = rake_sensitivity;
    const double ms_per_frame = ((double)t.hop / (double)t.sr) * 1000;
    p.rake_min_frames = (int)(10 / ms_per_frame); p.rake_max_frames = (int)(30 / ms_per_frame);
    launch_finalize_mel(p, h->dt, s);
    launch_decode(p, h->dt, s);
    HIPCHK(h, hipGetLastError());
    st->frames_done = F;
    st->closed = true;
    *n_frames = F;
    if (out) {
        auto back = [&](void *dst, const void *src, size_t bytes) { return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) : hipSuccess; };
        HIPCHK(h, back(out->f0, st->o_f0.p, F * 8)); HIPCHK(h, back(out->voiced_flag, st->o_voiced.p, F));
        HIPCHK(h, back(out->voiced_prob, st->o_vprob.p, F * 8)); HIPCHK(h, back(out->rms, st->o_rms.p, F * 4));
        HIPCHK(h, back(out->rake_mask, st->o_rake.p, F)); HIPCHK(h, back(out->S_dB, st->o_sdb.p, (size_t)F * t.n_mels * 4));
    }
    HIPCHK(h, hipStreamSynchronize(s));
    return AEGIS_OK;
    } catch (...) { return abi_fail((st ? st->h : nullptr)); }
}

int aegis_ghost_rsi(aegis_handle *h, const int64_t *ev_a, const int64_t *ev_b, const int64_t *event_off, int32_t n_series,
                    const int64_t *track_len, int32_t period, double *avg_gain, double *avg_loss) {
    try {
    if (!h) return AEGIS_ERR_INVALID;
    if (n_series < 0 || (n_series > 0 && (!event_off || !track_len))) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    if (period < 1 || period > 128) { h->err = "rsi period must be 1..128"; return AEGIS_ERR_INVALID; }
    if (h->device < 0) { h->err = "handle was created with device=-1 (host tables only)"; return AEGIS_ERR_DEVICE; }
    if (n_series == 0) return AEGIS_OK;
    const int64_t E = event_off[n_series] - event_off[0];
    if (E < 0) { h->err = "event_off must be non-decreasing"; return AEGIS_ERR_INVALID; }
    if (E == 0) return AEGIS_OK;
    if (!ev_a || !ev_b || !avg_gain || !avg_loss) { h->err = "null argument"; return AEGIS_ERR_INVALID; }
    std::vector<int64_t> toff((size_t)n_series + 1, 0);
    std::vector<int32_t> sid((size_t)E);
    for (int i = 0; i < n_series; ++i) {
        if (track_len[i] < 0 || event_off[i + 1] < event_off[i]) { h->err = "bad clip " + std::to_string(i); return AEGIS_ERR_INVALID; }
        toff[(size_t)i + 1] = toff[(size_t)i] + track_len[i];
        for (int64_t e = event_off[i]; e < event_off[i + 1]; ++e) sid[(size_t)(e - event_off[0])] = i;
    }
    const int64_t total = toff[(size_t)n_series];
    std::lock_guard<std::mutex> lock(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    int rc;
#define ENS(buf, bytes) if ((rc = ensure(h, h->buf, (size_t)(bytes))) != AEGIS_OK) return rc
    ENS(t_x, std::max<int64_t>(total, 1) * 8); ENS(t_a, std::max<int64_t>(total, 1) * 8); ENS(t_b, std::max<int64_t>(total, 1) * 8);
    ENS(t_off, (n_series + 1) * 8); ENS(t_i64a, 2 * E * 8); ENS(t_i64b, E * 4 + 8); ENS(t_c, 2 * E * 8);
#undef ENS
    int64_t *d_ab = static_cast<int64_t *>(h->t_i64a.p);
    int32_t *d_sid = static_cast<int32_t *>(h->t_i64b.p);
    double *d_out = static_cast<double *>(h->t_c.p);
    HIPCHK(h, hipMemcpyAsync(d_ab, ev_a + event_off[0], (size_t)E * 8, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(d_ab + E, ev_b + event_off[0], (size_t)E * 8, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(d_sid, sid.data(), (size_t)E * 4, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(h->t_off.p, toff.data(), ((size_t)n_series + 1) * 8, hipMemcpyHostToDevice, s));
    trend_ghost_rsi(d_ab, d_ab + E, d_sid, E, static_cast<const int64_t *>(h->t_off.p), n_series, total, period,
                    static_cast<double *>(h->t_x.p), static_cast<double *>(h->t_a.p), static_cast<double *>(h->t_b.p), d_out, d_out + E, s);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(avg_gain + event_off[0], d_out, (size_t)E * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(avg_loss + event_off[0], d_out + E, (size_t)E * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return AEGIS_OK;
    } catch (...) { return abi_fail(h); }
}

int aegis_trend(aegis_handle *h, int32_t op, const double *x, const int64_t *offsets, int32_t n_series,
                const double *params, int32_t n_params, void *const *outs, int32_t n_outs) {
    try {
    if (!h) return AEGIS_ERR_INVALID;
    if (n_series < 0 || (n_series > 0 && (!x || !offsets)) || !outs || n_params < 0 || (n_params > 0 && !params)) {
        h->err = "bad argument"; return AEGIS_ERR_INVALID;
    }
    if (h->device < 0) { h->err = "handle was created with device=-1 (host tables only)"; return AEGIS_ERR_DEVICE; }
    auto need = [&](int np, int no) {
        if (n_params < np || n_outs < no) { h->err = "op needs " + std::to_string(np) + " params and " + std::to_string(no) + " outputs"; return false; }
        for (int i = 0; i < no; ++i) if (!outs[i]) { h->err = "null output"; return false; }
        return true;
    };
    std::lock_guard<std::mutex> lock(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    int rc;
    int64_t total = n_series > 0 ? offsets[n_series] : 0;
    int64_t n_in = total;
    if (op == AEGIS_TREND_CONSENSUS) {       // x = k stacked rows of one series
        if (!need(1, 2) || n_series != 1) { if (n_series != 1) h->err = "consensus takes one series"; return AEGIS_ERR_INVALID; }
        const int k = (int)params[0];
        if (k < 1 || k > 8) { h->err = "consensus of 1..8 filters"; return AEGIS_ERR_INVALID; }
        n_in = total * k;
    }
    if (total == 0) return AEGIS_OK;
    for (int i = 0; i < n_series; ++i)
        if (offsets[i + 1] < offsets[i]) { h->err = "offsets must be non-decreasing"; return AEGIS_ERR_INVALID; }
#define ENS(buf, bytes) if ((rc = ensure(h, h->buf, (size_t)(bytes))) != AEGIS_OK) return rc
    ENS(t_x, n_in * 8); ENS(t_off, (n_series + 1) * 8);
    ENS(t_a, total * 8); ENS(t_b, total * 8); ENS(t_c, total * 8); ENS(t_d, total * 8); ENS(t_e, std::max<int64_t>(total, 256) * 8);
    ENS(t_i8, total); ENS(t_i64a, total * 8); ENS(t_i64b, (n_series + 1) * 8);
#undef ENS
    HIPCHK(h, hipMemcpyAsync(h->t_x.p, x, n_in * 8, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(h->t_off.p, offsets, (n_series + 1) * 8, hipMemcpyHostToDevice, s));
    TrendArgs a{static_cast<const double *>(h->t_x.p), static_cast<const int64_t *>(h->t_off.p), n_series, total};
    double *A = static_cast<double *>(h->t_a.p), *B = static_cast<double *>(h->t_b.p), *Cc = static_cast<double *>(h->t_c.p);
    double *D = static_cast<double *>(h->t_d.p), *E = static_cast<double *>(h->t_e.p);
    int8_t *I8 = static_cast<int8_t *>(h->t_i8.p);
    auto back = [&](void *dst, const void *src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s); };
    auto min_len = [&]() { int64_t m = INT64_MAX; for (int i = 0; i < n_series; ++i) m = std::min(m, offsets[i + 1] - offsets[i]); return m; };
    switch (op) {
    case AEGIS_TREND_SMA: {
        if (!need(1, 1)) return AEGIS_ERR_INVALID;
        const int w = (int)params[0];
        if (w < 1 || min_len() < w) { h->err = "series shorter than the window (the reference raises IndexError)"; return AEGIS_ERR_INVALID; }
        trend_sma(a, w, A, s);
        HIPCHK(h, back(outs[0], A, total * 8));
        break;
    }
    case AEGIS_TREND_EMA: {
        if (!need(1, 1)) return AEGIS_ERR_INVALID;
        trend_ema(a, (int)params[0], A, s);
        HIPCHK(h, back(outs[0], A, total * 8));
        break;
    }
    case AEGIS_TREND_BOLLINGER:
    case AEGIS_TREND_ARTICULATION: {
        const bool art = op == AEGIS_TREND_ARTICULATION;
        if (!need(2, art ? 1 : 3)) return AEGIS_ERR_INVALID;
        const int w = (int)params[0];
        if (w < 1 || w > 128 || min_len() < w) { h->err = "window must be 1..128 and not longer than any series"; return AEGIS_ERR_INVALID; }
        trend_bollinger(a, w, params[1], A, B, Cc, s);
        if (art) {
            trend_articulation(a, B, Cc, I8, s);
            HIPCHK(h, back(outs[0], I8, total));
        } else {
            HIPCHK(h, back(outs[0], A, total * 8)); HIPCHK(h, back(outs[1], B, total * 8)); HIPCHK(h, back(outs[2], Cc, total * 8));
        }
        break;
    }
    case AEGIS_TREND_MACD: {
        if (!need(3, 3)) return AEGIS_ERR_INVALID;
        trend_macd(a, (int)params[0], (int)params[1], (int)params[2], A, B, Cc, s);
        HIPCHK(h, back(outs[0], A, total * 8)); HIPCHK(h, back(outs[1], B, total * 8)); HIPCHK(h, back(outs[2], Cc, total * 8));
        break;
    }
    case AEGIS_TREND_SLIDES: {      // detect_slides_macd: hz_to_midi, macd(5, 20, 9), threshold test
        if (!need(1, 1)) return AEGIS_ERR_INVALID;
        trend_semitones(a.x, total, D, s);
        TrendArgs st{D, a.off, n_series, total};
        trend_macd(st, 5, 20, 9, A, B, Cc, s);
        trend_slides(A, Cc, total, params[0], I8, s);
        HIPCHK(h, back(outs[0], I8, total));
        break;
    }
    case AEGIS_TREND_RSI: {
        if (!need(1, 1)) return AEGIS_ERR_INVALID;
        const int per = (int)params[0];
        if (per < 1 || per > 128) { h->err = "rsi period must be 1..128"; return AEGIS_ERR_INVALID; }
        if (n_params >= 2 && params[1] != 0.0) {          // the two Wilder averages instead of the RSI (see trend.hip)
            if (!need(2, 2)) return AEGIS_ERR_INVALID;
            trend_rsi_averages(a, per, A, B, s);
            HIPCHK(h, back(outs[0], A, total * 8)); HIPCHK(h, back(outs[1], B, total * 8));
            break;
        }
        trend_rsi(a, per, A, s);
        HIPCHK(h, back(outs[0], A, total * 8));
        break;
    }
    case AEGIS_TREND_SAVGOL: {      // params: window, symmetric flag, then `window` reversed coefficients
        if (n_params < 2 || !need(2 + (int)params[0], 1)) { h->err = "savgol params: window, symmetric, coefficients"; return AEGIS_ERR_INVALID; }
        const int w = (int)params[0];
        if (w < 1 || (w & 1) == 0 || w > 255) { h->err = "savgol window must be odd, 1..255"; return AEGIS_ERR_INVALID; }
        HIPCHK(h, hipMemcpyAsync(E, params + 2, (size_t)w * 8, hipMemcpyHostToDevice, s));
        trend_savgol(a, E, w, (int)params[1], B, static_cast<int64_t *>(h->t_i64a.p), static_cast<int64_t *>(h->t_i64b.p), A, s);
        HIPCHK(h, back(outs[0], A, total * 8));
        break;
    }
    case AEGIS_TREND_KALMAN: {
        if (!need(2, 1)) return AEGIS_ERR_INVALID;
        trend_kalman(a, params[0], params[1], A, s);
        HIPCHK(h, back(outs[0], A, total * 8));
        break;
    }
    case AEGIS_TREND_HOLT: {
        if (!need(2, 1)) return AEGIS_ERR_INVALID;
        trend_holt(a, params[0], params[1], A, s);
        HIPCHK(h, back(outs[0], A, total * 8));
        break;
    }
    case AEGIS_TREND_CONSENSUS: {
        trend_consensus(a.x, (int)params[0], total, A, B, s);
        HIPCHK(h, back(outs[0], A, total * 8)); HIPCHK(h, back(outs[1], B, total * 8));
        break;
    }
    case AEGIS_TREND_PITCH_ANALYSIS: {
        // analyze_pitch_financial (financial_analysis.py:368-423): the same kernels as the single ops above, the four
        // independent sequential walks on four streams at once
        if (n_params < 2 || !need(2 + (int)params[0] + 7, 4)) { h->err = "pitch analysis params: sg window, symmetric, coefficients, q, r, alpha, beta, band window, num_std, slide threshold"; return AEGIS_ERR_INVALID; }
        const int w = (int)params[0];
        if (w < 1 || (w & 1) == 0 || w > 255) { h->err = "savgol window must be odd, 1..255"; return AEGIS_ERR_INVALID; }
        const double *pp = params + 2 + w;
        const int bw = (int)pp[4];
        if (bw < 1 || bw > 128 || min_len() < bw) { h->err = "band window must be 1..128 and not longer than any series"; return AEGIS_ERR_INVALID; }
        if ((rc = ensure(h, h->t_pa, (size_t)total * (12 * 8 + 1) + 256)) != AEGIS_OK) return rc;
        double *R = static_cast<double *>(h->t_pa.p);
        double *stack = R;                              // [3][total]: savgol, kalman, holt (the order multi_filter_consensus stacks them)
        double *ma = R + 3 * total, *up = R + 4 * total, *lo = R + 5 * total, *semi = R + 6 * total;
        double *mm = R + 7 * total, *sg = R + 8 * total, *hh = R + 9 * total, *cx = R + 10 * total, *conf = R + 11 * total;
        int8_t *slide_codes = reinterpret_cast<int8_t *>(R + 12 * total);
        hipStream_t q1 = h->stream2, q2 = h->stream3, q3 = h->stream4;
        while (h->sync_events.size() < 5) { hipEvent_t e; HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming)); h->sync_events.push_back(e); }
        HIPCHK(h, hipMemcpyAsync(E, params + 2, (size_t)w * 8, hipMemcpyHostToDevice, s));
        HIPCHK(h, hipEventRecord(h->sync_events[0], s));          // input, offsets and coefficients are on the device
        for (hipStream_t q : {q1, q2, q3}) HIPCHK(h, hipStreamWaitEvent(q, h->sync_events[0], 0));
        // s: MACD of the semitone track -> slide codes
        trend_semitones(a.x, total, semi, s);
        { TrendArgs st{semi, a.off, n_series, total}; trend_macd(st, 5, 20, 9, mm, sg, hh, s); }
        trend_slides(mm, hh, total, pp[6], slide_codes, s);
        // q1: Kalman, then the bands and the articulation state machine
        trend_kalman(a, pp[0], pp[1], stack + total, q1);
        trend_bollinger(a, bw, pp[5], ma, up, lo, q1);
        trend_articulation(a, up, lo, I8, q1);
        trend_band_confidence(a.x, up, lo, total, conf, q1);
        // q2: Holt; q3: NaN compaction + Savitzky-Golay
        trend_holt(a, pp[2], pp[3], stack + 2 * total, q2);
        trend_savgol(a, E, w, (int)params[1], cx, static_cast<int64_t *>(h->t_i64a.p), static_cast<int64_t *>(h->t_i64b.p), stack, q3);
        int ei = 1;
        for (hipStream_t q : {q1, q2, q3}) {
            HIPCHK(h, hipEventRecord(h->sync_events[ei], q));
            HIPCHK(h, hipStreamWaitEvent(s, h->sync_events[ei], 0));
            ++ei;
        }
        trend_consensus(stack, 3, total, A, B, s);
        HIPCHK(h, back(outs[0], A, total * 8)); HIPCHK(h, back(outs[1], I8, total));
        HIPCHK(h, back(outs[2], slide_codes, total)); HIPCHK(h, back(outs[3], conf, total * 8));
        break;
    }
    default:
        h->err = "unknown trend op " + std::to_string(op);
        return AEGIS_ERR_INVALID;
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(s));
    return AEGIS_OK;
    } catch (...) { return abi_fail(h); }
}

int aegis_set_table(aegis_handle *h, const char *name, const double *data, int64_t count) {
    try {
    if (!h || !name || !data) return AEGIS_ERR_INVALID;
    Tables &t = h->tab;
    const std::string n(name);
    struct Slot { std::vector<double> *host; const double *dev; };
    auto slot = [&](const std::string &nm) -> Slot {
        if (nm == "beta_probs") return {&t.beta_probs, h->dt.beta_probs};
        if (nm == "beta_cumsum") return {&t.beta_cumsum, h->dt.beta_cumsum};
        if (nm == "beta_suffix") return {&t.beta_suffix, h->dt.beta_suffix};
        if (nm == "boltz_fact") return {&t.boltz_fact, h->dt.boltz_fact};
        if (nm == "boltz_exp") return {&t.boltz_exp, h->dt.boltz_exp};
        if (nm == "freqs") return {&t.freqs, h->dt.freqs};
        return {nullptr, nullptr};
    };
    auto push = [&](const std::string &nm) -> int {
        Slot s = slot(nm);
        if (h->device < 0) return AEGIS_OK;
        HIPCHK(h, hipSetDevice(h->device));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipMemcpy(const_cast<double *>(s.dev), s.host->data(), s.host->size() * 8, hipMemcpyHostToDevice));
        return AEGIS_OK;
    };
    Slot s = slot(n);
    if (!s.host || n == "beta_cumsum" || n == "beta_suffix") { h->err = "unknown or derived table: " + n; return AEGIS_ERR_INVALID; }
    if (count != (int64_t)s.host->size()) {
        h->err = "table " + n + " needs " + std::to_string(s.host->size()) + " entries";
        return AEGIS_ERR_INVALID;
    }
    std::copy(data, data + count, s.host->begin());
    int rc = push(n);
    if (rc != AEGIS_OK) return rc;
    if (n == "beta_probs") {
        for (int k = 0; k <= kNThresholds; ++k) t.beta_cumsum[k] = np_pairwise_sum(t.beta_probs.data(), k);
        t.beta_suffix.assign(kNThresholds + 1, 0.0);
        for (int k = kNThresholds - 1; k >= 0; --k) t.beta_suffix[k] = t.beta_suffix[k + 1] + t.beta_probs[k];
        if ((rc = push("beta_cumsum")) != AEGIS_OK) return rc;
        if ((rc = push("beta_suffix")) != AEGIS_OK) return rc;
    }
    return AEGIS_OK;
    } catch (...) { return abi_fail(h); }
}

int64_t aegis_get_param(const aegis_handle *h, const char *name) {
    try {
    if (!h || !name) return AEGIS_ERR_INVALID;
    const Tables &t = h->tab;
    const std::string n(name);
    if (n == "min_period") return t.min_period;
    if (n == "max_period") return t.max_period;
    if (n == "n_lags") return t.n_lags;
    if (n == "n_pitch_bins") return t.n_bins;
    if (n == "transition_width") return t.width;
    if (n == "n_trans_classes") return t.n_cls;
    if (n == "max_frames_per_pass") return h->max_frames_per_pass;
    if (n == "lag_stride") return h->lag_stride;
    if (n == "yin_stride") return h->yin_stride;
    if (n == "obs_stride") return h->obs_stride;
    const PassPlan *lp = last_pass(h);      // the last call's plan (its last pass; the split segments of all its passes)
    if (n == "last_frames") return lp ? lp->fp : 0;
    if (n == "last_passes") return (int64_t)h->plan.passes.size();
    if (n == "last_split_segments") { int64_t v = 0; for (const PassPlan &q : h->plan.passes) v += q.tsplit ? q.n_seg : 0; return v; }
    if (n == "split_passes") return h->split_stats[0];
    if (n == "split_segments") return h->split_stats[1];
    if (n == "split_flagged_clips") return h->split_stats[2];
    if (n == "split_unlocked_clips") return h->split_stats[3];
    if (n == "split_rounds") return h->last_carried_steps;
    if (n == "split_viterbi_us") return (int64_t)(h->last_split_viterbi_ms * 1e3);
    if (n == "split_cooldown") return h->split_cooldown;
    if (n == "last_chunks") return lp ? lp->nk() : 0;
    if (n == "last_dense") return lp ? lp->dense : 0;
    if (n == "last_proportional") return lp ? lp->proportional : 0;
    if (n == "last_balanced") return lp ? lp->balanced : 0;
    if (n == "last_hybrid_step") return lp ? lp->hyb_S : 0;
    if (n == "last_persistent") return lp ? lp->persistent : 0;
    if (n == "pyin_init") return t.pyin_init;
    return AEGIS_ERR_INVALID;
    } catch (...) { return abi_fail(const_cast<aegis_handle *>(h)); }
}

int64_t aegis_get_table(const aegis_handle *h, const char *name, void *dst, int64_t cap) {
    try {
    if (!h || !name) return AEGIS_ERR_INVALID;
    const Tables &t = h->tab;
    const std::string n(name);
    const void *src = nullptr;
    int64_t count = 0;
    size_t esz = 8;
    auto setd = [&](const std::vector<double> &v) { src = v.data(); count = (int64_t)v.size(); esz = 8; };
    if (n == "hann") setd(t.hann);
    else if (n == "thresholds") setd(t.thresholds);
    else if (n == "beta_probs") setd(t.beta_probs);
    else if (n == "beta_cumsum") setd(t.beta_cumsum);
    else if (n == "beta_suffix") setd(t.beta_suffix);
    else if (n == "boltz_fact") setd(t.boltz_fact);
    else if (n == "boltz_exp") setd(t.boltz_exp);
    else if (n == "log_trans_band") setd(t.log_trans_band);
    else if (n == "log_trans_pack") setd(t.log_trans_pack);
    else if (n == "freqs") setd(t.freqs);
    else if (n == "twiddle") setd(t.twiddle);
    else if (n == "mel_dense") { src = t.mel_dense.data(); count = (int64_t)t.mel_dense.size(); esz = 4; }
    else return AEGIS_ERR_INVALID;
    if (dst && cap > 0) std::memcpy(dst, src, (size_t)std::min(count, cap) * esz);
    return count;
    } catch (...) { return abi_fail(const_cast<aegis_handle *>(h)); }
}

int64_t aegis_debug_plan(aegis_handle *h, const int64_t *n_samples, int32_t n_clips, int32_t entry, int32_t sync,
                         int32_t n_cus, int64_t *dst, int64_t cap) {
    try {
    if (!h || n_clips < 0 || (n_clips > 0 && !n_samples) || cap < 0 || (cap > 0 && !dst)) return AEGIS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(h->mu);
    std::vector<int64_t> off((size_t)n_clips + 1, 0);
    for (int i = 0; i < n_clips; ++i) {
        if (n_samples[i] < 0 || 1 + n_samples[i] / h->tab.hop > h->max_frames_per_pass) { h->err = "bad clip " + std::to_string(i); return AEGIS_ERR_INVALID; }
        off[i + 1] = off[i] + n_samples[i];
    }
    const int kind = entry & 3;
    const PlanKnobs &kn = h->knobs;
    PlanInput in = plan_input(h, off.data(), n_clips, AEGIS_STAGE_ALL, kind == AEGIS_PLAN_HOST_FED, kind == AEGIS_PLAN_CALLER_STREAM,
                              sync, n_cus, [&kn, n_cus](int n) { return masked_streams_fit(kn, n_cus, n); });
    if (entry & AEGIS_PLAN_COOLING) in.cooling = split_allowed(in) && kn.split_seglen < 0;
    if (entry & AEGIS_PLAN_NO_PERSIST) in.persistent = false;
    const CallPlan c = plan_call(in);
    std::vector<int64_t> v{(int64_t)c.passes.size()};
    for (const PassPlan &m : c.passes) {
        const int64_t flags = m.tsplit * AEGIS_PLAN_F_SPLIT | m.split_auto * AEGIS_PLAN_F_SPLIT_AUTO | m.want_hybrid * AEGIS_PLAN_F_WANT_HYBRID |
                              m.hybrid * AEGIS_PLAN_F_HYBRID | m.hyb_part * AEGIS_PLAN_F_HYBRID_PART | m.balanced * AEGIS_PLAN_F_BALANCED |
                              m.may_persist * AEGIS_PLAN_F_MAY_PERSIST | m.persistent * AEGIS_PLAN_F_PERSISTENT | m.dense * AEGIS_PLAN_F_DENSE |
                              m.proportional * AEGIS_PLAN_F_PROPORTIONAL | m.two_fs * AEGIS_PLAN_F_TWO_FRAME_STREAMS | m.use_fb * AEGIS_PLAN_F_FRAME_B;
        const int64_t lanes = (int64_t)m.fa | (int64_t)m.fb << 4 | (int64_t)m.sv << 8 | (int64_t)m.sd << 12 | (int64_t)m.sa << 16;
        uint64_t hash = 1469598103934665603ull;      // FNV-1a over the tables' bytes, each led by its length
        auto mix = [&hash](const void *p, size_t n) {
            for (size_t i = 0; i < n; ++i) { hash ^= static_cast<const unsigned char *>(p)[i]; hash *= 1099511628211ull; }
        };
        auto table = [&mix](const auto &t) { const uint64_t n = t.size(); mix(&n, 8); mix(t.data(), n * sizeof(t[0])); };
        table(m.seg32); table(m.seg64); table(m.sel_off); table(m.clip_tb);
        for (int64_t x : {(int64_t)m.nc(), m.fp, m.maxF, flags, m.seglen, m.hyb_S, (int64_t)m.n_seg, (int64_t)m.n_lock, (int64_t)m.nk(),
                          (int64_t)m.ramp_k, lanes, (int64_t)hash}) v.push_back(x);
        v.insert(v.end(), m.cb.begin(), m.cb.end());
    }
    if (cap > 0) std::memcpy(dst, v.data(), (size_t)std::min<int64_t>(cap, (int64_t)v.size()) * 8);
    return (int64_t)v.size();
    } catch (...) { return abi_fail(h); }
}

int64_t aegis_debug_fetch(aegis_handle *h, const char *name, void *dst, int64_t cap) {
    try {
    if (!h || !name) return AEGIS_ERR_INVALID;
    const std::string n(name);
    // test hooks of the exception barrier (tests/test_abi_and_tables.py): the body throws, the entry returns a code
    if (n == "throw_bad_alloc") throw std::bad_alloc();
    if (n == "throw_length_error") throw std::length_error("test hook");
    if (n == "throw_runtime_error") throw std::runtime_error("test hook: runtime_error");
    if (n == "throw_int") throw 42;
    if (n == "fail_allocs") { h->fail_allocs = (int)std::max<int64_t>(0, cap); return 0; }      // (count in `cap`, nothing copied)
    const PassPlan *lp = last_pass(h);
    const int64_t F = lp ? lp->fp : 0;
    const int last_pass_segments = lp && lp->tsplit ? lp->n_seg : 0;
    const void *src = nullptr;
    int64_t count = 0;
    size_t esz = 8;
    const aegis_handle::Work &lw = h->work[last_work(h)];      // rows in the order the last pass took its clips: longest first
    if (n == "dfn") { src = lw.dfn.p; count = F * h->lag_stride; }
    else if (n == "yin") { src = lw.yin.p; count = F * h->yin_stride; }
    else if (n == "logobs") {            // dense rows: the segments the kernel did not store (obs_seg) are all log(tiny)
        count = F * h->obs_stride;
        if (h->device < 0 || !lw.logobs.p || !lw.obs_seg.p) { h->err = "stage was not run"; return AEGIS_ERR_INVALID; }
        if (dst && cap > 0) {
            HIPCHK(h, hipSetDevice(h->device));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            std::vector<double> rows((size_t)count);
            std::vector<int32_t> seg((size_t)F);
            HIPCHK(h, hipMemcpy(rows.data(), lw.logobs.p, (size_t)count * 8, hipMemcpyDeviceToHost));
            HIPCHK(h, hipMemcpy(seg.data(), lw.obs_seg.p, (size_t)F * 4, hipMemcpyDeviceToHost));
            const double log_tiny = h->tab.log_tiny;
            for (int64_t f = 0; f < F; ++f)
                for (int b = 0; b < h->obs_stride; ++b)
                    if (!(seg[(size_t)f] & (0x40000000 | (1 << (b >> 6))))) rows[(size_t)(f * h->obs_stride + b)] = log_tiny;
            std::memcpy(dst, rows.data(), (size_t)std::min(count, cap) * 8);
        }
        return count;
    }
    else if (n == "logunv") { src = lw.logunv.p; count = F; }
    else if (n == "states") { src = lw.states.p; count = F; esz = 4; }
    else if (n == "melpow") { src = lw.melpow.p; count = F * h->tab.n_mels; esz = 4; }
    else if (n == "persistent_fallbacks") {
        if (dst && cap > 0) *static_cast<int64_t *>(dst) = h->persistent_fallbacks;
        return 1;
    }
    else if (n == "viterbi_stats" || n == "viterbi_stats_peek") {      // [wave-steps, observed-sources-only wave-steps, skipped voiced wave-steps]
        if (h->device < 0 || !h->vstats.p) return AEGIS_ERR_INVALID;
        if (dst && cap > 0) {
            long long v[3];
            std::lock_guard<std::mutex> lock(h->mu);
            HIPCHK(h, hipSetDevice(h->device));
            HIPCHK(h, hipDeviceSynchronize());
            HIPCHK(h, hipMemcpy(v, h->vstats.p, 24, hipMemcpyDeviceToHost));
            if (n == "viterbi_stats") HIPCHK(h, hipMemset(h->vstats.p, 0, 24));
            std::memcpy(dst, v, (size_t)std::min<int64_t>(cap, 3) * 8);
        }
        return 3;
    }
    else if (n == "obs_cycles") {
        if (h->device < 0) return AEGIS_ERR_INVALID;
        if (dst && cap > 0) {
            long long v[16];
            HIPCHK(h, hipSetDevice(h->device));
            HIPCHK(h, hipDeviceSynchronize());
            HIPCHK(h, obs_debug_fetch(v));
            std::memcpy(dst, v, (size_t)std::min<int64_t>(cap, 16) * 8);
        }
        return 16;
    }
    else if (n == "frame_cycles") {
        if (h->device < 0) return AEGIS_ERR_INVALID;
        if (dst && cap > 0) {
            long long v[24];
            HIPCHK(h, hipSetDevice(h->device));
            HIPCHK(h, hipDeviceSynchronize());
            HIPCHK(h, frame_debug_fetch(v));
            std::memcpy(dst, v, (size_t)std::min<int64_t>(cap, 24) * 8);
        }
        return 24;
    }
    else if (n == "seg_lock") {           // lock-on run lengths of the last time-split pass, one per segment (0: first of its clip, -1: never met)
        if (h->device < 0 || last_pass_segments <= 0) return 0;
        const int ns = last_pass_segments;
        if (dst && cap > 0) {
            std::vector<int32_t> v((size_t)ns), st((size_t)ns);
            HIPCHK(h, hipSetDevice(h->device));
            HIPCHK(h, hipDeviceSynchronize());
            HIPCHK(h, hipMemcpy(v.data(), static_cast<const int32_t *>(lw.seg_i32.p) + ns, (size_t)ns * 4, hipMemcpyDeviceToHost));
            HIPCHK(h, hipMemcpy(st.data(), static_cast<const int32_t *>(lw.seg32.p) + ns, (size_t)ns * 4, hipMemcpyDeviceToHost));
            int64_t *o = static_cast<int64_t *>(dst);
            for (int i = 0; i < std::min<int64_t>(cap, ns); ++i) o[i] = v[i] > 0 ? v[i] - st[i] : v[i];
        }
        return ns;
    }
    else if (n == "split_flags") {
        if (dst && cap > 0) std::memcpy(dst, h->last_split_flags.data(), (size_t)std::min<int64_t>(cap, (int64_t)h->last_split_flags.size()) * 8);
        return (int64_t)h->last_split_flags.size();
    }
    else if (n == "split_verify") {
        if (h->device < 0) return AEGIS_ERR_INVALID;
        if (dst && cap > 0) {                     // reading resets the counters
            long long v[16];
            HIPCHK(h, hipSetDevice(h->device));
            HIPCHK(h, hipDeviceSynchronize());
            HIPCHK(h, viterbi_verify_fetch(v, true));
            std::memcpy(dst, v, (size_t)std::min<int64_t>(cap, 16) * 8);
        }
        return 16;
    }
    else if (n == "viterbi_cycles") {
        if (h->device < 0) return AEGIS_ERR_INVALID;
        if (dst && cap > 0) {                     // reading resets the counters
            long long v[128];
            HIPCHK(h, hipSetDevice(h->device));
            HIPCHK(h, hipDeviceSynchronize());
            HIPCHK(h, viterbi_debug_fetch(v, true));
            std::memcpy(dst, v, (size_t)std::min<int64_t>(cap, 128) * 8);
        }
        return 128;
    }
    else if (n == "viterbi_spans") {
        if (h->device < 0) return AEGIS_ERR_INVALID;
        if (dst && cap > 0) {                     // reading resets the counters
            long long v[272];
            HIPCHK(h, hipSetDevice(h->device));
            HIPCHK(h, hipDeviceSynchronize());
            HIPCHK(h, viterbi_span_fetch(v));
            std::memcpy(dst, v, (size_t)std::min<int64_t>(cap, 272) * 8);
        }
        return 272;
    }
    else if (n == "cqt_cycles") {
        if (h->device < 0) return AEGIS_ERR_INVALID;
        long long v[16];
        HIPCHK(h, hipSetDevice(h->device));
        HIPCHK(h, hipDeviceSynchronize());
        HIPCHK(h, cqt_debug_fetch(v));
        if (dst && cap > 0) std::memcpy(dst, v, (size_t)std::min<int64_t>(cap, 16) * 8);
        return 16;
    }
    else return AEGIS_ERR_INVALID;
    if (h->device < 0 || !src) { h->err = "stage was not run"; return AEGIS_ERR_INVALID; }
    if (dst && cap > 0) {
        HIPCHK(h, hipSetDevice(h->device));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipMemcpy(dst, src, (size_t)std::min(count, cap) * esz, hipMemcpyDeviceToHost));
    }
    return count;
    } catch (...) { return abi_fail(h); }
}

}  // extern "C"
