// Handle life cycle and introspection of libaegis_hip.so: create / destroy, the owned device buffers and events every
// other file allocates through, profiling, tables and parameters, aegis_debug_plan / aegis_debug_fetch.
#include "aegis_internal.h"
#include "effects.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <stdexcept>
#include <thread>

using namespace aegis;

static std::string g_create_error;

int aegis::grow_buf(aegis_handle *h, std::vector<DevBuf *> &owner, DevBuf &b, size_t bytes) {
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
    if (!b.listed) { owner.push_back(&b); b.listed = true; }
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

void aegis::free_bufs(std::vector<DevBuf *> &owner) noexcept {
    for (DevBuf *b : owner) {
        if (b->p) (void)hipFree(b->p);
        *b = DevBuf{};
    }
    owner.clear();
}

int aegis::new_event(aegis_handle *h, hipEvent_t *e, unsigned flags) {
    HIPCHK(h, hipEventCreateWithFlags(e, flags));
    h->owned_events.push_back(*e);
    return AEGIS_OK;
}

// The fixed events of a device handle (sync_events' slots: EV_* in aegis_internal.h; split_ev times kernels, the others only order)
static int create_events(aegis_handle *h) {
    int rc = new_event(h, &h->copy_event, hipEventDisableTiming);
    h->sync_events.assign(EV_FIXED, nullptr);
    for (hipEvent_t &e : h->sync_events) if (rc == AEGIS_OK) rc = new_event(h, &e, hipEventDisableTiming);
    for (hipEvent_t &e : h->split_ev) if (rc == AEGIS_OK) rc = new_event(h, &e, hipEventDefault);
    for (hipEvent_t &e : h->hyb_ev) if (rc == AEGIS_OK) rc = new_event(h, &e, hipEventDisableTiming);
    for (hipEvent_t &e : h->fin_ev) if (rc == AEGIS_OK) rc = new_event(h, &e, hipEventDisableTiming);
    return rc;
}

template <typename T>
static int upload_table(aegis_handle *h, const std::vector<T> &v, const T **dst) {
    void *d = nullptr;
    const size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
    HIPCHK(h, hipMalloc(&d, bytes));
    h->table_allocs.push_back(d);
    if (!v.empty()) HIPCHK(h, hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *dst = static_cast<const T *>(d);
    return AEGIS_OK;
}

void aegis::begin_event(aegis_handle *h, const char *name, hipStream_t s) {
    if (!h->profiling) return;
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
    (void)hipEventRecord(a, s);
    h->events.push_back({name, {a, b}});
}
void aegis::end_event(aegis_handle *h, hipStream_t s) {
    if (!h->profiling || h->events.empty()) return;
    (void)hipEventRecord(h->events.back().second.second, s);
}
void aegis::drop_events(aegis_handle *h) noexcept {
    for (auto &ev : h->events) { (void)hipEventDestroy(ev.second.first); (void)hipEventDestroy(ev.second.second); }
    h->events.clear();
}
void aegis::collect_events(aegis_handle *h) {
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
    }
    drop_events(h);
    h->last_ms["total"] = total;
}

int aegis::drain_stream(aegis_handle *h, hipStream_t s, bool collect) {
    const hipError_t e3 = h->plan_in_flight ? hipStreamSynchronize(h->stream3) : hipSuccess, e = hipStreamSynchronize(s);
    h->plan_in_flight = false;
    if (!collect || e3 != hipSuccess || e != hipSuccess) drop_events(h);
    if (!collect) return AEGIS_OK;
    HIPCHK(h, e3);
    HIPCHK(h, e);
    if (h->profiling && !h->events.empty()) collect_events(h);
    return AEGIS_OK;
}

int aegis::abi_fail(aegis_handle *h) noexcept {
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

// The domain the Viterbi kernels are exact on (include/aegis_hip.h): rows pyin_obs_kernel can emit.  Host arithmetic only.
int aegis::check_observation_rows(aegis_handle *h, const double *logobs, const double *logunv, int64_t F) {
    const int B = h->tab.n_bins;
    const double log_tiny = h->tab.log_tiny, easy_min = std::log(std::ldexp(1.0, -53) / B);
    auto reject = [&](int64_t f, const char *why) {
        h->err = "injected observations, frame " + std::to_string(f) + ": " + why;
        return AEGIS_ERR_INVALID;
    };
    for (int64_t f = 0; f < F; ++f) {
        const double u = logunv[f];
        const bool hard = u == log_tiny;
        if (u != u) return reject(f, "logunv is NaN");
        if (!hard && !(u >= easy_min && u <= 0.0)) return reject(f, "logunv must be log(tiny) or within [log(2^-53 / n_pitch_bins), 0]");
        const double *row = logobs + f * B;
        bool observed = false;
        for (int b = 0; b < B; ++b) {
            if (row[b] != row[b]) return reject(f, "logobs is NaN");
            if (!(row[b] >= log_tiny && row[b] <= 0.0)) return reject(f, "logobs must be within [log(tiny), 0]");
            observed = observed || row[b] != log_tiny;
        }
        if (hard && !observed) return reject(f, "a hard frame (logunv == log(tiny)) needs a bin above log(tiny)");
    }
    return AEGIS_OK;
}

// the last call's plan: its last pass, and the workspace that pass used
static const PassPlan *last_pass(const aegis_handle *h) { return h->plan.passes.empty() ? nullptr : &h->plan.passes.back(); }
static int last_work(const aegis_handle *h) { return h->plan.passes.empty() ? 0 : (int)((h->plan.passes.size() - 1) & 1); }

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
    h->persist.on = h->knobs.persistent_wanted;

    h->lag_stride = (h->tab.max_period + 1 + 7) & ~7;
    // a dfn row also holds the frame's trough list when the frame kernel finds the troughs (PassParams::troughs)
    h->lag_stride = std::max<int32_t>(h->lag_stride, (trough_row_doubles_host(h->tab.n_lags) + 7) & ~7);
    h->yin_stride = (h->tab.n_lags + 7) & ~7;
    h->obs_stride = (h->tab.n_bins + 7) & ~7;
    // (read before a host-only handle returns: its launch-rule parameters answer what a device handle would run)
    if (const char *e = std::getenv("AEGIS_DEBUG_STAGES")) h->debug_stages = (e[0] == '1');
    if (const char *e = std::getenv("AEGIS_CMND_IN_FRAME")) h->cmnd_off = (e[0] == '0');
    if (const char *e = std::getenv("AEGIS_TROUGHS_IN_FRAME")) h->troughs_off = (e[0] == '0');
    if (const char *e = std::getenv("AEGIS_OBS_BIN_TABLE")) h->bin_table_off = (e[0] == '0');
    if (const char *e = std::getenv("AEGIS_CQT_BANKS")) { const int v = std::atoi(e); if (v >= 1 && v <= 32) h->cqt_bank_cap = v; }
    if (const char *e = std::getenv("AEGIS_DTW_PASS_BYTES")) { const long long v = std::atoll(e); if (v >= 1) h->dtw_pass_bytes = v; }
    h->tuning_edges.resize(kTunCells + 1);
    tuning_edges(h->tuning_edges.data());
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
    if (const char *e = std::getenv("AEGIS_NOTEFIT_STORE")) h->notefit_store = (e[0] == '1');  // aegis_note_fit: candidates stored once instead of recomputed per frame
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
    CRT(create_events(h));
    CRTHIP(configure_lds_limits());
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
    CRT(upload_table(h, t.bin_edges, &h->dt.bin_edges));
    {
        const double *tw = nullptr;
        CRT(upload_table(h, t.twiddle, &tw));
        h->dt.twiddle = reinterpret_cast<const double2 *>(tw);
    }
    CRT(upload_table(h, h->tuning_edges, &h->d_tuning_edges));
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

void aegis_destroy(aegis_handle *h) {
    if (!h) return;
    {
        std::lock_guard<std::mutex> lock(h->mu);
        if (h->open_streams > 0) { h->destroy_requested = true; return; }   // the last aegis_stream_free() finishes the job
    }
    destroy_now(h);
}

}  // extern "C"

void aegis::destroy_now(aegis_handle *h) noexcept {
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
    // tears a queue down -- and hipStreamDestroy sat in that for ever after
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
    drop_events(h);
    for (hipEvent_t e : h->owned_events) (void)hipEventDestroy(e);
    T("free tables");
    for (void *p : h->table_allocs) (void)hipFree(p);
    for (auto &cb : h->cqt_banks) if (cb.bank.dev) (void)hipFree(cb.bank.dev);
    h->cqt_banks.clear();
    T("free workspaces and staging");
    free_bufs(h->bufs);
    T("destroy streams");
    for (hipStream_t q : {h->stream, h->stream2, h->stream3, h->stream4}) if (q) (void)hipStreamDestroy(q);
    T("done");
    delete h;
}

extern "C" {

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
    if (n == "split_passes") return h->tsplit.stats[0];
    if (n == "split_segments") return h->tsplit.stats[1];
    if (n == "split_flagged_clips") return h->tsplit.stats[2];
    if (n == "split_unlocked_clips") return h->tsplit.stats[3];
    if (n == "split_rounds") return h->tsplit.last_carried_steps;
    if (n == "split_viterbi_us") return (int64_t)(h->tsplit.last_viterbi_ms * 1e3);
    if (n == "split_cooldown") return h->tsplit.cooldown;
    if (n == "last_chunks") return lp ? lp->nk() : 0;
    if (n == "last_dense") return lp ? lp->dense : 0;
    if (n == "last_proportional") return lp ? lp->proportional : 0;
    if (n == "last_balanced") return lp ? lp->balanced : 0;
    if (n == "last_hybrid_step") return lp ? lp->hyb_S : 0;
    if (n == "last_persistent") return lp ? lp->persistent : 0;
    if (n == "pyin_init") return t.pyin_init;
    if (n == "rake_min_frames") return rake_frame_bounds(t).min_frames;
    if (n == "rake_max_frames") return rake_frame_bounds(t).max_frames;
    if (n == "cqt_bank_builds") return h->cqt_bank_builds;
    if (n == "cqt_banks") return (int64_t)h->cqt_banks.size();
    if (n == "cqt_bank_cap") return h->cqt_bank_cap;
    if (n == "cqt_bank_bytes") return h->cqt_bank_bytes;
    if (n == "cqt_bank_build_us") return h->cqt_bank_build_us;
    // the launch rules at this geometry, from the host functions the launches themselves call
    if (n == "cmnd_in_frame") return cmnd_in_frame(h);
    if (n == "troughs_in_frame") return troughs_in_frame(h);
    if (n == "frame_fpw") return frame_batch_fpw(t.max_period);
    if (n == "obs_waves") { PassParams q = base_params(t); q.n_sel = 4096; return pyin_obs_waves(q); }
    if (n == "viterbi_kernel") { const int k = viterbi_kernel_choice(base_params(t), rule_tables(h)); return k < 0 ? AEGIS_ERR_UNSUPPORTED : k; }
    if (n == "split_applies") return viterbi_split_applies(base_params(t), rule_tables(h)) ? 1 : 0;
    if (n == "fx_tile") return kFxRevTile;
    if (n == "fx_chunk") return kFxChunk;
    if (n == "fx_max_taps") return kFxMaxTaps;
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
    else if (n == "bin_edges") setd(t.bin_edges);
    else if (n == "twiddle") setd(t.twiddle);
    else if (n == "tuning_edges") setd(h->tuning_edges);
    else if (n == "mel_dense") { src = t.mel_dense.data(); count = (int64_t)t.mel_dense.size(); esz = 4; }
    else return AEGIS_ERR_INVALID;
    if (dst && cap > 0) std::memcpy(dst, src, (size_t)std::min(count, cap) * esz);
    return count;
    } catch (...) { return abi_fail(const_cast<aegis_handle *>(h)); }
}

int64_t aegis_debug_plan(aegis_handle *h, const int64_t *n_samples, int32_t n_clips, int32_t entry, int32_t sync,
                         int32_t n_cus, int64_t *dst, int64_t cap) {
    ENTRY(h)
    if (n_clips < 0 || (n_clips > 0 && !n_samples) || cap < 0 || (cap > 0 && !dst)) return AEGIS_ERR_INVALID;
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
    ENTRY_END(h)
}

// The kernels' debug counters behind aegis_debug_fetch: device-wide synchronisation, then `count` int64 through the kernel
// file's own fetch (at most 272).  Nothing is touched when the caller passes no room -- except for "cqt_cycles", which
// synchronises and fetches even then.
struct Counter { const char *name; int count; hipError_t (*fetch)(long long *); bool always_sync; };
static const Counter kCounters[] = {
    {"obs_cycles", 16, obs_debug_fetch, false},
    {"frame_cycles", 24, frame_debug_fetch, false},
    {"split_verify", 16, [](long long *v) { return viterbi_verify_fetch(v, true); }, false},       // reading resets the counters
    {"viterbi_cycles", 128, [](long long *v) { return viterbi_debug_fetch(v, true); }, false},     // reading resets the counters
    {"viterbi_spans", 272, viterbi_span_fetch, false},                                             // reading resets the counters
    {"cqt_cycles", 16, cqt_debug_fetch, true},
};

int64_t aegis_debug_fetch(aegis_handle *h, const char *name, void *dst, int64_t cap) {
    ENTRY(h)
    if (!name) return AEGIS_ERR_INVALID;
    const std::string n(name);
    // test hooks of the exception barrier (tests/test_abi_and_tables.py): the body throws, the entry returns a code
    if (n == "throw_bad_alloc") throw std::bad_alloc();
    if (n == "throw_length_error") throw std::length_error("test hook");
    if (n == "throw_runtime_error") throw std::runtime_error("test hook: runtime_error");
    if (n == "throw_int") throw 42;
    if (n == "fail_allocs") { h->fail_allocs = (int)std::max<int64_t>(0, cap); return 0; }      // (count in `cap`, nothing copied)
    for (const Counter &c : kCounters) {
        if (n != c.name) continue;
        if (h->device < 0) return AEGIS_ERR_INVALID;
        if (c.always_sync || (dst && cap > 0)) {
            long long v[272];
            HIPCHK(h, hipSetDevice(h->device));
            HIPCHK(h, hipDeviceSynchronize());
            HIPCHK(h, c.fetch(v));
            if (dst && cap > 0) std::memcpy(dst, v, (size_t)std::min<int64_t>(cap, c.count) * 8);
        }
        return c.count;
    }
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
    else if (n == "obs_seg") { src = lw.obs_seg.p; count = F; esz = 4; }
    else if (n == "states") { src = lw.states.p; count = F; esz = 4; }
    else if (n == "melpow") { src = lw.melpow.p; count = F * h->tab.n_mels; esz = 4; }
    else if (n == "rake_raw") { src = lw.rake_raw.p; count = F; esz = 1; }
    else if (n == "tuning_peak_off") {    // what the most recent aegis_estimate_tuning left: each clip's room in the peak lists
        const std::vector<int64_t> &po = h->tn_last_peak_off;
        if (dst && cap > 0) std::memcpy(dst, po.data(), (size_t)std::min<int64_t>(cap, (int64_t)po.size()) * 8);
        return (int64_t)po.size();
    }
    else if (n == "tuning_pitch" || n == "tuning_mag" || n == "tuning_median") {
        if (h->tn_last_peak_off.empty()) return 0;
        if (n == "tuning_median") { src = h->tn_median.p; count = (int64_t)h->tn_last_peak_off.size() - 1; }
        else { src = n == "tuning_pitch" ? h->tn_pitch.p : h->tn_mag.p; count = h->tn_last_peak_off.back(); }
        esz = 4;
    }
    else if (n == "synth_mix" || n == "synth_clip_peak") {      // the last render pass (render_into): 0 before one
        if (h->sy_last_total.empty()) return 0;
        if (n == "synth_clip_peak") { src = h->sy_clip_peak.p; count = (int64_t)h->sy_last_total.size(); }   // the bits of a double
        else { src = h->sy_mix.p; for (int64_t t : h->sy_last_total) count += t; }
    }
    else if (n == "synth_note_peak") {    // osc_peak[notes[q].osc], gathered here: which notes share an oscillator stays inside
        count = (int64_t)h->sy_last_osc.size();
        if (count == 0 || !dst || cap <= 0) return count;
        int32_t n_oscs = 0;
        for (int32_t g : h->sy_last_osc) n_oscs = std::max(n_oscs, g + 1);
        std::vector<double> peak((size_t)n_oscs);
        HIPCHK(h, hipSetDevice(h->device));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipMemcpy(peak.data(), h->sy_osc_peak.p, (size_t)n_oscs * 8, hipMemcpyDeviceToHost));
        double *o = static_cast<double *>(dst);
        for (int64_t q = 0; q < std::min(count, cap); ++q) o[q] = peak[(size_t)h->sy_last_osc[(size_t)q]];
        return count;
    }
    else if (n == "persistent_fallbacks") {
        if (dst && cap > 0) *static_cast<int64_t *>(dst) = h->persist.fallbacks;
        return 1;
    }
    else if (n == "viterbi_stats" || n == "viterbi_stats_peek") {      // [wave-steps, observed-sources-only wave-steps, skipped voiced wave-steps]
        if (h->device < 0 || !h->vstats.p) return AEGIS_ERR_INVALID;
        if (dst && cap > 0) {
            long long v[3];
            HIPCHK(h, hipSetDevice(h->device));
            HIPCHK(h, hipDeviceSynchronize());
            HIPCHK(h, hipMemcpy(v, h->vstats.p, 24, hipMemcpyDeviceToHost));
            if (n == "viterbi_stats") HIPCHK(h, hipMemset(h->vstats.p, 0, 24));
            std::memcpy(dst, v, (size_t)std::min<int64_t>(cap, 3) * 8);
        }
        return 3;
    }
    else if (n == "seg_lock") {           // lock-on run lengths of the last time-split pass, one per segment (0: first of its clip, -1: never met)
        if (h->device < 0 || last_pass_segments <= 0) return 0;
        const int ns = last_pass_segments;
        if (dst && cap > 0) {
            std::vector<int32_t> v((size_t)ns), st((size_t)ns);
            HIPCHK(h, hipSetDevice(h->device));
            HIPCHK(h, hipDeviceSynchronize());
            const SegLayout L(ns, lp->nc(), lp->n_lock);
            HIPCHK(h, hipMemcpy(v.data(), lw.seg_i32.as<const int32_t>() + L.lock, (size_t)ns * 4, hipMemcpyDeviceToHost));
            HIPCHK(h, hipMemcpy(st.data(), lw.seg32.as<const int32_t>() + L.store, (size_t)ns * 4, hipMemcpyDeviceToHost));
            int64_t *o = static_cast<int64_t *>(dst);
            for (int i = 0; i < std::min<int64_t>(cap, ns); ++i) o[i] = v[i] > 0 ? v[i] - st[i] : v[i];
        }
        return ns;
    }
    else if (n == "split_flags") {
        if (dst && cap > 0) std::memcpy(dst, h->tsplit.last_flags.data(), (size_t)std::min<int64_t>(cap, (int64_t)h->tsplit.last_flags.size()) * 8);
        return (int64_t)h->tsplit.last_flags.size();
    }
    else return AEGIS_ERR_INVALID;
    if (h->device < 0 || !src) { h->err = "stage was not run"; return AEGIS_ERR_INVALID; }
    if (dst && cap > 0) {
        HIPCHK(h, hipSetDevice(h->device));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipMemcpy(dst, src, (size_t)std::min(count, cap) * esz, hipMemcpyDeviceToHost));
    }
    return count;
    ENTRY_END(h)
}

int aegis_debug_rake_columns(aegis_handle *h, const float *mel_power, int64_t n_rows, int32_t n_mels, float clip_max,
                             double ratio, int32_t from_power, uint8_t *flags_out) {
    ENTRY(h)
    if (n_rows < 0 || n_mels <= 0 || n_mels > 128 || (n_rows > 0 && (!mel_power || !flags_out))) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    if (n_rows == 0) return AEGIS_OK;
    DEVICE_ONLY(h);
    HIPCHK(h, hipSetDevice(h->device));
    const size_t bytes = (size_t)n_rows * n_mels * 4;
    ENSURE(h, io_sdb, bytes); ENSURE(h, rk_raw, n_rows); ENSURE(h, io_rake, 32);        // (io_rake: frame_off[2] | clipmax)
    hipStream_t s = h->stream;
    struct { int64_t frame_off[2]; uint32_t clipmax; } geo = {{0, n_rows}, 0};
    std::memcpy(&geo.clipmax, &clip_max, 4);
    StreamScope scope(h);
    HIPCHK(h, hipMemcpyAsync(h->io_sdb.p, mel_power, bytes, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(h->io_rake.p, &geo, sizeof geo, hipMemcpyHostToDevice, s));
    PassParams p{};
    p.n_mels = n_mels; p.n_clips = 1; p.n_frames = n_rows; p.stages = AEGIS_STAGE_MEL;
    p.frame_off = h->io_rake.as<const int64_t>();
    p.clipmax = reinterpret_cast<uint32_t *>(h->io_rake.as<char>() + 16);
    p.melpow = h->io_sdb.as<float>();
    p.rake_raw = h->rk_raw.as<uint8_t>();
    p.rake_ratio = ratio;
    launch_rake_columns(p, from_power != 0, s);
    HIPCHK(h, hipGetLastError());
    FETCH(h, flags_out, h->rk_raw.p, n_rows, s);
    return scope.finish();
    ENTRY_END(h)
}

int aegis_debug_pitch_bins(aegis_handle *h, const double *periods, int64_t n, int16_t *bin_table, int16_t *bin_exact, uint8_t *fell_through) {
    ENTRY(h)
    if (n < 0 || (n > 0 && (!periods || !bin_table || !bin_exact || !fell_through))) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    if (n == 0) return AEGIS_OK;
    DEVICE_ONLY(h);
    HIPCHK(h, hipSetDevice(h->device));
    ENSURE(h, dbg_bins, (size_t)n * 13);     // periods f64 | table i16 | exact i16 | fell u8
    hipStream_t s = h->stream;
    double *d_per = h->dbg_bins.as<double>();
    int16_t *d_fast = reinterpret_cast<int16_t *>(d_per + n), *d_exact = d_fast + n;
    uint8_t *d_fell = reinterpret_cast<uint8_t *>(d_exact + n);
    StreamScope scope(h);
    HIPCHK(h, hipMemcpyAsync(d_per, periods, (size_t)n * 8, hipMemcpyHostToDevice, s));
    launch_pitch_bins(base_params(h->tab), h->dt, d_per, n, d_fast, d_exact, d_fell, s);
    HIPCHK(h, hipGetLastError());
    FETCH(h, bin_table, d_fast, n, s); FETCH(h, bin_exact, d_exact, n, s); FETCH(h, fell_through, d_fell, n, s);
    return scope.finish();
    ENTRY_END(h)
}

int aegis_debug_set_observations(aegis_handle *h, const double *logobs, const double *logunv, int64_t F) {
    ENTRY(h)
    h->inject.armed = false;
    if (!logobs) return AEGIS_OK;
    if (!logunv || F <= 0) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    if (h->inject_d.armed) { h->err = "injected observations: injected difference rows are armed already (one hook per call)"; return AEGIS_ERR_INVALID; }
    if (h->inject_r.armed) { h->err = "injected observations: injected rake columns are armed already (one hook per call)"; return AEGIS_ERR_INVALID; }
    int rc;
    if ((rc = check_observation_rows(h, logobs, logunv, F)) != AEGIS_OK) return rc;
    const int B = h->tab.n_bins;
    DEVICE_ONLY(h);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());        // (an earlier armed call that returned without a sync may still read the rows)
    ENSURE(h, inject.obs, (size_t)F * B * 8); ENSURE(h, inject.unv, (size_t)F * 8);
    HIPCHK(h, hipMemcpy(h->inject.obs.p, logobs, (size_t)F * B * 8, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->inject.unv.p, logunv, (size_t)F * 8, hipMemcpyHostToDevice));
    h->inject.F = F;
    h->inject.armed = true;
    return AEGIS_OK;
    ENTRY_END(h)
}

int aegis_debug_set_difference(aegis_handle *h, const double *d, int64_t F) {
    ENTRY(h)
    h->inject_d.armed = false;
    if (!d) return AEGIS_OK;
    if (F <= 0) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    if (h->inject.armed) { h->err = "injected difference rows: injected observations are armed already (one hook per call)"; return AEGIS_ERR_INVALID; }
    if (h->inject_r.armed) { h->err = "injected difference rows: injected rake columns are armed already (one hook per call)"; return AEGIS_ERR_INVALID; }
    const int64_t W = (int64_t)h->tab.max_period + 1;
    for (int64_t f = 0; f < F; ++f)
        for (int64_t tau = 0; tau < W; ++tau)
            if (!std::isfinite(d[f * W + tau])) {
                h->err = "injected difference rows, frame " + std::to_string(f) + ": d[" + std::to_string(tau) + "] is not finite";
                return AEGIS_ERR_INVALID;
            }
    DEVICE_ONLY(h);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());        // (an earlier armed call that returned without a sync may still read the rows)
    ENSURE(h, inject_d.d, (size_t)F * W * 8);
    HIPCHK(h, hipMemcpy(h->inject_d.d.p, d, (size_t)F * W * 8, hipMemcpyHostToDevice));
    h->inject_d.F = F;
    h->inject_d.armed = true;
    return AEGIS_OK;
    ENTRY_END(h)
}

int aegis_debug_set_rake_columns(aegis_handle *h, const uint8_t *flags, int64_t F) {
    ENTRY(h)
    h->inject_r.armed = false;
    if (!flags) return AEGIS_OK;
    if (F <= 0) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    if (h->inject.armed || h->inject_d.armed) {
        h->err = std::string("injected rake columns: injected ") + (h->inject.armed ? "observations" : "difference rows") + " are armed already (one hook per call)";
        return AEGIS_ERR_INVALID;
    }
    // (every byte is in the domain: a flag is set where the byte is not 0; nothing to validate but the handle itself)
    if (h->device < 0) { h->err = "injected rake columns: the handle was created with device=-1 (host tables only), no analyze call can take them"; return AEGIS_ERR_INVALID; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());        // (an earlier armed call that returned without a sync may still read the flags)
    ENSURE(h, inject_r.flags, (size_t)F);
    HIPCHK(h, hipMemcpy(h->inject_r.flags.p, flags, (size_t)F, hipMemcpyHostToDevice));
    h->inject_r.F = F;
    h->inject_r.armed = true;
    return AEGIS_OK;
    ENTRY_END(h)
}

}  // extern "C"
