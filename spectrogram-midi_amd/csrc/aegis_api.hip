// The batch entries behind the C ABI of libaegis_hip.so (include/aegis_hip.h; aegis_internal.h lists the files of the
// other entries): what the planner is told about a call, the host and raw-byte feeds, the recovery policy, the three
// analyze entries.  The passes plan.cpp plans are enqueued by aegis_exec.hip (analyze_device_locked).
#include "aegis_internal.h"

#include <cmath>
#include <numeric>

#include "bin_decide.h"
#include "pcm.h"

using namespace aegis;

RakeBounds aegis::rake_frame_bounds(const Tables &t) {
    const double ms_per_frame = ((double)t.hop / (double)t.sr) * 1000;      // vision.py:23-25
    return {(int)(10 / ms_per_frame), (int)(30 / ms_per_frame)};
}

PassParams aegis::base_params(const Tables &t) {
    PassParams p{};
    p.sr = t.sr; p.hop = t.hop; p.n_mels = t.n_mels;
    p.min_period = t.min_period; p.max_period = t.max_period; p.n_lags = t.n_lags;
    p.n_bins = t.n_bins; p.half_width = t.half_width; p.width = t.width; p.n_cls = t.n_cls;
    p.f0_unvoiced = NAN;
    p.fmin = t.fmin; p.bin_scale = bin_guess_scale(t.sr, t.fmin); p.log_tiny = t.log_tiny; p.log_pinit_v = t.log_pinit[0]; p.log_pinit_u = t.log_pinit[1];
    const RakeBounds rb = rake_frame_bounds(t);
    p.rake_min_frames = rb.min_frames; p.rake_max_frames = rb.max_frames;
    return p;
}

// The frame kernel's epilogue forms the CMND unless the stage tests want the difference function and the CMND as separate
// buffers (AEGIS_DEBUG_STAGES=1), AEGIS_CMND_IN_FRAME=0 was set when the handle was created, or the lag range does not fit
// its LDS.
int aegis::cmnd_in_frame(const aegis_handle *h) {
    return (!h->cmnd_off && !h->debug_stages && frame_cmnd_supported(h->tab.max_period)) ? 1 : 0;
}
// ... and finds the CMND's troughs there as well (AEGIS_TROUGHS_IN_FRAME=0 at create: pyin_obs_kernel loads the CMND row and
// finds them, the round-3 path; tests compare the two)
int aegis::troughs_in_frame(const aegis_handle *h) { return (cmnd_in_frame(h) && !h->troughs_off) ? 1 : 0; }

void aegis::bind_core(PassParams &p, const aegis_handle *h, const PassBufs &w) {
    p.dfn = w.dfn.as<double>(); p.logobs = w.logobs.as<double>(); p.logunv = w.logunv.as<double>();
    p.obs_seg = w.obs_seg.as<int32_t>();
    p.ptr = w.ptr.as<uint16_t>(); p.cmap = w.cmap.as<uint16_t>(); p.bnd = w.bnd.as<int32_t>();
    p.states = w.states.as<int32_t>(); p.vstate = w.vstate.as<double>();
    p.melpow = w.melpow.as<float>(); p.clipmax = w.clipmax.as<uint32_t>(); p.rake_raw = w.rake_raw.as<uint8_t>();
    p.lag_stride = h->lag_stride; p.yin_stride = h->yin_stride; p.obs_stride = h->obs_stride;
    p.cmnd_in_frame = cmnd_in_frame(h); p.troughs = troughs_in_frame(h); p.bin_table = h->bin_table_off ? 0 : 1;
}

// (in the order the host-fed entries size, bind and copy them back)
const OutField aegis::kOutFields[8] = {
    {AEGIS_STAGE_PYIN, 8, false, offsetof(aegis_outputs, f0), &aegis_handle::io_f0, &aegis_stream::o_f0},
    {AEGIS_STAGE_PYIN, 1, false, offsetof(aegis_outputs, voiced_flag), &aegis_handle::io_voiced, &aegis_stream::o_voiced},
    {AEGIS_STAGE_MEL, 12, false, offsetof(aegis_outputs, sdb_col_means), &aegis_handle::io_colmean, nullptr},
    {AEGIS_STAGE_PYIN, 2, false, offsetof(aegis_outputs, pitch_bin), &aegis_handle::io_bin, nullptr},
    {AEGIS_STAGE_PYIN, 8, false, offsetof(aegis_outputs, voiced_prob), &aegis_handle::io_vprob, &aegis_stream::o_vprob},
    {AEGIS_STAGE_RMS, 4, false, offsetof(aegis_outputs, rms), &aegis_handle::io_rms, &aegis_stream::o_rms},
    {AEGIS_STAGE_RAKE, 1, false, offsetof(aegis_outputs, rake_mask), &aegis_handle::io_rake, &aegis_stream::o_rake},
    {AEGIS_STAGE_MEL, 4, true, offsetof(aegis_outputs, S_dB), &aegis_handle::io_sdb, &aegis_stream::o_sdb},
};

// The tables the Viterbi launch rules look at (whether a packed transition table exists).  A host-only handle has uploaded
// none: it stands in the host copy of the packed table the device would hold, so the rules answer alike.
DevTables aegis::rule_tables(const aegis_handle *h) {
    DevTables dt = h->dt;
    if (h->device < 0 && !h->tab.log_trans_pack.empty()) dt.lt_pack = h->tab.log_trans_pack.data();
    return dt;
}

// What the planner needs to know about a call.  masked: whether a CU-masked stream set exists for n clips (the executor
// creates them through split_streams; aegis_debug_plan only asks whether they would be laid out).
PlanInput aegis::plan_input(aegis_handle *h, const int64_t *sample_offsets, int32_t n_clips, uint32_t stages, bool feed,
                            bool caller_stream, int32_t sync, int n_cus, std::function<bool(int)> masked) {
    const Tables &t = h->tab;
    PlanInput in;
    in.sample_offsets.assign(sample_offsets, sample_offsets + n_clips + 1);
    in.max_frames_per_pass = h->max_frames_per_pass;
    in.n_cus = n_cus; in.hop = t.hop; in.half_width = t.half_width;
    in.py = stages & AEGIS_STAGE_PYIN;
    in.feed = feed; in.caller_stream = caller_stream; in.sync = sync;
    const DevTables dt = rule_tables(h);
    in.band_applies = viterbi_band_applies(base_params(t), dt);
    in.split_applies = viterbi_split_applies(base_params(t), dt);
    in.masked_streams = std::move(masked);
    in.knobs = h->knobs;
    in.persistent = h->persist.on;
    if (split_allowed(in) && in.knobs.split_seglen < 0 && h->tsplit.cooldown > 0) in.cooling = true;
    return in;
}

static int64_t pcm_width(int32_t fmt) {
    return fmt == AEGIS_PCM_U8 ? 1 : fmt == AEGIS_PCM_S16 ? 2 : fmt == AEGIS_PCM_S24 ? 3 : fmt == AEGIS_PCM_S32 || fmt == AEGIS_PCM_F32 ? 4 : 0;
}

extern "C" {

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
        const int64_t fb = (int64_t)c.ch * pcm_width(c.fmt);
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

// Frame t reads samples [t*hop - 1024, t*hop + 1024): what chunk k needs of each clip of the pass and has not got yet.
int HostFeed::bring(aegis_handle *h, const PassPlan &m, int k, hipStream_t fs) {
    const int nc = m.nc(), hop = h->tab.hop, half = h->tab.n_fft / 2;
    cis.assign(m.clips.begin(), m.clips.end());
    need.resize((size_t)nc);
    bool any = false;
    for (int i = 0; i < nc; ++i) {
        const int64_t n = m.sample_len[i];
        need[(size_t)i] = (k == m.nk() - 1) ? n : std::min(n, (m.clip_hi(k, i) - 1) * (int64_t)hop + half);
        any = any || need[(size_t)i] > copied[(size_t)m.clips[i]];
    }
    if (!any) return AEGIS_OK;
    if (raw) {      // the same samples, decoded on the device from the raw bytes
        const int rc = pcm_feed(h, *this, cis, need);
        if (rc != AEGIS_OK) return rc;
    } else {
        for (int i = 0; i < nc; ++i) {
            int64_t &done = copied[(size_t)m.clips[i]];
            if (need[(size_t)i] <= done) continue;
            HIPCHK(h, hipMemcpyAsync(dst + m.sample_off[i] + done, pcm[m.clips[i]] + done, (size_t)(need[(size_t)i] - done) * 4,
                                     hipMemcpyHostToDevice, h->stream3));
            done = need[(size_t)i];
        }
    }
    HIPCHK(h, hipEventRecord(h->copy_event, h->stream3));
    HIPCHK(h, hipStreamWaitEvent(fs, h->copy_event, 0));
    return AEGIS_OK;
}

// Runs `attempt` (one planned execution of a blocking call, up to the point where persist.gave_up is known) under the
// handle's recovery policy.
//  - The default pass size was taken from the device memory free when the handle was created; other handles, the caller's
//    own buffers or a second workspace may have taken it since: on an allocation failure the passes are halved (down to
//    2^21 frames) and the call planned again.
//  - The single Viterbi launch of a balanced pass found the frame stage not running beside it (a profiler collecting
//    counters serialises kernels, for one): this handle goes back to one launch per chunk for the next 16 calls and the
//    call is repeated, once.  The give-up is not for good: whatever serialised the kernels may be gone by then.
static int run_with_recovery(aegis_handle *h, const std::function<int()> &attempt) {
    aegis_handle::Persistent &ps = h->persist;
    if (!ps.on && h->knobs.persistent_wanted && ps.cooldown > 0 && --ps.cooldown == 0) ps.on = true;
    for (bool repeated = false;;) {
        const int rc = attempt();
        if (rc == AEGIS_ERR_NOMEM && h->max_frames_per_pass > ((int64_t)1 << 21)) {
            (void)hipDeviceSynchronize();
            (void)hipGetLastError();
            h->max_frames_per_pass = std::max<int64_t>((int64_t)1 << 21, h->max_frames_per_pass / 2);
            continue;
        }
        if (rc == AEGIS_OK || !ps.gave_up || repeated) return rc;
        ps.gave_up = false;
        ps.on = false;
        ps.cooldown = 16;
        ++ps.fallbacks;
        repeated = true;
    }
}

// aegis_debug_set_observations, aegis_debug_set_difference and aegis_debug_set_rake_columns arm ONE analyze call: every analyze entry holds one of these from its first line on, so
// the handle is disarmed when the entry returns, whatever it returns (declared in front of the entry's frame, behind a null
// check of its own: it runs after the frame has released the lock, and takes it again)
struct DisarmInjection {
    aegis_handle *h;
    ~DisarmInjection() { std::lock_guard<std::mutex> lock(h->mu); h->inject.armed = false; h->inject_d.armed = false; h->inject_r.armed = false; }
};

int aegis_analyze_batch_device(aegis_handle *h, const float *d_pcm, const int64_t *sample_offsets,
                               int32_t n_clips, double rake_sensitivity, uint32_t stages,
                               aegis_outputs *dout, void *stream_v, int32_t sync) {
    if (!h) return AEGIS_ERR_INVALID;
    DisarmInjection disarm{h};
    ENTRY(h)
    // (sync = 1: analyze_device_locked synchronises and reads the abort flag itself)
    return run_with_recovery(h, [&] { return analyze_device_locked(h, d_pcm, sample_offsets, n_clips, rake_sensitivity, stages, dout, stream_v, sync); });
    ENTRY_END(h)
}

// The device half of a host-fed analysis (handle locked, io_pcm sized): the staging buffer of every output `want` names is
// sized and entered in d, and the pipeline fed by make_feed() (a fresh feed for every attempt) is enqueued on the handle's
// stream.  Not synchronised, unless the single Viterbi launch had to be checked.
static int host_fed_run_locked(aegis_handle *h, const std::vector<int64_t> &off, int64_t F, int32_t n_clips, double rake_sensitivity,
                               uint32_t stages, const aegis_outputs *want, aegis_outputs &d, const std::function<HostFeed()> &make_feed) {
    hipStream_t s = h->stream;
    // the previous call's kernels may still read io_pcm only if it returned without a sync -- it never does
    const int nm = h->tab.n_mels;
    for (const OutField &f : kOutFields) {
        if (!(stages & f.stage) || !f.get(want)) continue;
        const int rc = ensure(h, h->*f.io, f.size(F, nm));      // (a member pointer: not ENSURE's h->buf)
        if (rc != AEGIS_OK) return rc;
        f.set(&d, (h->*f.io).p);
    }
    // stream_v = NULL (the handle's own stream) and sync = 2: the schedule the device-pointer entry takes with
    // sync = 1, single Viterbi launch included -- the attempt synchronises itself before it reads the abort flag
    return run_with_recovery(h, [&]() -> int {
        HostFeed feed = make_feed();
        const int r = analyze_device_locked(h, static_cast<const float *>(h->io_pcm.p), off.data(), n_clips,
                                            rake_sensitivity, stages, &d, nullptr, 2, &feed);
        if (r != AEGIS_OK || !h->persist.pending) return r;
        HIPCHK(h, hipStreamSynchronize(s));
        return persistent_check(h);
    });
}

// The blocking host-fed analysis of aegis_analyze_batch and aegis_analyze_pcm (handle locked, io_pcm sized): the device
// half above, the outputs back to the host.
static int host_fed_locked(aegis_handle *h, const std::vector<int64_t> &off, int64_t F, int32_t n_clips, double rake_sensitivity,
                           uint32_t stages, aegis_outputs *out, const std::function<HostFeed()> &make_feed) {
    hipStream_t s = h->stream;
    aegis_outputs d{};
    const int nm = h->tab.n_mels;
    const int rc = host_fed_run_locked(h, off, F, n_clips, rake_sensitivity, stages, out, d, make_feed);
    if (rc != AEGIS_OK) return rc;
    for (const OutField &f : kOutFields)
        if (f.get(&d)) HIPCHK(h, hipMemcpyAsync(f.get(out), f.get(&d), f.size(F, nm), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipStreamSynchronize(h->stream3));      // (a raw-byte feed's decoded samples back to the host)
    h->plan_in_flight = false;
    if (h->profiling) collect_events(h);
    return finite_result(h, stages, off.data(), n_clips);
}

// (declared in aegis_internal.h with C++ linkage: aegis_onset.hip runs it in front of its kernels)
}  // extern "C"
int aegis::mel_host_locked(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips, std::vector<int64_t> &off,
                           std::vector<int64_t> &foff) {
    struct Disarm { aegis_handle *h; ~Disarm() { h->inject.armed = false; h->inject_d.armed = false; h->inject_r.armed = false; } } disarm{h};   // as every analyze entry
    off.assign((size_t)n_clips + 1, 0);
    foff.assign((size_t)n_clips + 1, 0);
    for (int i = 0; i < n_clips; ++i) {
        off[(size_t)i + 1] = off[(size_t)i] + n_samples[i];
        foff[(size_t)i + 1] = foff[(size_t)i] + 1 + n_samples[i] / h->tab.hop;
    }
    ENSURE(h, io_pcm, off[(size_t)n_clips] * 4);
    aegis_outputs want{}, d{};
    want.S_dB = reinterpret_cast<float *>(h);          // any non-NULL value: the dB image is the one output wanted
    return host_fed_run_locked(h, off, foff[(size_t)n_clips], n_clips, 0.6, AEGIS_STAGE_MEL, &want, d, [&]() {
        return HostFeed{pcm, static_cast<float *>(h->io_pcm.p), std::vector<int64_t>((size_t)n_clips, 0)};
    });
}
extern "C" {

int aegis_analyze_batch(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips,
                        double rake_sensitivity, uint32_t stages, aegis_outputs *out) {
    if (!h) return AEGIS_ERR_INVALID;
    DisarmInjection disarm{h};
    ENTRY(h)
    if (n_clips < 0 || (n_clips > 0 && (!pcm || !n_samples || !out))) { h->err = "null argument"; return AEGIS_ERR_INVALID; }
    if (n_clips == 0) return AEGIS_OK;
    if (stages & AEGIS_STAGE_RAKE) stages |= AEGIS_STAGE_MEL;
    DEVICE_ONLY(h);
    HIPCHK(h, hipSetDevice(h->device));
    std::vector<int64_t> off;
    const int rc = clip_samples(h, "", pcm, n_samples, 0, n_clips, off);
    if (rc != AEGIS_OK) return rc;
    int64_t F = 0;
    for (int i = 0; i < n_clips; ++i) F += 1 + n_samples[i] / h->tab.hop;
    ENSURE(h, io_pcm, off[n_clips] * 4);
    return host_fed_locked(h, off, F, n_clips, rake_sensitivity, stages, out, [&]() {
        return HostFeed{pcm, static_cast<float *>(h->io_pcm.p), std::vector<int64_t>((size_t)n_clips, 0)};
    });
    ENTRY_END(h)
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

int aegis_pcm_geometry(int32_t handle_rate, const aegis_pcm_clip *clip, int64_t *out) {
    try {
    if (handle_rate <= 0 || !clip || !out) return AEGIS_ERR_INVALID;
    aegis_pcm_clip a = *clip;
    a.n_frames = 0; a.data = nullptr;              // the geometry is the format's and the rate pair's, not the length's
    if (pcm_samples(handle_rate, a, nullptr) < 0) return AEGIS_ERR_INVALID;
    PcmClipDev c{};
    c.fmt = a.format; c.ch = a.channels;
    c.up = 1; c.down = 1; c.P = 1; c.rm = 0;
    if (a.sample_rate != handle_rate) {
        const int32_t g = std::gcd(a.sample_rate, handle_rate);
        c.up = handle_rate / g; c.down = a.sample_rate / g;
        const std::vector<float> own = a.taps ? std::vector<float>(a.taps, a.taps + a.n_taps) : pcm_builtin_taps(c.up, c.down);
        std::vector<float> htf;
        c.P = pcm_filter_layout(own.data(), (int)own.size(), c.up, c.down, htf, &c.rm);
    }
    c.tile = pcm_tile(c);
    out[0] = c.up; out[1] = c.down; out[2] = c.P; out[3] = c.rm; out[4] = c.tile; out[5] = pcm_slabs_per_tile(c, c.tile);
    return AEGIS_OK;
    } catch (...) { return AEGIS_ERR_NOMEM; }
}

int aegis_analyze_pcm(aegis_handle *h, const aegis_pcm_clip *clips, int32_t n_clips, double rake_sensitivity, uint32_t stages,
                      aegis_outputs *out, float *y_out) {
    if (!h) return AEGIS_ERR_INVALID;
    DisarmInjection disarm{h};
    ENTRY(h)
    if (stages & AEGIS_STAGE_RAKE) stages |= AEGIS_STAGE_MEL;
    const bool analyse = (stages & AEGIS_STAGE_ALL) != 0;
    if (n_clips < 0 || (n_clips > 0 && (!clips || (analyse && !out)))) { h->err = "null argument"; return AEGIS_ERR_INVALID; }
    if (!analyse && !y_out) { h->err = "stages == 0 decodes only and needs y_out"; return AEGIS_ERR_INVALID; }
    if (n_clips == 0) return AEGIS_OK;
    DEVICE_ONLY(h);
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
    ENSURE(h, io_pcm, off[(size_t)n_clips] * 4); ENSURE(h, pcm_raw, (size_t)raw_bytes + 16);
    pf.range_cap = (int64_t)n_clips * 32;
    ENSURE(h, pcm_ranges, (size_t)pf.range_cap * sizeof(PcmRange));
    pf.range_cap = (int64_t)(h->pcm_ranges.cap / sizeof(PcmRange));
    PUT(h, pcm_clips, pf.clips, h->stream3); PUT(h, pcm_taps, taps, h->stream3);
    float *d_pcm = static_cast<float *>(h->io_pcm.p);
    if (!analyse) {      // decode only: every clip at once
        HostFeed feed{nullptr, d_pcm, std::vector<int64_t>((size_t)n_clips, 0), &pf};
        pf.done_in.assign((size_t)n_clips, 0);
        std::vector<int32_t> cis((size_t)n_clips);
        std::vector<int64_t> need((size_t)n_clips);
        for (int i = 0; i < n_clips; ++i) { cis[(size_t)i] = i; need[(size_t)i] = off[(size_t)i + 1] - off[(size_t)i]; }
        const int rc = pcm_feed(h, feed, cis, need);
        if (rc != AEGIS_OK) return rc;
        if (stages & AEGIS_OPT_CHECK_FINITE) {
            ENSURE(h, finite_flag, 8);
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
    ENTRY_END(h)
}

}  // extern "C"
