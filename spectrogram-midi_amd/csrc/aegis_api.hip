// The batch pipeline behind the C ABI of libaegis_hip.so (include/aegis_hip.h; aegis_internal.h lists the files of the
// other entries).  Host-side orchestration: workspace management, kernel launches of the passes plan.cpp plans on the
// handle's streams, optional hipEvent timing per kernel, the recovery policy, the three analyze entries.
#include "aegis_internal.h"

#include <climits>
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

// After a synchronisation: a persistent Viterbi launch that gave up waiting for its chunk flags says so here.
static int persistent_check(aegis_handle *h) {
    if (!h->persist.pending) return AEGIS_OK;
    h->persist.pending = false;
    uint32_t aborted = 0;
    HIPCHK(h, hipMemcpy(&aborted, h->abort_flag.p, 4, hipMemcpyDeviceToHost));
    if (aborted) {
        HIPCHK(h, hipMemset(h->abort_flag.p, 0, 4));
        h->err = "the Viterbi kernel gave up waiting for the frame stage (AEGIS_VITERBI_PERSISTENT=0 launches it per chunk)";
        h->persist.gave_up = true;
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
    h->tsplit.last_flags.assign(flags.begin(), flags.end());
    for (int i = 0; i < nc; ++i)
        if (flags[i]) { redo.push_back(i); if (flags[i] & 1u) ++h->tsplit.stats[3]; }
    uint32_t counts[2] = {0, 0};
    HIPCHK(h, hipMemcpy(counts, sc.p.tube_count, 8, hipMemcpyDeviceToHost));
    h->tsplit.last_carried_steps = counts[1];
    // The planning rule's estimate against the clock.  A split pass's Viterbi kernels come behind its frame stage, and their
    // time depends on the material: a lock-on run that never meets the speculative one runs its whole segment, and the
    // segments behind it speculate again (one more segment time per round).  When frame stage + measured Viterbi time is
    // not clearly below what the pass would have taken sequentially twice in a row, the next 32 calls of this handle plan
    // their passes sequentially.  Once per call, at its last split pass: from its first split pass's Viterbi kernels to its
    // last's.
    bool last_split = true;
    for (size_t j = (size_t)sc.pass + 1; j < h->plan.passes.size(); ++j) last_split = last_split && !h->plan.passes[j].tsplit;
    if (m.split_auto && last_split) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, h->split_ev[0], h->split_ev[1]) == hipSuccess) {
            h->tsplit.last_viterbi_ms = ms;
            if (!split_clock_pays(h->plan, ms)) { if (++h->tsplit.bad >= 2) { h->tsplit.cooldown = 32; h->tsplit.bad = 0; } }
            else h->tsplit.bad = 0;
        }
    }
    if (redo.empty()) return AEGIS_OK;
    h->tsplit.stats[2] += (int64_t)redo.size();
    if (m.split_auto) {
        // the redo is sequential and comes on top of the split pass: when it costs too much of what the pass would have
        // taken sequentially (material without voiced notes never locks on and keeps its tubes open: noise, silence), the
        // next 32 calls of this handle plan their passes sequentially
        int64_t redoF = 0;
        for (int i : redo) redoF = std::max(redoF, m.frames(i));
        if (!split_redo_pays(m, redoF, t.half_width)) h->tsplit.cooldown = 32;
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

static int ensure_pass(aegis_handle *h, aegis_handle::Work &w, const PassPlan &m, uint32_t stages) {
    PassGeometry g;
    g.F = m.fp; g.S = 2 * h->tab.n_bins; g.cmap_rows = m.chunk_off[m.nc()] + 1; g.clips = m.nc(); g.nk = m.nk();
    g.lag_stride = h->lag_stride; g.yin_stride = h->yin_stride; g.obs_stride = h->obs_stride; g.n_mels = h->tab.n_mels;
    g.pyin = stages & AEGIS_STAGE_PYIN; g.mel = stages & AEGIS_STAGE_MEL;
    g.debug_stages = h->debug_stages; g.proportional = m.proportional; g.tsplit = m.tsplit;
    g.n_seg = m.n_seg; g.tube_cap = m.tube_cap; g.tube_record_ints = viterbi_tube_record_ints();
    g.seg64_size = (int64_t)m.seg64.size(); g.seg32_size = (int64_t)m.seg32.size();
    const PassBytes b = pass_bytes(g);
    int rc;
    // (a buffer the pass does not use asks for 0 bytes, which never grows anything)
#define ENS(buf) if ((rc = ensure(h, w.buf, b.buf)) != AEGIS_OK) return rc
    ENS(sample_off); ENS(sample_len); ENS(out_off); ENS(frame_off); ENS(order); ENS(chunk_off); ENS(sel_off);
    ENS(dfn); ENS(yin); ENS(logobs); ENS(logunv); ENS(obs_seg); ENS(ptr); ENS(cmap); ENS(bnd); ENS(states); ENS(vstate);
    ENS(chunk_lo); ENS(chunk_flag); ENS(clip_tb);
    ENS(seg64); ENS(seg32); ENS(seg_col); ENS(seg_map); ENS(seg_i32); ENS(colhist); ENS(colG); ENS(colkg); ENS(clip_flag);
    ENS(flag_order); ENS(tube_buf); ENS(tube_at); ENS(tube_count);
    ENS(melpow); ENS(clipmax); ENS(rake_raw);
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
        HIPCHK(h, hipMemsetAsync(w.seg_i32.p, 0, SegLayout(m.n_seg, nc, m.n_lock).n_i32 * 4, fa));       // seg_lock = 0 for the segments without a lock-on run
        HIPCHK(h, hipMemsetAsync(w.clip_flag.p, 0, nc * 4, fa));
        HIPCHK(h, hipMemsetAsync(w.tube_at.p, 0, (size_t)m.fp * 4, fa));
        HIPCHK(h, hipMemsetAsync(w.tube_count.p, 0, 8, fa));       // tubes recorded, rounds of second speculation that had work
    }
    if (m.persistent) {
        if (!h->abort_flag.p) {
            ENSURE(h, abort_flag, 4);
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
    p.sample_off = w.sample_off.as<const int64_t>(); p.sample_len = w.sample_len.as<const int64_t>();
    p.frame_off = w.frame_off.as<const int64_t>(); p.out_off = w.out_off.as<const int64_t>();
    p.order = w.order.as<const int32_t>(); p.chunk_off = w.chunk_off.as<int64_t>();
    p.n_clips = nc; p.n_frames = m.fp;
    bind_core(p, h, w);
    p.yin = (py && h->debug_stages) ? w.yin.as<double>() : nullptr;
    p.vstats = h->vstats.as<unsigned long long>();
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
    if (opts & AEGIS_OPT_F0_ZERO) p.f0_unvoiced = 0.0;
    p.dense = m.dense ? 1 : 0;
    if (m.tsplit) {
        const SegLayout L(n_seg, nc, m.n_lock);
        const int64_t *g64 = w.seg64.as<const int64_t>();
        const int32_t *g32 = w.seg32.as<const int32_t>();
        p.seg_f0 = g64 + L.f0; p.seg_ch0 = g64 + L.ch0; p.vf_off = g64 + L.vf_off; p.vf_total = m.seg64.back();
        p.seg_T = g32 + L.T; p.seg_store = g32 + L.store; p.seg_prev = g32 + L.prev; p.seg_clip = g32 + L.clip;
        p.clip_seg0 = g32 + L.clip_seg0;
        p.seg_col = w.seg_col.as<double>(); p.seg_col2 = p.seg_col + (size_t)n_seg * S;
        p.seg_map = w.seg_map.as<uint16_t>();
        int32_t *i32 = w.seg_i32.as<int32_t>();
        p.seg_kg = i32 + L.kg; p.seg_lock = i32 + L.lock; p.seg_end = i32 + L.end; p.clip_first = i32 + L.clip_first; p.clip_dirty = i32 + L.clip_dirty;
        p.colhist = w.colhist.as<double>(); p.colG = w.colG.as<double>(); p.colkg = w.colkg.as<int32_t>();
        p.clip_flag = w.clip_flag.as<uint32_t>();
        p.tube_buf = w.tube_buf.as<int32_t>(); p.tube_cap = m.tube_cap; p.tube_count = w.tube_count.as<uint32_t>();
        p.tube_at = w.tube_at.as<int32_t>();
        p.n_seg = n_seg;
    }
    if (m.persistent) {
        p.chunk_flag = w.chunk_flag.as<const uint32_t>();
        p.chunk_lo = w.chunk_lo.as<const int64_t>();
        p.n_chunks = m.nk();
        if (m.hybrid) { int ks = 0; while (ks < m.nk() && m.cb[ks] <= m.hyb_S) ++ks; p.n_chunks = ks; }      // (the launch ends at step S: chunks 0 .. ks - 1)
        p.abort_flag = h->abort_flag.as<uint32_t>();
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

// sync: 0 = return with the work enqueued, 1 = synchronise and report (give-up of the single Viterbi launch, non-finite
// samples), 2 = the caller synchronises and makes those checks itself right away (aegis_analyze_batch: the single Viterbi
// launch is allowed, as with 1)
static int analyze_device_locked(aegis_handle *h, const float *d_pcm, const int64_t *sample_offsets,
                                 int32_t n_clips, double rake_sensitivity, uint32_t stages,
                                 aegis_outputs *dout, void *stream_v, int32_t sync, HostFeed *feed = nullptr) {
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
    DEVICE_ONLY(h);
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
    {   // An armed injection hook (at most one: each setter refuses while another is armed) holds rows indexed by this call's
        // output frames: aegis_debug_set_observations, aegis_debug_set_difference, aegis_debug_set_rake_columns.
        const struct { bool armed; int64_t F; uint32_t stage; const char *what, *stage_name; } hooks[] = {
            {h->inject.armed, h->inject.F, AEGIS_STAGE_PYIN, "injected observations", "PYIN"},
            {h->inject_d.armed, h->inject_d.F, AEGIS_STAGE_PYIN, "injected difference rows", "PYIN"},
            {h->inject_r.armed, h->inject_r.F, AEGIS_STAGE_RAKE, "injected rake columns", "RAKE"},
        };
        int64_t F = 0;
        for (int i = 0; i < n_clips; ++i) F += 1 + (sample_offsets[i + 1] - sample_offsets[i]) / t.hop;
        for (const auto &k : hooks) {
            if (!k.armed || ((stages & k.stage) && F == k.F)) continue;
            h->err = std::string(k.what) + ": the call needs the " + k.stage_name + " stage and exactly " + std::to_string(k.F) +
                     " frames (it has " + std::to_string(F) + ")";
            return AEGIS_ERR_INVALID;
        }
    }
    // host arrays of the previous call's plan are no longer referenced once the stream drained
    if (h->plan_in_flight) { HIPCHK(h, hipStreamSynchronize(s)); h->plan_in_flight = false; }
    h->tsplit.checks.clear();
    drop_events(h);

    // ---- plan ---------------------------------------------------------------------------------------------------------
    const PlanInput in = plan_input(h, sample_offsets, n_clips, stages, feed != nullptr, stream_v != nullptr, sync, h->n_cus,
                                    [h](int n) { return split_streams(h, n) != nullptr; });
    if (in.cooling) --h->tsplit.cooldown;
    h->plan = plan_call(in);
    h->plan_in_flight = true;
    const bool py = in.py;

    // fixed slots of sync_events: 0 call start, 1/2 pass done (workspace parity), 3 frame_b joined, 4 frame_a final, 5.. per chunk
    enum { EV_START = 0, EV_DONE0 = 1, EV_DONE1 = 2, EV_FB = 3, EV_FA = 4, EV_META = 5, EV_CHUNK0 = 6 };
    // (the fixed events exist since aegis_create; the call's longest pass may need more per-chunk ones)
    for (const PassPlan &m : h->plan.passes)
        while ((int)h->sync_events.size() < EV_CHUNK0 + m.nk()) {
            hipEvent_t e;
            const int rc = new_event(h, &e, hipEventDisableTiming);
            if (rc != AEGIS_OK) return rc;
            h->sync_events.push_back(e);
        }
    bool done_recorded[2] = {false, false}, split_started = false;
    std::vector<hipStream_t> joined;          // streams whose work s must wait for before the call returns
    for (int pi = 0; pi < (int)h->plan.passes.size(); ++pi) {
        const PassPlan &m = h->plan.passes[pi];
        const int nc = m.nc(), nk = m.nk();
        aegis_handle::Work &w = h->work[pi & 1];
        int rc;
        // ---- wait for the workspace: a split verdict of the pass two back is read (and acted on) before anything
        // overwrites it or ensure() moves its buffers
        if (!h->tsplit.checks.empty() && h->tsplit.checks.front().pass == pi - 2) {
            HIPCHK(h, hipEventSynchronize(h->sync_events[EV_DONE0 + (pi & 1)]));
            const aegis_handle::SplitCheck sc = h->tsplit.checks.front();
            h->tsplit.checks.erase(h->tsplit.checks.begin());
            if ((rc = split_check(h, sc, s)) != AEGIS_OK) return rc;
        }
        const aegis_handle::SplitSet *ss = m.fa == Lane::masked_frame_a ? split_streams(h, nc) : nullptr;
        hipStream_t fa = lane_stream(h, m.fa, s, ss), fb = lane_stream(h, m.fb, s, ss), sv = lane_stream(h, m.sv, s, ss);
        hipStream_t sd = lane_stream(h, m.sd, s, ss), sa = lane_stream(h, m.sa, s, ss);
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
        const SegLayout L(m.n_seg, nc, m.n_lock);
        const int32_t *d_seg_order = m.tsplit ? w.seg32.as<const int32_t>() + L.seg_order : nullptr;
        const int32_t *d_lock_order = m.tsplit ? w.seg32.as<const int32_t>() + L.lock_order : nullptr;
        if (m.persistent) {
            p.chunk_gen = ++h->chunk_gen;
            if (p.chunk_gen == 0) p.chunk_gen = ++h->chunk_gen;
            h->persist.pending = true;
        }

        // A time-split launch (a plain split pass's, a hybrid pass's): an automatic call is timed from its first one to its
        // last one (split_ev), and each leaves a verdict that split_check reads once the pass is done.
        auto launch_split = [&](const PassParams &q, int n_spec, hipStream_t sq, hipStream_t aux) -> int {
            hipError_t ve = hipSuccess;
            TIMED(h, "viterbi", sq,
                  if (m.split_auto && !split_started) { HIPCHK(h, hipEventRecord(h->split_ev[0], sq)); split_started = true; }
                  ve = launch_viterbi_split(q, h->dt, t.log_trans_band.data(), d_seg_order, n_spec, d_lock_order, m.n_lock, sq, aux, h->fin_ev);
                  if (m.split_auto) HIPCHK(h, hipEventRecord(h->split_ev[1], sq)));
            VCHK(ve);
            h->tsplit.checks.push_back({pi, q});
            ++h->tsplit.stats[0]; h->tsplit.stats[1] += m.n_seg;
            return AEGIS_OK;
        };
        std::vector<int32_t> cis;
        std::vector<int64_t> need;          // (a host feed: samples of each clip the chunk at hand needs)

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
            if (feed) {      // frame t reads samples [t*hop - 1024, t*hop + 1024): what this chunk needs of each clip
                cis.assign(m.clips.begin(), m.clips.end());
                need.resize((size_t)nc);
                bool any = false;
                for (int i = 0; i < nc; ++i) {
                    const int64_t n = m.sample_len[i];
                    need[(size_t)i] = (k == nk - 1) ? n : std::min(n, (m.clip_hi(k, i) - 1) * (int64_t)t.hop + t.n_fft / 2);
                    any = any || need[(size_t)i] > feed->copied[(size_t)m.clips[i]];
                }
                if (any && feed->raw) {      // the same samples, decoded on the device from the raw bytes
                    if ((rc = pcm_feed(h, *feed, cis, need)) != AEGIS_OK) return rc;
                } else if (any) {
                    for (int i = 0; i < nc; ++i) {
                        int64_t &done = feed->copied[(size_t)m.clips[i]];
                        if (need[(size_t)i] <= done) continue;
                        HIPCHK(h, hipMemcpyAsync(feed->dst + m.sample_off[i] + done, feed->pcm[m.clips[i]] + done,
                                                 (size_t)(need[(size_t)i] - done) * 4, hipMemcpyHostToDevice, h->stream3));
                        done = need[(size_t)i];
                    }
                }
                if (any) {
                    HIPCHK(h, hipEventRecord(h->copy_event, h->stream3));
                    HIPCHK(h, hipStreamWaitEvent(fs, h->copy_event, 0));
                }
            }
            TIMED(h, "frame", fs, launch_frame(p, h->dt, fs, h->inject_d.armed ? static_cast<const double *>(h->inject_d.d.p) : nullptr));
            if (!py) continue;
            TIMED(h, "pyin_obs", fs,
                  if (h->inject.armed) launch_inject_obs(p, static_cast<const double *>(h->inject.obs.p), static_cast<const double *>(h->inject.unv.p), fs);
                  else launch_pyin_obs(p, h->dt, fs));
            if (m.persistent) {
                if (k != h->test_drop_signal)      // AEGIS_TEST_DROP_CHUNK_SIGNAL=k: the kernel's bounded wait is tested with it
                    launch_chunk_signal(static_cast<uint32_t *>(w.chunk_flag.p) + k, p.chunk_gen, fs);
                if (k == 0) {        // the one launch, ordered behind chunk 0 (its first column reads frame 0)
                    HIPCHK(h, hipEventRecord(h->sync_events[EV_CHUNK0], fs));
                    HIPCHK(h, hipStreamWaitEvent(sv, h->sync_events[EV_CHUNK0], 0));
                    PassParams pv = p;
                    pv.vt_begin = 0; pv.vt_end = m.hybrid ? m.hyb_S + 1 : INT64_MAX;
                    hipError_t ve = hipSuccess;
                    TIMED(h, "viterbi", sv, ve = launch_viterbi(pv, h->dt, t.log_trans_band.data(), sv));
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
            if (m.tsplit && !m.hybrid) {
                if ((rc = launch_split(p, m.n_seg, sv, h->stream4 != sv ? h->stream4 : nullptr)) != AEGIS_OK) return rc;
                continue;
            }
            hipError_t ve = hipSuccess;
            TIMED(h, "viterbi", sv, ve = launch_viterbi(p, h->dt, t.log_trans_band.data(), sv));
            VCHK(ve);
        }
        if (m.use_fb) {                    // the dB / rake finalisation needs every chunk's mel rows and clip maxima
            HIPCHK(h, hipEventRecord(h->sync_events[EV_FB], fb));
            HIPCHK(h, hipStreamWaitEvent(fa, h->sync_events[EV_FB], 0));
        }
        if (m.hybrid) {
            // the segments behind step S: after the last chunk's observations (fa; fb has joined it above) and the sequential
            // kernel's last launch (sv), on the unmasked stream
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
            if ((rc = launch_split(ph, 0, sd, h->stream4)) != AEGIS_OK) return rc;
        }
        // ---- finalize ---------------------------------------------------------------------------------------------------
        hipStream_t se = m.hybrid ? sd : sv;       // the stream the pass ends on
        TIMED(h, "finalize", fa, launch_finalize_mel(p, h->dt, fa, h->inject_r.armed ? h->inject_r.flags.as<const uint8_t>() : nullptr));
        if (py) TIMED(h, "finalize", se, launch_decode(p, h->dt, se));
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
        ENSURE(h, finite_flag, 8);
        HIPCHK(h, hipMemsetAsync(h->finite_flag.p, 0xff, 8, s));
        const int64_t lo = sample_offsets[0], hi = sample_offsets[n_clips];
        launch_finite_check(d_pcm + lo, hi - lo, static_cast<unsigned long long *>(h->finite_flag.p), s);
    }
    if (!h->tsplit.checks.empty()) {         // (sync != 0: time-split passes are planned for blocking calls only)
        HIPCHK(h, hipStreamSynchronize(s));
        for (const auto &sc : h->tsplit.checks) {
            const int rc = split_check(h, sc, s);
            if (rc != AEGIS_OK) return rc;
        }
        h->tsplit.checks.clear();
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
