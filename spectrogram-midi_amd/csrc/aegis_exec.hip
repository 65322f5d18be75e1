// The batch executor: analyze_device_locked enqueues the passes plan.cpp plans on the handle's streams, one named step
// after the other (check_call, then per pass open_pass / workspace / chunks / hybrid_segments / close_pass, then join_call
// and the split verdicts).  What a pass owns while it is enqueued is a PassRun.  Which Viterbi launch follows chunk k is
// the plan's statement (PassPlan::viterbi_behind); viterbi_behind_chunk carries it out.
#include "aegis_internal.h"

using namespace aegis;

int aegis::persistent_check(aegis_handle *h) {
    if (!h->persist.pending) return AEGIS_OK;
    h->persist.pending = false;
    uint32_t aborted = 0;
    HIPCHK(h, hipMemcpy(&aborted, h->abort_flag.p, 4, hipMemcpyDeviceToHost));
    if (!aborted) return AEGIS_OK;
    HIPCHK(h, hipMemset(h->abort_flag.p, 0, 4));
    h->err = "the Viterbi kernel gave up waiting for the frame stage (AEGIS_VITERBI_PERSISTENT=0 launches it per chunk)";
    h->persist.gave_up = true;
    return AEGIS_ERR_DEVICE;
}

int aegis::finite_result(aegis_handle *h, uint32_t opts, const int64_t *sample_offsets, int32_t n_clips) {
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

#define VCHK(expr) do { hipError_t ve__ = (expr); if (ve__ != hipSuccess) { h->err = std::string("viterbi launch: ") + hipGetErrorString(ve__); return AEGIS_ERR_DEVICE; } } while (0)

// a pass's parameters for a launch that walks every clip from its first step to its last
static PassParams whole_clip(PassParams p) { p.vt_begin = 0; p.vt_end = INT64_MAX; return p; }

// After a time-split pass has finished: the clips whose decode the verification kernel could not certify (or whose lock-on
// run never met the speculative run) go into `redo`, and the adaptive rule that stops planning split passes when they do
// not pay keeps its books.
static int split_verdict(aegis_handle *h, const aegis_handle::SplitCheck &sc, std::vector<int32_t> &redo) {
    const PassPlan &m = h->plan.passes[sc.pass];
    const int nc = m.nc();
    std::vector<uint32_t> flags((size_t)nc);
    HIPCHK(h, hipMemcpy(flags.data(), sc.p.clip_flag, (size_t)nc * 4, hipMemcpyDeviceToHost));
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
        if (!split_redo_pays(m, redoF, h->tab.half_width)) h->tsplit.cooldown = 32;
    }
    return AEGIS_OK;
}

// The flagged clips are decoded again by the sequential kernel, and the pass is decoded into the outputs once more.  Rare
// (a near-tie on the decoded path that involves a voiced state; a boundary inside a long stretch without a voiced note).
static int redo_flagged(aegis_handle *h, const aegis_handle::SplitCheck &sc, const std::vector<int32_t> &redo, hipStream_t s) {
    aegis_handle::Work &w = h->work[sc.pass & 1];
    HIPCHK(h, hipMemcpy(w.flag_order.p, redo.data(), redo.size() * 4, hipMemcpyHostToDevice));
    PassParams q = whole_clip(sc.p);
    q.order = static_cast<const int32_t *>(w.flag_order.p); q.n_clips = (int32_t)redo.size();
    q.clip_t0 = nullptr; q.clip_t1 = nullptr; q.chunk_flag = nullptr; q.dense = 0;
    VCHK(launch_viterbi(q, h->dt, h->tab.log_trans_band.data(), s));
    launch_decode(sc.p, h->dt, s);
    HIPCHK(h, hipStreamSynchronize(s));
    return AEGIS_OK;
}

// Waits for the call's split passes up to through_pass (inside the call: that pass's done event; behind the last pass: the
// stream), reads their verdicts and redoes what they flag.  A verdict is read before anything overwrites its workspace
// or ensure() moves its buffers: by the pass two further on, or here at the end of the call.
static int read_split_verdicts(aegis_handle *h, hipStream_t s, int through_pass) {
    std::vector<aegis_handle::SplitCheck> &checks = h->tsplit.checks;
    if (checks.empty() || checks.front().pass > through_pass) return AEGIS_OK;
    if (through_pass + 1 < (int)h->plan.passes.size()) HIPCHK(h, hipEventSynchronize(h->sync_events[EV_DONE0 + (through_pass & 1)]));
    else HIPCHK(h, hipStreamSynchronize(s));         // (sync != 0: time-split passes are planned for blocking calls only)
    while (!checks.empty() && checks.front().pass <= through_pass) {
        const aegis_handle::SplitCheck sc = checks.front();
        checks.erase(checks.begin());
        std::vector<int32_t> redo;
        int rc = split_verdict(h, sc, redo);
        if (rc == AEGIS_OK && !redo.empty()) rc = redo_flagged(h, sc, redo, s);
        if (rc != AEGIS_OK) return rc;
    }
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
        uint32_t fm[8] = {}, vm[8] = {};
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
    p.out_f0 = py ? dout->f0 : nullptr; p.out_voiced = py ? dout->voiced_flag : nullptr;
    p.out_vprob = py ? dout->voiced_prob : nullptr; p.out_bin = py ? dout->pitch_bin : nullptr;
    p.out_rms = (stages & AEGIS_STAGE_RMS) ? dout->rms : nullptr; p.out_rake = (stages & AEGIS_STAGE_RAKE) ? dout->rake_mask : nullptr;
    p.out_sdb = mel ? dout->S_dB : nullptr; p.out_colmean = mel ? dout->sdb_col_means : nullptr;
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
        p.n_chunks = m.sequential_chunks();      // (a hybrid pass's launch ends at step S)
        p.abort_flag = h->abort_flag.as<uint32_t>();
        // bound of one chunk wait: a chunk's frame stage takes well under a millisecond per 10 k frames, so 0.1 s plus
        // 0.1 s per million frames of the pass is two orders of magnitude of slack, and a pass that cannot overlap
        // (kernels serialised) costs that much once instead of 1.5 s
        p.wait_ticks = (uint64_t)std::min<int64_t>(150000000, 10000000 + m.fp * 10);
    }
    return p;
}

// ---- a call, and one pass of it, while they are enqueued ------------------------------------------------------------------
struct CallRun {
    aegis_handle *h;
    hipStream_t s;                            // the caller's stream, or the handle's own
    uint32_t stages, opts;
    HostFeed *feed;                           // aegis_analyze_batch / _pcm: the samples come chunk by chunk
    bool done_recorded[2] = {false, false}, split_started = false;   // EV_DONE0 / EV_DONE1 hold a pass of this call; split_ev[0] is recorded
    std::vector<hipStream_t> joined;          // streams whose work s must wait for before the call returns
};

struct PassRun {
    CallRun &c;
    aegis_handle *h; const PassPlan &m;
    aegis_handle::Work &w;                    // passes alternate between the handle's two
    int pi;
    hipStream_t s, fa = nullptr, fb = nullptr, sv = nullptr, sd = nullptr, sa = nullptr;   // the call's stream; the plan's lanes, resolved
    PassParams p{};
    const int32_t *d_seg_order = nullptr, *d_lock_order = nullptr;

    PassRun(CallRun &c_, int pi_) : c(c_), h(c_.h), m(c_.h->plan.passes[pi_]), w(c_.h->work[pi_ & 1]), pi(pi_), s(c_.s) {}
    bool pyin() const { return c.stages & AEGIS_STAGE_PYIN; }
    int open_pass(), workspace(const float *d_pcm, const aegis_outputs *dout, double rake_sensitivity), chunks(), hybrid_segments(), close_pass();
    void chunk_params(int k);
    int viterbi_behind_chunk(int k, hipStream_t fs), launch_split(const PassParams &q, int n_spec, hipStream_t sq, hipStream_t aux);
};

// Acts on the verdict of the pass two back (this pass takes over its workspace), then resolves the plan's lanes and orders
// them behind the caller's earlier work on s and behind the workspace's previous pass.
int PassRun::open_pass() {
    const int rc = read_split_verdicts(h, s, pi - 2);
    if (rc != AEGIS_OK) return rc;
    const aegis_handle::SplitSet *ss = m.fa == Lane::masked_frame_a ? split_streams(h, m.nc()) : nullptr;
    fa = lane_stream(h, m.fa, s, ss); fb = lane_stream(h, m.fb, s, ss); sv = lane_stream(h, m.sv, s, ss);
    sd = lane_stream(h, m.sd, s, ss); sa = lane_stream(h, m.sa, s, ss);
    std::vector<hipStream_t> &joined = c.joined;
    auto join_later = [&](hipStream_t q) { if (q != s && std::find(joined.begin(), joined.end(), q) == joined.end()) joined.push_back(q); };
    const hipEvent_t done = h->sync_events[EV_DONE0 + (pi & 1)];      // this workspace's previous pass, two back
    if (pi == 0) HIPCHK(h, hipEventRecord(h->sync_events[EV_START], s));
    for (hipStream_t q : {fa, fb, sv, sd, sa}) {
        if (q == s || q == nullptr) continue;
        if (std::find(joined.begin(), joined.end(), q) == joined.end())
            HIPCHK(h, hipStreamWaitEvent(q, h->sync_events[EV_START], 0));      // the caller's earlier work on s comes first
        if (c.done_recorded[pi & 1]) HIPCHK(h, hipStreamWaitEvent(q, done, 0));      // everything of that pass must have finished
    }
    if (fa == s && c.done_recorded[pi & 1]) HIPCHK(h, hipStreamWaitEvent(s, done, 0));
    join_later(fa); join_later(sv); if (m.use_fb) join_later(fb); if (sd) { join_later(sd); join_later(sa); }
    return AEGIS_OK;
}

// The workspace sized, filled from the plan and bound into p.
int PassRun::workspace(const float *d_pcm, const aegis_outputs *dout, double rake_sensitivity) {
    int rc;
    if ((rc = ensure_pass(h, w, m, c.stages)) != AEGIS_OK) return rc;
    if ((rc = upload_pass(h, w, m, c.stages, fa)) != AEGIS_OK) return rc;
    if (m.use_fb || m.persistent) {      // the metadata precedes the second frame stream's kernels and the Viterbi
        HIPCHK(h, hipEventRecord(h->sync_events[EV_META], fa));
        if (m.use_fb) HIPCHK(h, hipStreamWaitEvent(fb, h->sync_events[EV_META], 0));
        if (m.persistent) HIPCHK(h, hipStreamWaitEvent(sv, h->sync_events[EV_META], 0));
    }
    p = bind_pass(h, m, w, d_pcm, c.stages, c.opts, dout, rake_sensitivity);
    const SegLayout L(m.n_seg, m.nc(), m.n_lock);
    d_seg_order = m.tsplit ? w.seg32.as<const int32_t>() + L.seg_order : nullptr;
    d_lock_order = m.tsplit ? w.seg32.as<const int32_t>() + L.lock_order : nullptr;
    if (m.persistent) {
        p.chunk_gen = ++h->chunk_gen;
        if (p.chunk_gen == 0) p.chunk_gen = ++h->chunk_gen;
        h->persist.pending = true;
    }
    return AEGIS_OK;
}

// p as the kernels of time chunk k read it: the chunk's frames, and the Viterbi steps of a launch for this chunk alone
void PassRun::chunk_params(int k) {
    const int nc = m.nc();
    p.sel_off = static_cast<const int64_t *>(w.sel_off.p) + (size_t)k * (nc + 1);
    p.t_begin = m.cb[k]; p.n_sel = m.sel_off[(size_t)k * (nc + 1) + nc];
    p.vt_begin = m.cb[k];
    p.vt_end = (k == m.nk() - 1) ? INT64_MAX : m.cb[k + 1];
    p.clip_t0 = m.proportional ? static_cast<const int64_t *>(w.clip_tb.p) + (size_t)k * nc : nullptr;
    p.clip_t1 = m.proportional ? static_cast<const int64_t *>(w.clip_tb.p) + (size_t)(k + 1) * nc : nullptr;
}

// The time chunks: a host feed's samples, the frame stage, the observations, then the Viterbi launch the plan puts behind them.
int PassRun::chunks() {
    for (int k = 0; k < m.nk(); ++k) {
        hipStream_t fs = ((m.two_fs || k < m.ramp_k) && (k & 1)) ? fb : fa;
        chunk_params(k);
        int rc;
        if (c.feed && (rc = c.feed->bring(h, m, k, fs)) != AEGIS_OK) return rc;
        TIMED(h, "frame", fs, launch_frame(p, h->dt, fs, h->inject_d.armed ? static_cast<const double *>(h->inject_d.d.p) : nullptr));
        if (pyin()) {
            TIMED(h, "pyin_obs", fs,
                  if (h->inject.armed) launch_inject_obs(p, static_cast<const double *>(h->inject.obs.p), static_cast<const double *>(h->inject.unv.p), fs);
                  else launch_pyin_obs(p, h->dt, fs));
            if ((rc = viterbi_behind_chunk(k, fs)) != AEGIS_OK) return rc;
        }
    }
    if (m.use_fb) {                    // the dB / rake finalisation needs every chunk's mel rows and clip maxima
        HIPCHK(h, hipEventRecord(h->sync_events[EV_FB], fb));
        HIPCHK(h, hipStreamWaitEvent(fa, h->sync_events[EV_FB], 0));
    }
    return AEGIS_OK;
}

// A time-split launch (a plain split pass's, a hybrid pass's): an automatic call is timed from its first one to its last
// one (split_ev), and each leaves a verdict that read_split_verdicts reads once the pass is done.
int PassRun::launch_split(const PassParams &q, int n_spec, hipStream_t sq, hipStream_t aux) {
    hipError_t ve = hipSuccess;
    TIMED(h, "viterbi", sq,
          if (m.split_auto && !c.split_started) { HIPCHK(h, hipEventRecord(h->split_ev[0], sq)); c.split_started = true; }
          ve = launch_viterbi_split(q, h->dt, h->tab.log_trans_band.data(), d_seg_order, n_spec, d_lock_order, m.n_lock, sq, aux, h->fin_ev);
          if (m.split_auto) HIPCHK(h, hipEventRecord(h->split_ev[1], sq)));
    VCHK(ve);
    h->tsplit.checks.push_back({pi, q});
    ++h->tsplit.stats[0]; h->tsplit.stats[1] += m.n_seg;
    return AEGIS_OK;
}

// What follows chunk k's observations (on fs): the chunk signal of a persistent pass, and the launch the plan names.
int PassRun::viterbi_behind_chunk(int k, hipStream_t fs) {
    const ViterbiBehind what = m.viterbi_behind(k);
    if (m.persistent && k != h->test_drop_signal)      // AEGIS_TEST_DROP_CHUNK_SIGNAL=k: the kernel's bounded wait is tested with it
        launch_chunk_signal(static_cast<uint32_t *>(w.chunk_flag.p) + k, p.chunk_gen, fs);
    if (what == ViterbiBehind::none) return AEGIS_OK;
    if (sv != fs || what == ViterbiBehind::single_launch) {      // (the one launch is ordered behind chunk 0 on any stream)
        HIPCHK(h, hipEventRecord(h->sync_events[EV_CHUNK0 + k], fs));
        HIPCHK(h, hipStreamWaitEvent(sv, h->sync_events[EV_CHUNK0 + k], 0));
    }
    if (what == ViterbiBehind::segments) return launch_split(p, m.n_seg, sv, h->stream4 != sv ? h->stream4 : nullptr);
    PassParams pv = what == ViterbiBehind::single_launch ? whole_clip(p) : p;      // every chunk in one launch, or this one
    if (what == ViterbiBehind::single_launch && m.hybrid) pv.vt_end = m.hyb_S + 1;     // (a hybrid pass's ends at step S)
    hipError_t ve = hipSuccess;
    TIMED(h, "viterbi", sv, ve = launch_viterbi(pv, h->dt, h->tab.log_trans_band.data(), sv));
    VCHK(ve);
    return AEGIS_OK;
}

// A hybrid pass's segments behind step S: after the last chunk's observations (fa; fb has joined it) and the sequential
// kernel's last launch (sv), on the unmasked stream.
int PassRun::hybrid_segments() {
    PassParams ph = whole_clip(p);
    ph.split_hybrid = 1; ph.hybrid_step = (int32_t)m.hyb_S;
    // the speculative runs need the observations only: they start behind the frame stage, on the compute units it has
    // left, while the sequential kernel walks its last chunks; lock-on runs and everything after wait for both
    if (sa != fa) {
        HIPCHK(h, hipEventRecord(h->hyb_ev[0], fa));
        HIPCHK(h, hipStreamWaitEvent(sa, h->hyb_ev[0], 0));
    }
    VCHK(launch_viterbi_split_spec(ph, h->dt, h->tab.log_trans_band.data(), d_seg_order, m.n_lock, sa));
    HIPCHK(h, hipEventRecord(h->hyb_ev[2], sa));
    if (sd != sv) {
        HIPCHK(h, hipEventRecord(h->hyb_ev[1], sv));
        HIPCHK(h, hipStreamWaitEvent(sd, h->hyb_ev[1], 0));
    }
    HIPCHK(h, hipStreamWaitEvent(sd, h->hyb_ev[2], 0));
    return launch_split(ph, 0, sd, h->stream4);
}

// Finalize and decode; pass done = its last kernels on the frame stream and on the Viterbi stream.
int PassRun::close_pass() {
    hipStream_t se = m.hybrid ? sd : sv;       // the stream the pass ends on
    TIMED(h, "finalize", fa, launch_finalize_mel(p, h->dt, fa, h->inject_r.armed ? h->inject_r.flags.as<const uint8_t>() : nullptr));
    if (pyin()) TIMED(h, "finalize", se, launch_decode(p, h->dt, se));
    if (se != fa) {
        HIPCHK(h, hipEventRecord(h->sync_events[EV_FA], fa));
        HIPCHK(h, hipStreamWaitEvent(se, h->sync_events[EV_FA], 0));
    }
    HIPCHK(h, hipEventRecord(h->sync_events[EV_DONE0 + (pi & 1)], se));
    c.done_recorded[pi & 1] = true;
    HIPCHK(h, hipGetLastError());
    if (const HostFeed *feed = c.feed; feed && feed->raw && feed->raw->y_out) {      // the pass's samples back to the host, behind its last decode
        for (int i = 0; i < m.nc(); ++i)
            if (m.sample_len[i] > 0)
                HIPCHK(h, hipMemcpyAsync(feed->raw->y_out + m.sample_off[i], feed->dst + m.sample_off[i], (size_t)m.sample_len[i] * 4,
                                         hipMemcpyDeviceToHost, h->stream3));
    }
    return AEGIS_OK;
}

// Arguments, clips and an armed injection hook.  stages comes back with what RAKE implies and without the option bits,
// which go to opts.  (n_clips == 0 is AEGIS_OK: the caller has nothing to do.)
static int check_call(aegis_handle *h, const float *d_pcm, const int64_t *sample_offsets, int32_t n_clips, uint32_t &stages,
                      uint32_t &opts, const aegis_outputs *dout, int32_t sync) {
    if (n_clips < 0 || (n_clips > 0 && (!sample_offsets || !dout))) { h->err = "null argument"; return AEGIS_ERR_INVALID; }
    if (n_clips == 0) return AEGIS_OK;
    if (stages & AEGIS_STAGE_RAKE) stages |= AEGIS_STAGE_MEL;
    opts = stages & (AEGIS_OPT_CHECK_FINITE | AEGIS_OPT_F0_ZERO);
    stages &= AEGIS_STAGE_ALL;
    if ((opts & AEGIS_OPT_CHECK_FINITE) && sync == 0) {      // the verdict is read after a synchronisation: nobody would read it
        h->err = "AEGIS_OPT_CHECK_FINITE needs sync != 0 (the verdict is reported by the call that synchronises)";
        return AEGIS_ERR_INVALID;
    }
    const Tables &t = h->tab;
    DEVICE_ONLY(h);
    HIPCHK(h, hipSetDevice(h->device));
    int64_t F = 0;
    for (int i = 0; i < n_clips; ++i) {
        const int64_t n = sample_offsets[i + 1] - sample_offsets[i];
        if (n < 0) { h->err = "sample_offsets must be non-decreasing"; return AEGIS_ERR_INVALID; }
        if (n > 0 && !d_pcm) { h->err = "d_pcm == NULL"; return AEGIS_ERR_INVALID; }
        if (1 + n / t.hop > h->max_frames_per_pass) {
            h->err = "clip of " + std::to_string(1 + n / t.hop) + " frames exceeds max_frames_per_pass=" + std::to_string(h->max_frames_per_pass);
            return AEGIS_ERR_INVALID;
        }
        F += 1 + n / t.hop;
    }
    // An armed injection hook (at most one: each setter refuses while another is armed) holds rows indexed by this call's
    // output frames: aegis_debug_set_observations, aegis_debug_set_difference, aegis_debug_set_rake_columns.
    const struct { bool armed; int64_t F; uint32_t stage; const char *what, *stage_name; } hooks[] = {
        {h->inject.armed, h->inject.F, AEGIS_STAGE_PYIN, "injected observations", "PYIN"},
        {h->inject_d.armed, h->inject_d.F, AEGIS_STAGE_PYIN, "injected difference rows", "PYIN"},
        {h->inject_r.armed, h->inject_r.F, AEGIS_STAGE_RAKE, "injected rake columns", "RAKE"},
    };
    for (const auto &k : hooks) {
        if (!k.armed || ((stages & k.stage) && F == k.F)) continue;
        h->err = std::string(k.what) + ": the call needs the " + k.stage_name + " stage and exactly " + std::to_string(k.F) + " frames (it has " + std::to_string(F) + ")";
        return AEGIS_ERR_INVALID;
    }
    return AEGIS_OK;
}

// (the fixed events exist since aegis_create; the call's longest pass may need more per-chunk ones)
static int reserve_chunk_events(aegis_handle *h) {
    for (const PassPlan &m : h->plan.passes)
        while ((int)h->sync_events.size() < EV_CHUNK0 + m.nk()) {
            hipEvent_t e;
            const int rc = new_event(h, &e, hipEventDisableTiming);
            if (rc != AEGIS_OK) return rc;
            h->sync_events.push_back(e);
        }
    return AEGIS_OK;
}

// The caller's stream continues after everything the passes enqueued; the finite check comes behind the last sample copy
// of a host feed (every sample is on the device by then).
static int join_call(CallRun &c, const float *d_pcm, const int64_t *sample_offsets, int32_t n_clips) {
    aegis_handle *h = c.h;
    for (int q = 0; q < 2; ++q)
        if (c.done_recorded[q]) HIPCHK(h, hipStreamWaitEvent(c.s, h->sync_events[EV_DONE0 + q], 0));
    if (c.opts & AEGIS_OPT_CHECK_FINITE) {
        ENSURE(h, finite_flag, 8);
        HIPCHK(h, hipMemsetAsync(h->finite_flag.p, 0xff, 8, c.s));
        const int64_t lo = sample_offsets[0], hi = sample_offsets[n_clips];
        launch_finite_check(d_pcm + lo, hi - lo, static_cast<unsigned long long *>(h->finite_flag.p), c.s);
    }
    return AEGIS_OK;
}

int aegis::analyze_device_locked(aegis_handle *h, const float *d_pcm, const int64_t *sample_offsets, int32_t n_clips,
                                 double rake_sensitivity, uint32_t stages, aegis_outputs *dout, void *stream_v, int32_t sync,
                                 HostFeed *feed) {
    if (!h) return AEGIS_ERR_INVALID;
    uint32_t opts = 0;
    int rc = check_call(h, d_pcm, sample_offsets, n_clips, stages, opts, dout, sync);
    if (rc != AEGIS_OK || n_clips == 0) return rc;
    hipStream_t s = stream_v ? static_cast<hipStream_t>(stream_v) : h->stream;
    // host arrays of the previous call's plan are no longer referenced once the stream drained
    if (h->plan_in_flight) { HIPCHK(h, hipStreamSynchronize(s)); h->plan_in_flight = false; }
    h->tsplit.checks.clear();
    drop_events(h);
    const PlanInput in = plan_input(h, sample_offsets, n_clips, stages, feed != nullptr, stream_v != nullptr, sync, h->n_cus,
                                    [h](int n) { return split_streams(h, n) != nullptr; });
    if (in.cooling) --h->tsplit.cooldown;
    h->plan = plan_call(in);
    h->plan_in_flight = true;
    if ((rc = reserve_chunk_events(h)) != AEGIS_OK) return rc;
    CallRun c{h, s, stages, opts, feed};
    const int n_passes = (int)h->plan.passes.size();
    for (int pi = 0; pi < n_passes; ++pi) {
        PassRun r(c, pi);
        if ((rc = r.open_pass()) != AEGIS_OK) return rc;
        if ((rc = r.workspace(d_pcm, dout, rake_sensitivity)) != AEGIS_OK) return rc;
        if ((rc = r.chunks()) != AEGIS_OK) return rc;
        if (r.m.hybrid && (rc = r.hybrid_segments()) != AEGIS_OK) return rc;
        if ((rc = r.close_pass()) != AEGIS_OK) return rc;
    }
    if ((rc = join_call(c, d_pcm, sample_offsets, n_clips)) != AEGIS_OK) return rc;
    if ((rc = read_split_verdicts(h, s, n_passes - 1)) != AEGIS_OK) return rc;
    if (sync != 1) return AEGIS_OK;
    HIPCHK(h, hipStreamSynchronize(s));
    h->plan_in_flight = false;
    if (h->profiling) collect_events(h);
    if ((rc = persistent_check(h)) != AEGIS_OK) return rc;
    return finite_result(h, opts, sample_offsets, n_clips);
}
