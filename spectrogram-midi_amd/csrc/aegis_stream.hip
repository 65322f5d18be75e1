// Streaming entries of libaegis_hip.so (aegis_stream_*): one clip fed push by push, the fixed-size push captured as a
// hipGraph, delivery of the frames whose decode is already final.
#include "aegis_internal.h"

#include <cstdlib>
#include <new>

using namespace aegis;

extern "C" {

// The kernels' view of the stream: a pass of one clip whose offset tables are the meta block at dm (device: the stream's
// own copy, or the one inside the graph's control block).
static PassParams stream_params(aegis_stream *st, const int64_t *dm) {
    aegis_handle *h = st->h;
    PassParams p = base_params(h->tab);
    p.stages = AEGIS_STAGE_ALL;
    p.pcm = st->pcm.as<const float>();
    p.sample_off = dm + kMetaSampleOff; p.sample_len = dm + kMetaSampleOff + 1;
    p.frame_off = dm + kMetaFrameOff; p.out_off = dm + kMetaFrameOff; p.sel_off = dm + kMetaSelOff;
    p.chunk_off = const_cast<int64_t *>(dm + kMetaChunkOff);
    p.order = reinterpret_cast<const int32_t *>(dm + kMetaOrder);
    p.n_clips = 1;
    bind_core(p, h, *st);
    p.live_states = st->live.as<int32_t>();
    p.out_vprob = st->o_vprob.as<double>(); p.out_rms = st->o_rms.as<float>();
    p.out_f0 = st->o_f0.as<double>(); p.out_voiced = st->o_voiced.as<uint8_t>();
    p.out_rake = st->o_rake.as<uint8_t>(); p.out_sdb = st->o_sdb.as<float>();
    p.rake_ratio = 0.6;
    return p;
}
// Chunk maps a clip of F frames composes (its F - 1 steps, kViterbiChunk to a map).
static int64_t stream_chunks(int64_t F) { return (F - 1 + kViterbiChunk - 1) / kViterbiChunk; }

static StreamCommitCtl *stream_commit_ctl(aegis_stream *st) {
    return reinterpret_cast<StreamCommitCtl *>(static_cast<unsigned char *>(st->ctl.p) + sizeof(StreamCtl));
}

// aegis_debug_stream_set_observations: behind every launch of the observation kernel of an armed stream, the same frames
// take their rows from the stream's own copy (one more node of the one chain; the kernel reads its geometry as
// pyin_obs_kernel does, so it replays under ctl).  The entries have checked that no selected frame is >= inject.F.
static void stream_inject(aegis_stream *st, const PassParams &p, hipStream_t s) {
    if (st->inject.armed)
        launch_inject_obs(p, static_cast<const double *>(st->inject.obs.p), static_cast<const double *>(st->inject.unv.p), s);
}
// An armed stream has rows for inject.F frames: a push may complete at most that many, close() decodes exactly that many.
// `frames`: the count the push would reach, or close()'s.  AEGIS_ERR_INVALID names both counts.
static int stream_inject_fits(aegis_stream *st, int64_t frames, bool closing) {
    if (!st->inject.armed || (closing ? frames == st->inject.F : frames <= st->inject.F)) return AEGIS_OK;
    st->h->err = std::string("injected observations: ") + (closing ? "close() would decode " : "the push would complete ") +
                 std::to_string(frames) + " frames, the stream was armed with " + std::to_string(st->inject.F);
    return AEGIS_ERR_INVALID;
}

// Captures one fixed-size push as a hipGraph: H2D of the samples, advance (append + geometry), the four
// analysis kernels reading their geometry from the device control block, result gather, D2H.
static bool stream_build_graph(aegis_stream *st, int64_t n_push, hipStream_t s, int commit) {
    aegis_handle *h = st->h;
    const Tables &t = h->tab;
    if (!st->pin_samples || !st->pin_result || (commit && !st->pin_commit) || !stream_push_replays(n_push, t.hop)) return false;
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
    stream_inject(st, p, s);
    ok &= launch_viterbi(p, h->dt, t.log_trans_band.data(), s) == hipSuccess;
    if (commit)
        ok &= launch_stream_commit(ctl, 0, stream_commit_ctl(st), p.ptr, p.vstate, t.n_bins, static_cast<int16_t *>(st->c_bins.p),
                                   st->c_result.p, s) == hipSuccess;
    launch_stream_gather(ctl, p.out_rms, p.out_vprob, p.live_states, st->g_result.p, s);
    ok &= hipMemcpyAsync(st->pin_result, st->g_result.p, kGatherBytes, hipMemcpyDeviceToHost, s) == hipSuccess;
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
    const int64_t Ftot = final_pass ? f_hi : st->cap_frames;     // clip length as far as the kernels know
    st->host_meta.assign(kMetaSlots, 0);
    st->host_meta[kMetaSampleOff + 1] = st->n_samples;
    st->host_meta[kMetaFrameOff + 1] = Ftot;
    st->host_meta[kMetaSelOff + 1] = f_hi - f_lo;
    st->host_meta[kMetaChunkOff + 1] = stream_chunks(Ftot);
    HIPCHK(h, hipMemcpyAsync(st->meta.p, st->host_meta.data(), kMetaSlots * 8, hipMemcpyHostToDevice, s));
    PassParams p = stream_params(st, st->meta.as<const int64_t>());
    p.n_frames = Ftot;
    p.t_begin = f_lo; p.n_sel = f_hi - f_lo;
    p.vt_begin = f_lo; p.vt_end = final_pass ? INT64_MAX : f_hi;
    if (p.n_sel > 0) {
        launch_frame(p, h->dt, s);
        launch_pyin_obs(p, h->dt, s);
        stream_inject(st, p, s);
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
    free_bufs(st->bufs);
    delete st;
}

static int stream_open_locked(aegis_handle *h, int64_t max_samples, aegis_stream *st) {
    HIPCHK(h, hipSetDevice(h->device));
    st->h = h;
    const Tables &t = h->tab;
    st->cap_samples = max_samples;
    st->cap_frames = 1 + max_samples / t.hop;
    const int64_t F = st->cap_frames;
    PassGeometry g;                           // one clip of the stream's capacity, every stage
    g.F = F; g.S = 2 * t.n_bins; g.cmap_rows = stream_chunks(F) + 1;
    g.lag_stride = h->lag_stride; g.yin_stride = h->yin_stride; g.obs_stride = h->obs_stride; g.n_mels = t.n_mels;
    const PassBytes b = pass_bytes(g);
    const size_t clipmax_bytes = std::max<size_t>(b.clipmax, 16);      // (16: what a stream has always asked for its one maximum)
    int rc = AEGIS_OK;
    auto need = [&](DevBuf &buf, size_t bytes) { if (rc == AEGIS_OK) rc = ensure(st, buf, bytes); };      // (the handle's fail_allocs hook, the stream's list)
    need(st->pcm, max_samples * 4); need(st->dfn, b.dfn);
    need(st->logobs, b.logobs); need(st->logunv, b.logunv); need(st->obs_seg, b.obs_seg); need(st->ptr, b.ptr);
    need(st->cmap, b.cmap); need(st->bnd, b.bnd); need(st->states, b.states); need(st->live, F * 4);
    need(st->melpow, b.melpow); need(st->clipmax, clipmax_bytes); need(st->rake_raw, b.rake_raw); need(st->vstate, b.vstate);
    need(st->meta, kMetaSlots * 8); need(st->ctl, sizeof(StreamCtl) + sizeof(StreamCommitCtl)); need(st->g_staging, kStreamStaging * 4); need(st->g_result, kGatherBytes);
    need(st->c_bins, F * 2); need(st->c_result, kCommitResultBytes);
    need(st->o_f0, F * 8); need(st->o_voiced, F); need(st->o_vprob, F * 8); need(st->o_rms, F * 4); need(st->o_rake, F);
    need(st->o_sdb, F * t.n_mels * 4);
    if (rc != AEGIS_OK) return rc;
    HIPCHK(h, hipMemsetAsync(st->clipmax.p, 0, clipmax_bytes, h->stream));
    // The band Viterbi leaves the back-pointer of a dead voiced state unwritten, and a launch that starts inside a 16-step
    // chunk (any push that is not a whole number of chunks) walks the rows of the chunk's earlier steps for EVERY state to
    // rebuild its chunk map (viterbi_band.inc, "rebuilds org from the HBM pointers").  What it reads for a dead state is
    // never used, but it is used as the next index: with recycled memory behind the rows an index up to 65535 reaches
    // 128 KB past a short stream's last row (an illegal access on a 0.5 s stream, met in the test suite).  Zeroed rows keep
    // every such index at state 0.
    HIPCHK(h, hipMemsetAsync(st->ptr.p, 0, b.ptr, h->stream));
    {
        struct { StreamCtl ctl; StreamCommitCtl commit; } c0{};
        static_assert(sizeof(c0) == sizeof(StreamCtl) + sizeof(StreamCommitCtl), "the commit block sits right behind the control block");
        c0.ctl.meta[kMetaFrameOff + 1] = F;
        c0.ctl.meta[kMetaChunkOff + 1] = stream_chunks(F);
        c0.commit.frontier = -1; c0.commit.newest = -1;
        HIPCHK(h, hipMemcpyAsync(st->ctl.p, &c0, sizeof(c0), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (hipHostMalloc(reinterpret_cast<void **>(&st->pin_samples), kStreamStaging * 4, hipHostMallocDefault) != hipSuccess) st->pin_samples = nullptr;
    if (hipHostMalloc(reinterpret_cast<void **>(&st->pin_result), kGatherBytes, hipHostMallocDefault) != hipSuccess) st->pin_result = nullptr;
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
    ENTRY(h)
    if (!out || max_samples <= 0) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    *out = nullptr;
    DEVICE_ONLY(h);
    if (h->destroy_requested) { h->err = "handle was destroyed"; return AEGIS_ERR_INVALID; }
    // nothing leaks on a failed open: a stream not handed out is released on the way out, by a return or an exception
    struct HalfBuilt { aegis_stream *st; ~HalfBuilt() { if (st) stream_release(st); } } half{new (std::nothrow) aegis_stream()};
    if (!half.st) { h->err = "out of host memory"; return AEGIS_ERR_NOMEM; }
    const int rc = stream_open_locked(h, max_samples, half.st);
    if (rc != AEGIS_OK) return rc;
    ++h->open_streams;
    *out = half.st;
    half.st = nullptr;
    return AEGIS_OK;
    ENTRY_END(h)
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
    if (n < 0 || (n > 0 && !samples) || !n_frames) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    if (commit && (commit->cap < 0 || (commit->cap > 0 && !commit->pitch_bin))) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    if (st->closed) { h->err = "stream is closed"; return AEGIS_ERR_INVALID; }
    if (st->n_samples + n > st->cap_samples) { h->err = "stream capacity exceeded"; return AEGIS_ERR_INVALID; }
    if (st->inject.armed) {      // before anything is consumed: no row past inject.F is ever read
        const int rc = stream_inject_fits(st, stream_frames_ready(st->n_samples + n, h->tab.hop), false);
        if (rc != AEGIS_OK) return rc;
    }
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const int ci = commit ? 1 : 0;
    // ---- fixed-size pushes replay a captured hipGraph ---------------------------------------------
    if (stream_push_replays(n, h->tab.hop) && !st->graph_failed && (st->graph_exec[ci] == nullptr || st->graph_push[ci] == n)) {
        if (st->graph_exec[ci] == nullptr && !stream_build_graph(st, n, s, ci)) st->graph_failed = true;
        if (st->graph_exec[ci] != nullptr && st->graph_push[ci] == n) {
            std::memcpy(st->pin_samples, samples, (size_t)n * 4);
            HIPCHK(h, hipGraphLaunch(st->graph_exec[ci], s));
            HIPCHK(h, hipStreamSynchronize(s));
            st->n_samples += n;
            const int64_t lo = st->frames_done, hi = std::max(lo, stream_frames_ready(st->n_samples, h->tab.hop));
            int64_t got = 0;
            std::memcpy(&got, st->pin_result + kGatherCount, 8);
            if (got != hi - lo) { h->err = "stream graph and host disagree on the frame count"; return AEGIS_ERR_DEVICE; }
            st->frames_done = hi;
            *n_frames = got;
            if (out) {
                if (out->rms) std::memcpy(out->rms, st->pin_result + kGatherRms, (size_t)got * 4);
                if (out->voiced_prob) std::memcpy(out->voiced_prob, st->pin_result + kGatherVprob, (size_t)got * 8);
                if (out->live_state) std::memcpy(out->live_state, st->pin_result + kGatherLive, (size_t)got * 4);
            }
            return commit ? stream_deliver(st, st->pin_commit, commit) : AEGIS_OK;
        }
    }
    // ---- plain launches.  The stream reads `samples`, st->host_meta (stream_run) and `counters`, and writes the caller's
    // out->rms / voiced_prob / live_state and the commit result block (pinned, or st->commit_host): all of them outlive
    // the scope
    int64_t counters[2];
    StreamScope scope(h);
    if (n > 0)
        HIPCHK(h, hipMemcpyAsync(static_cast<float *>(st->pcm.p) + st->n_samples, samples, n * 4, hipMemcpyHostToDevice, s));
    st->n_samples += n;
    const int64_t lo = st->frames_done, hi = std::max(lo, stream_frames_ready(st->n_samples, h->tab.hop));
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
    // the device control block of the graph path mirrors the host counters
    counters[0] = st->n_samples; counters[1] = st->frames_done;
    HIPCHK(h, hipMemcpyAsync(st->ctl.p, counters, 16, hipMemcpyHostToDevice, s));
    // commit: one more launch behind the Viterbi, when there is a frame the last walk has not seen (also the frames of
    // earlier plain pushes: the walk goes from the newest frame back to the frontier, however far that is)
    unsigned char *cres = nullptr;
    if (commit && st->frames_done > 0 && st->frames_done - 1 != st->c_newest) {
        cres = st->pin_commit ? st->pin_commit : st->commit_host;
        hipError_t ce = launch_stream_commit(nullptr, st->frames_done, stream_commit_ctl(st), st->ptr.as<const uint16_t>(),
                                             st->vstate.as<const double>(), h->tab.n_bins, st->c_bins.as<int16_t>(), st->c_result.p, s);
        if (ce != hipSuccess) { h->err = std::string("stream commit launch: ") + hipGetErrorString(ce); return AEGIS_ERR_DEVICE; }
        HIPCHK(h, hipMemcpyAsync(cres, st->c_result.p, kCommitResultBytes, hipMemcpyDeviceToHost, s));
    }
    const int rc = scope.finish();
    if (rc != AEGIS_OK) return rc;
    return commit ? stream_deliver(st, cres, commit) : AEGIS_OK;      // (after the drain: it may end in a synchronous copy)
}

int aegis_stream_push(aegis_stream *st, const float *samples, int64_t n, aegis_stream_frames *out, int64_t *n_frames) {
    STREAM_ENTRY(st)
    return stream_push_locked(st, samples, n, out, n_frames, nullptr);
    STREAM_ENTRY_END(st)
}

int aegis_stream_push_commit(aegis_stream *st, const float *samples, int64_t n, aegis_stream_frames *out, int64_t *n_frames,
                             aegis_stream_commit *commit) {
    STREAM_ENTRY(st)
    return stream_push_locked(st, samples, n, out, n_frames, commit);
    STREAM_ENTRY_END(st)
}

int aegis_stream_close(aegis_stream *st, double rake_sensitivity, aegis_outputs *out, int64_t *n_frames) {
    STREAM_ENTRY(st)
    aegis_handle *h = st->h;
    if (!n_frames) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    if (st->closed) { h->err = "stream is closed"; return AEGIS_ERR_INVALID; }
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const Tables &t = h->tab;
    const int64_t F = 1 + st->n_samples / t.hop;
    int rc = stream_inject_fits(st, F, true);
    if (rc != AEGIS_OK) return rc;                              // (the stream stays open: more samples may still make it F)
    // The stream reads st->host_meta (stream_run) and writes the caller's arrays behind `out`: they outlive the scope.
    StreamScope scope(h);
    rc = stream_run(st, st->frames_done, F, true, s);           // zero-padded tail frames + back-trace
    if (rc != AEGIS_OK) return rc;
    // clip-global stages over all F frames: the selection is the whole clip (the frame offsets; the meta block's own
    // selection still counts the frames of the last launch)
    PassParams p = stream_params(st, st->meta.as<const int64_t>());
    p.sel_off = p.frame_off; p.n_frames = F; p.n_sel = F;
    p.rake_ratio = rake_sensitivity;
    launch_finalize_mel(p, h->dt, s);
    launch_decode(p, h->dt, s);
    HIPCHK(h, hipGetLastError());
    st->frames_done = F;
    st->closed = true;
    *n_frames = F;
    if (out) {
        for (const OutField &f : kOutFields)
            if (f.st && f.get(out)) HIPCHK(h, hipMemcpyAsync(f.get(out), (st->*f.st).p, f.size(F, t.n_mels), hipMemcpyDeviceToHost, s));
    }
    return scope.finish();
    STREAM_ENTRY_END(st)
}

int aegis_debug_stream_set_observations(aegis_stream *st, const double *logobs, const double *logunv, int64_t F) {
    STREAM_ENTRY(st)
    aegis_handle *h = st->h;
    if (st->closed) { h->err = "stream is closed"; return AEGIS_ERR_INVALID; }
    if (st->n_samples > 0) { h->err = "injected observations: a stream is armed before its first sample (it has " + std::to_string(st->n_samples) + ")"; return AEGIS_ERR_INVALID; }
    if (!logobs || !logunv || F <= 0) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    if (F > st->cap_frames) {
        h->err = "injected observations: " + std::to_string(F) + " frames, the stream holds at most " + std::to_string(st->cap_frames);
        return AEGIS_ERR_INVALID;
    }
    int rc;
    if ((rc = check_observation_rows(h, logobs, logunv, F)) != AEGIS_OK) return rc;
    const int B = h->tab.n_bins;
    HIPCHK(h, hipSetDevice(h->device));
    st->inject.armed = false;                 // (arming again replaces the rows; nothing of this stream is in flight: no sample yet)
    if ((rc = ensure(st, st->inject.obs, (size_t)F * B * 8)) != AEGIS_OK) return rc;
    if ((rc = ensure(st, st->inject.unv, (size_t)F * 8)) != AEGIS_OK) return rc;
    HIPCHK(h, hipMemcpy(st->inject.obs.p, logobs, (size_t)F * B * 8, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(st->inject.unv.p, logunv, (size_t)F * 8, hipMemcpyHostToDevice));
    st->inject.F = F;
    st->inject.armed = true;
    return AEGIS_OK;
    STREAM_ENTRY_END(st)
}

int64_t aegis_debug_stream_fetch(aegis_stream *st, const char *name, void *dst, int64_t cap) {
    STREAM_ENTRY(st)
    aegis_handle *h = st->h;
    if (!name) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    const std::string n(name);
    const void *src = nullptr;
    int64_t count = 0, esz = 0;
    if (n == "states") {
        if (!st->closed) { h->err = "stream fetch: \"states\" exists after close()"; return AEGIS_ERR_INVALID; }
        src = st->states.p; count = st->frames_done; esz = 4;
    } else if (n == "vstate") {
        if (st->closed || st->frames_done == 0) { h->err = "stream fetch: \"vstate\" exists between the first frame and close()"; return AEGIS_ERR_INVALID; }
        src = st->vstate.p; count = 2 * (int64_t)h->tab.n_bins; esz = 8;
    } else { h->err = "stream fetch: unknown name " + n; return AEGIS_ERR_INVALID; }
    if (dst && cap > 0) {
        HIPCHK(h, hipSetDevice(h->device));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipMemcpy(dst, src, (size_t)(std::min(count, cap) * esz), hipMemcpyDeviceToHost));
    }
    return count;
    STREAM_ENTRY_END(st)
}

}  // extern "C"
