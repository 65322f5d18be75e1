// aegis_dtw and aegis_align_chroma of libaegis_hip.so: dynamic time warping of feature sequences (dtw.h states the
// semantics; the kernels are in dtw.hip).  The first takes the caller's sequences from host memory; the second runs the
// CQT (aegis_cqt.hip's cqt_host_locked) and the chroma fold into device buffers and the same kernels behind them.  A call
// is cut into passes of whole pairs whose step codes and boundary rows fit the handle's dtw_pass_bytes; the codes are
// walked on the device, pass by pass, and only paths, lengths and costs cross (the probes of aegis_dtw apart).
#include "aegis_internal.h"
#include "dtw.h"

using namespace aegis;

namespace {

// Host arrays the stream reads or writes: they live in the entry's frame, declared before its StreamScope.
struct DtwHost {
    std::vector<int64_t> foff;                   // frames in front of every sequence [n_seq + 1]
    std::vector<DtwPair> pairs;
    std::vector<int32_t> pass_end;               // per pass, the first pair behind it
    std::vector<std::vector<uint32_t>> codes;    // per pass, for steps_out
    int64_t path_cells = 0, cells = 0;
    int64_t max_words = 0, max_bnd = 0;          // of the largest pass
};

int dtw_request(aegis_handle *h, const char *pre, const aegis_dtw_params *p, DtwParams &o) {
    const aegis_dtw_params all{0, 0, 0, 0};
    if (!p) p = &all;
    const char *msg = dtw_fill(p->metric, p->subsequence, p->band, o);
    if (msg[0]) { h->err = std::string(pre) + msg; return AEGIS_ERR_INVALID; }
    return AEGIS_OK;
}

// The pairs against B.foff, their records and the passes.  K floats per frame.
int dtw_plan(aegis_handle *h, const char *pre, int32_t n_seq, int32_t K, const int32_t *pair_a, const int32_t *pair_b, int32_t n_pairs,
             bool probes, DtwHost &B) {
    B.pairs.resize((size_t)n_pairs);
    int64_t words = 0, bnd = 0;
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int32_t ia = pair_a[p], ib = pair_b[p];
        const std::string who = std::string(pre) + "pair " + std::to_string(p) + ": ";
        if (ia < 0 || ia >= n_seq || ib < 0 || ib >= n_seq) { h->err = who + "sequence index outside 0.." + std::to_string(n_seq - 1); return AEGIS_ERR_INVALID; }
        const int64_t N = B.foff[(size_t)ia + 1] - B.foff[(size_t)ia], M = B.foff[(size_t)ib + 1] - B.foff[(size_t)ib];
        if (N < 1 || M < 1) { h->err = who + "sequence " + std::to_string(N < 1 ? ia : ib) + " is empty"; return AEGIS_ERR_INVALID; }
        if (N > kDtwMaxCells || M > kDtwMaxCells || N * M > kDtwMaxCells) { h->err = who + "more than 2^28 cells"; return AEGIS_ERR_INVALID; }
        const int64_t w = dtw_code_words(N, M);
        if (words + bnd && (words + w) * 4 + (bnd + M) * 8 > h->dtw_pass_bytes) {
            B.pass_end.push_back(p);
            words = bnd = 0;
        }
        DtwPair &P = B.pairs[(size_t)p];
        P.a_off = (int64_t)K * B.foff[(size_t)ia]; P.b_off = (int64_t)K * B.foff[(size_t)ib];
        P.code_off = words; P.bnd_off = bnd; P.path_off = B.path_cells; P.probe_off = B.cells;
        P.N = (int32_t)N; P.M = (int32_t)M; P.out = p; P.reserved = 0;
        words += w; bnd += M;
        B.max_words = std::max(B.max_words, words); B.max_bnd = std::max(B.max_bnd, bnd);
        B.path_cells += N + M - 1;
        B.cells += N * M;
    }
    if (n_pairs) B.pass_end.push_back(n_pairs);
    if (probes && B.cells > kDtwProbeCells) { h->err = std::string(pre) + "D_out / steps_out: more than 2^22 cells in the call"; return AEGIS_ERR_INVALID; }
    return AEGIS_OK;
}

// d_seq / d_foff (device): the sequences and their frame offsets.  Enqueues everything; the caller finishes its scope and
// then runs dtw_deliver.
int dtw_run_locked(aegis_handle *h, const float *d_seq, const int64_t *d_foff, int32_t n_seq, int32_t K, const DtwParams &o, DtwHost &B,
                   int32_t *path_out, int64_t *path_len, double *cost_out, double *D_out, bool want_steps) {
    hipStream_t s = h->stream;
    const int32_t n_pairs = (int32_t)B.pairs.size();
    const int64_t F = B.foff[(size_t)n_seq];
    const float *u = d_seq;
    if (o.metric == kDtwCosine) {
        ENSURE(h, dw_unit, (size_t)F * K * 4);
        TIMED(h, "dtw_cost", s, launch_dtw_unit(d_seq, d_foff, n_seq, F, K, h->dw_unit.as<float>(), s));
        u = h->dw_unit.as<const float>();
    }
    PUT(h, dw_pairs, B.pairs, s);
    ENSURE(h, dw_codes, (size_t)B.max_words * 4); ENSURE(h, dw_bnd, (size_t)B.max_bnd * 8);
    ENSURE(h, dw_paths, (size_t)B.path_cells * 8); ENSURE(h, dw_len, (size_t)n_pairs * 8); ENSURE(h, dw_cost, (size_t)n_pairs * 8);
    const bool probe = D_out || want_steps;
    if (probe) ENSURE(h, dw_probe, (size_t)B.cells * 8);
    if (want_steps) B.codes.resize(B.pass_end.size());
    int32_t p0 = 0;
    for (size_t k = 0; k < B.pass_end.size(); ++k) {
        const int32_t p1 = B.pass_end[k];
        const DtwPair *d_pairs = h->dw_pairs.as<const DtwPair>() + p0;
        TIMED(h, "dtw_forward", s, launch_dtw_forward(u, d_pairs, p1 - p0, K, o, h->dw_codes.as<uint32_t>(), h->dw_bnd.as<double>(),
                                                      probe ? h->dw_probe.as<double>() : nullptr, s));
        TIMED(h, "dtw_walk", s, launch_dtw_walk(d_pairs, p1 - p0, o, h->dw_codes.as<const uint32_t>(), h->dw_bnd.as<const double>(),
                                                h->dw_paths.as<int32_t>(), h->dw_len.as<int64_t>(), h->dw_cost.as<double>(), s));
        if (want_steps) {
            const DtwPair &L = B.pairs[(size_t)p1 - 1];
            B.codes[k].resize((size_t)(L.code_off + dtw_code_words(L.N, L.M)));
            FETCH(h, B.codes[k].data(), h->dw_codes.p, B.codes[k].size(), s);
        }
        p0 = p1;
    }
    FETCH(h, path_out, h->dw_paths.p, (size_t)B.path_cells * 2, s);
    FETCH(h, path_len, h->dw_len.p, n_pairs, s);
    FETCH(h, cost_out, h->dw_cost.p, n_pairs, s);
    if (D_out) FETCH(h, D_out, h->dw_probe.p, B.cells, s);
    return AEGIS_OK;
}

// after the stream has drained: every path from the tail of its region to the head, the codes unpacked
int dtw_deliver(aegis_handle *h, const DtwHost &B, int32_t *path_out, const int64_t *path_len, uint8_t *steps_out) {
    size_t pass = 0;
    for (size_t p = 0; p < B.pairs.size(); ++p) {
        const DtwPair &P = B.pairs[p];
        const int64_t cap = (int64_t)P.N + P.M - 1, L = path_len[p];
        if (L < 1 || L > cap) { h->err = "dtw: pair " + std::to_string(p) + ": the walk returned a path of " + std::to_string(L) + " cells"; return AEGIS_ERR_DEVICE; }
        int32_t *region = path_out + 2 * P.path_off;
        std::memmove(region, region + 2 * (cap - L), (size_t)L * 8);
        if (steps_out) {
            while ((int32_t)p >= B.pass_end[pass]) ++pass;
            const uint32_t *words = B.codes[pass].data() + P.code_off;
            uint8_t *out = steps_out + P.probe_off;
            for (int64_t i = 0; i < P.N; ++i)
                for (int64_t j = 0; j < P.M; ++j) out[i * P.M + j] = (uint8_t)dtw_code_at(words, i, j, P.M);
        }
    }
    return AEGIS_OK;
}

}  // namespace

extern "C" {

int aegis_dtw(aegis_handle *h, const float *seq, const int64_t *n_frames, int32_t n_seq, int32_t K, const int32_t *pair_a,
              const int32_t *pair_b, int32_t n_pairs, const aegis_dtw_params *params, int32_t *path_out, int64_t *path_len,
              double *cost_out, double *D_out, uint8_t *steps_out) {
    ENTRY(h)
    DtwParams o;
    int rc = dtw_request(h, "dtw: ", params, o);
    if (rc != AEGIS_OK) return rc;
    if (K < 1 || K > kDtwMaxK) { h->err = "dtw: K must be 1..24"; return AEGIS_ERR_INVALID; }
    if (n_seq < 0 || n_pairs < 0 || (n_seq > 0 && !n_frames) || (n_pairs > 0 && (!pair_a || !pair_b || !path_out || !path_len || !cost_out))) {
        h->err = "dtw: null argument";
        return AEGIS_ERR_INVALID;
    }
    DtwHost B;
    int64_t maxF = 0;
    if ((rc = frame_offsets(h, "dtw: ", "dtw: ", n_frames, n_seq, B.foff, maxF)) != AEGIS_OK) return rc;
    const int64_t F = B.foff[(size_t)n_seq];
    if (F > 0 && !seq) { h->err = "dtw: null argument"; return AEGIS_ERR_INVALID; }
    if ((rc = dtw_plan(h, "dtw: ", n_seq, K, pair_a, pair_b, n_pairs, D_out || steps_out, B)) != AEGIS_OK) return rc;
    for (int32_t q = 0; q < n_seq; ++q) {
        const int64_t n = B.foff[(size_t)q + 1] - B.foff[(size_t)q];
        const float *x = seq + (int64_t)K * B.foff[(size_t)q];
        for (int64_t e = 0; e < n * K; ++e)
            if (!std::isfinite(x[e])) {
                h->err = "dtw: sequence " + std::to_string(q) + ", frame " + std::to_string(e % n) + ": value is not finite";
                return AEGIS_ERR_INVALID;
            }
    }
    DEVICE_ONLY(h);
    if (n_pairs == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    drop_events(h);
    StreamScope scope(h);
    ENSURE(h, dw_seq, (size_t)F * K * 4);
    HIPCHK(h, upload(h->dw_seq, seq, (size_t)F * K * 4, h->stream));
    PUT(h, dw_foff, B.foff, h->stream);
    if ((rc = dtw_run_locked(h, h->dw_seq.as<const float>(), h->dw_foff.as<const int64_t>(), n_seq, K, o, B, path_out, path_len, cost_out, D_out,
                             steps_out != nullptr)) != AEGIS_OK) return rc;
    if ((rc = scope.finish()) != AEGIS_OK) return rc;
    return dtw_deliver(h, B, path_out, path_len, steps_out);
    ENTRY_END(h)
}

int aegis_align_chroma(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips, int32_t n_bins,
                       int32_t bins_per_octave, double fmin, double filter_scale, int32_t n_chroma, const int32_t *bin_class,
                       const int32_t *pair_a, const int32_t *pair_b, int32_t n_pairs, const aegis_dtw_params *params,
                       int32_t *path_out, int64_t *path_len, double *cost_out) {
    ENTRY(h)
    DtwParams o;
    int rc = dtw_request(h, "align: ", params, o);
    if (rc != AEGIS_OK) return rc;
    if (n_chroma < 1 || n_chroma > kDtwMaxK) { h->err = "align: n_chroma (K) must be 1..24"; return AEGIS_ERR_INVALID; }
    if (n_clips < 0 || n_pairs < 0 || (n_clips > 0 && (!pcm || !n_samples)) || !bin_class ||
        (n_pairs > 0 && (!pair_a || !pair_b || !path_out || !path_len || !cost_out))) {
        h->err = "align: null argument";
        return AEGIS_ERR_INVALID;
    }
    DtwHost B;
    int64_t maxF = 0;
    if ((rc = clip_frames(h, "align: ", pcm, n_samples, n_clips, B.foff, maxF)) != AEGIS_OK) return rc;
    if ((rc = dtw_plan(h, "align: ", n_clips, n_chroma, pair_a, pair_b, n_pairs, false, B)) != AEGIS_OK) return rc;
    for (int32_t c = 0; c < n_clips; ++c)
        for (int64_t e = 0; e < n_samples[c]; ++e)
            if (!std::isfinite(pcm[c][e])) {
                h->err = "align: sequence " + std::to_string(c) + ", frame " + std::to_string(e / h->tab.hop) + " (sample " + std::to_string(e) +
                         "): value is not finite";
                return AEGIS_ERR_INVALID;
            }
    DEVICE_ONLY(h);
    if (n_pairs == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    int64_t F = 0;
    StreamScope scope(h);
    if ((rc = cqt_host_locked(h, pcm, n_samples, n_clips, n_bins, bins_per_octave, fmin, filter_scale, n_chroma, bin_class, &F)) != AEGIS_OK) return rc;
    if (F != B.foff[(size_t)n_clips]) { h->err = "align: the CQT's frame counts differ from 1 + n_samples / hop"; return AEGIS_ERR_DEVICE; }
    TIMED(h, "chroma", s, launch_chroma_fold(h->q_out.as<const float>(), h->q_foff.as<const int64_t>(), n_clips, F, n_bins, n_chroma,
                                             h->q_cls.as<const int32_t>(), h->q_chroma.as<float>(), s));
    if ((rc = dtw_run_locked(h, h->q_chroma.as<const float>(), h->q_foff.as<const int64_t>(), n_clips, n_chroma, o, B, path_out, path_len, cost_out,
                             nullptr, false)) != AEGIS_OK) return rc;
    if ((rc = scope.finish()) != AEGIS_OK) return rc;
    return dtw_deliver(h, B, path_out, path_len, nullptr);
    ENTRY_END(h)
}

}  // extern "C"
