// Trend entries of libaegis_hip.so: aegis_trend (the financial filters over pitch tracks) and aegis_ghost_rsi.
#include "aegis_internal.h"
#include "trend.h"

using namespace aegis;

extern "C" {

int aegis_ghost_rsi(aegis_handle *h, const int64_t *ev_a, const int64_t *ev_b, const int64_t *event_off, int32_t n_series,
                    const int64_t *track_len, int32_t period, double *avg_gain, double *avg_loss) {
    ENTRY(h)
    if (n_series < 0 || (n_series > 0 && (!event_off || !track_len))) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    if (period < 1 || period > 128) { h->err = "rsi period must be 1..128"; return AEGIS_ERR_INVALID; }
    DEVICE_ONLY(h);
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
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    ENSURE(h, t_x, std::max<int64_t>(total, 1) * 8); ENSURE(h, t_a, std::max<int64_t>(total, 1) * 8); ENSURE(h, t_b, std::max<int64_t>(total, 1) * 8);
    ENSURE(h, t_off, (n_series + 1) * 8); ENSURE(h, t_i64a, 2 * E * 8); ENSURE(h, t_i64b, E * 4 + 8); ENSURE(h, t_c, 2 * E * 8);
    int64_t *d_ab = h->t_i64a.as<int64_t>();
    int32_t *d_sid = h->t_i64b.as<int32_t>();
    double *d_out = h->t_c.as<double>();
    StreamScope scope(h);
    HIPCHK(h, hipMemcpyAsync(d_ab, ev_a + event_off[0], (size_t)E * 8, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(d_ab + E, ev_b + event_off[0], (size_t)E * 8, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(d_sid, sid.data(), (size_t)E * 4, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(h->t_off.p, toff.data(), ((size_t)n_series + 1) * 8, hipMemcpyHostToDevice, s));
    trend_ghost_rsi(d_ab, d_ab + E, d_sid, E, h->t_off.as<const int64_t>(), n_series, total, period,
                    h->t_x.as<double>(), h->t_a.as<double>(), h->t_b.as<double>(), d_out, d_out + E, s);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(avg_gain + event_off[0], d_out, (size_t)E * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(avg_loss + event_off[0], d_out + E, (size_t)E * 8, hipMemcpyDeviceToHost, s));
    return scope.finish();
    ENTRY_END(h)
}

int aegis_trend(aegis_handle *h, int32_t op, const double *x, const int64_t *offsets, int32_t n_series,
                const double *params, int32_t n_params, void *const *outs, int32_t n_outs) {
    ENTRY(h)
    if (n_series < 0 || (n_series > 0 && (!x || !offsets)) || !outs || n_params < 0 || (n_params > 0 && !params)) {
        h->err = "bad argument"; return AEGIS_ERR_INVALID;
    }
    DEVICE_ONLY(h);
    auto need = [&](int np, int no) {
        if (n_params < np || n_outs < no) { h->err = "op needs " + std::to_string(np) + " params and " + std::to_string(no) + " outputs"; return false; }
        for (int i = 0; i < no; ++i) if (!outs[i]) { h->err = "null output"; return false; }
        return true;
    };
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
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
    ENSURE(h, t_x, n_in * 8); ENSURE(h, t_off, (n_series + 1) * 8);
    ENSURE(h, t_a, total * 8); ENSURE(h, t_b, total * 8); ENSURE(h, t_c, total * 8); ENSURE(h, t_d, total * 8); ENSURE(h, t_e, std::max<int64_t>(total, 256) * 8);
    ENSURE(h, t_i8, total); ENSURE(h, t_i64a, total * 8); ENSURE(h, t_i64b, (n_series + 1) * 8);
    StreamScope scope(h);
    HIPCHK(h, hipMemcpyAsync(h->t_x.p, x, n_in * 8, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(h->t_off.p, offsets, (n_series + 1) * 8, hipMemcpyHostToDevice, s));
    TrendArgs a{h->t_x.as<const double>(), h->t_off.as<const int64_t>(), n_series, total};
    double *A = h->t_a.as<double>(), *B = h->t_b.as<double>(), *Cc = h->t_c.as<double>();
    double *D = h->t_d.as<double>(), *E = h->t_e.as<double>();
    int8_t *I8 = h->t_i8.as<int8_t>();
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
        trend_savgol(a, E, w, (int)params[1], B, h->t_i64a.as<int64_t>(), h->t_i64b.as<int64_t>(), A, s);
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
        ENSURE(h, t_pa, (size_t)total * (12 * 8 + 1) + 256);
        double *R = h->t_pa.as<double>();
        double *stack = R;                              // [3][total]: savgol, kalman, holt (the order multi_filter_consensus stacks them)
        double *ma = R + 3 * total, *up = R + 4 * total, *lo = R + 5 * total, *semi = R + 6 * total;
        double *mm = R + 7 * total, *sg = R + 8 * total, *hh = R + 9 * total, *cx = R + 10 * total, *conf = R + 11 * total;
        int8_t *slide_codes = reinterpret_cast<int8_t *>(R + 12 * total);
        hipStream_t q1 = h->stream2, q2 = h->stream3, q3 = h->stream4;
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
        trend_savgol(a, E, w, (int)params[1], cx, h->t_i64a.as<int64_t>(), h->t_i64b.as<int64_t>(), stack, q3);
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
    return scope.finish();
    ENTRY_END(h)
}

}  // extern "C"
