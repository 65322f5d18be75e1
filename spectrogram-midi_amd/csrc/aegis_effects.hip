// Effect entries of libaegis_hip.so: aegis_reverb_ir, aegis_effects (the reference's apply_effect_chain,
// aegis_engine_core/effect_learning_loop.py:56-275, and the two WAV conversions around it, :301-304 and :334-337).  The
// host turns every effect into a per-clip record with the reference's Python-float arithmetic (gains, sample counts, the
// echo list, the mix ratios) and validates the whole request before the device is looked at; the kernels are in effects.hip.
#include "aegis_internal.h"
#include "effects.h"

#include <cmath>
#include <random>

using namespace aegis;

namespace {

// np.sum of a contiguous float64 array (numpy's pairwise summation: blocks of at most 128, eight partial sums)
double numpy_sum(const double *a, int64_t n) {
    if (n < 8) {
        double r = 0.0;
        for (int64_t i = 0; i < n; ++i) r += a[i];
        return r;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        int64_t i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    return numpy_sum(a, n2) + numpy_sum(a + n2, n - n2);
}

// int(sr * (room_size * 3.0)) (:101-102), -1 when it does not fit the tap limit
int64_t reverb_taps(double room_size, int32_t sr) {
    const double len = (double)sr * (room_size * 3.0);
    if (!(len < (double)kFxMaxTaps + 1.0)) return -1;
    return len <= 0.0 ? 0 : (int64_t)len;
}

// apply_reverb's impulse response (:108-117): exp(-decay_rate * t / sr) * RandomState(42).uniform(0.8, 1.0), over the sum of
// magnitudes.  std::mt19937(42) is RandomState(42)'s generator; a double is ((a >> 5) * 2^26 + (b >> 6)) / 2^53.
void builtin_ir(double room_size, int32_t sr, int64_t n, std::vector<double> &ir) {
    ir.resize((size_t)n);
    const double duration = room_size * 3.0;
    const double decay_rate = 5.0 / std::max(duration, 0.01);
    const double scale = 1.0 - 0.8;                              // uniform(low, high): low + (high - low) * draw
    std::mt19937 gen(42);
    for (int64_t k = 0; k < n; ++k) {
        const double e = std::exp(-decay_rate * (double)k / (double)sr);
        const uint32_t a = (uint32_t)gen() >> 5, b = (uint32_t)gen() >> 6;
        const double draw = ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
        ir[(size_t)k] = e * (0.8 + scale * draw);
    }
    const double total = std::max(numpy_sum(ir.data(), n), 1e-6);    // every tap is positive: np.abs changes nothing
    for (double &v : ir) v /= total;
}

struct Planned {
    std::vector<std::vector<FxClip>> chain;      // per clip: the effects that are not copies, off / src / ir_off still open
    std::vector<std::vector<int64_t>> ir_at;     // per clip and effect: its reverb's first tap in `taps`
    std::vector<double> taps;                    // every impulse response of the call, each zero-padded to a multiple of 8
};

bool fail(aegis_handle *h, const std::string &why) { h->err = why; return false; }

// The whole request, on the host: false with h->err set for what the reference would raise on or what the entry refuses.
bool plan_effects(aegis_handle *h, int32_t sr, int32_t n_clips, const void *const *in, int32_t in_format, const int64_t *n_samples,
                  const aegis_effect *fx, const int64_t *fx_off, Planned &P) {
    std::map<std::pair<double, int32_t>, int64_t> built;        // built-in designs by room size
    std::map<std::pair<const double *, int32_t>, int64_t> given;
    P.chain.resize((size_t)n_clips);
    P.ir_at.resize((size_t)n_clips);
    for (int32_t c = 0; c < n_clips; ++c) {
        const std::string where = " (clip " + std::to_string(c) + ")";
        const int64_t n = n_samples[c];
        if (n < 0 || (n > 0 && !in[c])) return fail(h, "bad sample count or missing samples" + where);
        if (fx_off[c + 1] < fx_off[c] || (fx_off[c + 1] > fx_off[c] && !fx)) return fail(h, "fx_off must be non-decreasing");
        if (n < 1 && fx_off[c + 1] > fx_off[c]) return fail(h, "an effect on an empty clip" + where);   // np.max of an empty array raises
        if (in_format == AEGIS_PCM_F64) {
            const double *x = static_cast<const double *>(in[c]);
            for (int64_t i = 0; i < n; ++i)
                if (!std::isfinite(x[i])) return fail(h, "sample " + std::to_string(i) + " is not finite" + where);
        }
        for (int64_t q = fx_off[c]; q < fx_off[c + 1]; ++q) {
            const aegis_effect &e = fx[q];
            const std::string what = "effect " + std::to_string(q - fx_off[c]) + where;
            if (e.kind < AEGIS_FX_DISTORTION || e.kind > AEGIS_FX_CHORUS) return fail(h, "unknown kind of " + what);
            const bool two = e.kind == AEGIS_FX_DELAY || e.kind == AEGIS_FX_CHORUS;
            if (!std::isfinite(e.p0) || (two && !std::isfinite(e.p1))) return fail(h, "non-finite parameter of " + what);
            FxClip r{};
            r.n = n;
            r.kind = e.kind;
            r.sr = (double)sr;
            int64_t ir_at = -1;
            if (e.kind == AEGIS_FX_DISTORTION) {
                r.a = 1.0 + e.p0 * 19.0;                        // :72
                r.norm = kFxNormUnit;
            } else if (e.kind == AEGIS_FX_REVERB) {
                const int64_t len = reverb_taps(e.p0, sr);
                if (len < 0) return fail(h, "impulse response above " + std::to_string(kFxMaxTaps) + " taps: " + what);
                if (e.ir && (e.n_ir < 1 || e.n_ir > kFxMaxTaps)) return fail(h, "bad tap count of " + what);
                if (len <= 0) continue;                         // ir_length <= 0: audio.copy() (:104-105)
                const int64_t taps = e.ir ? e.n_ir : len;
                const int64_t padded = (taps + 7) / 8 * 8;
                if (e.ir) {
                    auto key = std::make_pair(e.ir, e.n_ir);
                    auto it = given.find(key);
                    if (it == given.end()) {
                        for (int64_t k = 0; k < taps; ++k)
                            if (!std::isfinite(e.ir[k])) return fail(h, "tap " + std::to_string(k) + " is not finite: " + what);
                        it = given.emplace(key, (int64_t)P.taps.size()).first;
                        P.taps.insert(P.taps.end(), e.ir, e.ir + taps);
                        P.taps.resize(P.taps.size() + (size_t)(padded - taps), 0.0);
                    }
                    ir_at = it->second;
                } else {
                    auto key = std::make_pair(e.p0, sr);
                    auto it = built.find(key);
                    if (it == built.end()) {
                        std::vector<double> ir;
                        builtin_ir(e.p0, sr, taps, ir);
                        it = built.emplace(key, (int64_t)P.taps.size()).first;
                        P.taps.insert(P.taps.end(), ir.begin(), ir.end());
                        P.taps.resize(P.taps.size() + (size_t)(padded - taps), 0.0);
                    }
                    ir_at = it->second;
                }
                r.n_ir_pad = padded;
                r.b = e.p0 * 0.6;                               // wet_ratio (:124)
                r.a = 1.0 - r.b * 0.5;                          // dry_ratio (:125)
                r.norm = kFxNormAbove1;
            } else if (e.kind == AEGIS_FX_DELAY) {
                const double ds = (e.p0 / 1000.0) * (double)sr;
                if (!(std::fabs(ds) < 9.0e18)) return fail(h, "delay out of range: " + what);
                r.delay = (int64_t)ds;                          // :154
                if (r.delay <= 0 || e.p1 <= 0.0) continue;      // audio.copy(), and NO normalisation (:156-157)
                const double ratio = std::log(0.01) / std::log(std::max(e.p1, 0.01));      // :163
                if (!std::isfinite(ratio)) return fail(h, "feedback 1 (the reference raises): " + what);
                const int64_t max_echoes = std::min<int64_t>((int64_t)ratio, kFxMaxEchoes);
                for (int64_t i = 1; i <= max_echoes; ++i) {
                    const double gain = std::pow(e.p1, (double)i);
                    if (r.delay > (n - 1) / i || gain < 0.01) break;      // offset >= len(output) or gain < 0.01 (:170)
                    r.gain[r.n_echo++] = gain;
                }
                r.norm = kFxNormAbove1;
            } else {
                r.delay = (int64_t)(0.007 * (double)sr);        // :207
                r.a = e.p0 * (double)sr;                        // :208
                r.b = 2.0 * 3.141592653589793 * e.p1;           // :209
                r.norm = kFxNormAbove1;
            }
            P.chain[(size_t)c].push_back(r);
            P.ir_at[(size_t)c].push_back(ir_at);
        }
    }
    return true;
}

// clips [c0, c1) as one device pass (handle locked)
int effects_group(aegis_handle *h, const Planned &P, int32_t c0, int32_t c1, const void *const *in, int32_t in_format,
                  const int64_t *n_samples, double *const *out_f64, int16_t *const *out_i16) {
    const size_t nc = (size_t)(c1 - c0);
    size_t stages = 0;
    std::vector<int64_t> off(nc + 1, 0);
    for (size_t c = 0; c < nc; ++c) {
        off[c + 1] = off[c] + n_samples[c0 + (int32_t)c];
        stages = std::max(stages, P.chain[(size_t)c0 + c].size());
    }
    const int64_t total = off[nc];
    if (total == 0) return AEGIS_OK;
    // records: row s < stages is stage s, the last row says where every clip's result lies
    std::vector<FxClip> recs((stages + 1) * nc);
    std::vector<FxTile> point, reverb, all, whole;
    std::vector<size_t> point_at(stages + 1, 0), reverb_at(stages + 1, 0), all_at(stages + 1, 0);
    std::vector<int32_t> src(nc, 0);
    for (size_t s = 0; s <= stages; ++s) {
        for (size_t c = 0; c < nc; ++c) {
            const auto &chain = P.chain[(size_t)c0 + c];
            FxClip &r = recs[s * nc + c];
            if (s < stages && s < chain.size()) {
                r = chain[s];
                if (r.kind == AEGIS_FX_REVERB) r.ir_off = P.ir_at[(size_t)c0 + c][s];
            }
            r.off = off[c];
            r.n = off[c + 1] - off[c];
            r.src = src[c];
            const int32_t rec = (int32_t)(s * nc + c);
            if (s == stages) {
                for (int64_t t = 0; t < r.n; t += kFxTile) whole.push_back(FxTile{rec, 0, t});
            } else if (r.kind == AEGIS_FX_REVERB) {
                for (int64_t t = 0; t < r.n; t += kFxRevTile) reverb.push_back(FxTile{rec, 0, t});
            } else if (r.kind != 0) {
                for (int64_t t = 0; t < r.n; t += kFxTile) point.push_back(FxTile{rec, 0, t});
            }
            if (s < stages && r.kind != 0) {
                if (r.norm != kFxNormNone)
                    for (int64_t t = 0; t < r.n; t += kFxTile) all.push_back(FxTile{rec, 0, t});
                src[c] ^= 1;
            }
        }
        if (s < stages) { point_at[s + 1] = point.size(); reverb_at[s + 1] = reverb.size(); all_at[s + 1] = all.size(); }
    }
    if (recs.size() > (size_t)INT32_MAX || whole.size() > (size_t)INT32_MAX) { h->err = "batch too large"; return AEGIS_ERR_INVALID; }
    // one tile table: stage tiles of the three kinds, then the whole-clip tiles
    std::vector<FxTile> tiles;
    tiles.reserve(point.size() + reverb.size() + all.size() + whole.size());
    const size_t at_point = 0, at_reverb = point.size(), at_all = at_reverb + reverb.size(), at_whole = at_all + all.size();
    tiles.insert(tiles.end(), point.begin(), point.end());
    tiles.insert(tiles.end(), reverb.begin(), reverb.end());
    tiles.insert(tiles.end(), all.begin(), all.end());
    tiles.insert(tiles.end(), whole.begin(), whole.end());

    hipStream_t s = h->stream;
    const bool s16 = in_format == AEGIS_PCM_S16;
    bool want_i16 = false;
    for (size_t c = 0; c < nc; ++c) want_i16 = want_i16 || (out_i16 && out_i16[c0 + (int32_t)c]);
    ENSURE(h, fx_a, (size_t)total * 8); ENSURE(h, fx_b, (size_t)total * 8);
    ENSURE(h, fx_peak, recs.size() * 8);
    if (s16 || want_i16) ENSURE(h, fx_i16, (size_t)total * 2);
    StreamScope scope(h);                                       // (the host vectors above are in front of it)
    PUT(h, fx_recs, recs, s); PUT(h, fx_tiles, tiles, s); PUT(h, fx_taps, P.taps, s);
    double *buf0 = h->fx_a.as<double>(), *buf1 = h->fx_b.as<double>();
    int16_t *d_i16 = h->fx_i16.as<int16_t>();
    const FxClip *d_recs = h->fx_recs.as<const FxClip>();
    const FxTile *d_tiles = h->fx_tiles.as<const FxTile>();
    unsigned long long *d_peak = h->fx_peak.as<unsigned long long>();
    const double *d_taps = h->fx_taps.as<const double>();
    HIPCHK(h, hipMemsetAsync(h->fx_peak.p, 0, recs.size() * 8, s));
    for (size_t c = 0; c < nc; ++c) {
        const int64_t n = off[c + 1] - off[c];
        if (n == 0) continue;
        if (s16) HIPCHK(h, hipMemcpyAsync(d_i16 + off[c], in[c0 + (int32_t)c], (size_t)n * 2, hipMemcpyHostToDevice, s));
        else HIPCHK(h, hipMemcpyAsync(buf0 + off[c], in[c0 + (int32_t)c], (size_t)n * 8, hipMemcpyHostToDevice, s));
    }
    // (tiles hold absolute record indices)
    if (s16) TIMED(h, "fx_load", s, fx_load_s16(d_recs, d_tiles + at_whole, d_i16, buf0, (int32_t)whole.size(), s));
    for (size_t st = 0; st < stages; ++st) {
        const int32_t np = (int32_t)(point_at[st + 1] - point_at[st]), nr = (int32_t)(reverb_at[st + 1] - reverb_at[st]);
        const int32_t na = (int32_t)(all_at[st + 1] - all_at[st]);
        if (np > 0) TIMED(h, "fx_point", s, fx_point(d_recs, d_tiles + at_point + point_at[st], buf0, buf1, d_peak, np, s));
        if (nr > 0) TIMED(h, "fx_reverb", s, fx_reverb(d_recs, d_tiles + at_reverb + reverb_at[st], d_taps, buf0, buf1, d_peak, nr, s));
        if (na > 0) TIMED(h, "fx_scale", s, fx_scale(d_recs, d_tiles + at_all + all_at[st], buf0, buf1, d_peak, na, s));
    }
    if (want_i16) TIMED(h, "fx_i16", s, fx_i16(d_recs, d_tiles + at_whole, buf0, buf1, d_i16, (int32_t)whole.size(), s));
    for (size_t c = 0; c < nc; ++c) {
        const int64_t n = off[c + 1] - off[c];
        if (n == 0) continue;
        const int32_t cc = c0 + (int32_t)c;
        if (out_f64 && out_f64[cc]) FETCH(h, out_f64[cc], (src[c] ? buf1 : buf0) + off[c], n, s);
        if (out_i16 && out_i16[cc]) FETCH(h, out_i16[cc], d_i16 + off[c], n, s);
    }
    return scope.finish();
}

}  // namespace

extern "C" {

int64_t aegis_reverb_ir(double room_size, int32_t sample_rate, double *dst, int64_t cap) {
    try {
    if (!std::isfinite(room_size) || sample_rate <= 0 || cap < 0 || (cap > 0 && !dst)) return AEGIS_ERR_INVALID;
    const int64_t n = reverb_taps(room_size, sample_rate);
    if (n < 0) return AEGIS_ERR_INVALID;
    if (n == 0 || cap == 0) return n;
    std::vector<double> ir;
    builtin_ir(room_size, sample_rate, n, ir);
    std::memcpy(dst, ir.data(), (size_t)std::min(n, cap) * 8);
    return n;
    } catch (...) { return abi_fail(nullptr); }
}

int aegis_effects(aegis_handle *h, int32_t sample_rate, int32_t n_clips, const void *const *in, int32_t in_format,
                  const int64_t *n_samples, const aegis_effect *fx, const int64_t *fx_off, double *const *out_f64,
                  int16_t *const *out_i16) {
    ENTRY(h)
    if (sample_rate <= 0 || n_clips < 0 || (in_format != AEGIS_PCM_S16 && in_format != AEGIS_PCM_F64) ||
        (n_clips > 0 && (!in || !n_samples || !fx_off))) {
        h->err = "bad argument"; return AEGIS_ERR_INVALID;
    }
    Planned P;
    if (!plan_effects(h, sample_rate, n_clips, in, in_format, n_samples, fx, fx_off, P)) return AEGIS_ERR_INVALID;
    DEVICE_ONLY(h);
    if (n_clips == 0) return AEGIS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    return run_halving(h, n_clips, [&](int32_t c0, int32_t c1) {
        return effects_group(h, P, c0, c1, in, in_format, n_samples, out_f64, out_i16);
    });
    ENTRY_END(h)
}

}  // extern "C"
