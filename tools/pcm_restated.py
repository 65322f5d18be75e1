"""pcm_decode_resample_kernel (csrc/pcm.hip) restated in NumPy: the specification the device is held to bit for bit.

  decode_f32      raw frames -> float32 mono, written without audio_io.decode: an explicit float64 scale and one rounding
                  per sample, then the kernel's channel mean (mean_emulation)
  emulate         scipy.signal.resample_poly on float32 as the kernel computes it: per output the tap loop k = 0 .. P-1,
                  one float32 multiply and one float32 add per tap
  emulate_tiled   the same sum walked as the kernel walks it -- output tiles, the input window of a tile in slabs, per slab
                  the part [k0, k1) of every output's taps -- so that what can go wrong in that walk can be stated: the
                  MUTANTS below are deliberately wrong variants, and tests/test_pcm_restated.py shows that each of them
                  differs from the restatement on a case of tools/pcm_cases.py (a device kernel with that fault would fail)
  resample_f64    the same sum in float64, and bound(): how far a float32 evaluation in any order may be from it

CPU only, NumPy only."""
import numpy as np

PCM_U8, PCM_S16, PCM_S24, PCM_S32, PCM_F32 = 1, 2, 3, 4, 5
WIDTH = {PCM_U8: 1, PCM_S16: 2, PCM_S24: 3, PCM_S32: 4, PCM_F32: 4}
F32_TINY = np.float32(2.0 ** -126)                 # FLT_MIN: below it a float32 is a denormal

# name -> what the variant does wrong (the argument `mutant` of decode_f32 / emulate_tiled)
MUTANTS = {
    "slabs_descending": "taps descending across slabs: a tile's slabs are accumulated last to first",
    "fused_multiply_add": "multiply-add fused: the float64 product is added and the sum rounded once",
    "slab_first_tap_dropped": "the first tap of every second slab is dropped",
    "i_last_one_short": "i_last one short: the last input frame of a tile's window is not read",
    "denormals_flushed": "denormal inputs and results of every float32 operation are flushed to zero",
    "s24_sign_from_bit_22": "s24 sign extension from bit 22",
    "s32_float32_after_truncation": "s32 truncated to float32, then scaled in float32",
    "mean8_plain_order": "the 8-channel sum in plain channel order instead of NumPy's pairwise block",
    "tile_last_output_from_next": "the last output of a full tile duplicated from the first of the next",
}


def _flush(a):
    a = np.asarray(a, np.float32)
    return np.where(np.abs(a) < F32_TINY, np.float32(0) * a, a).astype(np.float32)


def mean_emulation(x, mutant=None):
    """The device kernel's channel mean: 2..7 channels in channel order, 8 as NumPy's pairwise block, the sum added to
    NumPy's initial +0 (a frame of nothing but -0.0 has the mean +0.0), then / ch."""
    ch = x.shape[1]
    if ch == 1:
        return x[:, 0]
    if mutant == "denormals_flushed":
        x = _flush(x)
    if ch == 8 and mutant != "mean8_plain_order":
        s = ((x[:, 0] + x[:, 1]) + (x[:, 2] + x[:, 3])) + ((x[:, 4] + x[:, 5]) + (x[:, 6] + x[:, 7]))
    else:
        s = x[:, 0].copy()
        for c in range(1, ch):
            s = s + x[:, c]
            if mutant == "denormals_flushed":
                s = _flush(s)
    s = np.float32(0) + s
    if mutant == "denormals_flushed":
        return _flush(_flush(s) / np.float32(ch))
    return s / np.float32(ch)


def sample_codes(raw, fmt):
    """The integer codes of raw little-endian samples (int64), or the float32 values of PCM_F32."""
    raw = np.frombuffer(bytes(raw), np.uint8) if not isinstance(raw, np.ndarray) else raw.view(np.uint8).ravel()
    w = WIDTH[fmt]
    b = raw[:len(raw) // w * w].reshape(-1, w).astype(np.int64)
    if fmt == PCM_F32:
        return np.ascontiguousarray(raw[:len(raw) // 4 * 4]).view("<f4")
    if fmt == PCM_U8:
        return b[:, 0]
    v = sum(b[:, i] << (8 * i) for i in range(w))
    return v - ((v >> (8 * w - 1)) << (8 * w))         # two's complement: the top bit weighs -2^(bits-1)


def decode_f32(raw, fmt, ch, mutant=None):
    """Raw interleaved frames -> float32 mono.  Integer codes are scaled in float64 (exact: a code has at most 32 bits)
    and rounded to float32 once: u8 (v - 128) / 2^7, s16 v / 2^15, s24 v / 2^23, s32 v / 2^31; f32 is taken as stored,
    bit for bit.  Then the channel mean."""
    v = sample_codes(raw, fmt)
    with np.errstate(over="ignore", invalid="ignore"):
        if fmt == PCM_F32:
            x = v.astype(np.float32)
        elif fmt == PCM_U8:
            x = ((v - 128).astype(np.float64) / 128.0).astype(np.float32)
        elif fmt == PCM_S32 and mutant == "s32_float32_after_truncation":
            a = np.abs(v)
            drop = np.maximum(0, np.floor(np.log2(np.maximum(a, 1))).astype(np.int64) - 23)      # bits below the 24 kept
            x = (np.sign(v) * ((a >> drop) << drop)).astype(np.float32) / np.float32(2147483648.0)
        else:
            bits = 8 * WIDTH[fmt]
            if fmt == PCM_S24 and mutant == "s24_sign_from_bit_22":
                u = v & 0xFFFFFF
                v = (u & 0x7FFFFF) - ((u >> 22 & 1) << 23)
            x = (v.astype(np.float64) / 2.0 ** (bits - 1)).astype(np.float32)
        return np.ascontiguousarray(mean_emulation(x.reshape(-1, ch), mutant), np.float32)


def layout(h, up, down):
    """resample_poly's filter arrangement: h (the designed taps times up) behind pre = down - half % down zeros, padded
    to P * up taps, phase-major and flipped.  -> (htf [up, P], P, rm)."""
    h = np.asarray(h, np.float32)
    half = (len(h) - 1) // 2
    pre = down - half % down
    hp = np.concatenate([np.zeros(pre, np.float32), h])
    P = -(-len(hp) // up)
    hp = np.pad(hp, (0, P * up - len(hp)))
    return np.ascontiguousarray(hp.reshape(P, up).T[:, ::-1]), P, (half + pre) // down


def emulate(x, up, down, h):
    """scipy.signal.resample_poly(x, up, down) on float32 as pcm_decode_resample_kernel computes it: the filter h
    (after `h *= up`) behind down - half % down zeros, stored phase-major and flipped (htf), and for every output j
    the tap loop k = 0 .. P-1 over inputs i0 - P + 1 + k, one float32 multiply and one float32 add per tap."""
    x = np.asarray(x, np.float32)
    half = (len(h) - 1) // 2
    pre = down - half % down
    hp = np.concatenate([np.zeros(pre, np.float32), np.asarray(h, np.float32)])
    P = -(-len(hp) // up)
    hp = np.pad(hp, (0, P * up - len(hp)))
    htf = hp.reshape(P, up).T[:, ::-1].ravel()
    rm = (half + pre) // down
    n_res = (len(x) * up + down - 1) // down
    j = np.arange(n_res, dtype=np.int64)
    q = (j + rm) * down
    i0, t = q // up, q % up
    acc = np.zeros(n_res, np.float32)
    for k in range(P):
        i = i0 - P + 1 + k
        ok = (i >= 0) & (i < len(x))
        term = x[np.clip(i, 0, len(x) - 1)] * htf[t * P + k]
        acc = acc + np.where(ok, term, np.float32(0))
    return acc


def emulate_batch(xs, up, down, h):
    """emulate() for several clips of one rate pair in one tap loop (the same multiply and add per output and tap, the
    clips side by side in the vectors): what the tests use where P is in the thousands.  -> list of arrays."""
    xs = [np.asarray(x, np.float32) for x in xs]
    htf, P, rm = layout(h, up, down)
    n_in = np.array([len(x) for x in xs], np.int64)
    n_res = (n_in * up + down - 1) // down
    xcat = np.concatenate(xs + [np.zeros(1, np.float32)])
    start = np.repeat(np.cumsum(n_in) - n_in, n_res)
    n = np.repeat(n_in, n_res)
    j = np.concatenate([np.arange(k, dtype=np.int64) for k in n_res] + [np.zeros(0, np.int64)])
    q = (j + rm) * down
    i0, t = q // up, q % up
    acc = np.zeros(len(j), np.float32)
    for k in range(P):
        i = i0 - P + 1 + k
        ok = (i >= 0) & (i < n)
        term = xcat[start + np.clip(i, 0, n - 1)] * htf[t, k]
        acc = acc + np.where(ok, term, np.float32(0))
    return np.split(acc, np.cumsum(n_res)[:-1])


def emulate_tiled(x, up, down, h, tile, slab, mutant=None):
    """emulate() in the kernel's walk: outputs in tiles of `tile`, a tile's inputs [i_first, i_last) in slabs of `slab`
    frames, and per slab the taps [k0, k1) of every output that fall into it, k ascending.  Without a mutant the result
    is emulate()'s for any tile and slab (the order of the additions per output is the same)."""
    x = np.asarray(x, np.float32)
    if mutant == "denormals_flushed":
        x = _flush(x)
    htf, P, rm = layout(h, up, down)
    n_in = len(x)
    n_res = (n_in * up + down - 1) // down
    out = np.zeros(n_res, np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for j0 in range(0, n_res, tile):
            jl = min(n_res, j0 + tile)
            j = np.arange(j0, jl, dtype=np.int64)
            q = (j + rm) * down
            i0, t = q // up, q % up
            base = i0 - P + 1
            i_first = max(0, (j0 + rm) * down // up - P + 1)
            i_last = min(n_in, (jl - 1 + rm) * down // up + 1)
            if mutant == "i_last_one_short":
                i_last -= 1
            starts = list(range(i_first, i_last, slab))
            if mutant == "slabs_descending":
                starts.reverse()
            acc = np.zeros(len(j), np.float32)
            for s in starts:
                n = min(slab, i_last - s)
                k0, k1 = np.maximum(0, s - base), np.minimum(P, s + n - base)
                if mutant == "slab_first_tap_dropped" and ((s - i_first) // slab) & 1:
                    k0 = k0 + 1
                for k in range(int(k0.min()), int(k1.max())):
                    on = (k >= k0) & (k < k1)
                    if not on.any():
                        continue
                    xi = x[np.clip(base + k, 0, max(n_in - 1, 0))]
                    hk = htf[t, k]
                    if mutant == "fused_multiply_add":
                        new = (acc.astype(np.float64) + xi.astype(np.float64) * hk.astype(np.float64)).astype(np.float32)
                    elif mutant == "denormals_flushed":
                        new = _flush(acc + _flush(xi * hk))
                    else:
                        new = acc + xi * hk
                    acc = np.where(on, new, acc)
            out[j0:jl] = acc
        if mutant == "tile_last_output_from_next":
            for j0 in range(tile, n_res, tile):
                out[j0 - 1] = out[j0]
    return out


def resample_f64(x, up, down, h):
    """The sum of emulate() in float64 (inputs and taps as the float32 values they are)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    htf, P, rm = layout(h, up, down)
    htf = htf.astype(np.float64)
    n_res = (len(x) * up + down - 1) // down
    q = (np.arange(n_res, dtype=np.int64) + rm) * down
    i0, t = q // up, q % up
    acc = np.zeros(n_res, np.float64)
    for k in range(P):
        i = i0 - P + 1 + k
        ok = (i >= 0) & (i < len(x))
        acc = acc + np.where(ok, x[np.clip(i, 0, max(len(x) - 1, 0))] * htf[t, k], 0.0)
    return acc


def gamma(n):
    """gamma_n = n u / (1 - n u) with u = 2^-24, float32's unit roundoff."""
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)


def bound(x, up, down, h):
    """Per output: gamma_{P+1} * sum |x_k| |h_k|, the forward error of a float32 dot product of P terms in any order
    (each term rounded once in the product and at most P times in the sums; Higham, Accuracy and Stability, 3.1), plus
    P * 2^-150 for products that underflow: a product below FLT_MIN is rounded to a multiple of 2^-149, an absolute error
    of at most 2^-150 that the relative bound does not cover (sums of denormals are exact)."""
    x = np.abs(np.asarray(x, np.float32).astype(np.float64))
    htf, P, rm = layout(h, up, down)
    htf = np.abs(htf.astype(np.float64))
    n_res = (len(x) * up + down - 1) // down
    q = (np.arange(n_res, dtype=np.int64) + rm) * down
    i0, t = q // up, q % up
    acc = np.zeros(n_res, np.float64)
    for k in range(P):
        i = i0 - P + 1 + k
        ok = (i >= 0) & (i < len(x))
        acc = acc + np.where(ok, x[np.clip(i, 0, max(len(x) - 1, 0))] * htf[t, k], 0.0)
    return gamma(P + 1) * acc + P * 2.0 ** -150
