"""A float64 numpy restatement of the high-bit-depth sample I/O (DESIGN.md §5 "High-bit-depth I/O"), written from
the definitions: no fp32 anywhere, the constants unrounded, the chroma filters as explicit per-sample sums.  Depth d
in [8, 16]: maxv = 2^d - 1, half = 2^(d-1), s = 2^(d-8); a word is LSB-aligned (the sample is min(word, maxv)) or
MSB-aligned (the sample is word >> (16 - d)).  The tests compare the library's torch restatement (and through it the
kernels) with this."""
import numpy as np

MATRIX = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}


def samples(words, d, msb):
    w = np.asarray(words).astype(np.int64)
    return w >> (16 - d) if msb else np.minimum(w, (1 << d) - 1)


def words(smp, d, msb):
    s = np.asarray(smp).astype(np.int64)
    return (s << (16 - d) if msb else s).astype(np.uint16)


def params(matrix, full_range, d):
    Kr, Kb = MATRIX[matrix]
    maxv, s = float((1 << d) - 1), float(1 << (d - 8))
    ys, cs, yo = (maxv, maxv, 0.0) if full_range else (219.0 * s, 224.0 * s, 16.0 * s)
    return Kr, Kb, 1.0 - Kr - Kb, ys, cs, yo


def clampi(v, n):
    return min(max(v, 0), n - 1)


def upsample16(c, H, W, sub, site_x):
    """Chroma plane [ch, cw] of integer samples -> int64 [H, W], sixteenths."""
    sx, sy = sub
    c = np.asarray(c, dtype=np.int64)
    ch, cw = c.shape
    hor = np.zeros((ch, W), np.int64)  # quarters
    for x in range(W):
        if sx == 1:
            hor[:, x] = 4 * c[:, x]
        else:
            i = x >> 1
            if site_x == "centre":
                hor[:, x] = 3 * c[:, i] + c[:, clampi(i + 1 if x & 1 else i - 1, cw)]
            elif x & 1:
                hor[:, x] = 2 * c[:, i] + 2 * c[:, clampi(i + 1, cw)]
            else:
                hor[:, x] = 4 * c[:, i]
    out = np.zeros((H, W), np.int64)
    for y in range(H):
        if sy == 1:
            out[y] = 4 * hor[y]
        else:
            j = y >> 1
            out[y] = 3 * hor[j] + hor[clampi(j + 1 if y & 1 else j - 1, ch)]
    return out


def ingest_rgb(words_, d, msb):
    """uint16 words of any shape -> float64 sample / maxv."""
    return samples(words_, d, msb).astype(np.float64) / float((1 << d) - 1)


def egress_rgb(x, d):
    """float (any values) -> int64 samples floor(clip(v, 0, 1) * maxv), NaN -> 0, evaluated as the kernel does: the
    product in fp32 (this one step is the definition itself, not an approximation of it)."""
    x = np.asarray(x, dtype=np.float32)
    x = np.clip(np.where(np.isnan(x), np.float32(0), x), np.float32(0), np.float32(1))
    return np.floor(x * np.float32((1 << d) - 1)).astype(np.int64)


def ingest(y, cb, cr, sub, matrix, full_range, site_x, d, msb=False):
    """One frame (uint16 words [H, W] and two chroma planes) -> float64 [3, H, W] in [0, 1]."""
    Kr, Kb, Kg, ys, cs, yo = params(matrix, full_range, d)
    half = float(1 << (d - 1))
    Y, Cb, Cr = (samples(p, d, msb) for p in (y, cb, cr))
    H, W = Y.shape
    u = upsample16(Cb, H, W, sub, site_x) / 16.0 - half
    v = upsample16(Cr, H, W, sub, site_x) / 16.0 - half
    a = (Y.astype(np.float64) - yo) / ys
    r = a + 2.0 * (1.0 - Kr) / cs * v
    g = a - 2.0 * Kb * (1.0 - Kb) / (Kg * cs) * u - 2.0 * Kr * (1.0 - Kr) / (Kg * cs) * v
    b = a + 2.0 * (1.0 - Kb) / cs * u
    return np.clip(np.stack([r, g, b]), 0.0, 1.0)


def downsample(t, sub, site_x):
    """Full-resolution chroma float64 [H, W] -> [ch, cw]."""
    sx, sy = sub
    H, W = t.shape
    ch, cw = -(-H // sy), -(-W // sx)
    out = np.zeros((ch, cw))
    for j in range(ch):
        rows = [clampi(sy * j + r, H) for r in range(sy)]
        for i in range(cw):
            s = 0.0
            for r in rows:
                if sx == 1:
                    s += t[r, i]
                elif site_x == "centre":
                    s += (t[r, clampi(2 * i, W)] + t[r, clampi(2 * i + 1, W)]) / 2.0
                else:
                    s += (t[r, clampi(2 * i - 1, W)] + 2.0 * t[r, clampi(2 * i, W)] + t[r, clampi(2 * i + 1, W)]) / 4.0
            out[j, i] = s / sy
    return out


def egress_unrounded(x, sub, matrix, full_range, site_x, d):
    """float [3, H, W] (any values) -> the unrounded (t_Y [H, W], t_Cb, t_Cr [ch, cw]) in float64, half included."""
    Kr, Kb, Kg, ys, cs, yo = params(matrix, full_range, d)
    half = float(1 << (d - 1))
    x = np.asarray(x, dtype=np.float64)
    x = np.clip(np.where(np.isnan(x), 0.0, x), 0.0, 1.0)
    r, g, b = x
    yl = Kr * r + Kg * g + Kb * b
    ty = yo + ys * yl
    tb = cs * (b - yl) / (2.0 * (1.0 - Kb))
    tr = cs * (r - yl) / (2.0 * (1.0 - Kr))
    return ty, downsample(tb, sub, site_x) + half, downsample(tr, sub, site_x) + half


def to_sample(t, d):
    return np.floor(np.clip(t + 0.5, 0.0, float((1 << d) - 1))).astype(np.int64)


def band(d):
    """The undecided band around a rounding boundary: 16 fp32 ulps at 2^d (about 8 roundings on the longest path),
    and never below the 8-bit test's 1e-3."""
    return max(1e-3, 2.0 ** (d - 20))


def decided(t, d):
    """Samples whose t + 0.5 is farther than band(d) from an integer."""
    f = t + 0.5
    return np.abs(f - np.round(f)) > band(d)
