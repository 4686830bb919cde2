"""A float64 numpy restatement of the Y'CbCr frame I/O (DESIGN.md §5 "YCbCr I/O"), written from the definitions:
no fp32 anywhere, the constants unrounded, the chroma filters as explicit per-sample sums.  The tests compare the
library's torch restatement (and through it the kernels) with this."""
import numpy as np

MATRIX = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def params(matrix, full_range):
    Kr, Kb = MATRIX[matrix]
    ys, cs, yo = (255.0, 255.0, 0.0) if full_range else (219.0, 224.0, 16.0)
    return Kr, Kb, 1.0 - Kr - Kb, ys, cs, yo


def clampi(v, n):
    return min(max(v, 0), n - 1)


def upsample16(c, H, W, sub, site_x):
    """Chroma plane [ch, cw] of integers -> int64 [H, W], sixteenths."""
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


def ingest(y, cb, cr, sub, matrix, full_range, site_x):
    """One frame (uint8 [H, W] and two chroma planes) -> float64 [3, H, W] in [0, 1]."""
    Kr, Kb, Kg, ys, cs, yo = params(matrix, full_range)
    H, W = y.shape
    u = upsample16(cb, H, W, sub, site_x) / 16.0 - 128.0
    v = upsample16(cr, H, W, sub, site_x) / 16.0 - 128.0
    a = (y.astype(np.float64) - yo) / ys
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


def egress_unrounded(x, sub, matrix, full_range, site_x):
    """float [3, H, W] (any values) -> the unrounded (t_Y [H, W], t_Cb, t_Cr [ch, cw]) in float64, 128 included."""
    Kr, Kb, Kg, ys, cs, yo = params(matrix, full_range)
    x = np.asarray(x, dtype=np.float64)
    x = np.clip(np.where(np.isnan(x), 0.0, x), 0.0, 1.0)
    r, g, b = x
    yl = Kr * r + Kg * g + Kb * b
    ty = yo + ys * yl
    tb = cs * (b - yl) / (2.0 * (1.0 - Kb))
    tr = cs * (r - yl) / (2.0 * (1.0 - Kr))
    return ty, downsample(tb, sub, site_x) + 128.0, downsample(tr, sub, site_x) + 128.0


def to_byte(t):
    return np.floor(np.clip(t + 0.5, 0.0, 255.0)).astype(np.uint8)


def decided(t, margin=1e-3):
    """Samples whose t + 0.5 is farther than margin from an integer."""
    f = t + 0.5
    return np.abs(f - np.round(f)) > margin
