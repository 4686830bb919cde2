"""The deep residual layer's definitions (DESIGN.md §5 "Residual coding", "Deep samples") restated in NumPy for the
tests: quantise, split, context, histogram, digest, low-bit plane and the shift rule.  Written from the definitions,
not from the kernels or from codec.py's restatement: the 3 x 3 window is an explicit loop over clamped coordinates,
the plane is packed bit by bit in Python integers, the digest is a Python-integer sum.

Samples are int64 arrays [3,H,W] (one image) already clamped to 0..2^d-1."""
import numpy as np

K = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1


def quantise(x, base, tau):
    """(q, rec) for integer arrays or Python integers; d is not needed for q."""
    step = 2 * tau + 1
    r = np.asarray(x, np.int64) - np.asarray(base, np.int64)
    mag = (np.abs(r) + tau) // step
    return np.where(r < 0, -mag, mag)


def reconstruct(base, q, tau, depth):
    return np.clip(np.asarray(base, np.int64) + np.asarray(q, np.int64) * (2 * tau + 1), 0, (1 << depth) - 1)


def split(q, s):
    """(hi, lo): hi = floor(q / 2^s), lo = q - hi 2^s in 0..2^s-1."""
    q = np.asarray(q, np.int64)
    hi = np.floor_divide(q, 1 << s)
    return hi, q - hi * (1 << s)


def join(hi, lo, s):
    return np.asarray(hi, np.int64) * (1 << s) + np.asarray(lo, np.int64)


def fits(max_abs_q, s):
    return (int(max_abs_q) + (1 << s) - 1) >> s <= 255


def shift_rule(depth, n, max_abs_q, sum_abs_q):
    for s in range(depth - 6):
        if fits(max_abs_q, s) and sum_abs_q <= 8 * n * (1 << s):
            return s
    return depth - 7


def klass(a):
    return 0 if a < 2 else int(a).bit_length() - 1


def contexts(base, depth):
    """uint8 [3,H,W]: 8 c + class((max - min over the clamped 3 x 3 neighbourhood) >> (depth - 8))."""
    _, H, W = base.shape
    ys = np.clip(np.arange(-1, H + 1), 0, H - 1)
    xs = np.clip(np.arange(-1, W + 1), 0, W - 1)
    mx = np.full(base.shape, -1, np.int64)
    mn = np.full(base.shape, 1 << 20, np.int64)
    for dy in range(3):
        for dx in range(3):
            nb = base[:, ys[dy:dy + H]][:, :, xs[dx:dx + W]]
            mx, mn = np.maximum(mx, nb), np.minimum(mn, nb)
    a = (mx - mn) >> (depth - 8)
    cls = np.vectorize(klass, otypes=[np.int64])(a)
    return (cls + 8 * np.arange(3).reshape(3, 1, 1)).astype(np.uint8)


def histogram(hi, ctx):
    """int64 [24,128]: bin hi + 63 for |hi| <= 63, the escape bin 127 otherwise."""
    h = np.zeros((24, 128), np.int64)
    b = np.where(np.abs(hi) <= 63, hi + 63, 127)
    np.add.at(h, (ctx.reshape(-1).astype(np.int64), b.reshape(-1)), 1)
    return h


def digest(base):
    """The sum over i of (base_i + 1) ((i + 1) K) mod 2^64, in Python integers."""
    tot = 0
    for i, v in enumerate(base.reshape(-1).tolist()):
        tot += (v + 1) * (i + 1)
    return (tot * K) & MASK


def pack_plane(lo, s):
    """uint64 [3 H G s]: word ((c H + y) G + g) s + j has bit x mod 64 = bit j of lo(c, y, x); zero beyond column W."""
    _, H, W = lo.shape
    G = -(-W // 64)
    words = [0] * (3 * H * G * s)
    rows = lo.reshape(3 * H, W).tolist()
    for r, row in enumerate(rows):
        for x, v in enumerate(row):
            for j in range(s):
                if (v >> j) & 1:
                    words[(r * G + x // 64) * s + j] |= 1 << (x % 64)
    return np.array(words, np.uint64).reshape(-1)


def front(base, x, depth, tau, s):
    """Everything the front pass gives for one image (x may be None)."""
    ctx = contexts(base, depth)
    out = {"ctx": ctx, "ctx_count": np.bincount(ctx.reshape(-1), minlength=24).astype(np.int64), "digest": digest(base)}
    if x is None:
        return out
    q = quantise(x, base, tau)
    rec = reconstruct(base, q, tau, depth)
    hi, lo = split(q, s)
    out.update(q=q, sym=np.clip(hi, -32768, 32767).astype(np.int16), plane=pack_plane(lo, s), hist=histogram(hi, ctx),
               max_err=int(np.abs(x - rec).max()), max_abs_q=int(np.abs(q).max()), sum_abs_q=int(np.abs(q).sum()),
               rec=rec)
    return out
