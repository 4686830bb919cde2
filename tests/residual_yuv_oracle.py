"""The Y'CbCr residual layer's definitions (DESIGN.md §5 "Residual coding", "Y'CbCr frames") restated in NumPy for
the tests: samples of words, canonical order, quantise, split, context, histogram, digest, low-bit plane, shift rule.
Written from the definitions, not from the kernels or from codec.py's restatement and with no call into codec: the
3 x 3 window is an explicit loop over coordinates clamped into the plane, the low-bit plane is packed a byte at a
time (and bit by bit in Python integers, for small frames, as a check of that), the digest is a Python-integer sum.

A frame is a list of three int64 sample arrays [h_p, w_p] (Y', Cb, Cr), already samples (see samples())."""
import numpy as np

K = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1


def samples(words, depth, msb):
    """Words (uint8 at depth 8, uint16 above) -> int64 samples: min(word, maxv) LSB-aligned, word >> (16 - d) MSB."""
    w = np.asarray(words).astype(np.int64)
    if depth == 8:
        return w
    return w >> (16 - depth) if msb else np.minimum(w, (1 << depth) - 1)


def words(smp, depth, msb):
    """Samples -> words of the plane's type; MSB-aligned words carry zero low bits."""
    s = np.asarray(smp, np.int64)
    if depth == 8:
        return s.astype(np.uint8)
    return (s << (16 - depth) if msb else s).astype(np.uint16)


def chroma_size(H, W, sub):
    return -(-H // sub[1]), -(-W // sub[0])


def n_samples(H, W, sub):
    hc, wc = chroma_size(H, W, sub)
    return H * W + 2 * hc * wc


def plane_words(H, W, sub, s):
    """Brute force: count the 64-column groups row by row."""
    hc, wc = chroma_size(H, W, sub)
    groups = 0
    for h, w in ((H, W), (hc, wc), (hc, wc)):
        for _ in range(h):
            groups += len(range(0, w, 64))
    return groups * s


def max_shift(depth):
    return 0 if depth == 8 else depth - 7


def fits(max_abs_q, s):
    return (int(max_abs_q) + (1 << s) - 1) >> s <= 255


def shift_rule(depth, n, max_abs_q, sum_abs_q):
    if depth == 8:
        return 0
    for s in range(depth - 6):
        if fits(max_abs_q, s) and sum_abs_q <= 8 * n * (1 << s):
            return s
    return depth - 7


def quantise(x, base, tau):
    step = 2 * tau + 1
    r = np.asarray(x, np.int64) - np.asarray(base, np.int64)
    mag = (np.abs(r) + tau) // step
    return np.where(r < 0, -mag, mag)


def reconstruct(base, q, tau, depth):
    """Clamped to [0, maxv], not to the legal range."""
    return np.clip(np.asarray(base, np.int64) + np.asarray(q, np.int64) * (2 * tau + 1), 0, (1 << depth) - 1)


def split(q, s):
    q = np.asarray(q, np.int64)
    hi = np.floor_divide(q, 1 << s)
    return hi, q - hi * (1 << s)


def klass(a):
    return 0 if a < 2 else int(a).bit_length() - 1


def contexts(frame, depth):
    """uint8 [N] in canonical order: 8 p + class((max - min over the 3 x 3 neighbourhood clamped into plane p) >> (d - 8))."""
    out = []
    for p, v in enumerate(frame):
        v = np.asarray(v, np.int64)
        h, w = v.shape
        ys = np.clip(np.arange(-1, h + 1), 0, h - 1)  # row y + dy - 1, clamped into this plane
        xs = np.clip(np.arange(-1, w + 1), 0, w - 1)
        mx = np.full((h, w), -1, np.int64)
        mn = np.full((h, w), 1 << 20, np.int64)
        for dy in range(3):
            for dx in range(3):
                nb = v[ys[dy:dy + h]][:, xs[dx:dx + w]]
                mx, mn = np.maximum(mx, nb), np.minimum(mn, nb)
        cls = np.vectorize(klass, otypes=[np.int64])((mx - mn) >> (depth - 8))
        out.append((cls + 8 * p).astype(np.uint8).reshape(-1))
    return np.concatenate(out)


def canonical(frame):
    """The frame's samples in canonical order: plane-major, then row, then column."""
    return np.concatenate([np.asarray(v, np.int64).reshape(-1) for v in frame])


def histogram(hi, ctx):
    h = np.zeros((24, 128), np.int64)
    b = np.where(np.abs(hi) <= 63, hi + 63, 127)
    np.add.at(h, (ctx.astype(np.int64), b), 1)
    return h


def digest(frame):
    tot = 0
    for i, v in enumerate(canonical(frame).tolist()):
        tot += (v + 1) * (i + 1)
    return (tot * K) & MASK


def pack_plane(lo_frame, s):
    """uint64 words: rows in canonical order (luma rows, Cb rows, Cr rows); word (rowbase_p + y G_p + g) s + j has bit
    x mod 64 = bit j of lo; zero beyond the plane's width.  Bit j of a row is packed eight columns a byte, the lowest
    column in the lowest bit, and eight bytes make a little-endian word."""
    out = []
    for v in lo_frame:
        v = np.asarray(v, np.int64)
        h, w = v.shape
        G = -(-w // 64)
        words_ = np.zeros((h, G, s), np.uint64)
        for j in range(s):
            bits = np.zeros((h, 64 * G), np.uint8)
            bits[:, :w] = (v >> j) & 1
            words_[:, :, j] = np.packbits(bits, axis=1, bitorder="little").view("<u8")
        out.append(words_.reshape(-1))
    return np.concatenate(out) if out else np.zeros(0, np.uint64)


def pack_plane_bitwise(lo_frame, s):
    """pack_plane bit by bit in Python integers (slow: for small frames)."""
    out = []
    for v in lo_frame:
        h, w = v.shape
        G = -(-w // 64)
        ws = [0] * (h * G * s)
        for y, row in enumerate(np.asarray(v).tolist()):
            for x, val in enumerate(row):
                for j in range(s):
                    if (val >> j) & 1:
                        ws[(y * G + x // 64) * s + j] |= 1 << (x % 64)
        out += ws
    return np.array(out, np.uint64).reshape(-1)


def unpack_plane(plane, shapes, s):
    out, at = [], 0
    for h, w in shapes:
        G = -(-w // 64)
        lo = np.zeros((h, w), np.int64)
        for y in range(h):
            for x in range(w):
                for j in range(s):
                    lo[y, x] |= ((int(plane[at + (y * G + x // 64) * s + j]) >> (x % 64)) & 1) << j
        at += h * G * s
        out.append(lo)
    return out


def front(base, x, depth, tau, s):
    """Everything the front pass gives for one frame (x may be None): base, x lists of three sample planes."""
    ctx = contexts(base, depth)
    out = {"ctx": ctx, "ctx_count": np.bincount(ctx, minlength=24).astype(np.int64), "digest": digest(base)}
    if x is None:
        return out
    q = [quantise(a, b, tau) for a, b in zip(x, base)]
    rec = [reconstruct(b, v, tau, depth) for b, v in zip(base, q)]
    parts = [split(v, s) for v in q]
    hi = canonical([h for h, _ in parts])
    qa = np.abs(canonical(q))
    out.update(q=q, sym=np.clip(hi, -32768, 32767).astype(np.int16), plane=pack_plane([lo for _, lo in parts], s),
               hist=histogram(hi, ctx), max_err=max(int(np.abs(a - r).max()) for a, r in zip(x, rec)),
               max_abs_q=int(qa.max()), sum_abs_q=int(qa.sum()), rec=rec)
    return out


def apply(base, sym, plane, depth, tau, s, ref=None):
    """rec planes of (base, sym, plane); a sym outside +-255 sets `bad` and that sample is base.  With ref also the
    per-plane squared errors and the largest |rec - ref|."""
    shapes = [v.shape for v in base]
    lo = unpack_plane(plane, shapes, s) if s else [np.zeros(sh, np.int64) for sh in shapes]
    rec, at, bad = [], 0, False
    for p, b in enumerate(base):
        h, w = b.shape
        hi = np.asarray(sym[at:at + h * w], np.int64).reshape(h, w)
        at += h * w
        wrong = np.abs(hi) > 255
        bad = bad or bool(wrong.any())
        q = np.where(wrong, 0, hi * (1 << s) + lo[p])
        rec.append(reconstruct(b, q, tau, depth))
    out = {"rec": rec, "bad": bad}
    if ref is not None:
        d = [r - np.asarray(v, np.int64) for r, v in zip(rec, ref)]
        out.update(sq_err=[int((v * v).sum()) for v in d], max_err=max(int(np.abs(v).max()) for v in d))
    return out
