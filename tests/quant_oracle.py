"""Test-side oracle of the entropy front: the slice loop's quantisation (quant_phase), the decoder's
scale indexes and dequantisation (phase_indexes, phase_dequant), the reciprocal plane, the checkerboard
mask and the entropy bottleneck (eb_forward, eb_dequant), restated in numpy from their definitions.

The contract, as the kernels must keep it (fp32, one rounding per operation, no fused multiply-add):

    anchor(h, w)   (h + w) odd; phase 0 codes the anchor pixels, phase 1 the others
    q              rint((y - m) * g), or rint(y - m) without a gain (rint: ties to even), and + 0 after it:
                   a -0 (from y - m in [-0.5, -0]) becomes +0, which is what the decoder makes of the symbol 0
    y_hat          q * r + m, or q + m without a gain; r = the fp32 1 / g
    index          (n - 1) - #{t in table[:-1] : max(s * g, 0.11) <= t}   (s alone without a gain)
    squeezed pos.  (c * H + h) * (W / 2) + (w >> 1) within an image, images contiguous
    phase 0        y_hat is +0 at the non-anchor pixels;  phase 1 leaves the anchor pixels untouched
    sym16          q saturated to [-nlim - 1, nlim] (a NaN saturates high); the overflow flag is set
                   exactly when some q did not fit
    likelihood     GaussianConditional at (y, s, m) * g, with (s, m) from the anchor phase's parameters
                   at anchor pixels and from the phase's own elsewhere
    bottleneck     r = rint(z - med) + 0, z_hat = r + med, sym = r; the decoder's z_hat = float(sym) + med

The integer and y_hat / z_hat paths are exact in fp32 and are compared bit for bit.  The two likelihoods
are evaluated in float64 from the fp32 quantities the definition fixes (the rounding decision, |y_hat - m|
and the bounded scale for the Gaussian; z_hat for the bottleneck)."""
import math

import numpy as np
import torch

F = np.float32
FLOOR = F(1e-9)          # compressai's likelihood lower bound, as fp32
SCALE_BOUND = F(0.11)


def anchors(H, W):
    """[H][W] bool: the checkerboard's anchor pixels."""
    h = np.arange(H).reshape(-1, 1)
    w = np.arange(W).reshape(1, -1)
    return ((h + w) & 1) == 1


def bits(a):
    """The bit patterns of a float32 array (so that -0 != +0 and NaN == NaN of the same payload)."""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def scale_index(s, table):
    """compressai build_indexes on fp32 scales of any shape -> int32."""
    table = np.asarray(table, F)
    sb = np.fmax(np.asarray(s, F), SCALE_BOUND)   # fmax: a NaN scale is bounded to 0.11 as fmaxf does
    le = sb[..., None] <= table[:-1]
    return (len(table) - 1 - le.sum(-1)).astype(np.int32)


def squeeze(x, phase):
    """[B][C][H][W] -> [B][C][H][W/2]: the pixels of `phase` in squeezed order, by explicit position."""
    B, C, H, W = x.shape
    out = np.zeros((B, C, H * (W // 2)), x.dtype)
    mine = anchors(H, W) == (phase == 0)
    for h in range(H):
        for w in range(W):
            if mine[h, w]:
                out[:, :, h * (W // 2) + (w >> 1)] = x[:, :, h, w]
    return out.reshape(B, C, H, W // 2)


def _gain(g, B, H, W):
    """None | [B] per image | [B][H][W] per pixel -> (g, r) broadcastable to [B][C][H][W], r = fp32 1 / g."""
    if g is None:
        return None, None
    g = np.asarray(g, F)
    g = g.reshape(B, 1, 1, 1) if g.ndim == 1 else g.reshape(B, 1, H, W)
    return g, (F(1.0) / g).astype(F)


def std_cum64(x):
    x = torch.from_numpy(np.ascontiguousarray(x, np.float64))
    return (0.5 * torch.erfc(-math.sqrt(0.5) * x)).numpy()        # float64 erfc (numpy has none)


def gauss_lik64(y, s, m):
    """GaussianConditional.forward (eval) of fp32 y, s, m -> (float64 likelihood before the floor).
    The dequantised value, its distance from the mean and the bounded scale are the fp32 quantities of the
    definition (the rounding decision lives there); the two normal cumulatives and their difference are
    float64."""
    y, s, m = (np.asarray(a, F) for a in (y, s, m))
    with np.errstate(invalid="ignore"):
        outv = (np.rint((y - m).astype(F)).astype(F) + m).astype(F)
        v = np.abs((outv - m).astype(F)).astype(np.float64)
        sb = np.fmax(s, SCALE_BOUND).astype(np.float64)
        return std_cum64((0.5 - v) / sb) - std_cum64((-0.5 - v) / sb)


def quant_phase(y, params, table, phase, gain=None, params_a=None, nlim=32767):
    """y [B][C][H][W], params / params_a [B][2C][H][W] (scales then means), gain as _gain ->
    dict: mine [H][W] bool (the phase's pixels), yh [B][C][H][W] (valid at `mine`; phase 0: +0 elsewhere),
    q fp32 and sym int32, idx int32, sym16 int16, idx8 uint8 in squeezed form [B][C][H][W/2], ovf 0 | 1,
    sym_defined (squeezed bool: q is finite and inside int32, so the cast is defined),
    lik64 [B][C][H][W] (when params_a is given; before the floor)."""
    y = np.asarray(y, F)
    params = np.asarray(params, F)
    B, C, H, W = y.shape
    assert params.shape == (B, 2 * C, H, W) and W % 2 == 0 and phase in (0, 1)
    s, m = params[:, :C], params[:, C:]
    g, r = _gain(gain, B, H, W)
    mine = anchors(H, W) == (phase == 0)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (y - m).astype(F)
        q = (np.rint(d if g is None else (d * g).astype(F)) + F(0.0)).astype(F)
        yh = (q + m).astype(F) if g is None else ((q * r).astype(F) + m).astype(F)
    yh = np.where(mine, yh, F(0.0)).astype(F)
    se = s if g is None else (s * g).astype(F)
    out = {"mine": mine, "yh": yh}
    qs = squeeze(q, phase)
    out["q"] = qs
    out["sym_defined"] = np.isfinite(qs) & (np.abs(qs) < F(2.0 ** 31))
    out["sym"] = np.where(out["sym_defined"], qs, F(0)).astype(np.int64).astype(np.int32)
    out["idx"] = squeeze(scale_index(se, table), phase)
    out["idx8"] = out["idx"].astype(np.uint8)
    lim = F(nlim)
    with np.errstate(invalid="ignore"):
        fits = (qs >= -lim - F(1.0)) & (qs <= lim)          # a NaN does not fit ...
        sat = np.where(qs < F(0.0), -lim - F(1.0), lim)     # ... and saturates high
    out["sym16"] = np.where(fits, qs, sat).astype(np.int16)
    out["ovf"] = int(not fits.all())
    if params_a is not None:
        pa = np.asarray(params_a, F)
        anc = anchors(H, W)
        ss = np.where(anc, pa[:, :C], s)
        mm = np.where(anc, pa[:, C:], m)
        if g is None:
            out["lik64"] = gauss_lik64(y, ss, mm)
        else:
            out["lik64"] = gauss_lik64((y * g).astype(F), (ss * g).astype(F), (mm * g).astype(F))
    return out


def phase_dequant(sym, params, phase, gain=None):
    """The decoder's y_hat from squeezed integer symbols [B][C][H][W/2] (int16 or int32) -> (mine, yh)."""
    params = np.asarray(params, F)
    B, C2, H, W = params.shape
    C = C2 // 2
    m = params[:, C:]
    g, r = _gain(gain, B, H, W)
    mine = anchors(H, W) == (phase == 0)
    q = np.zeros((B, C, H, W), F)
    for h in range(H):
        for w in range(W):
            if mine[h, w]:
                q[:, :, h, w] = np.asarray(sym)[:, :, h, w >> 1].astype(F)
    yh = (q + m).astype(F) if g is None else ((q * r).astype(F) + m).astype(F)
    return mine, np.where(mine, yh, F(0.0)).astype(F)


def ckbd_mask(x, keep_anchor):
    x = np.asarray(x, F)
    keep = anchors(x.shape[-2], x.shape[-1]) == bool(keep_anchor)
    return np.where(keep, x, F(0.0)).astype(F)


# ------------------------------------------------------------------------------- entropy bottleneck
EB_NAMES = ("quantiles", "m0", "m1", "m2", "m3", "m4", "b0", "b1", "b2", "b3", "b4", "f0", "f1", "f2", "f3")


def eb_quant(z, quantiles):
    """z [B][C][H][W], quantiles [C][1][3] -> (z_hat fp32, sym int32)."""
    z = np.asarray(z, F)
    med = np.asarray(quantiles, F)[:, 0, 1].reshape(1, -1, 1, 1)
    r = (np.rint((z - med).astype(F)) + F(0.0)).astype(F)
    return (r + med).astype(F), r.astype(np.int32)


def eb_dequant(sym, quantiles):
    med = np.asarray(quantiles, F)[:, 0, 1].reshape(1, -1, 1, 1)
    return (np.asarray(sym).astype(F) + med).astype(F)


def _softplus64(x):
    x = np.asarray(x, np.float64)
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))   # F.softplus(beta=1, threshold=20)


def eb_logits64(p, x):
    """The factorised cumulative's logits (filters 3, 3, 3, 3) at x [B][C][H][W], float64, written out per
    output unit: layer l maps v [.., k] to softplus(M_l)[o][k] . v + b_l[o], then adds tanh(f_l[o]) tanh(.)."""
    C = p["quantiles"].shape[0]
    per = lambda a, *shape: np.asarray(a, np.float64).reshape(C, *shape)  # noqa: E731
    ch = lambda a: a.reshape(1, C, 1, 1)  # noqa: E731
    x = np.asarray(x, np.float64)
    m0, b0, f0 = per(p["m0"], 3), per(p["b0"], 3), per(p["f0"], 3)
    v = []
    for o in range(3):
        a = ch(_softplus64(m0[:, o])) * x + ch(b0[:, o])
        v.append(a + ch(np.tanh(f0[:, o])) * np.tanh(a))
    for l in (1, 2, 3):
        M, b, f = per(p[f"m{l}"], 3, 3), per(p[f"b{l}"], 3), per(p[f"f{l}"], 3)
        u = []
        for o in range(3):
            a = sum(ch(_softplus64(M[:, o, k])) * v[k] for k in range(3)) + ch(b[:, o])
            u.append(a + ch(np.tanh(f[:, o])) * np.tanh(a))
        v = u
    M4, b4 = per(p["m4"], 3), per(p["b4"])
    return sum(ch(_softplus64(M4[:, k])) * v[k] for k in range(3)) + ch(b4)


def eb_lik64(p, z_hat):
    """float64 likelihood of the fp32 z_hat before the floor: sigmoid(logits(z_hat + .5)) - sigmoid(logits(z_hat - .5))."""
    zh = np.asarray(z_hat, F).astype(np.float64)
    sig = lambda t: 1.0 / (1.0 + np.exp(-t))  # noqa: E731
    with np.errstate(over="ignore"):
        return sig(eb_logits64(p, zh + 0.5)) - sig(eb_logits64(p, zh - 0.5))


def eb_case(shape, seed):
    """The bottleneck test case of `shape` (B, C, H, W): (z fp32, params dict of fp32 arrays, EB_NAMES).
    Per-channel random parameters; channel 1's matrices carry entries at 19.5, 20, 20.5 and 30 (both softplus
    branches, either side of the threshold and on it); factors near 0 and near +-3; non-integer medians; z holds
    exact ties about the median (+-0.5, +-1.5, +-2.5) and values 40 either side of it (likelihood at the floor).
    The medians sit next to each channel's own median and z is drawn across its central mass, as a trained model's are."""
    B, C, H, W = shape
    rng = np.random.default_rng(seed)
    p = {"m0": rng.normal(0.5, 0.8, (C, 3, 1)), "m1": rng.normal(-0.5, 0.8, (C, 3, 3)),
         "m2": rng.normal(-0.5, 0.8, (C, 3, 3)), "m3": rng.normal(-0.5, 0.8, (C, 3, 3)),
         "m4": rng.normal(-0.5, 0.8, (C, 1, 3))}
    for i in range(4):
        p[f"b{i}"] = rng.uniform(-0.5, 0.5, (C, 3, 1))
        f = rng.normal(0.0, 1.0, (C, 3, 1))
        f[0::3] = rng.normal(0.0, 1e-3, f[0::3].shape)                                     # near 0
        f[2::3] = rng.choice([-3.0, 3.0], f[2::3].shape) + rng.normal(0, 0.05, f[2::3].shape)  # near +-3
        p[f"f{i}"] = f
    p["b4"] = rng.uniform(-0.5, 0.5, (C, 1, 1))
    # channel 1: the planted matrix entries (a steep cumulative: nearly all mass in one bin)
    p["m0"][1, 0, 0] = 19.5
    p["m0"][1, 1, 0] = 20.0
    p["m1"][1, 0, 0] = 20.5
    p["m1"][1, 2, 1] = 30.0
    p["m2"][1, 1, 1] = 20.0
    p["m3"][1, 0, 2] = 19.5
    p["m4"][1, 0, 1] = 30.0
    p = {k: np.ascontiguousarray(v, F) for k, v in p.items()}
    # where each channel's density is: the logits are increasing in x, so bisect for logits = -3, 0, 3
    # (cumulative 0.05, 0.5, 0.95) -- what training does to the quantiles
    p["quantiles"] = np.zeros((C, 1, 3), F)
    at = []
    for target in (-3.0, 0.0, 3.0):
        lo, hi = np.full(C, -1e3), np.full(C, 1e3)
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            below = eb_logits64(p, mid.reshape(1, C, 1, 1)).reshape(C) < target
            lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
        at.append(0.5 * (lo + hi))
    x_lo, x_med, x_hi = at
    med = (2 * np.floor(x_med * 32) + 1) / 64.0          # odd / 64 next to the median: never an integer,
    q = np.stack([x_lo, med, x_hi], 1).reshape(C, 1, 3)   # and med + k + 0.5 is exact in fp32
    p["quantiles"] = np.ascontiguousarray(q, F)
    med = p["quantiles"][:, 0, 1].astype(np.float64).reshape(1, C, 1, 1)
    half = 0.5 * (x_hi - x_lo)
    half[np.arange(C) != 1] = np.maximum(half[np.arange(C) != 1], 1.0)   # symbols -1, 0, 1 outside the steep channel
    half = half.reshape(1, C, 1, 1)
    z = (x_med.reshape(1, C, 1, 1) + half * rng.uniform(-1.2, 1.2, shape)).astype(F)
    flat = z.reshape(B, C, H * W)
    plant = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 40.0, -40.0], F)
    for c in range(C):
        at = (np.arange(len(plant)) * 2 + c) % (H * W)
        flat[c % B, c, at] = (p["quantiles"][c, 0, 1] + plant).astype(F)
    return z, p


# ------------------------------------------------------------------------------- quantisation test cases
ROI_GAINS = (0.002424, 0.06556, 0.13944, 0.19293, 0.37268, 0.51801, 1.0)   # the VBR models' Gain tables


def planted_rows(table, nlim, overflow, nan):
    """The planted (kind, a, b) rows, the ones most worth keeping first (a small shape holds a prefix):
    ties, narrow-range edges, clamped scales, one NaN, then every table entry with its two fp32 neighbours,
    as the scale itself and as the scale that the gain brings there."""
    rows = [("tie", m, k) for m in (0.25, -0.0, -1.75, 3.0) for k in range(-3, 4)
            if overflow or (-nlim - 1 <= k and k + 1 <= nlim)]   # under an inexact gain a tie rounds either way
    if overflow:
        rows += [("sym", float(v), 0.0) for v in (nlim, nlim + 1, -nlim - 1, -nlim - 2)]
        if nlim != 32767:
            rows += [("sym", float(v), 0.0) for v in (32767, 32768, -32768, -32769)]
    else:
        rows += [("sym", float(v), 0.0) for v in (nlim, -nlim - 1, nlim - 1, -nlim)]
    rows += [("scale", v, 0.0) for v in (0.0, -1.0, 0.05, 0.10999999, 0.11)]
    if nan:
        rows.append(("nan", 0.0, 0.0))
    t = np.asarray(table, F)
    for e in t:
        for nb in (e, np.nextafter(e, F(0)), np.nextafter(e, F(1e9))):
            rows.append(("scale", float(nb), 0.0))
            rows.append(("scale/g", float(e), float(nb) - float(e)))
    return rows


def quant_case(shape, seed, table, gain=None, nlim=32767, overflow=True, nan=False):
    """One quant_phase case: (y [B][C][H][W], params, params_a [B][2C][H][W]) fp32.  Random values (two independent
    parameter draws, so that a likelihood taken from the wrong one differs at every pixel), with the planted rows
    written into the phase's own parameters at consecutive element pairs from element 0 of every image on -- W is even,
    so a pair is one anchor and one non-anchor pixel and each row is met in either phase.  `gain` as in quant_phase:
    a row is built for the gain of the pixel it lands on (a tie under a gain of 0.5 or 2 is exact)."""
    B, C, H, W = shape
    rng = np.random.default_rng(seed)
    n = C * H * W

    def draw():
        s = np.exp(rng.uniform(math.log(0.03), math.log(400.0), (B, C, H, W)))
        s[rng.random((B, C, H, W)) < 0.05] *= -1.0
        m = 3.0 * rng.normal(0, 1, (B, C, H, W))
        return np.concatenate([s, m], 1).astype(F)

    params, params_a = draw(), draw()
    s, m = params[:, :C], params[:, C:]
    g, _ = _gain(gain, B, H, W)
    gfull = np.ones((B, C, H, W), F) if g is None else np.broadcast_to(g, (B, C, H, W))
    d = np.minimum(np.abs(s), 30.0) * rng.normal(0, 1, (B, C, H, W))
    if not overflow:
        d = np.clip(d * gfull, -(nlim + 0.4), nlim + 0.4) / gfull     # every random symbol inside the narrow range
    y = (m + d).astype(F)
    rows = planted_rows(table, nlim, overflow, nan)
    yf, sf, mf, gf = (a.reshape(B, n) for a in (y, s, m, gfull))   # views of y / params (s, m are slices: write through)
    s_w, m_w = params[:, :C].reshape(B, n), params[:, C:].reshape(B, n)
    assert np.shares_memory(yf, y)
    kinds = set()
    for j, (kind, a, b) in enumerate(rows[:n // 2]):
        for bi, i in ((bi, i) for bi in range(B) for i in (2 * j, 2 * j + 1)):
            gi = float(gf[bi, i])
            if kind == "tie":
                mv, yv, sv = a, a + (b + 0.5) / gi, 1.0
            elif kind == "sym":
                mv, yv, sv = 0.0, a / gi, 300.0
            elif kind == "scale":
                mv, yv, sv = 0.5, 0.75, a
            elif kind == "scale/g":
                mv, yv, sv = 0.5, 0.75, float(np.nextafter(F(a / gi), F(1e9) if b > 0 else F(0))) if b else a / gi
            else:
                mv, yv, sv = 0.0, float("nan"), 1.0
            yf[bi, i], mv32 = F(yv), F(mv)
            params[bi].reshape(-1)[i] = F(sv)
            params[bi].reshape(-1)[n + i] = mv32
        kinds.add(kind)
    return y, params, params_a, kinds


def eb_lik_torch(p, z_hat, dtype):
    """compressai's EntropyBottleneck._likelihood in its own form (matmuls over [C][.][N] in torch), evaluated in
    `dtype` on the CPU, before the floor: the plain fp32 restatement whose error against float64 calibrates the
    kernel's bound, and in float64 an independent check of eb_lik64."""
    import torch.nn.functional as Fn
    zh = torch.from_numpy(np.ascontiguousarray(z_hat, F))
    B, C, H, W = zh.shape
    t = {k: torch.from_numpy(v).to(dtype) for k, v in p.items()}
    v = zh.permute(1, 0, 2, 3).reshape(C, 1, -1).to(dtype)

    def logits(x):
        for i in range(5):
            x = torch.matmul(Fn.softplus(t[f"m{i}"]), x) + t[f"b{i}"]
            if i < 4:
                x = x + torch.tanh(t[f"f{i}"]) * torch.tanh(x)
        return x

    lik = torch.sigmoid(logits(v + 0.5)) - torch.sigmoid(logits(v - 0.5))
    return lik.reshape(C, B, H, W).permute(1, 0, 2, 3).contiguous().numpy()
