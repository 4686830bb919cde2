"""The linear attention kernels (ctx_partial / ctx_reduce / attn_apply, and the fused form's
linatt_pack), the channel LayerNorm and g_s's tap gather, each alone through its kernel-level C entry
against a float64 restatement of the operation, at shapes that take every branch: several key splits
with ragged last chunks, splits shorter than a chunk, empty splits, pixel counts around the launch
blocks, the checkerboard masks.

Every output buffer is NaN-filled (0xFF bytes for the fp16 one) before the call, so an element no
kernel wrote shows.  Each test prints the error it measured before it asserts."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# the project's factor for a GPU path against the fp32 CPU path of the same operation, and the conv
# tests' rtol as the cap that keeps the calibration from drifting loose
GPU_VS_CPU32 = 8.0
G_CAP = 2e-5


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def anchors(H, W):
    """[H*W] bool: the checkerboard's anchor pixels, (y + x) odd."""
    y = torch.arange(H).view(-1, 1)
    x = torch.arange(W).view(1, -1)
    return (((y + x) % 2) == 1).reshape(-1)


# =============================================================================================
# linear attention

# (B, heads, hd, H, W, nsplit, kmask, qmask)
CASES = [
    (2, 3, 32, 24, 34, 3, 0, 0),     # splits of 272 = 4 * 64 + 16
    (2, 2, 16, 24, 34, 3, 1, 1),     # the intra form
    (1, 2, 32, 68, 120, -1, 0, 0),   # the 1080p latent: the policy's 31 x 264
    (1, 2, 16, 68, 120, -1, 1, 1),   # the same latent, intra form
    (2, 1, 32, 13, 21, 1, 0, 0),     # 273 px: one split; attn_apply's second block holds 17 px
    (1, 2, 16, 14, 22, 5, 1, 1),     # splits shorter than one 64-pixel chunk
    (1, 1, 32, 9, 10, 64, 0, 0),     # 90 px in 64 splits of 2: splits 45..63 are empty
]
KINDS = ("plain", "ramp", "spike")
CASE_IDS = ["-".join(str(v) for v in c) for c in CASES]


def splits_of(case):
    from mlic_amd import _lib
    B, heads, hd, H, W, nsplit, kmask, qmask = case
    if nsplit > 0:
        return nsplit
    n = C.c_int()
    _lib.call("mlic_linatt_splits", H * W, C.byref(n))
    return n.value


def spike_pixels(case):
    """(an anchor-or-any pixel, a non-anchor pixel) inside the last 64-pixel chunk of a middle split --
    ragged in every case (the split length is no multiple of 64)."""
    B, heads, hd, H, W, nsplit, kmask, qmask = case
    HW, ns = H * W, splits_of(case)
    per = -(-HW // ns)
    filled = -(-HW // per)                       # splits that hold pixels
    s = filled // 2
    pbeg, pend = s * per, min(HW, (s + 1) * per)
    c0 = pbeg + (pend - pbeg - 1) // 64 * 64     # the last chunk's first pixel
    assert (pend - c0) % 64 != 0 and pend - c0 >= 2
    anc = anchors(H, W)
    mid = c0 + (pend - c0) // 2
    order = list(range(mid, pend)) + list(range(c0, mid))
    p_on = next(p for p in order if anc[p] or not kmask)
    p_off = next(p for p in order if not anc[p])
    return p_on, p_off


def make_inputs(case, kind, seed):
    """fp32 CPU K, V, Q [B][heads*hd][HW].  Masked cases: K is NaN at the non-anchor pixels and Q at the
    anchor pixels -- the reference squeezes them away (ckbd_*_sequeeze) and never reads them.  V stays
    finite everywhere: the kernel multiplies a masked key's V by a zero weight, and 0 * NaN is NaN."""
    B, heads, hd, H, W, nsplit, kmask, qmask = case
    D, HW = heads * hd, H * W
    g = torch.Generator().manual_seed(seed)
    K = 4 * torch.randn(B, D, HW, generator=g)
    V = 2 * torch.randn(B, D, HW, generator=g)
    Q = 3 * torch.randn(B, D, HW, generator=g)
    anc = anchors(H, W)
    keep = {}
    if kind == "ramp":
        # split maxima differ by tens; the global maximum sits in the first or the last split
        drift = torch.linspace(-40.0, 40.0, HW)
        sign = torch.tensor([1.0, -1.0]).repeat(D // 2).view(1, D, 1)
        K = K + sign * drift.view(1, 1, HW)
    elif kind == "spike":
        p_on, p_off = spike_pixels(case)
        K[:, :, p_on] += 90.0
        if kmask:
            # the odd channels' spike sits on a non-anchor pixel instead and must be ignored.  It stays
            # finite among the NaNs: fmaxf drops a NaN, so only a finite key shows a maximum taken over
            # the inactive keys
            K[:, 1::2, p_on] -= 90.0
            keep = {p_off: K[:, 1::2, p_off] + 90.0}
    if kmask:
        K[:, :, ~anc] = float("nan")
        for p, val in keep.items():
            K[:, 1::2, p] = val
    if qmask:
        Q[:, :, anc] = float("nan")
    return K, V, Q


def restatement(K, V, Q, case, dtype):
    """context.py:180-187 / 235-239 per head, from the definition: ctx = softmax_L(K) . V^T over the keys
    (the anchor pixels alone under kmask: the reference's squeezed half), out = ctx^T . softmax_c(Q) at
    the query pixels (the non-anchor pixels alone under qmask, 0 at the anchors)."""
    B, heads, hd, H, W, nsplit, kmask, qmask = case
    HW = H * W
    anc = anchors(H, W)
    k = K.to(dtype).view(B, heads, hd, HW)
    v = V.to(dtype).view(B, heads, hd, HW)
    q = Q.to(dtype).view(B, heads, hd, HW)
    if kmask:
        k, v = k[..., anc], v[..., anc]
    ctx = torch.softmax(k, dim=-1) @ v.transpose(-1, -2)          # [B][heads][c][d]
    qsel = q[..., ~anc] if qmask else q
    att = ctx.transpose(-1, -2) @ torch.softmax(qsel, dim=-2)     # [B][heads][d][queries]
    if qmask:
        out = torch.zeros(B, heads, hd, HW, dtype=dtype)
        out[..., ~anc] = att
    else:
        out = att
    return out.reshape(B, heads * hd, HW), ctx


def gpu_linatt(K, V, Q, case):
    from mlic_amd import _lib
    B, heads, hd, H, W, nsplit, kmask, qmask = case
    B = K.shape[0]
    dev = torch.device("cuda")
    k, v, q = K.to(dev).contiguous(), V.to(dev).contiguous(), Q.to(dev).contiguous()
    out = torch.full((B, heads * hd, H * W), float("nan"), device=dev)
    ctx = torch.full((B, heads, hd, hd), float("nan"), device=dev)
    _lib.call("mlic_linear_attention_run", stream(), ptr(k), ptr(v), ptr(q), ptr(out), ptr(ctx), B, heads, hd, H, W,
              nsplit, kmask, qmask)
    return out, ctx


@functools.lru_cache(maxsize=None)
def computed(ci, kind):
    """Inputs, the float64 reference, the fp32 CPU evaluation's error and the GPU result of one case,
    computed once and shared (read-only) by the tests below."""
    case = CASES[ci]
    K, V, Q = make_inputs(case, kind, 1000 * ci + KINDS.index(kind))
    ref_out, ref_ctx = restatement(K, V, Q, case, torch.float64)
    c32_out, c32_ctx = restatement(K, V, Q, case, torch.float32)
    out, ctx = gpu_linatt(K, V, Q, case)
    return dict(K=K, V=V, Q=Q, ref_out=ref_out, ref_ctx=ref_ctx, out=out, ctx=ctx,
                cpu32_out=(c32_out.double() - ref_out).abs().max().item(),
                cpu32_ctx=(c32_ctx.double() - ref_ctx).abs().max().item())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_linear_attention_vs_float64(ci, kind):
    """out and ctx within g * max|V| of float64 (out and ctx rows are convex combinations of V's values,
    so max|V| is their scale); g = 8 x the same error of the fp32 CPU evaluation of the restatement on the
    same inputs, capped at 2e-5."""
    case = CASES[ci]
    B, heads, hd, H, W, nsplit, kmask, qmask = case
    r = computed(ci, kind)
    vmax = r["V"].abs().max().item()
    out, ctx = r["out"].cpu(), r["ctx"].cpu()
    e_out = (out.double() - r["ref_out"]).abs().max().item()
    e_ctx = (ctx.double() - r["ref_ctx"]).abs().max().item()
    g_out = min(GPU_VS_CPU32 * r["cpu32_out"] / vmax, G_CAP)
    g_ctx = min(GPU_VS_CPU32 * r["cpu32_ctx"] / vmax, G_CAP)
    print(f"\nlinatt {CASE_IDS[ci]} {kind} ({splits_of(case)} splits): out err {e_out / vmax:.3e} (cpu32 "
          f"{r['cpu32_out'] / vmax:.3e}, bound {g_out:.3e}), ctx err {e_ctx / vmax:.3e} (cpu32 "
          f"{r['cpu32_ctx'] / vmax:.3e}, bound {g_ctx:.3e}) of max|V|")
    assert torch.isfinite(out).all() and torch.isfinite(ctx).all(), "unwritten or non-finite outputs"
    assert e_ctx <= g_ctx * vmax, f"ctx: max err {e_ctx:.3e}, bound {g_ctx * vmax:.3e}"
    assert e_out <= g_out * vmax, f"out: max err {e_out:.3e}, bound {g_out * vmax:.3e}"
    if qmask:
        assert (out[:, :, anchors(H, W)].view(torch.int32) == 0).all(), "anchor outputs must be +0 exactly"
    if kind == "spike":
        # a key 90 above the rest takes the whole softmax: that ctx row is the spiked pixel's V
        p_on, p_off = spike_pixels(case)
        step = 2 if kmask else 1  # under kmask the odd channels' spike is on an inactive pixel (checked above by ref)
        want = r["V"].view(B, heads, hd, H * W)[..., p_on]                # [B][heads][d]
        rows = ctx[:, :, ::step, :]                                        # [B][heads][spiked c][d]
        e_row = (rows.double() - want.double().unsqueeze(2)).abs().max().item()
        assert e_row <= max(g_ctx, 1e-7) * vmax, f"spiked ctx rows differ from V[p] by {e_row:.3e}"
        if kmask:
            off = r["V"].view(B, heads, hd, H * W)[..., p_off]
            far = (ctx[:, :, 1::2, :].double() - off.double().unsqueeze(2)).abs().max().item()
            assert far > 0.1 * vmax, "an inactive key's spike took the softmax"


@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_linear_attention_bits_repeat_and_batch(ci):
    """A second call gives the same bits, and image b of a batched call equals the call of that image
    alone (the decoder relies on both)."""
    case = CASES[ci]
    r = computed(ci, "ramp")
    out2, ctx2 = gpu_linatt(r["K"], r["V"], r["Q"], case)
    assert torch.equal(out2.view(torch.int32), r["out"].view(torch.int32))
    assert torch.equal(ctx2.view(torch.int32), r["ctx"].view(torch.int32))
    if case[0] > 1:
        for b in range(case[0]):
            o1, c1 = gpu_linatt(r["K"][b:b + 1], r["V"][b:b + 1], r["Q"][b:b + 1], case)
            assert torch.equal(o1[0].view(torch.int32), r["out"][b].view(torch.int32)), b
            assert torch.equal(c1[0].view(torch.int32), r["ctx"][b].view(torch.int32)), b


@pytest.mark.parametrize("K", [5, 3])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_linatt_pack_halves_equal_attn_apply_bits(ci, K):
    """The fused form's pack, fed the unfused call's ctx: every interior line is hi = fp16(out) | lo =
    fp16(out - float(hi)) of the unfused call's fp32 out as bit patterns (the kernel header's claim); the
    pad ring and, under qmask, the anchor lines are 64 halves of +0; nothing is written past the last line."""
    from mlic_amd import _lib
    case = CASES[ci]
    B, heads, hd, H, W, nsplit, kmask, qmask = case
    r = computed(ci, "plain")
    dev = torch.device("cuda")
    D, pad = heads * hd, K // 2
    Hp, Wp, nch = H + 2 * pad, W + 2 * pad, D // 32
    n = B * nch * Hp * Wp * 64
    guard = 64 * 64
    buf = torch.full((n + guard,), -1, dtype=torch.int16, device=dev)  # 0xFF bytes
    q = r["Q"].to(dev).contiguous()
    _lib.call("mlic_linatt_pack_run", stream(), ptr(q), ptr(r["ctx"]), ptr(buf), B, heads, hd, H, W, K, qmask)
    out = r["out"].cpu().view(B, nch, 32, H, W)
    hi = out.half()
    lo = (out - hi.float()).half()
    lines = torch.cat([hi, lo], dim=2).permute(0, 1, 3, 4, 2)            # [B][chunk][H][W][64]
    want = torch.zeros(B, nch, Hp, Wp, 64, dtype=torch.float16)
    want[:, :, pad:pad + H, pad:pad + W] = lines
    got = buf.cpu()
    assert (got[n:] == -1).all(), "written past the last line"
    got = got[:n].view(B, nch, Hp, Wp, 64)
    want = want.view(torch.int16)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} halves differ, first at [b, chunk, y, x, half] = {bad[0].tolist()}"
    ring = torch.ones(Hp, Wp, dtype=torch.bool)
    ring[pad:pad + H, pad:pad + W] = False
    assert (got[:, :, ring] == 0).all(), "pad ring must be +0"
    if qmask:
        inner = got[:, :, pad:pad + H, pad:pad + W].reshape(B, nch, H * W, 64)
        assert (inner[:, :, anchors(H, W)] == 0).all(), "anchor lines must be +0"


# =============================================================================================
# LayerNorm over channels

def gpu_layernorm(x, gamma, beta):
    from mlic_amd import _lib
    B, Cn, HW = x.shape
    dev = torch.device("cuda")
    xd, gd, bd = x.to(dev).contiguous(), gamma.to(dev), beta.to(dev)
    y = torch.full((B, Cn, HW), float("nan"), device=dev)
    _lib.call("mlic_ln_channels_run", stream(), ptr(xd), ptr(gd), ptr(bd), ptr(y), B, Cn, HW)
    return y.cpu()


def ln_reference(x, gamma, beta, dtype):
    y = F.layer_norm(x.to(dtype).transpose(1, 2), (x.shape[1],), gamma.to(dtype), beta.to(dtype), 1e-5)
    return y.transpose(1, 2)


LN_C = [32, 64, 128]
LN_HW = [1, 127, 128, 129, 273]  # around the 128-thread block; 273 = two blocks + 17


def ln_params(Cn, seed):
    g = torch.Generator().manual_seed(seed)
    return 1.0 + 0.5 * torch.randn(Cn, generator=g), torch.randn(Cn, generator=g), g


@pytest.mark.parametrize("HW", LN_HW)
@pytest.mark.parametrize("Cn", LN_C)
def test_layernorm_vs_float64(Cn, HW):
    gamma, beta, g = ln_params(Cn, 7 * Cn + HW)
    x = 3 * torch.randn(2, Cn, HW, generator=g)
    ref = ln_reference(x, gamma, beta, torch.float64)
    scale = ref.abs().max().item()
    cpu32 = (ln_reference(x, gamma, beta, torch.float32).double() - ref).abs().max().item()
    y = gpu_layernorm(x, gamma, beta)
    err = (y.double() - ref).abs().max().item()
    bound = min(GPU_VS_CPU32 * cpu32 / scale, G_CAP)
    print(f"\nlayernorm C {Cn} HW {HW}: err {err / scale:.3e} (cpu32 {cpu32 / scale:.3e}, bound {bound:.3e}) of max|ref|")
    assert torch.isfinite(y).all(), "unwritten or non-finite outputs"
    assert err <= bound * scale, f"max err {err:.3e}, bound {bound * scale:.3e}"


@pytest.mark.parametrize("Cn", LN_C)
def test_layernorm_constant_pixel_gives_beta_exactly(Cn):
    """A pixel whose C values are all equal has mean = that value and every deviation 0, so the output is
    beta exactly.  The values have at most 13 significant bits, so every partial sum k * v (k <= 128) is
    a float and the sum of the C copies is exact in any order.  (For an arbitrary float v the partial
    sums of a sequential fp32 sum round and need not reach C * v; the deviation from the mean is then
    ~1e-7 |v|, which 1 / sqrt(eps) = 316 amplifies to ~5e-5 |v gamma|.  That is fp32 arithmetic, not a
    kernel defect: it is printed below for v = 0.3f and 10.1f and not asserted.)"""
    gamma, beta, g = ln_params(Cn, 99 + Cn)
    HW = 129
    x = 3 * torch.randn(2, Cn, HW, generator=g)
    consts = {0: 1.5, 5: -3.25, 127: 1000.125, 128: 0.0, 64: -2.0 ** -10}
    for p, v in consts.items():
        x[:, :, p] = v
    x[1, :, 77] = 0.3
    x[1, :, 78] = 10.1
    y = gpu_layernorm(x, gamma, beta)
    assert torch.isfinite(y).all()
    dev = (y[1, :, 77:79] - beta.view(-1, 1)).abs().max(dim=0).values
    print(f"\nlayernorm C {Cn}: |y - beta| at a constant pixel of 0.3f: {dev[0]:.3e}, of 10.1f: {dev[1]:.3e}")
    for p in consts:
        for b in range(2):
            assert torch.equal(y[b, :, p].view(torch.int32), beta.view(torch.int32)), (b, p)


@pytest.mark.parametrize("HW", [129])
@pytest.mark.parametrize("Cn", LN_C)
def test_layernorm_offset_inputs_derived_bound(Cn, HW):
    """mean 10, sigma 1: the cancellation in x - mean is what a wrong summation would lose.  The bound is
    derived, per element, from the kernel's operation sequence (u = 2^-24, the fp32 unit roundoff; mu,
    e = x - mu, r = 1 / sqrt(var + eps) the exact per-pixel values):
      * the sequential sum of C terms is off by at most (C - 1) u sum|x|, and the division by C adds u |mu|,
        so |mean - mu| <= C u sum|x| / C = u sum|x| =: dm;
      * d = fl(x - mean) = (e - (mean - mu)) (1 + u'): |d - e| <= dm + u |d|;
      * sum (e - t)^2 = C var + C t^2 exactly for t = mean - mu (sum e = 0), so the computed variance is
        var + t^2 up to a relative (C + 4) u (2 u of d^2, C u of the fma chain, the division by C, the eps
        add); the square root halves that and adds its own u, the reciprocal another:
        |rstd - r| / r <= dm^2 r^2 / 2 + (C / 2 + 4) u;
      * y = fl(fl(fl(d rstd) gamma) + beta): two product roundings on |e r gamma|, one u |y| of the add.
    Together, with the u |d| above: |y - ref| <= |gamma| r (dm + |e| (dm^2 r^2 / 2 + (C / 2 + 7) u)) + u |ref|.
    The assert takes C / 2 + 8 and a factor 1 + 1e-3 for the second-order terms dropped."""
    gamma, beta, g = ln_params(Cn, 31 * Cn)
    x = 10.0 + torch.randn(2, Cn, HW, generator=g)
    ref = ln_reference(x, gamma, beta, torch.float64)
    xd = x.double()
    u = 2.0 ** -24
    mu = xd.mean(dim=1, keepdim=True)
    e = xd - mu
    r = 1.0 / torch.sqrt((e * e).mean(dim=1, keepdim=True) + 1e-5)
    dm = u * xd.abs().sum(dim=1, keepdim=True)
    ga = gamma.double().abs().view(1, Cn, 1)
    bound = (ga * r * (dm + e.abs() * (0.5 * dm * dm * r * r + (Cn / 2 + 8) * u)) + u * ref.abs()) * (1 + 1e-3)
    y = gpu_layernorm(x, gamma, beta)
    err = (y.double() - ref).abs()
    print(f"\nlayernorm offset C {Cn}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}, "
          f"max bound {bound.max():.3e}")
    assert torch.isfinite(y).all()
    assert (err <= bound).all(), f"max err / bound {(err / bound).max():.3f}"


# =============================================================================================
# g_s's tap gather

TAPS_SHAPES = [(2, 5, 7), (1, 4, 64), (1, 9, 65), (2, 3, 130)]  # 64 columns and 4 rows per block
TAPS_IDS = ["-".join(str(v) for v in s) for s in TAPS_SHAPES]


def gpu_taps_gather(part, bias):
    from mlic_amd import _lib
    B, _, H, W = part.shape
    dev = torch.device("cuda")
    pd = part.to(dev).contiguous()
    bd = bias.to(dev) if bias is not None else None
    out = torch.full((B, 3, 2 * H, 2 * W), float("nan"), device=dev)
    _lib.call("mlic_taps_gather_run", stream(), ptr(pd), ptr(bd), ptr(out), B, H, W)
    return out.cpu()


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", TAPS_SHAPES, ids=TAPS_IDS)
def test_taps_gather_bits(shape, with_bias):
    """Bit-equal to fp32 additions of the nine shifted planes in tap order 0..8, then the bias (additions
    only: nothing to contract).  Magnitudes 1 and 1e4 are mixed, so another order changes bits."""
    B, H, W = shape
    g = torch.Generator().manual_seed(H * 1000 + W)
    part = torch.randn(B, 108, H, W, generator=g)
    part = part * torch.where(torch.rand(B, 108, H, W, generator=g) < 0.5, 1.0, 1e4)
    bias = torch.randn(12, generator=g) if with_bias else None
    acc = torch.zeros(B, 12, H, W)
    for t in range(9):
        dy, dx = t // 3 - 1, t % 3 - 1
        plane = F.pad(part[:, t * 12:(t + 1) * 12], (1, 1, 1, 1))       # zero outside the image
        acc = acc + plane[:, :, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]   # acc[h][w] += part_t[h + dy][w + dx]
    acc = acc + (bias if with_bias else torch.zeros(12)).view(1, 12, 1, 1)
    want = F.pixel_shuffle(acc, 2)
    out = gpu_taps_gather(part, bias)
    assert torch.isfinite(out).all(), "unwritten outputs"
    bad = (out.view(torch.int32) != want.view(torch.int32)).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} elements differ, first at {bad[0].tolist()}"


@pytest.mark.parametrize("shape", TAPS_SHAPES, ids=TAPS_IDS)
def test_taps_gather_is_the_3x3_conv_and_shuffle(shape):
    """Independent of the restatement above (pins the shift direction and the shuffle): per-tap partial
    products built in float64 from a random x and w, rounded to fp32, gathered on the GPU, against
    pixel_shuffle(conv2d(x, w, b, padding=1), 2) in float64."""
    B, H, W = shape
    g = torch.Generator().manual_seed(H * 77 + W)
    x = torch.randn(B, 8, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(12, 8, 3, 3, generator=g, dtype=torch.float64)
    bias = torch.randn(12, generator=g)
    part = torch.einsum("cnt,bnhw->btchw", w.view(12, 8, 9), x).reshape(B, 108, H, W).float()
    ref = F.pixel_shuffle(F.conv2d(x, w, bias.double(), padding=1), 2)
    out = gpu_taps_gather(part, bias)
    err = (out.double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"\ntaps_gather {shape}: err {err / scale:.3e} of max|ref|")
    assert torch.isfinite(out).all(), "unwritten outputs"
    assert err <= 1e-6 * scale, f"max err {err:.3e} (scale {scale:.3e})"
