"""conv_x4's lean epilogue (blocks whose whole 8 x 32 tile and whole Cout tile are stored with aligned 16-byte
stores: staged bias, hoisted addressing, compile-time flags, pair GELU, pipelined iterations) against the
generic epilogue that every other block keeps: `mlic_set_kernel_option("x4_epi", 0)` sends every block down
the generic path, 2 takes the lean path in every tile class, 1 (the default) in the classes that measured
faster with it (3 x 3 convs, 1 x 1 convs on 128- / 256-row tiles; conv_x4.hip launch_x4).  Per case the three
outputs are bit-identical, all pass the float64 check of tests/test_gpu_conv.py at its x4 tolerance (rtol
2e-5), and the outputs are NaN-filled first, so an element no store reaches fails.

`lean_blocks` restates the kernel's block rule (conv_x4.hip) from the shape alone, and every case declares
whether it holds a lean block under setting 2; the test asserts that the declaration and the rule agree, so a change of the
tile rule cannot turn a case into generic against generic unnoticed.  Cases with no lean block: the partial
Cout tile, the unaligned output view, and the two odd-width grids 19 x 45 and 17 x 30 (Wo % 4 != 0 rules out
16-byte stores for the whole launch: conv_vec_ok) -- 19 x 44 and 18 x 28 are their aligned twins, which do
mix full and ragged tiles in one launch."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GELU, GDN, IGDN, TANH, MASK_A, MASK_N, RES, SHUFFLE, SQUARE = 1, 2, 4, 8, 16, 32, 64, 128, 256
X4, X4H = 7, 8
TR, TC = 8, 32


def reference(x, w, b, stride, epi, res):  # tests/test_gpu_conv.py's
    y = F.conv2d((x * x) if epi & SQUARE else x, w, b, stride=stride, padding=w.shape[-1] // 2)
    if epi & GELU:
        y = F.gelu(y)
    if epi & GDN:
        y = x * torch.rsqrt(y)
    if epi & IGDN:
        y = x * torch.sqrt(y)
    if epi & TANH:
        y = 0.5 * torch.tanh(y)
    if epi & (MASK_A | MASK_N):  # checkerboard: anchor cells have (h + w) odd
        hh = torch.arange(y.shape[-2], device=y.device).view(-1, 1)
        ww = torch.arange(y.shape[-1], device=y.device).view(1, -1)
        anchor = ((hh + ww) % 2) == 1
        y = y * (anchor if epi & MASK_A else ~anchor).to(y.dtype)
    if epi & SHUFFLE:
        y = F.pixel_shuffle(y, 2)
    if epi & RES:
        y = y + res
    return y


def check(y, ref, rtol=2e-5):
    assert torch.isfinite(y).all(), "unwritten or non-finite outputs"
    err = (y - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err <= rtol * scale + 1e-6, f"max err {err:.3e} (scale {scale:.3e})"


def x4_bm(cout):  # conv_x4.hip x4_bm, default switches
    if cout <= 64:
        return 64
    if cout == 1280:
        return 128
    if cout <= 96:
        return 96
    if 128 < cout <= 192:
        return 192
    if 192 < cout <= 224:
        return 224
    w256, w128 = -(-cout // 256) * 256 - cout, -(-cout // 128) * 128 - cout
    return 256 if cout >= 192 and 8 * (w256 - w128) <= cout else 128


def lean_blocks(cout, Ho, Wo, K, epi, aligned=True):
    """(lean, all) block counts of one image's launch, by the kernel's rule."""
    bm = x4_bm(cout)
    npix = Ho * Wo
    H, W = (-(-npix // TC), TC) if K == 1 else (Ho, Wo)  # K = 1 folds the pixels into rows of 32
    nct, nty, ntx = -(-cout // bm), -(-H // TR), -(-W // TC)
    vec = aligned and Wo % 4 == 0 and not (epi & SHUFFLE and epi & (GDN | IGDN | MASK_A | MASK_N))
    if epi & SHUFFLE and (K == 1 or epi & ~(SHUFFLE | GELU | SQUARE)):
        vec = False
    lean = 0
    for ct in range(nct):
        for ty in range(nty):
            for tx in range(ntx):
                full = (ty + 1) * TR <= H and (tx + 1) * TC <= W and (ct + 1) * bm <= cout
                if K == 1:
                    full = full and (ty + 1) * TR * TC <= npix
                lean += bool(full and vec)
    return lean, nct * nty * ntx


def operands(B, cin, cout, H, W, K, stride, epi, seed=0):  # tests/test_gpu_conv.py run()'s
    g = torch.Generator().manual_seed(seed)
    dev = torch.device("cuda")
    x = (torch.rand(B, cin, H, W, generator=g) - 0.5).to(dev)
    w = ((torch.rand(cout, cin, K, K, generator=g) - 0.5) / (cin * K * K) ** 0.5).to(dev)
    b = (torch.rand(cout, generator=g) - 0.5).to(dev)
    if epi & (GDN | IGDN):
        x = x * 4
        w = w.abs() * 0.1
        b = 1.0 + b.abs()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    oshape = (B, cout // 4, 2 * Ho, 2 * Wo) if epi & SHUFFLE else (B, cout, Ho, Wo)
    res = (torch.rand(*oshape, generator=g) - 0.5).to(dev) if epi & RES else None
    return x, w, b, res, oshape


def conv(impl, x, w, b, res, oshape, stride, epi, offset=0):
    """One mlic_conv_run into a NaN-filled output; offset: the output is a view that many floats into its buffer."""
    from mlic_amd import _lib
    n = 1
    for d in oshape:
        n *= d
    buf = torch.full((n + offset,), float("nan"), device=x.device)
    y = buf[offset:].view(oshape)
    B, cin, H, W = x.shape
    aux = x if epi & (GDN | IGDN) else None
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    _lib.call("mlic_conv_run", C.c_void_p(st), impl, ptr(x), ptr(w), ptr(b), ptr(y), B, cin, w.shape[0], H, W,
              w.shape[-1], stride, epi, ptr(aux), ptr(res))
    torch.cuda.synchronize()
    return y


def both(impl, B, cin, cout, H, W, K, epi, stride=1, offset=0, rtol=2e-5):
    from mlic_amd import _lib
    x, w, b, res, oshape = operands(B, cin, cout, H, W, K, stride, epi)
    ref = reference(x.double(), w.double(), b.double(), stride, epi, res.double() if res is not None else None).float()
    ys = {}
    try:
        for v in (2, 1, 0):
            _lib.call("mlic_set_kernel_option", b"x4_epi", v)
            ys[v] = conv(impl, x, w, b, res, oshape, stride, epi, offset)
    finally:
        _lib.call("mlic_set_kernel_option", b"x4_epi", -1)
    for v in (2, 1, 0):
        check(ys[v], ref, rtol)
    assert torch.equal(ys[2], ys[0])
    assert torch.equal(ys[1], ys[0])


# (B, Cin, Cout, H, W, K, epi, holds a lean block)
CASES = [
    (2, 192, 768, 16, 64, 3, SHUFFLE, True),               # full tiles only: 3 x 256-row tiles, 2 x 2 pixel tiles
    (2, 192, 768, 16, 64, 3, GELU | SHUFFLE, True),
    (2, 64, 256, 8, 32, 3, 0, True),                       # one full tile
    (2, 64, 256, 8, 32, 3, GELU, True),
    (2, 64, 256, 8, 32, 3, RES, True),
    (2, 64, 256, 8, 32, 3, GELU | RES, True),
    (1, 192, 768, 19, 45, 3, SHUFFLE, False),              # ragged at every edge; odd width: no 16-byte stores
    (1, 192, 768, 19, 44, 3, SHUFFLE, True),               # ... aligned width: full and ragged tiles in one launch
    (1, 192, 768, 19, 44, 3, GELU | SHUFFLE, True),
    (1, 100, 200, 9, 33, 3, 0, False),                     # partial Cout tile (200 of 224 rows): every block generic
    (2, 640, 224, 16, 32, 1, GELU, True),                  # K = 1, folded rows, full tiles, 224-row tile
    (2, 640, 224, 17, 30, 1, GELU, False),                 # K = 1, ragged, odd width
    (2, 640, 224, 18, 28, 1, GELU, True),                  # ... aligned width: a full and a ragged folded tile
    (2, 960, 320, 16, 32, 1, GELU, True),                  # 128-row tiles: two whole, the third half (generic)
    (2, 256, 96, 16, 32, 5, 0, True),                      # 96-row tile
    (2, 800, 64, 16, 32, 1, RES, True),                    # 64-row tile
    (2, 192, 192, 16, 32, 3, GDN | SQUARE | RES, True),    # 192-row tile
    (2, 128, 128, 16, 32, 3, IGDN | SQUARE, True),         # 128-row tile
    (2, 96, 64, 16, 32, 1, MASK_A, True),                  # masks
    (2, 96, 64, 16, 32, 1, MASK_N, True),
    (2, 96, 64, 16, 32, 1, MASK_A | RES, True),
    (2, 96, 64, 16, 24, 1, MASK_N | RES, True),            # masks on a folded grid that is not the image grid
    (2, 96, 64, 16, 64, 3, TANH | MASK_A | RES, True),     # the LRP head's combination, K = 3
    (1, 64, 64, 8, 32, 1, TANH, True),                     # TANH_HALF
    (1, 192, 192, 16, 64, 3, GELU, True),                  # 192-row tile, GELU on 4 x 2 waves
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c[:7]))
def test_x4_lean_vs_generic(case):
    B, cin, cout, H, W, K, epi, has_lean = case
    lean, blocks = lean_blocks(cout, H, W, K, epi)
    assert (lean > 0) == has_lean, (lean, blocks)
    both(X4, B, cin, cout, H, W, K, epi)


def test_x4_lean_vs_generic_stride2():
    """3 x 3 stride 2 (per-tap form): the tiling grid is the output grid (16 x 64), not the input's."""
    assert lean_blocks(192, 16, 64, 3, GELU)[0] > 0
    both(X4, 1, 192, 192, 32, 128, 3, GELU, stride=2)


def test_x4_lean_vs_generic_fp16_operands():
    """The reduced-precision form's instantiations (fp16 x fp16 products): the same epilogues.  Against the
    fp32 float64 reference the bound is the operand rounding's (2e-3, tests/test_gpu_conv.py)."""
    assert lean_blocks(768, 16, 64, 3, GELU | SHUFFLE)[0] > 0
    both(X4H, 2, 192, 768, 16, 64, 3, GELU | SHUFFLE, rtol=2e-3)


def test_x4_unaligned_output_is_generic():
    """`out` offset by one float: conv_vec_ok is false, every block takes the generic path under both settings."""
    assert lean_blocks(256, 8, 32, 3, 0, aligned=False)[0] == 0
    assert lean_blocks(256, 8, 32, 3, 0)[0] > 0
    both(X4, 2, 64, 256, 8, 32, 3, 0, offset=1)


def test_whole_model_same_bits():
    """compress + decompress of one 128 x 192 MLICPP_L image: byte-identical strings and equal x_hat under every
    setting of "x4_epi"."""
    from mlic_amd import _lib, get_model, synthetic
    dev = torch.device("cuda:0")
    net = get_model("MLICPP_L")
    net.load_state_dict(synthetic.synth_state_dict("MLICPP_L", 0))
    net = net.to(dev).eval()
    net.update()
    x = synthetic.synth_image(128, 192, 18).to(dev)
    outs = {}
    try:
        for v in (2, 1, 0):
            _lib.call("mlic_set_kernel_option", b"x4_epi", v)
            c = net.compress(x)
            d = net.decompress(c["strings"], c["shape"])
            torch.cuda.synchronize()
            outs[v] = (c["strings"], d["x_hat"].cpu())
    finally:
        _lib.call("mlic_set_kernel_option", b"x4_epi", -1)
    assert outs[2][0] == outs[0][0] and outs[1][0] == outs[0][0]
    assert torch.isfinite(outs[0][1]).all()
    assert torch.equal(outs[2][1], outs[0][1]) and torch.equal(outs[1][1], outs[0][1])
