"""Rate and error maps, the parts that need no GPU: every refusal of the three C entries by its message (they are
made before any HIP call, and the library loads without a device), the CPU restatements against plain Python loops,
the Python argument checks, and the CLI's flags."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from mlic_amd import _lib, bitstream, codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# addresses that are never dereferenced: every call below is refused before the library touches the device
P = C.c_void_p(1 << 20)
NULL = None
DENSE = (3 * 40 * 72, 3 * 72, 3, 1)  # hwc strides of a 40 x 72 image


def s4(*v):
    return (C.c_int64 * 4)(*v)


# ----------------------------------------------------------------------------------------- refusals
def rate_args(**kw):
    a = dict(y_lik=P, y_bs=8 * 8 * 12, z_lik=P, z_bs=4 * 2 * 3, B=2, M=8, S=2, h=8, w=12, N=4, y_map=P, z_map=P,
             cell_bits=P, slice_bits=P)
    a.update(kw)
    return [None, a["y_lik"], a["y_bs"], a["z_lik"], a["z_bs"], a["B"], a["M"], a["S"], a["h"], a["w"], a["N"],
            a["y_map"], a["z_map"], a["cell_bits"], a["slice_bits"]]


RATE_REFUSALS = [
    (dict(y_lik=NULL), "null likelihood"), (dict(z_lik=NULL), "null likelihood"),
    (dict(y_map=NULL, z_map=NULL, cell_bits=NULL, slice_bits=NULL), "at least one output"),
    (dict(B=0), "must be positive"), (dict(M=0, S=1), "must be positive"), (dict(S=0), "must be positive"),
    (dict(N=0), "must be positive"), (dict(h=0), "must be positive"), (dict(w=-4), "must be positive"),
    (dict(S=3), "multiple of S"), (dict(h=6), "multiples of 4"), (dict(w=10), "multiples of 4"),
    (dict(y_bs=8 * 8 * 12 - 1), "batch stride"), (dict(z_bs=0), "batch stride"),
    (dict(y_bs=1 << 62), "batch stride overflows"), (dict(B=(1 << 20) + 1), "above 2\\^20"),
    (dict(y_lik=C.c_void_p((1 << 20) + 2)), "4-byte aligned"), (dict(cell_bits=C.c_void_p((1 << 20) + 4)), "8-byte aligned"),
]


@pytest.mark.parametrize("kw,word", RATE_REFUSALS)
def test_rate_map_refusals(kw, word):
    with pytest.raises(_lib.MlicError, match=word):
        _lib.call("mlic_rate_map_run", *rate_args(**kw))


def blocks_args(**kw):
    a = dict(a=P, a_s=s4(*DENSE), b=P, b_s=s4(*DENSE), B=2, H=40, W=72, block=16, out=P)
    a.update(kw)
    return [None, a["a"], a["a_s"], a["b"], a["b_s"], a["B"], a["H"], a["W"], a["block"], a["out"]]


BIG = 1 << 62
BLOCKS_REFUSALS = [
    (dict(a=NULL), "null image"), (dict(b_s=None), "null image"), (dict(out=NULL), "out must be"),
    (dict(out=C.c_void_p((1 << 20) + 2)), "4-byte aligned"),
    (dict(B=0), "must be positive"), (dict(H=0), "must be positive"), (dict(W=-1), "must be positive"),
    (dict(H=(1 << 24) + 1), "above 2\\^24"),
    (dict(block=12), "block must be"), (dict(block=0), "block must be"), (dict(block=128), "block must be"),
    (dict(a_s=s4(DENSE[0], DENSE[1], 0, 1)), "zero column or channel stride"),
    (dict(b_s=s4(DENSE[0], DENSE[1], 3, 0)), "zero column or channel stride"),
    (dict(a_s=s4(BIG, DENSE[1], 3, 1), B=4), "overflow"), (dict(b_s=s4(DENSE[0], BIG, 3, 1)), "overflow"),
    (dict(a_s=s4(-(1 << 63), DENSE[1], 3, 1)), "overflow"),
]


@pytest.mark.parametrize("kw,word", BLOCKS_REFUSALS)
def test_sq_err_blocks_refusals(kw, word):
    with pytest.raises(_lib.MlicError, match=word):
        _lib.call("mlic_image_sq_err_blocks_u8", *blocks_args(**kw))


def heat_args(**kw):
    a = dict(plane=P, B=2, ph=3, pw=5, cell=16, lo=0.0, hi=1.0, cmap=1, H=40, W=72, dst=P, d_s=s4(*DENSE), under=P,
             u_s=s4(*DENSE), alpha=77)
    a.update(kw)
    return [None, a["plane"], a["B"], a["ph"], a["pw"], a["cell"], a["lo"], a["hi"], a["cmap"], a["H"], a["W"], a["dst"],
            a["d_s"], a["under"], a["u_s"], a["alpha"]]


HEAT_REFUSALS = [
    (dict(plane=NULL), "null plane"), (dict(dst=NULL), "null plane"), (dict(d_s=None), "null plane"),
    (dict(plane=C.c_void_p((1 << 20) + 4)), "8-byte aligned"),
    (dict(B=0), "must be positive"), (dict(H=0), "must be positive"), (dict(ph=0), "must be positive"),
    (dict(cell=0), "cell must be"), (dict(cell=24), "cell must be"), (dict(cell=128), "cell must be"),
    (dict(ph=2), "do not cover"), (dict(pw=4), "do not cover"),
    (dict(cmap=2), "cmap"), (dict(cmap=-1), "cmap"),
    (dict(alpha=257), "alpha must be"), (dict(alpha=-1), "alpha must be"),
    (dict(hi=0.0), "finite lo < hi"), (dict(lo=2.0), "finite lo < hi"), (dict(hi=math.inf), "finite lo < hi"),
    (dict(lo=-math.inf), "finite lo < hi"), (dict(lo=math.nan), "finite lo < hi"), (dict(hi=math.nan), "finite lo < hi"),
    (dict(lo=-1.7e308, hi=1.7e308), "finite lo < hi"),
    (dict(under=NULL, alpha=255), "needs an under-image"), (dict(under=NULL, alpha=0), "needs an under-image"),
    (dict(u_s=None), "under-image needs strides"),
    (dict(d_s=s4(DENSE[0], DENSE[1], 0, 1)), "stride.*dst"), (dict(d_s=s4(DENSE[0], DENSE[1], 3, 0)), "stride.*dst"),
    (dict(u_s=s4(DENSE[0], DENSE[1], 0, 1)), "stride.*under"), (dict(u_s=s4(BIG, DENSE[1], 3, 1), B=4), "overflow.*under"),
    (dict(d_s=s4(DENSE[0], BIG, 3, 1)), "overflow.*dst"),
]


@pytest.mark.parametrize("kw,word", HEAT_REFUSALS)
def test_heat_refusals(kw, word):
    with pytest.raises(_lib.MlicError, match=word):
        _lib.call("mlic_image_heat_u8", *heat_args(**kw))


def test_python_refusals():
    img = torch.zeros(1, 64, 64, 3, dtype=torch.uint8)
    for name, word in (("tile", "tiled"), ("scale", "scaled"), ("coded_size", "scaled"), ("depth", "deeper than 8"),
                       ("yuv", "Y'CbCr"), ("max_bpp", "rate loop")):
        with pytest.raises(ValueError, match=f"{name}=.*{word}"):
            codec.rate_map(None, img, **{name: 1})  # refused before the model is touched
    with pytest.raises(TypeError, match="unexpected argument 'bogus'"):
        codec.rate_map(None, img, bogus=1)
    x = torch.zeros(1, 3, 64, 64)
    for kw, name in ((dict(tile=256), "tile"), (dict(yuv=codec.YuvFormat()), "yuv"), (dict(max_bpp=1.0), "max_bpp"),
                     (dict(scale=2), "scale"), (dict(coded_size=(32, 32)), "coded_size"), (dict(depth=10), "depth")):
        with pytest.raises(ValueError, match=f"rate_map=True together with {name}="):
            bitstream.code_image(None, x, rate_map=True, **kw)
    plane = torch.zeros(3, 5, dtype=torch.float64)
    for kw, word in ((dict(cell=24), "cell must be"), (dict(cmap="jet"), "cmap"), (dict(alpha=300), "alpha"),
                     (dict(alpha=128), "under="), (dict(lo=1.0, hi=1.0), "lo < hi"), (dict(hi=math.inf), "lo < hi"),
                     (dict(H=49), "does not cover"), (dict(layout="nhwc"), "layout")):
        a = dict(plane=plane, H=40, W=72, cell=16, lo=0.0, hi=1.0)
        a.update(kw)
        with pytest.raises(ValueError, match=word):
            codec.heat_u8(**a)
    with pytest.raises(ValueError, match="float64 plane"):
        codec.heat_u8(plane.float(), 40, 72, 16)
    with pytest.raises(ValueError, match="under must have shape"):
        codec.heat_u8(plane, 40, 72, 16, under=torch.zeros(1, 40, 70, 3, dtype=torch.uint8), alpha=10)
    a = torch.zeros(1, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="block must be"):
        codec.sq_err_blocks(a, a, block=4)
    with pytest.raises(ValueError, match="one shape"):
        codec.sq_err_blocks(a, a[:, :8])
    lik = torch.ones(1, 8, 8, 12)
    with pytest.raises(ValueError, match="do not split"):
        codec.rate_maps(lik, torch.ones(1, 4, 2, 3), 3)
    with pytest.raises(ValueError, match="z_lik"):
        codec.rate_maps(lik, torch.ones(1, 4, 2, 4), 2)
    with pytest.raises(ValueError, match="float32"):
        codec.rate_maps(lik.double(), torch.ones(1, 4, 2, 3), 2)


# ------------------------------------------------------------------------------------- restatements
@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("block", [8, 16, 64])
def test_sq_err_blocks_cpu_against_a_plain_loop(layout, block):
    g = torch.Generator().manual_seed(5)
    B, H, W = 2, 19, 37
    shape = (B, H, W, 3) if layout == "hwc" else (B, 3, H, W)
    a = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
    b = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
    b[0] = a[0]
    got = codec._sq_err_blocks_cpu(a, b, block, layout)
    an, bn = (t.numpy() if layout == "hwc" else t.permute(0, 2, 3, 1).numpy() for t in (a, b))
    nby, nbx = -(-H // block), -(-W // block)
    want = np.zeros((B, nby, nbx))
    for i in range(B):
        for y in range(H):
            for x in range(W):
                for c in range(3):
                    want[i, y // block, x // block] += (float(an[i, y, x, c]) - float(bn[i, y, x, c])) ** 2
    assert got.dtype == torch.int64 and tuple(got.shape) == (B, nby, nbx)
    assert np.array_equal(got.numpy().astype(np.float64), want)
    assert int(got[0].abs().sum()) == 0
    assert torch.equal(codec.sq_err_blocks(a, b, block, layout), got)  # the public call on CPU tensors
    assert torch.equal(got.flatten(1).sum(1), codec.sq_err_roi(a, b, torch.ones(B, H, W, dtype=torch.uint8), layout)[:, 0])


def heat_plane(ph, pw, lo, hi, seed):
    """Values across and beyond [lo, hi], with NaN, +-inf, lo, hi and rounding midpoints among them; as many images
    as it takes to hold them and as many random cells."""
    r = np.random.default_rng(seed)
    p = lo + (hi - lo) * r.uniform(-0.2, 1.2, (max(2, -(-26 // (ph * pw))), ph, pw))
    flat = p.reshape(-1)
    special = [math.nan, math.inf, -math.inf, lo, hi] + [lo + (hi - lo) * (k + 0.5) / 255.0 for k in (0, 1, 84, 85, 127, 169, 170, 254)]
    flat[r.permutation(flat.size)[:len(special)]] = special
    return torch.from_numpy(p)


def heat_loop(p, H, W, cell, lo, hi, cmap, under, alpha):
    """Per pixel, in Python floats (IEEE doubles) and ints; under: numpy [B,H,W,3] or None -> numpy [B,H,W,3]."""
    B = p.shape[0]
    out = np.zeros((B, H, W, 3), np.uint8)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                v = float(p[b, y // cell, x // cell])
                if math.isnan(v):
                    out[b, y, x] = (255, 0, 255)
                    continue
                t = (v - lo) / (hi - lo) * 255.0 + 0.5
                q = 0 if t < 0 else 255 if t > 255 else int(math.floor(t))
                col = (q, q, q) if cmap == "gray" else (min(255, 3 * q), min(max(3 * q - 255, 0), 255),
                                                         min(max(3 * q - 510, 0), 255))
                for c in range(3):
                    o = col[c]
                    if under is not None:
                        o = (alpha * o + (256 - alpha) * int(under[b, y, x, c]) + 128) >> 8
                    out[b, y, x, c] = o
    return out


@pytest.mark.parametrize("cell,lo,hi", [(16, 0.0, 1.0), (64, -3.0, 252.0), (16, 0.0, 37.3)])
@pytest.mark.parametrize("cmap", ["hot", "gray"])
def test_heat_u8_cpu_against_a_pixel_loop(cell, lo, hi, cmap):
    H, W = 40, 72  # cropped last cells for both cell sizes
    ph, pw = -(-H // cell), -(-W // cell)
    p = heat_plane(ph, pw, lo, hi, seed=cell)
    assert torch.isnan(p).any() and torch.isinf(p).any() and (p == lo).any() and (p == hi).any()
    under = torch.randint(0, 256, (p.size(0), H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(2))
    for alpha in (0, 128, 256):
        want = heat_loop(p.numpy(), H, W, cell, lo, hi, cmap, under.numpy(), alpha)
        got = codec.heat_u8(p, H, W, cell, lo, hi, cmap, under=under, alpha=alpha, layout="hwc")
        assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want), alpha
        chw = codec.heat_u8(p, H, W, cell, lo, hi, cmap, under=under.permute(0, 3, 1, 2), alpha=alpha, layout="chw")
        assert np.array_equal(chw.permute(0, 2, 3, 1).numpy(), want)
    want = heat_loop(p.numpy(), H, W, cell, lo, hi, cmap, None, 256)
    assert np.array_equal(codec.heat_u8(p, H, W, cell, lo, hi, cmap).numpy(), want)
    assert np.array_equal(codec.heat_u8(p, H, W, cell, lo, hi, cmap, under=under, alpha=256).numpy(), want)
    nan = np.isnan(p.numpy())[:, np.arange(H) // cell][:, :, np.arange(W) // cell]
    assert (want[nan] == (255, 0, 255)).all()


def test_heat_default_hi_is_the_finite_maximum():
    p = torch.tensor([[0.0, 2.0, math.nan], [math.inf, 8.0, 4.0]], dtype=torch.float64)
    got = codec.heat_u8(p, 32, 48, 16, cmap="gray")
    assert torch.equal(got, codec.heat_u8(p, 32, 48, 16, 0.0, 8.0, cmap="gray"))
    assert got[0, 20, 20].tolist() == [255, 255, 255] and got[0, 0, 20].tolist() == [64, 64, 64]
    flat = codec.heat_u8(torch.zeros(2, 3, dtype=torch.float64), 32, 48, 16, cmap="gray")  # nothing above lo: hi = lo + 1
    assert int(flat.max()) == 0


def plane_sum_loop(p):
    """One plane [ph][pw] of Python floats: lanes, fold in halves, rows top to bottom."""
    total = 0.0
    for row in p:
        lanes = [0.0] * 64
        for x, v in enumerate(row):
            lanes[x % 64] = lanes[x % 64] + v
        for off in (32, 16, 8, 4, 2, 1):
            for l in range(off):
                lanes[l] = lanes[l] + lanes[l + off]
        total = total + lanes[0]
    return total


@pytest.mark.parametrize("S,h,w", [(3, 8, 132), (2, 4, 4), (1, 12, 64)])
def test_cell_and_slice_bits_against_sequential_sums(S, h, w):
    g = torch.Generator().manual_seed(S * h + w)
    B = 2
    y = torch.rand(B, S, h, w, dtype=torch.float64, generator=g) * 40
    z = torch.rand(B, h // 4, w // 4, dtype=torch.float64, generator=g) * 7
    y[0, 0, 1, 2] = 0.0
    cell = codec._cell_bits_cpu(y, z)
    sl = codec._slice_bits_cpu(y, z)
    assert cell.dtype == torch.float64 and tuple(cell.shape) == (B, h, w) and tuple(sl.shape) == (B, S + 1)
    yl, zl = y.tolist(), z.tolist()
    for b in range(B):
        for i in range(h):
            for j in range(w):
                v = zl[b][i // 4][j // 4] / 16
                for s in range(S):
                    v = v + yl[b][s][i][j]
                assert cell[b, i, j].item() == v
        for s in range(S):
            assert sl[b, s].item() == plane_sum_loop(yl[b][s])
        assert sl[b, S].item() == plane_sum_loop(zl[b])
    # a NaN stays where it is
    y[1, S - 1, 2, 3] = math.nan
    cell, sl = codec._cell_bits_cpu(y, z), codec._slice_bits_cpu(y, z)
    assert int(torch.isnan(cell).sum()) == 1 and bool(torch.isnan(cell[1, 2, 3]))
    assert int(torch.isnan(sl).sum()) == 1 and bool(torch.isnan(sl[1, S - 1]))


def test_rate_maps_on_cpu_tensors():
    """The CPU path: the same definitions on torch's fp32 log2, within the log2f bound of the float64 sums."""
    g = torch.Generator().manual_seed(3)
    B, M, S, N, h, w = 2, 8, 2, 4, 8, 12
    y = torch.rand(B, M, h, w, generator=g).clamp_(1e-9, 1.0)
    z = torch.rand(B, N, h // 4, w // 4, generator=g).clamp_(1e-9, 1.0)
    y[0, 0, 0, 0], y[0, 1, 0, 0], y[0, 2, 0, 0], y[0, 3, 0, 0] = 1.0, 1.0, 1.0, 1.0
    m = codec.rate_maps(y, z, S)
    assert {k: tuple(v.shape) for k, v in m.items()} == {"y_map": (B, S, h, w), "z_map": (B, h // 4, w // 4),
                                                         "cell_bits": (B, h, w), "slice_bits": (B, S + 1)}
    assert all(v.dtype == torch.float64 and not bool(torch.signbit(v).any()) for v in m.values())
    assert m["y_map"][0, 0, 0, 0].item() == 0.0
    ty = -torch.log2(y.double())
    want = ty.reshape(B, S, M // S, h, w).sum(2)
    assert bool(((m["y_map"] - want).abs() <= 4 * 2.0 ** -23 * want.abs()).all())
    assert torch.equal(m["cell_bits"], codec._cell_bits_cpu(m["y_map"], m["z_map"]))
    assert torch.equal(m["slice_bits"], codec._slice_bits_cpu(m["y_map"], m["z_map"]))


# ---------------------------------------------------------------------------------------------- CLI
def _cli():
    spec = importlib.util.spec_from_file_location("mlic_codec_cli", os.path.join(ROOT, "tools", "mlic_codec.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_ratemap_arguments(capsys):
    cli = _cli()
    base = ["ratemap", "a.ppm", "-o", "heat.ppm", "--model", "MLICPP_S", "--synthetic", "0"]
    a = cli.parse_args(base)
    assert (a.mode, a.src, a.output, a.what, a.cmap, a.alpha, a.hi, a.csv) == \
        ("ratemap", "a.ppm", "heat.ppm", ("bits", None), "hot", 256, None, None)
    a = cli.parse_args(base + ["--what", "slice", "3", "--cmap", "gray", "--alpha", "77", "--hi", "12.5", "--csv", "m.csv",
                               "--level", "2"])
    assert (a.what, a.cmap, a.alpha, a.hi, a.csv, a.level) == (("slice", 3), "gray", 77, 12.5, "m.csv", 2)
    assert cli.parse_args(base + ["--what", "z"]).what == ("z", None)
    assert cli.parse_args(base + ["--what", "error"]).what == ("error", None)
    a = cli.parse_args(base + ["--roi", "m.ppm", "--roi-levels", "0", "5"])
    assert a.roi == "m.ppm" and a.roi_levels == [0, 5]
    bad = [base + ["--what", "slice"], base + ["--what", "slice", "x"], base + ["--what", "bits", "3"],
           base + ["--what", "heat"], base + ["--alpha", "257"], base + ["--alpha", "-1"], base + ["--hi", "0"],
           base + ["--hi", "inf"], base + ["--cmap", "jet"], base + ["--max-bpp", "1"], base + ["--tile", "256"],
           base + ["--scale", "1/2"], base + ["--depth", "10"], base + ["--level", "auto"], base + ["--roi", "m.ppm"],
           base + ["--roi", "m.ppm", "--roi-levels", "0", "5", "--level", "1"],
           ["ratemap", "a.ppm", "--model", "MLICPP_S", "--synthetic", "0"],             # no -o
           ["ratemap", "a.ppm", "b.ppm", "-o", "h.ppm", "--synthetic", "0"],             # two files
           ["ratemap", "a.y4m", "-o", "h.ppm", "--synthetic", "0"],                      # a frame file
           ["ratemap", "a.ppm", "-o", "h.ppm"],                                          # no weights
           ["encode", "a.ppm", "a.bit", "--synthetic", "0", "--what", "z"],              # map flags elsewhere
           ["decode", "a.bit", "a.ppm", "--synthetic", "0", "-o", "h.ppm"],
           ["info", "a.bit", "--cmap", "hot"], ["encode", "a.ppm", "a.bit", "--synthetic", "0", "--alpha", "3"]]
    for argv in bad:
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
    capsys.readouterr()
    # the other modes parse as before
    a = cli.parse_args(["encode", "a.ppm", "a.bit", "--synthetic", "0"])
    assert (a.mode, a.dst, a.output, a.what) == ("encode", "a.bit", None, None)
    assert cli.parse_args(["info", "a.bit"]).mode == "info"
