"""Rate-constrained encoding without a GPU: the prefilter's weights, the torch restatement of blur3_pad against
its definition, the argument refusals of mlic_image_blur3_pad, the policy of codec.rate_loop / encode_images
with a stub model whose file sizes are a known function of its input, and the command line's new flags.

The stub's "y string" has a length proportional to the image's mean absolute horizontal difference (which the
filter lowers) and, for a VBR stub, to a per-level factor that is NOT monotone in the level.  What each image
must get is computed here by the definition, one image at a time: the file of the first pass count that fits."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mlic_amd import _lib, bitstream, codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------ weights
def test_weights_are_the_fp32_gaussian_bit_for_bit():
    k, sigma = 3, 0.5
    i = torch.arange(k).float() - (k - 1) / 2.
    d2 = i.view(-1, 1) ** 2. + i.view(1, -1) ** 2.
    g = (1. / (2. * math.pi * sigma ** 2.)) * torch.exp(-d2 / (2 * sigma ** 2.))
    g = (g / torch.sum(g)).flatten()
    assert g.dtype == torch.float32
    w = torch.tensor(codec.BLUR3_WEIGHTS, dtype=torch.float32)
    assert len(codec.BLUR3_WEIGHTS) == 9 and torch.equal(_bits(w), _bits(g))
    assert [float(v) for v in w.double()] == list(codec.BLUR3_WEIGHTS)  # the tuple holds fp32 values exactly
    corner, edge, centre = (float.fromhex(h) for h in ("0x1.73b62cp-7", "0x1.575320p-4", "0x1.3d1b0ep-1"))
    assert list(codec.BLUR3_WEIGHTS) == [corner, edge, corner, edge, centre, edge, corner, edge, corner]


# ------------------------------------------------------------------------- blur3_pad, the CPU form
def _float_images(B, H, W, seed=0):
    """fp32 [B,3,Hp,Wp] as ingest_u8 makes it (u8 / 255, zeros in the padding) and the uint8 source."""
    r = np.random.default_rng(100 * H + W + seed)
    u8 = torch.from_numpy(r.integers(0, 256, (B, H, W, 3), dtype=np.uint8))
    return codec.ingest_u8(u8, "hwc"), u8


def _definition(x, H, W, w9):
    """F.conv2d of the crop in float64 with padding 1, zero-padded back to the buffer's size."""
    w = torch.tensor(w9, dtype=torch.float32).double().view(1, 1, 3, 3).repeat(3, 1, 1, 1)
    y = F.conv2d(x[:, :, :H, :W].double(), w, padding=1, groups=3)
    return F.pad(y, (0, x.size(3) - W, 0, x.size(2) - H))


@pytest.mark.parametrize("shape", [(1, 1), (64, 64), (65, 70), (3, 130)])
def test_cpu_blur_matches_the_definition(shape):
    H, W = shape
    x, _ = _float_images(3, H, W)
    x_before = x.clone()
    got = codec.blur3_pad(x, H, W)
    assert torch.equal(x, x_before) and got.dtype == torch.float32 and got.shape == x.shape
    err = float((got.double() - _definition(x, H, W, codec.BLUR3_WEIGHTS)).abs().max())
    print(f"blur3_pad CPU vs float64 conv2d, {H} x {W}: max abs err {err:.3e}")
    # 9 products and 8 effective sums, each rounded once, on partial sums <= 1
    assert err <= 18 * 2.0 ** -24
    # exact +0.0 in the padding
    assert int(_bits(got[:, :, H:]).abs().sum()) == 0 and int(_bits(got[:, :, :, W:]).abs().sum()) == 0
    # garbage in the source's padding does not reach the image: v = 0 outside H x W, not outside the buffer
    dirty = x.clone()
    dirty[:, :, H:] = 7.0
    dirty[:, :, :, W:] = float("nan")
    assert torch.equal(_bits(codec.blur3_pad(dirty, H, W)), _bits(got))
    # gather, duplicate and compact
    sel = codec.blur3_pad(x, H, W, index=[2, 0, 2])
    assert torch.equal(_bits(sel), _bits(got[[2, 0, 2]]))
    assert torch.equal(_bits(codec.blur3_pad(x, H, W, index=torch.tensor([1]))), _bits(got[1:2]))
    # a non-symmetric filter: a transposed or reversed tap order would show
    w = [0.05, 0.1, 0.15, 0.2, -0.25, 0.3, 0.35, 0.4, 0.45]
    got_w = codec.blur3_pad(x, H, W, weights=w)
    w32 = [float(np.float32(v)) for v in w]
    assert float((got_w.double() - _definition(x, H, W, w32)).abs().max()) <= 18 * 2.0 ** -24 * sum(abs(v) for v in w)
    assert torch.equal(_bits(codec.blur3_pad(x, H, W, weights=torch.tensor(w))), _bits(got_w))


def test_cpu_blur_is_the_stated_loop():
    """acc = 0; acc = acc + w[t] * v[t], t row-major, in fp32 -- spelled out once more per element with numpy."""
    H, W = 5, 6
    x, _ = _float_images(1, H, W, seed=1)
    w = np.array([0.05, 0.1, 0.15, 0.2, -0.25, 0.3, 0.35, 0.4, 0.45], dtype=np.float32)
    got = codec.blur3_pad(x, H, W, weights=w).numpy()
    src = x.numpy()
    for c in range(3):
        for y in range(H):
            for xx in range(W):
                acc = np.float32(0)
                for t in range(9):
                    yy, xc = y + t // 3 - 1, xx + t % 3 - 1
                    v = src[0, c, yy, xc] if 0 <= yy < H and 0 <= xc < W else np.float32(0)
                    acc = np.float32(acc + np.float32(w[t] * v))
                assert got[0, c, y, xx].tobytes() == acc.tobytes(), (c, y, xx)


def test_blur_refuses_bad_arguments():
    x = torch.zeros(2, 3, 64, 128)
    for bad in (dict(H=65, W=10), dict(H=0, W=10), dict(H=10, W=129), dict(H=10, W=10, index=[2]),
                dict(H=10, W=10, index=[-1]), dict(H=10, W=10, index=[]), dict(H=10, W=10, weights=[1.0] * 8)):
        with pytest.raises(ValueError):
            codec.blur3_pad(x, **bad)
    with pytest.raises(ValueError):
        codec.blur3_pad(torch.zeros(1, 3, 60, 64), 10, 10)          # not a multiple of 64
    with pytest.raises(ValueError):
        codec.blur3_pad(torch.zeros(1, 3, 64, 64).double(), 10, 10)
    with pytest.raises(ValueError):
        codec.blur3_pad(torch.zeros(1, 1, 64, 64), 10, 10)


def _blur_rc(src=0x10000, dst=0x4000000, n=2, H=60, W=100, Hp=64, Wp=128):
    lib = _lib.lib()
    rc = lib.mlic_image_blur3_pad(None, C.c_void_p(src), None, n, H, W, Hp, Wp, None, C.c_void_p(dst))
    return rc, lib.mlic_last_error().decode() if rc else ""


PLANES = 2 * 3 * 64 * 128 * 4  # bytes of the n images of the default call


@pytest.mark.parametrize("kw, word", [
    (dict(n=0), "n must be positive"), (dict(H=0), "H and W must be positive"), (dict(W=-1), "H and W must be positive"),
    (dict(Hp=96), "multiples of 64"), (dict(Wp=64), "multiples of 64"), (dict(H=65), "multiples of 64"),
    (dict(src=0), "null"), (dict(dst=0), "null"),
    (dict(dst=0x10000), "overlaps"), (dict(dst=0x10000 + PLANES - 4), "overlaps"),
    (dict(src=0x4000000 + PLANES - 4), "overlaps"), (dict(src=0x4000000 + 16), "overlaps"),
])
def test_blur_entry_point_refuses_without_a_device(kw, word):
    """Each refusal has its own message and comes before any GPU call (this runs without a device; the pointers
    are never dereferenced).  Ranges that only touch are not an overlap: that call would go on to the launch, so
    it is made in the GPU test."""
    rc, msg = _blur_rc(**kw)
    assert rc != 0 and "image_blur3_pad" in msg and word in msg, msg


# ------------------------------------------------------------------------------------------- policy
H0, W0 = 40, 50
HEADER = 8 + 12 + 4 + 4  # bytes of a fixed-rate file around its strings
LEVEL_FACTOR = [0.2, 1.6, 0.5, 2.0, 1.2]  # not monotone in the level


class StubNet:
    """compress() as the models have it, with a y string of int(scale * activity * factor[level]) bytes whose
    fill byte also depends on the image, and an empty z string.  calls records (batch size, levels)."""
    device = torch.device("cpu")

    def __init__(self, vbr=False, scale=4000.0):
        if vbr:
            self.levels = len(LEVEL_FACTOR)
        self.scale = scale
        self.calls = []

    def compress(self, x, s=None):
        B, _, Hp, Wp = x.shape
        assert Hp % 64 == 0 and Wp % 64 == 0 and x.is_contiguous()
        assert (s is None) == (not hasattr(self, "levels")) and (s is None or len(s) == B)
        self.calls.append((B, None if s is None else list(s)))
        ys = []
        for b in range(B):
            act = float((x[b, :, :, 1:] - x[b, :, :, :-1]).abs().mean())
            n = int(self.scale * act * (1.0 if s is None else LEVEL_FACTOR[s[b]]))
            ys.append(bytes([int(float(x[b].double().sum()) * 1000) % 251]) * n)
        return {"strings": [ys, [b""] * B], "shape": (Hp // 64, Wp // 64)}


def _stub_images():
    """uint8 [3, H0, W0, 3]: flat, mildly noisy, very noisy."""
    r = np.random.default_rng(5)
    a = np.full((3, H0, W0, 3), 128, dtype=np.int64)
    a[1] += r.integers(-12, 13, (H0, W0, 3))
    a[2] += r.integers(-120, 121, (H0, W0, 3))
    return torch.from_numpy(a.clip(0, 255).astype(np.uint8))


def _bpp(f):
    return 8.0 * len(f) / (H0 * W0)


def _alone(img, max_bpp, max_passes, vbr=False, level=None):
    """The definition, for one image: (file, passes, level)."""
    net = StubNet(vbr)
    x = codec.ingest_u8(img, "hwc")

    def code(xx, lv):
        out = net.compress(xx, **({} if lv is None else {"s": [lv]}))
        return codec.write_container(H0, W0, out["shape"], out["strings"][0][0], b"", lv)

    lv = level
    if level == "auto":
        for lv in range(net.levels - 1, -1, -1):
            f = code(x, lv)
            if _bpp(f) <= max_bpp:
                return f, 0, lv
        lv = 0
    f, k = code(x, lv), 0
    while _bpp(f) > max_bpp and k < max_passes:
        x = codec.blur3_pad(x, H0, W0)
        f, k = code(x, lv), k + 1
    return f, k, lv


def test_loop_pass_counts_shrinking_batch_and_order(monkeypatch):
    imgs = _stub_images()
    plain = codec.encode_images(StubNet(), imgs)
    sizes = [_bpp(f) for f in plain]
    assert sizes[0] < sizes[1] < sizes[2]
    budget = sizes[1] * 0.8  # image 0 fits, image 1 needs some passes, image 2 cannot make it in 4
    want = [_alone(imgs[b], budget, 4) for b in range(3)]
    assert want[0][1] == 0 and 1 <= want[1][1] < 4 and want[2][1] == 4, [w[1] for w in want]
    net = StubNet()
    blurs = []
    real = codec.blur3_pad
    monkeypatch.setattr(codec, "blur3_pad", lambda x, H, W, index=None, weights=None:
                        (blurs.append((x.size(0), index)), real(x, H, W, index, weights))[1])
    files, info = codec.encode_images(net, imgs, max_bpp=budget, max_passes=4, return_info=True)
    assert files == [w[0] for w in want]
    assert [i["passes"] for i in info] == [w[1] for w in want]
    assert [i["met"] for i in info] == [True, True, False]
    for f, i in zip(files, info):
        assert i["bytes"] == len(f) and i["bpp"] == _bpp(f) and i["level"] is None and i["met"] == (_bpp(f) <= budget)
    # the batch shrinks: 3 images, then the two over budget, then image 2 alone once image 1 fits
    k1 = want[1][1]
    assert [c[0] for c in net.calls] == [3] + [2] * k1 + [1] * (4 - k1)
    # one launch per pass filters and compacts: first images [1, 2] of three, then (once) image 2 of those two
    assert blurs[0] == (3, [1, 2])
    assert blurs[1:] == [(2, None)] * (k1 - 1) + [(2, [1])] + [(1, None)] * (4 - k1 - 1)
    # input order is restored whatever the order of leaving: the same images reversed
    rfiles, rinfo = codec.encode_images(StubNet(), imgs.flip(0), max_bpp=budget, max_passes=4, return_info=True)
    assert rfiles == files[::-1] and [i["passes"] for i in rinfo] == [w[1] for w in want][::-1]
    # without return_info: the files alone
    assert codec.encode_images(StubNet(), imgs, max_bpp=budget, max_passes=4) == files


def test_no_budget_is_the_plain_call_and_never_filters(monkeypatch):
    imgs = _stub_images()

    def boom(*a, **k):
        raise AssertionError("blur3_pad called without a budget")
    monkeypatch.setattr(codec, "blur3_pad", boom)
    net = StubNet()
    files = codec.encode_images(net, imgs)
    assert net.calls == [(3, None)] and isinstance(files, list)
    x = codec.ingest_u8(imgs, "hwc")
    out = StubNet().compress(x)
    assert files == [codec.write_container(H0, W0, out["shape"], out["strings"][0][b], b"") for b in range(3)]
    f2, info = codec.encode_images(StubNet(), imgs, return_info=True)
    assert f2 == files and [i["passes"] for i in info] == [0, 0, 0] and all(i["met"] for i in info)
    # a budget everything meets, and max_passes = 0: no filter either
    assert codec.encode_images(StubNet(), imgs, max_bpp=1e9) == files
    f3, info = codec.encode_images(StubNet(), imgs, max_bpp=1e-9, max_passes=0, return_info=True)
    assert f3 == files and [i["met"] for i in info] == [False] * 3 and [i["passes"] for i in info] == [0] * 3


def test_fixed_level_runs_the_loop_at_that_level():
    imgs = _stub_images()
    plain = codec.encode_images(StubNet(vbr=True), imgs, level=[1, 3, 2])
    budget = _bpp(plain[1]) * 0.9
    net = StubNet(vbr=True)
    files, info = codec.encode_images(net, imgs, level=[1, 3, 2], max_bpp=budget, max_passes=3, return_info=True)
    want = [_alone(imgs[b], budget, 3, vbr=True, level=lv) for b, lv in enumerate([1, 3, 2])]
    assert files == [w[0] for w in want] and [i["passes"] for i in info] == [w[1] for w in want]
    assert [i["level"] for i in info] == [1, 3, 2] and info[1]["passes"] >= 1
    assert all(codec.peek(f, vbr=True)["level"] == lv for f, lv in zip(files, [1, 3, 2]))
    assert net.calls[0] == (3, [1, 3, 2]) and all(set(c[1]) <= {3, 2} for c in net.calls[1:])


def test_auto_picks_the_highest_fitting_level_without_monotonicity():
    imgs = _stub_images()
    top = len(LEVEL_FACTOR) - 1
    by_level = [codec.encode_images(StubNet(vbr=True), imgs[1], level=l)[0] for l in range(top + 1)]
    bpps = [_bpp(f) for f in by_level]
    # image 1: levels 4 and 3 are over the budget, 2 fits (and so does 0, while 1 does not)
    budget = bpps[2]
    assert bpps[4] > budget and bpps[3] > budget and bpps[1] > budget and bpps[0] < budget
    net = StubNet(vbr=True)
    files, info = codec.encode_images(net, imgs, level="auto", max_bpp=budget, max_passes=2, return_info=True)
    want = [_alone(imgs[b], budget, 2, vbr=True, level="auto") for b in range(3)]
    assert files == [w[0] for w in want]
    assert [i["passes"] for i in info] == [w[1] for w in want] and [i["level"] for i in info] == [w[2] for w in want]
    # the flat image fits at the top, image 1 at level 2, image 2 not even at level 0: it is filtered at level 0
    assert [i["level"] for i in info] == [top, 2, 0] and [i["passes"] for i in info] == [0, 0, 2]
    assert files[1] == by_level[2] and info[2]["met"] is False
    assert [codec.peek(f, vbr=True)["level"] for f in files] == [top, 2, 0]
    # images that fit leave the batch: each step of the scan codes only those still over
    assert net.calls == [(3, [4] * 3), (2, [3] * 2), (2, [2] * 2), (1, [1]), (1, [0]), (1, [0]), (1, [0])]


def test_budget_argument_refusals():
    imgs = _stub_images()
    for bad in (0, -1.0, float("nan"), float("inf"), "0.1", True):
        with pytest.raises(ValueError, match="max_bpp"):
            codec.encode_images(StubNet(), imgs, max_bpp=bad)
    for bad in (-1, 1.5, None):
        with pytest.raises(ValueError, match="max_passes"):
            codec.encode_images(StubNet(), imgs, max_bpp=1.0, max_passes=bad)
    with pytest.raises(ValueError, match="max_passes"):
        codec.encode_images(StubNet(), imgs, max_passes=-1)
    with pytest.raises(ValueError, match="needs max_bpp"):
        codec.encode_images(StubNet(vbr=True), imgs, level="auto")
    with pytest.raises(ValueError, match="fixed-rate"):
        codec.encode_images(StubNet(), imgs, level="auto", max_bpp=1.0)
    with pytest.raises(ValueError, match="auto"):
        codec.encode_images(StubNet(vbr=True), imgs, level="best", max_bpp=1.0)
    with pytest.raises(ValueError):
        codec.encode_images(StubNet(vbr=True), imgs, max_bpp=1.0)  # a VBR file needs its level
    with pytest.raises(ValueError):
        codec.encode_images(StubNet(vbr=True), imgs, level=len(LEVEL_FACTOR), max_bpp=1.0)


class StubCodecNet(StubNet):
    """StubNet with a decompress, for bitstream.code_image."""

    def decompress(self, strings, shape, **kw):
        return {"x_hat": torch.full((1, 3, 64 * shape[0], 64 * shape[1]), 0.5)}


def test_code_image_budget_fields():
    imgs = _stub_images()
    x = imgs[1:2].permute(0, 3, 1, 2).contiguous().float().div(255)
    plain = bitstream.code_image(StubCodecNet(), x)
    assert set(plain) == {"H", "W", "bytes", "bpp", "psnr", "enc_s", "dec_s", "x_hat"}
    budget = plain["bpp"] * 0.8
    r = bitstream.code_image(StubCodecNet(), x, max_bpp=budget, max_passes=4)
    assert set(r) == set(plain) | {"passes", "met"}
    f, k, _ = _alone(imgs[1], budget, 4)
    assert (r["bytes"], r["passes"], r["met"]) == (len(f), k, True) and k >= 1
    r = bitstream.code_image(StubCodecNet(), x, max_bpp=1e-9, max_passes=1)
    assert (r["passes"], r["met"]) == (1, False)
    r = bitstream.code_image(StubCodecNet(vbr=True), x, max_bpp=1e9, s=3)
    assert (r["passes"], r["met"]) == (0, True)


# ---------------------------------------------------------------------------------------------- CLI
def _cli():
    spec = importlib.util.spec_from_file_location("mlic_codec_cli", os.path.join(ROOT, "tools", "mlic_codec.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_budget_flags(capsys):
    cli = _cli()
    base = ["encode", "a.ppm", "a.bit", "--synthetic", "0"]
    a = cli.parse_args(base)
    assert (a.level, a.max_bpp, a.max_passes) == (None, None, 8)
    a = cli.parse_args(base + ["--level", "3"])
    assert a.level == 3 and isinstance(a.level, int)
    a = cli.parse_args(base + ["--max-bpp", "0.1", "--level", "auto", "--max-passes", "2"])
    assert (a.level, a.max_bpp, a.max_passes) == ("auto", 0.1, 2)
    a = cli.parse_args(base + ["--max-bpp", "0.25"])
    assert (a.level, a.max_bpp, a.max_passes) == (None, 0.25, 8)
    for bad in (["--level", "auto"], ["--level", "best", "--max-bpp", "0.1"], ["--level", "-1"], ["--max-bpp", "0"],
                ["--max-bpp", "nan"], ["--max-bpp", "inf"], ["--max-bpp", "x"], ["--max-bpp", "0.1", "--max-passes", "-1"]):
        with pytest.raises(SystemExit):
            cli.parse_args(base + bad)
    with pytest.raises(SystemExit):
        cli.parse_args(["decode", "a.bit", "a.ppm", "--synthetic", "0", "--max-bpp", "0.1"])
    capsys.readouterr()
