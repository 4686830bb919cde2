"""Rate and error maps on the GPU (needs a MI355X: `-m gpu`): the rate_map, sq_err_blocks and heat kernels, the
model and codec paths over them, and code_image(rate_map=True).

Exact claims (bit-identical across batch size, batch position, repeats and strides; cell_bits / slice_bits against
their CPU restatement; integer and byte results against the CPU restatements) are asserted with torch.equal.
Against float64 the gate is the error of log2f on its fp32 argument: HIP documents log2f at 1 ulp, so a term t
carries at most 2^-23 |t| and a sum of terms 2^-23 sum |t|; the gate is 4 times that (room for the fast path; the
double additions add 2^-53 per step, nothing at this scale).  An indexing mistake moves a cell by whole terms, and at
least 90 % of the drawn terms exceed 0.01 bit.  The worst measured ratio |err| / (2^-23 sum |t|) goes to
RATEMAP_PARITY ($MLIC_PARITY_OUT).  The suite's NaN poison is on: an output element a kernel does not write fails
the finiteness and equality checks."""
import math
import os

import numpy as np
import pytest
import torch

from mlic_amd import _lib, bitstream, codec, get_model, synthetic

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
RATE = {"MLICPP_S": 1, "MLICPP_L_VBR": 2}  # the parity tests' realistic-rate sets
_NETS = {}
_LIKS = {}
RATEMAP_PARITY = {"worst_log2f_ratio": 0.0}
BOUND = 4 * 2.0 ** -23


@pytest.fixture(scope="module", autouse=True)
def _dump_parity():
    yield
    out = os.environ.get("MLIC_PARITY_OUT")
    if out:
        import json
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        old = {}
        if os.path.exists(out):
            with open(out) as f:
                old = json.load(f)
        old["RATEMAP_PARITY"] = RATEMAP_PARITY
        with open(out, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)


@pytest.fixture(autouse=True)
def _no_range_fallbacks(request):
    yield
    hit = {k: n.range_fallbacks(reset=True) for k, n in _NETS.items()}
    hit = {k: v for k, v in hit.items() if any(v.values())}
    assert not hit, (request.node.name, hit)


def net_for(name):
    if name not in _NETS:
        n = get_model(name)
        n.load_state_dict(synthetic.synth_state_dict(name, rate=RATE[name]))
        n = n.to(DEV).eval()
        n.update()
        _NETS[name] = n
    return _NETS[name]


def images(B, H, W, seed=70):
    return torch.cat([synthetic.synth_image(H, W, seed + i) for i in range(B)])


def liks(B, M, S, N, h, w):
    """Seeded likelihoods in [1e-9, 1] (CPU fp32), 10^(-9 r^2) for uniform r: every decade is there and about 98 % of
    the terms exceed 0.01 bit.  Exact 1.0 and exact 1e-9 are planted in both tensors, and slice 0 of y's first pixel
    is all 1.0.  With them, at least 90 % of the terms of the input still exceed 0.01 bit (checked here)."""
    key = (B, M, S, N, h, w)
    if key not in _LIKS:
        g = torch.Generator().manual_seed(1000 + M + 7 * h + w + 13 * B)
        out = []
        for shape in ((B, M, h, w), (B, N, h // 4, w // 4)):
            r = torch.rand(shape, dtype=torch.float64, generator=g)
            t = torch.pow(10.0, -9.0 * r ** 2).float().clamp_(1e-9, 1.0)
            t[B - 1, shape[1] - 2, shape[2] - 1, 0] = 1.0
            t[0, shape[1] - 1, shape[2] - 1, shape[3] - 1] = 1e-9
            out.append(t)
        y, z = out
        y[0, :M // S, 0, 0] = 1.0  # slice 0 of one pixel: every term +0
        for t in out:
            assert float(t.min()) == float(torch.tensor(1e-9, dtype=torch.float32)) and float(t.max()) == 1.0
        terms = torch.cat([-torch.log2(t.double()).flatten() for t in out])
        assert float((terms > 0.01).double().mean()) >= 0.9
        _LIKS[key] = (y, z)
    return _LIKS[key]


def oracle(y, z, S):
    """float64 on the CPU: (y_map, z_map, sum |t| per y cell, sum |t| per z cell)."""
    B, M, h, w = y.shape
    ty, tz = -torch.log2(y.double()), -torch.log2(z.double())
    return ty.reshape(B, S, M // S, h, w).sum(2), tz.sum(1), ty.abs().reshape(B, S, M // S, h, w).sum(2), tz.abs().sum(1)


def check_log2f_bound(got, want, mag, what):
    err = (got.cpu() - want).abs()
    unit = 2.0 ** -23 * mag
    ratio = float((err[unit > 0] / unit[unit > 0]).max()) if bool((unit > 0).any()) else 0.0
    RATEMAP_PARITY["worst_log2f_ratio"] = max(RATEMAP_PARITY["worst_log2f_ratio"], ratio)
    print(f"{what}: worst |err| / (2^-23 sum|t|) = {ratio:.4f}")
    assert bool((err <= BOUND * mag).all()), (what, ratio)


def assert_same(a, b):
    for k in ("y_map", "z_map", "cell_bits", "slice_bits"):
        assert torch.equal(a[k], b[k]), k


# --------------------------------------------------------------------------- 1. rate_map, model-free
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("h,w", [(4, 4), (8, 12), (12, 260)])
@pytest.mark.parametrize("M,S,N", [(320, 10, 192), (8, 2, 4)])
def test_rate_maps_kernel(M, S, N, h, w, B):
    y, z = liks(B, M, S, N, h, w)
    yd, zd = y.to(DEV), z.to(DEV)
    m = codec.rate_maps(yd, zd, S)
    assert {k: tuple(v.shape) for k, v in m.items()} == {"y_map": (B, S, h, w), "z_map": (B, h // 4, w // 4),
                                                         "cell_bits": (B, h, w), "slice_bits": (B, S + 1)}
    for k, v in m.items():
        assert v.dtype == torch.float64 and v.is_cuda
        assert bool(torch.isfinite(v).all()), k          # no poison left: every element written
        assert not bool(torch.signbit(v).any()), k       # no -0.0
    assert float(m["y_map"][0, 0, 0, 0]) == 0.0          # a cell whose terms are all lik == 1
    assert_same(m, codec.rate_maps(yd, zd, S))           # repeats
    for b in range(B if B > 1 else 0):                   # image b of a batch equals the image alone
        one = codec.rate_maps(yd[b:b + 1], zd[b:b + 1], S)
        for k in one:
            assert torch.equal(one[k][0], m[k][b]), (k, b)
    # a batch-strided view (every image dense, a gap between images) equals its dense copy
    ybuf = torch.full((B, M * h * w + 12), 0.5, device=DEV)
    zbuf = torch.full((B, N * (h // 4) * (w // 4) + 4), 0.5, device=DEV)
    yv, zv = ybuf[:, :M * h * w].view(B, M, h, w), zbuf[:, 4:].view(B, N, h // 4, w // 4)
    yv.copy_(yd)
    zv.copy_(zd)
    assert (B == 1 or yv.stride(0) == yd.stride(0) + 12) and yv.data_ptr() == ybuf.data_ptr()
    assert_same(m, codec.rate_maps(yv, zv, S))
    # cell_bits and slice_bits are their restatement from the returned maps, bit for bit
    assert torch.equal(m["cell_bits"].cpu(), codec._cell_bits_cpu(m["y_map"], m["z_map"]))
    assert torch.equal(m["slice_bits"].cpu(), codec._slice_bits_cpu(m["y_map"], m["z_map"]))
    # permuting the latent pixels permutes y_map; swapping two slices' channel groups swaps their maps
    perm = torch.randperm(h * w, generator=torch.Generator().manual_seed(9)).to(DEV)
    yp = yd.flatten(2)[:, :, perm].reshape(B, M, h, w).contiguous()
    assert torch.equal(codec.rate_maps(yp, zd, S)["y_map"], m["y_map"].flatten(2)[:, :, perm].reshape(B, S, h, w))
    cps = M // S
    order = list(range(cps, 2 * cps)) + list(range(cps)) + list(range(2 * cps, M))
    sw = codec.rate_maps(yd[:, order].contiguous(), zd, S)["y_map"]
    assert torch.equal(sw[:, 0], m["y_map"][:, 1]) and torch.equal(sw[:, 1], m["y_map"][:, 0])
    assert torch.equal(sw[:, 2:], m["y_map"][:, 2:])
    # against float64
    wy, wz, my, mz = oracle(y, z, S)
    check_log2f_bound(m["y_map"], wy, my, f"y_map {(M, S, h, w, B)}")
    check_log2f_bound(m["z_map"], wz, mz, f"z_map {(N, h // 4, w // 4, B)}")


def test_rate_maps_nan_stays_in_its_cell():
    M, S, N, h, w, B = 8, 2, 4, 8, 12, 2
    y, z = liks(B, M, S, N, h, w)
    y = y.clone()
    y[1, 5, 3, 7] = math.nan  # channel 5 is in slice 1
    m = codec.rate_maps(y.to(DEV), z.to(DEV), S)
    for k, at in (("y_map", (1, 1, 3, 7)), ("cell_bits", (1, 3, 7)), ("slice_bits", (1, 1))):
        nan = torch.isnan(m[k])
        assert int(nan.sum()) == 1 and bool(nan[at]), k
    assert bool(torch.isfinite(m["z_map"]).all())
    z = z.clone()
    z[0, 2, 1, 2] = math.nan  # a z pixel covers 4 x 4 latent pixels
    m = codec.rate_maps(liks(B, M, S, N, h, w)[0].to(DEV), z.to(DEV), S)
    assert int(torch.isnan(m["z_map"]).sum()) == 1 and bool(torch.isnan(m["z_map"][0, 1, 2]))
    nan = torch.isnan(m["cell_bits"])
    assert int(nan.sum()) == 16 and bool(nan[0, 4:8, 8:12].all())
    assert int(torch.isnan(m["slice_bits"]).sum()) == 1 and bool(torch.isnan(m["slice_bits"][0, S]))
    assert bool(torch.isfinite(m["y_map"]).all())


# --------------------------------------------------------------------------- 2. rate_map with a model
@pytest.mark.parametrize("name,H,W,kw", [("MLICPP_S", 64, 64, {}), ("MLICPP_L_VBR", 128, 192, {"s": 3})])
def test_net_rate_map(name, H, W, kw):
    net = net_for(name)
    x = images(2, H, W).to(DEV)
    f = net(x, **kw)
    m = net.rate_map(x, **kw)
    yl, zl = f["likelihoods"]["y_likelihoods"], f["likelihoods"]["z_likelihoods"]
    assert_same(m, codec.rate_maps(yl, zl, net.slice_num))
    assert torch.equal(m["x_hat"], f["x_hat"])
    assert tuple(m["cell_bits"].shape) == (2, H // 16, W // 16) and tuple(m["slice_bits"].shape) == (2, net.slice_num + 1)
    assert all(bool(torch.isfinite(m[k]).all()) for k in m)
    ty, tz = -torch.log2(yl.double()), -torch.log2(zl.double())
    want = ty.flatten(1).sum(1) + tz.flatten(1).sum(1)
    mag = ty.abs().flatten(1).sum(1) + tz.abs().flatten(1).sum(1)
    check_log2f_bound(m["slice_bits"].sum(1), want.cpu(), mag.cpu(), f"{name} total bits")


def test_codec_rate_map_cropped_and_roi():
    net = net_for("MLICPP_L_VBR")
    H, W = 120, 200  # cropped cells: the padded image is 128 x 256
    img = bitstream.to_u8(images(2, H, W, 90)).permute(0, 2, 3, 1).contiguous()
    out = codec.rate_map(net, img, level=2)
    assert len(out) == 2
    for r in out:
        assert tuple(r["cell_bits"].shape) == (8, 16) and tuple(r["z_map"].shape) == (2, 4)
        assert tuple(r["y_map"].shape) == (net.slice_num, 8, 16) and tuple(r["x_hat"].shape) == (3, 128, 256)
        sb = r["slice_bits"].cpu().tolist()
        bits = 0.0
        for v in sb:
            bits = bits + v
        assert r["bits"] == bits and r["bpp"] == bits / (120 * 200) and (r["H"], r["W"]) == (H, W)
        assert bool(torch.isfinite(r["cell_bits"]).all())
    alone = codec.rate_map(net, img[1], level=2)[0]
    assert torch.equal(alone["cell_bits"], out[1]["cell_bits"]) and alone["bits"] == out[1]["bits"]
    # a split mask: left half at level 0, right half at the top level
    mask = torch.zeros(2, H, W, dtype=torch.uint8)
    mask[:, :, W // 2:] = 1
    roi = codec.rate_map(net, img, roi=mask, roi_levels=(0, net.levels - 1))
    halves = []
    for r in roi:
        assert all(bool(torch.isfinite(r[k]).all()) for k in ("y_map", "z_map", "cell_bits", "slice_bits"))
        cb = r["cell_bits"][:, :-(-W // 16)]  # the cells that show in the image: 13 columns, the 7th straddles the split
        halves.append((float(cb[:, :6].sum()), float(cb[:, 7:].sum())))
    RATEMAP_PARITY["roi_split_bits_left_right"] = halves  # information: synthetic weights promise nothing here
    with pytest.raises(ValueError, match="roi= together with level="):
        codec.rate_map(net, img, level=1, roi=mask, roi_levels=(0, 5))
    with pytest.raises(ValueError, match="tile="):
        codec.rate_map(net, img, level=1, tile=256)


# ------------------------------------------------------------------------------- 3. sq_err_blocks
def u8_images(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
    b = (a.int() + torch.randint(-40, 41, a.shape, generator=g)).clamp_(0, 255).to(torch.uint8)
    return a, b


def as_layout(t, layout):
    """A [B,H,W,3] uint8 tensor on the device as `layout`: "hwc", "chw", or "rgba" -- the RGB of an RGBA buffer, read
    in place (column stride 4: the general-stride kernel); -> (tensor, layout name for the codec)."""
    t = t.to(DEV)
    if layout == "hwc":
        return t.contiguous(), "hwc"
    if layout == "chw":
        return t.permute(0, 3, 1, 2).contiguous(), "chw"
    buf = torch.full((*t.shape[:3], 4), 7, dtype=torch.uint8, device=DEV)
    buf[..., :3] = t
    return buf[..., :3], "hwc"


@pytest.mark.parametrize("layout", ["hwc", "chw", "rgba"])
@pytest.mark.parametrize("H,W", [(16, 16), (40, 72), (33, 257)])
@pytest.mark.parametrize("block", [8, 16, 64])
def test_sq_err_blocks(block, H, W, layout):
    a, b = u8_images(2, H, W, H + W + block)
    b[1] = a[1]  # identical images: all zeros
    want = codec._sq_err_blocks_cpu(a, b, block, "hwc")
    ad, lay = as_layout(a, layout)
    bd, _ = as_layout(b, layout)
    got = codec.sq_err_blocks(ad, bd, block, lay)
    assert got.dtype == torch.int64 and tuple(got.shape) == (2, -(-H // block), -(-W // block))
    assert torch.equal(got.cpu(), want)
    assert int(got[1].abs().sum()) == 0 and int(got[0].sum()) > 0
    ones = torch.ones(2, H, W, dtype=torch.uint8, device=DEV)
    assert torch.equal(got.flatten(1).sum(1), codec.sq_err_roi(ad, bd, ones, lay)[:, 0])
    # a decode with its exact squared error: the grid of (reference, decode) sums to egress_u8's sq_err
    dec, sq = codec.egress_u8(b.to(DEV).permute(0, 3, 1, 2).float().div(255).contiguous(), H, W, "hwc", ref=a.to(DEV))
    assert torch.equal(codec.sq_err_blocks(a.to(DEV), dec, block, "hwc").flatten(1).sum(1), sq)
    assert torch.equal(got, codec.sq_err_blocks(bd, ad, block, lay))


# ------------------------------------------------------------------------------------- 4. heat_u8
def heat_plane(B, ph, pw, lo, hi, seed):
    r = np.random.default_rng(seed)
    p = lo + (hi - lo) * r.uniform(-0.2, 1.2, (B, ph, pw))
    flat = p.reshape(-1)
    special = [math.nan, math.inf, -math.inf, lo, hi] + [lo + (hi - lo) * (k + 0.5) / 255.0
                                                         for k in (0, 1, 84, 85, 127, 169, 170, 254)]
    flat[r.permutation(flat.size)[:len(special)]] = special
    return torch.from_numpy(p)


@pytest.mark.parametrize("layout", ["hwc", "chw", "rgba"])
@pytest.mark.parametrize("cell,H,W", [(16, 40, 72), (64, 40, 72), (16, 64, 260), (64, 64, 260)])
@pytest.mark.parametrize("cmap", ["hot", "gray"])
def test_heat_u8(cmap, cell, H, W, layout):
    ph, pw = -(-H // cell), -(-W // cell)
    B = max(2, -(-26 // (ph * pw)))
    lo, hi = (0.0, 37.3) if cell == 16 else (-3.0, 252.0)
    p = heat_plane(B, ph, pw, lo, hi, cell + W)
    assert torch.isnan(p).any() and torch.isinf(p).any()
    under = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4))
    pd = p.to(DEV)
    want0 = codec._heat_u8_cpu(p, H, W, cell, lo, hi, codec.CMAPS.index(cmap), None, 256, "hwc")
    got = codec.heat_u8(pd, H, W, cell, lo, hi, cmap, layout="chw" if layout == "chw" else "hwc")
    assert got.is_cuda and got.dtype == torch.uint8
    assert torch.equal(got.cpu() if layout != "chw" else got.cpu().permute(0, 2, 3, 1), want0)
    # a strided (non-dense) under-image, in the output's layout class or not
    ud, lay = as_layout(under, layout)
    wide = torch.zeros(B, H, W + 5, 3, dtype=torch.uint8, device=DEV)  # hwc rows with a gap after them
    wide[:, :, 2:W + 2] = under.to(DEV)
    for alpha in (0, 77, 256):
        want = codec._heat_u8_cpu(p, H, W, cell, lo, hi, codec.CMAPS.index(cmap), under, alpha, "hwc")
        got = codec.heat_u8(pd, H, W, cell, lo, hi, cmap, under=ud, alpha=alpha, layout=lay)
        assert torch.equal(got.cpu() if lay == "hwc" else got.cpu().permute(0, 2, 3, 1), want), alpha
        if layout == "hwc":
            got = codec.heat_u8(pd, H, W, cell, lo, hi, cmap, under=wide[:, :, 2:W + 2], alpha=alpha)
            assert torch.equal(got.cpu(), want), alpha
        if layout == "chw":  # an under-image of the other layout class: read as bytes
            got = codec.heat_u8(pd, H, W, cell, lo, hi, cmap, under=under.to(DEV).permute(0, 3, 1, 2), alpha=alpha,
                                layout="chw")
            assert torch.equal(got.cpu().permute(0, 2, 3, 1), want), alpha


@pytest.mark.parametrize("layout", ["hwc", "chw", "rgba"])
def test_heat_u8_writes_every_byte_and_nothing_else(layout):
    """The library call on a poisoned window of a larger canvas: every byte of the image is written, none outside."""
    import ctypes as C
    B, H, W, cell = 2, 40, 72, 16
    p = torch.full((B, 3, 5), 0.25, dtype=torch.float64, device=DEV)  # q = 64: no byte of the picture is 0xEE
    if layout == "chw":
        canvas = torch.full((B, 3, H + 2, W + 3), 0xEE, dtype=torch.uint8, device=DEV)
        win, lay = canvas[:, :, 1:H + 1, 1:W + 1], "chw"
    else:
        canvas = torch.full((B, H + 2, W + 3, 4 if layout == "rgba" else 3), 0xEE, dtype=torch.uint8, device=DEV)
        win, lay = canvas[:, 1:H + 1, 1:W + 1, :3], "hwc"
    outside = torch.ones_like(canvas, dtype=torch.bool)
    (outside[:, :, 1:H + 1, 1:W + 1] if layout == "chw" else outside[:, 1:H + 1, 1:W + 1, :3]).fill_(False)
    under = torch.randint(0, 256, tuple(win.shape), dtype=torch.uint8, generator=torch.Generator().manual_seed(6)).to(DEV)
    for und, alpha in ((None, 256), (under, 77)):  # the second call: a dense under-image of the window's layout
        canvas.fill_(0xEE)
        _lib.call("mlic_image_heat_u8", C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(p.data_ptr()), B,
                  3, 5, cell, 0.0, 1.0, 1, H, W, C.c_void_p(win.data_ptr()), (C.c_int64 * 4)(*codec._strides(win, lay)),
                  None if und is None else C.c_void_p(und.data_ptr()),
                  None if und is None else (C.c_int64 * 4)(*codec._strides(und, lay)), alpha)
        want = codec._heat_u8_cpu(p.cpu(), H, W, cell, 0.0, 1.0, 1, None if und is None else und.cpu(), alpha, lay)
        assert torch.equal(win.cpu(), want)
        assert und is not None or not bool((want == 0xEE).any())
        assert bool((canvas[outside] == 0xEE).all())


# ----------------------------------------------------------------------- 5. code_image(rate_map=True)
def test_code_image_rate_map(monkeypatch):
    net = net_for("MLICPP_S")
    img = images(1, 64, 64, 75).to(DEV)
    files = []
    real = bitstream.write_stream

    def recording(buf, *a, **k):
        n = real(buf, *a, **k)
        files.append(buf.getvalue())
        return n
    monkeypatch.setattr(bitstream, "write_stream", recording)
    plain = bitstream.code_image(net, img)
    withmap = bitstream.code_image(net, img, rate_map=True)
    assert len(files) == 2 and files[0] == files[1] and len(files[0]) == plain["bytes"]
    assert set(withmap) - set(plain) == {"slice_bits", "z_bits"} and set(plain) <= set(withmap)
    assert "slice_bits" not in plain and "z_bits" not in plain
    assert plain["bytes"] == withmap["bytes"] and torch.equal(plain["x_hat"], withmap["x_hat"])
    assert len(withmap["slice_bits"]) == net.slice_num and all(isinstance(v, float) and v >= 0 for v in withmap["slice_bits"])
    m = net.rate_map(bitstream.pad64(img))
    assert withmap["slice_bits"] + [withmap["z_bits"]] == m["slice_bits"][0].cpu().tolist()


def test_code_image_rate_map_with_roi():
    net = net_for("MLICPP_L_VBR")
    img = images(1, 128, 192, 77).to(DEV)
    mask = torch.zeros(128, 192, dtype=torch.uint8)
    mask[:, 96:] = 1
    a = bitstream.code_image(net, img, roi=mask, roi_levels=(0, 5))
    b = bitstream.code_image(net, img, roi=mask, roi_levels=(0, 5), rate_map=True)
    assert a["bytes"] == b["bytes"] and torch.equal(a["x_hat"], b["x_hat"])
    assert set(b) - set(a) == {"slice_bits", "z_bits"}
    g = codec.gain_plane(net, codec.roi_levels(mask.to(DEV), 0, 5))
    assert b["slice_bits"] + [b["z_bits"]] == net.rate_map(bitstream.pad64(img), gain_map=g)["slice_bits"][0].cpu().tolist()


# ------------------------------------------------------------------------------------------ 6. CLI
def test_cli_ratemap(tmp_path, capsys):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("mlic_codec_ratemap_gpu_cli", os.path.join(root, "tools", "mlic_codec.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    H, W = 72, 120  # 5 x 8 cells of 16, the last of each cropped; 2 x 2 cells of 64
    img = bitstream.to_u8(images(1, H, W, 95))[0].permute(1, 2, 0).contiguous()
    src, csv = str(tmp_path / "a.ppm"), str(tmp_path / "m.csv")
    with open(src, "wb") as f:
        f.write(cli.write_ppm(img.numpy()))
    model = ["--model", "MLICPP_S", "--synthetic", "0"]
    net = get_model("MLICPP_S")
    net.load_state_dict(synthetic.synth_state_dict("MLICPP_S", 0))
    net = net.to(DEV).eval()
    net.update()
    _NETS["MLICPP_S cli"] = net
    r = codec.rate_map(net, img)[0]
    dev_img = img.to(DEV)

    def run(name, *flags):
        out = str(tmp_path / name)
        cli.main(["ratemap", src, "-o", out] + model + list(flags))
        with open(out, "rb") as f:
            return cli.read_ppm(f.read())

    got = run("bits.ppm", "--csv", csv)
    want = codec.heat_u8(r["cell_bits"][:5, :8].contiguous(), H, W, 16)
    assert np.array_equal(got, want[0].cpu().numpy())
    assert f"{r['bpp']:.4f} bpp" in capsys.readouterr().out
    with open(csv) as f:
        lines = f.read().splitlines()
    sb = r["slice_bits"].cpu().tolist()
    assert lines[0] == "slice_bits," + ",".join(repr(v) for v in sb[:-1]) and lines[1] == "z_bits," + repr(sb[-1])
    assert lines[2] == "plane,bits,cell,16" and len(lines) == 3 + 5
    assert [float(v) for v in lines[3].split(",")] == r["cell_bits"][0, :8].cpu().tolist()
    got = run("s1.ppm", "--what", "slice", "1", "--cmap", "gray", "--alpha", "128", "--hi", "50")
    want = codec.heat_u8(r["y_map"][1, :5, :8].contiguous(), H, W, 16, 0.0, 50.0, "gray", under=dev_img, alpha=128)
    assert np.array_equal(got, want[0].cpu().numpy())
    got = run("z.ppm", "--what", "z")
    assert np.array_equal(got, codec.heat_u8(r["z_map"].contiguous(), H, W, 64)[0].cpu().numpy())
    got = run("err.ppm", "--what", "error")
    dec = codec.egress_u8(r["x_hat"].unsqueeze(0), H, W, "hwc")
    err = codec.sq_err_blocks(dev_img, dec, 16)[0].double()
    assert tuple(err.shape) == (5, 8) and np.array_equal(got, codec.heat_u8(err, H, W, 16)[0].cpu().numpy())
    with pytest.raises(SystemExit, match="slices"):
        run("bad.ppm", "--what", "slice", "99")
