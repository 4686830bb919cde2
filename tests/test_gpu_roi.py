"""ROI coding on the GPU (needs a MI355X: `-m gpu`): gain planes in the slice loop, the mask kernels, the codec
path and the refusals.

The bit-exact claims (a constant plane is the scalar call; decompress_g(compress_g(x)) is forward_g(x); lanes and
batching change nothing; the kernels against their integer definitions) are asserted with torch.equal / byte
equality.  Against the float oracle (tests/roi_oracle.py, the reference's VBR slice loop with the same plane) the
gates are the project's own: |dbpp| <= 1e-3, |dPSNR| <= 0.01 dB, assert_xhat_close's mean <= 5e-4 and max <= 0.25
(test_gpu_parity.test_forward_matches_oracle_batched), and coder symbols / indexes with at most a 1e-3 fraction
of mismatches (test_compress_streams_match_reference); the exact counts go to ROI_PARITY ($MLIC_PARITY_OUT).
Weights are the realistic-rate synthetic sets of the parity tests; the suite's NaN poison is on and the range
fallback counters must stay 0.  Shapes: 128 x 192 is 2 x 3 cells on an 8 x 12 latent grid (odd and even rows of
both checkerboard phases); 120 x 200 has cropped cells."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mlic_ref_cpu as ref
import roi_oracle
from mlic_amd import _lib, codec, get_model, synthetic

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
RATE = {"MLICPP_L_VBR": 2, "MLICPP_M_SMALL_DEC_VBR": 1}  # the parity tests' realistic-rate sets
_NETS = {}
ROI_PARITY = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_parity():
    yield
    out = os.environ.get("MLIC_PARITY_OUT")
    if out and ROI_PARITY:
        import json
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        old = {}
        if os.path.exists(out):
            with open(out) as f:
                old = json.load(f)
        old.update(ROI_PARITY)
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


def level_maps(kind, B, hz, wz, lo, hi):
    """uint8 [B,hz,wz]: "split" = left half lo, right half hi; "cell" = one high cell; "mixed" = image 0 split,
    the others one high cell each at different places."""
    m = torch.full((B, hz, wz), lo, dtype=torch.uint8)
    for b in range(B):
        k = kind if kind != "mixed" else ("split" if b == 0 else "cell")
        if k == "split":
            m[b, :, wz // 2:] = hi
        else:
            m[b, (hz - 1 + b) % hz, (1 + b) % wz] = hi
    return m


def const_plane(B, H, W, v):
    return torch.full((B, 1, H // 16, W // 16), float(v), device=DEV)


# ------------------------------------------------------------------------------ 1. constant plane
@pytest.mark.parametrize("name,H,W,level", [("MLICPP_L_VBR", 128, 192, 0), ("MLICPP_L_VBR", 128, 192, 5),
                                            ("MLICPP_M_SMALL_DEC_VBR", 128, 128, 4)])
def test_constant_plane_equals_scalar(name, H, W, level):
    """A plane that holds one gain everywhere is the per-image path: the library's reciprocal plane is the
    host's fp32 1 / gain bit for bit, so every tensor and every byte agrees."""
    net = net_for(name)
    x = images(1, H, W).to(DEV)
    gain = float(net.Gain[level])
    assert gain > 0  # forward takes Gain[s] as stored, the coder paths |Gain[s]|: the same number here
    g = const_plane(1, H, W, gain)
    a, b = net(x, gain_map=g), net(x, s=level)
    assert torch.equal(a["x_hat"], b["x_hat"])
    assert torch.equal(a["likelihoods"]["y_likelihoods"], b["likelihoods"]["y_likelihoods"])
    assert torch.equal(a["likelihoods"]["z_likelihoods"], b["likelihoods"]["z_likelihoods"])
    assert bool(torch.isfinite(a["x_hat"]).all())
    ca, cb = net.compress(x, gain_map=g[:, 0]), net.compress(x, s=level)  # [B,hy,wy] is accepted too
    assert ca["strings"] == cb["strings"] and tuple(ca["shape"]) == tuple(cb["shape"])
    d = net.decompress(ca["strings"], ca["shape"], gain_map=g)
    assert torch.equal(d["x_hat"], net.decompress(cb["strings"], cb["shape"], s=level)["x_hat"])
    assert torch.equal(d["x_hat"], a["x_hat"])


# ---------------------------------------------------------------------------------- 2. round trip
@pytest.mark.parametrize("name,B,H,W,kind", [("MLICPP_L_VBR", 1, 128, 192, "split"), ("MLICPP_L_VBR", 1, 128, 192, "cell"),
                                             ("MLICPP_L_VBR", 2, 128, 192, "mixed"),
                                             ("MLICPP_M_SMALL_DEC_VBR", 1, 128, 128, "split")])
def test_roundtrip_lanes_and_batching(name, B, H, W, kind):
    net = net_for(name)
    x = images(B, H, W, 80).to(DEV)
    lv = level_maps(kind, B, H // 64, W // 64, 0, net.levels - 1)
    g = codec.gain_plane(net, lv)
    assert g.shape == (B, 1, H // 16, W // 16) and len(g.unique()) == 2
    f = net(x, gain_map=g)
    outs = []
    try:
        for lanes in (1, 4):
            net.set_lanes(lanes)
            c = net.compress(x, gain_map=g)
            d = net.decompress(c["strings"], c["shape"], gain_map=g)
            assert torch.equal(d["x_hat"], f["x_hat"]), (lanes, float((d["x_hat"] - f["x_hat"]).abs().max()))
            outs.append(c["strings"])
    finally:
        net.set_lanes(2)
    assert outs[0] == outs[1]
    if B > 1:  # a batch equals per-image calls, bit for bit
        assert len(set(outs[0][0])) == B
        for i in range(B):
            fi = net(x[i:i + 1], gain_map=g[i:i + 1])
            assert torch.equal(fi["x_hat"], f["x_hat"][i:i + 1])
            assert torch.equal(fi["likelihoods"]["y_likelihoods"], f["likelihoods"]["y_likelihoods"][i:i + 1])
            ci = net.compress(x[i:i + 1], gain_map=g[i:i + 1])
            assert ci["strings"][0][0] == outs[0][0][i] and ci["strings"][1][0] == outs[0][1][i]
            di = net.decompress(ci["strings"], ci["shape"], gain_map=g[i:i + 1])
            assert torch.equal(di["x_hat"], f["x_hat"][i:i + 1])


# ------------------------------------------------------------------------------------- 3. oracle
def assert_xhat_close(a, b):
    d = (a.float() - b.float()).abs()
    assert float(d.mean()) <= 5e-4, float(d.mean())
    assert float(d.max()) <= 0.25, float(d.max())


@pytest.mark.parametrize("name,B,H,W", [("MLICPP_L_VBR", 2, 128, 192), ("MLICPP_M_SMALL_DEC_VBR", 1, 128, 128)])
def test_matches_float_oracle_with_the_same_plane(name, B, H, W):
    net = net_for(name)
    sd = synthetic.synth_state_dict(name, rate=RATE[name])
    xs = images(B, H, W, 90)
    lv = level_maps("mixed", B, H // 64, W // 64, 0, net.levels - 1)
    g = codec.gain_plane(net, lv)
    g_cpu = roi_oracle.expand_levels(lv, sd["Gain"].abs())
    assert torch.equal(g.cpu(), g_cpu)  # the kernel's plane is the oracle's
    rec = {}
    o = roi_oracle.RefMLICRoi(name, sd).forward_g(xs, g_cpu, record=lambda ph, s, i: rec.__setitem__(ph, (s, i)))
    out = net(xs.to(DEV), gain_map=g)
    net.compress(xs.to(DEV), gain_map=g)
    torch.cuda.synchronize()
    for i in range(B):
        bg = ref.bpp_from_likelihoods(out["likelihoods"]["y_likelihoods"][i:i + 1].cpu(),
                                      out["likelihoods"]["z_likelihoods"][i:i + 1].cpu(), H * W)
        bc = ref.bpp_from_likelihoods(o["likelihoods"]["y_likelihoods"][i:i + 1],
                                      o["likelihoods"]["z_likelihoods"][i:i + 1], H * W)
        pg = ref.psnr_uint8(xs[i:i + 1], out["x_hat"][i:i + 1].cpu())
        pc = ref.psnr_uint8(xs[i:i + 1], o["x_hat"][i:i + 1])
        ys, yi, _ = net.encoded_streams(i)
        os_ = np.concatenate([rec[ph][0][i].reshape(-1).numpy() for ph in sorted(rec)])
        oi = np.concatenate([rec[ph][1][i].reshape(-1).numpy() for ph in sorted(rec)])
        assert ys.shape == os_.shape
        r = {"bpp_gpu": bg, "bpp_oracle": bc, "psnr_gpu": pg, "psnr_oracle": pc, "y_n": int(ys.size),
             "y_symbol_mismatch": int((ys != os_).sum()), "y_index_mismatch": int((yi != oi).sum())}
        ROI_PARITY[f"roi_oracle_{name}_{H}x{W}_img{i}"] = r
        print(r)
        assert abs(bg - bc) <= 1e-3, r
        assert abs(pg - pc) <= 0.01, r
        assert r["y_symbol_mismatch"] <= r["y_n"] * 1e-3, r
        assert r["y_index_mismatch"] <= r["y_n"] * 1e-3, r
    assert_xhat_close(out["x_hat"].cpu(), o["x_hat"])


# ------------------------------------------------------------------------------------- 4. effect
def test_mapped_rate_lies_between_the_constant_levels():
    name, H, W = "MLICPP_L_VBR", 128, 192
    net = net_for(name)
    x = images(1, H, W, 95).to(DEV)
    lv = level_maps("split", 1, 2, 3, 0, 5)
    n_map = len(net.compress(x, gain_map=codec.gain_plane(net, lv))["strings"][0][0])
    n_lo = len(net.compress(x, s=0)["strings"][0][0])
    n_hi = len(net.compress(x, s=5)["strings"][0][0])
    print({"y_bytes_level0": n_lo, "y_bytes_mapped": n_map, "y_bytes_level5": n_hi})
    assert n_lo < n_map < n_hi, (n_lo, n_map, n_hi)


# ----------------------------------------------------------------------------- 5. roi_levels kernel
def _np_levels(mask, lo, hi):
    B, H, W = mask.shape
    hz, wz = -(-H // 64), -(-W // 64)
    out = np.zeros((B, hz, wz), np.uint8)
    for b in range(B):
        for i in range(hz):
            for j in range(wz):
                cell = mask[b, 64 * i:64 * i + 64, 64 * j:64 * j + 64]
                out[b, i, j] = lo + -(-(hi - lo) * int(np.count_nonzero(cell)) // cell.size)
    return out


def _random_mask(B, H, W, seed):
    r = np.random.default_rng(seed)
    m = (r.random((B, H, W)) < r.random((B, 1, 1))).astype(np.uint8) * r.integers(1, 256, (B, H, W), dtype=np.uint8)
    m[0, :, W // 2:] = 1
    m[-1, :min(H, 64), :min(W, 64)] = 0
    m[-1, H - 1, W - 1] = 9  # one pixel in the last (cropped) cell
    return m


@pytest.mark.parametrize("H,W", [(120, 200), (128, 192), (1, 1), (65, 129), (64, 64)])
def test_roi_levels_kernel(H, W):
    m = _random_mask(2, H, W, H * 1000 + W)
    t = torch.from_numpy(m).to(DEV)
    crop = torch.full((2, H + 5, W + 3), 77, dtype=torch.uint8, device=DEV)[:, 2:H + 2, 1:W + 1]  # a window
    crop.copy_(t)
    strided = torch.full((2, H + 1, 2 * W + 3), 77, dtype=torch.uint8, device=DEV)[:, 1:, 2:2 * W + 2:2]  # every other column
    strided.copy_(t)
    tr = t.transpose(1, 2).contiguous().transpose(1, 2)  # column-major
    for lo, hi in ((0, 5), (3, 3), (1, 15)):
        exp = _np_levels(m, lo, hi)
        for v in (t, crop, strided, tr, t != 0):
            got = codec.roi_levels(v, lo, hi)
            assert got.dtype == torch.uint8 and got.is_cuda and np.array_equal(got.cpu().numpy(), exp), (lo, hi)
    zeros, ones = torch.zeros(1, H, W, dtype=torch.uint8, device=DEV), torch.ones(1, H, W, dtype=torch.uint8, device=DEV)
    assert bool((codec.roi_levels(zeros, 2, 5) == 2).all()) and bool((codec.roi_levels(ones, 2, 5) == 5).all())
    assert torch.equal(codec.roi_levels(t, 0, 5).cpu(), codec.roi_levels(t.cpu(), 0, 5))  # the CPU restatement
    rc = _lib.lib().mlic_image_roi_levels_u8(None, C.c_void_p(t.data_ptr()), (C.c_int64 * 3)(*t.stride()), 2, H, W, 4, 3,
                                            C.c_void_p(zeros.data_ptr()))
    assert rc != 0 and "lo is above hi" in _lib.lib().mlic_last_error().decode()


# ----------------------------------------------------------------------------- 6. sq_err_roi kernel
@pytest.mark.parametrize("H,W,layout", [(120, 200, "hwc"), (63, 65, "chw"), (1, 1, "hwc"), (300, 1100, "hwc")])
def test_sq_err_roi_kernel(H, W, layout):
    r = np.random.default_rng(H + W)
    a = r.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    b = r.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    b[1] = 255 - a[1]  # large errors
    m = _random_mask(2, H, W, 5)
    sq = ((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum(-1).astype(np.uint64)
    inside = m != 0
    exp = np.stack([(sq * inside).sum((1, 2)), inside.sum((1, 2)), (sq * ~inside).sum((1, 2)), (~inside).sum((1, 2))],
                   1).astype(np.uint64)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    if layout == "chw":
        ta, tb = ta.permute(0, 3, 1, 2).contiguous(), tb.permute(0, 3, 1, 2).contiguous()
    tm = torch.from_numpy(m).to(DEV)
    pad = torch.zeros(2, H + 2, W + 3, dtype=torch.uint8, device=DEV)
    pm = pad[:, 1:H + 1, 2:W + 2]
    pm.copy_(tm)
    for mask in (tm, pm, tm != 0):
        got = codec.sq_err_roi(ta, tb, mask, layout=layout)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy().astype(np.uint64), exp)
    # inside + outside is the egress kernel's total, and the pixel counts add to H * W
    x = ((torch.from_numpy(a).float() + 0.5) / 255).permute(0, 3, 1, 2).contiguous().to(DEV)  # floors back to a
    back, total = codec.egress_u8(x, H, W, layout, ref=tb)
    assert torch.equal(back, ta)
    assert torch.equal(got[:, 0] + got[:, 2], total)
    assert bool((got[:, 1] + got[:, 3] == H * W).all())
    p = codec.psnr_roi(ta, tb, tm, layout=layout)
    for i in range(2):
        for key, s, n in (("psnr_roi", exp[i, 0], exp[i, 1]), ("psnr_bg", exp[i, 2], exp[i, 3])):
            assert p[i][key] == (codec.psnr_from_sq_err(int(s), 3 * int(n)) if n else None)


# --------------------------------------------------------------------------------- 7. codec path
def test_codec_end_to_end_cropped_cells():
    name, B, H, W = "MLICPP_L_VBR", 2, 120, 200
    net = net_for(name)
    imgs = (images(B, H, W, 60).clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    masks = torch.zeros(B, H, W, dtype=torch.uint8)
    masks[0, :, 100:] = 1
    masks[1, 100:, 150:] = 255  # part of the cropped bottom cells (56 rows) ...
    masks[1, 64:, 192:] = 255   # ... and all of the bottom-right one (56 x 8 pixels)
    files, info = codec.encode_images(net, imgs, roi=masks, roi_levels=(0, 5), return_info=True)
    lmap = codec.roi_levels(masks.to(DEV), 0, 5)
    assert lmap.cpu().tolist() == [[[0, 3, 5, 5], [0, 3, 5, 5]], [[0, 0, 0, 0], [0, 0, 2, 5]]]
    x = codec.ingest_u8(imgs.to(DEV), "hwc")
    g = codec.gain_plane(net, lmap)
    f = net(x, gain_map=g)
    c = net.compress(x, gain_map=g)
    for b, data in enumerate(files):
        d = codec.peek(data, vbr=True, n_levels=net.levels)
        assert np.array_equal(d["roi_levels"], lmap[b].cpu().numpy()) and (d["H"], d["W"], d["level"]) == (H, W, 5)
        n = C.c_size_t()
        ys, zs = c["strings"][0][b], c["strings"][1][b]
        _lib.call("mlic_container_write_roi", H, W, 5, 2, 4, ys, len(ys), zs, len(zs), None, None, 0, C.byref(n))
        assert len(data) == n.value == info[b]["bytes"]
        assert data == codec.write_container_roi(H, W, (2, 4), ys, zs, 5, lmap[b])
    dec, dinfo = codec.decode_images(net, files, ref=imgs)
    assert torch.equal(dec, codec.egress_u8(f["x_hat"], H, W, "hwc"))
    p = codec.psnr_roi(imgs.to(DEV), dec, masks.to(DEV))
    for b in range(B):
        assert np.array_equal(dinfo[b]["roi_levels"], lmap[b].cpu().numpy())
        assert p[b]["sq_err_roi"] + p[b]["sq_err_bg"] == dinfo[b]["sq_err"]
        assert p[b]["n_roi"] == int((masks[b] != 0).sum()) and p[b]["n_roi"] + p[b]["n_bg"] == H * W
    print([{k: p[b][k] for k in ("psnr_roi", "psnr_bg")} for b in range(B)])
    # the harness record
    from mlic_amd import bitstream
    img0 = x[:1, :, :H, :W]
    r = bitstream.code_image(net, img0, roi=masks[0], roi_levels=(0, 5))
    q = codec.psnr_roi(bitstream.to_u8(img0), bitstream.to_u8(r["x_hat"]), masks[:1].to(DEV), layout="chw")[0]
    assert r["bytes"] == len(files[0]) and r["psnr_roi"] == q["psnr_roi"] and r["psnr_bg"] == q["psnr_bg"]
    assert torch.equal(r["x_hat"], f["x_hat"][:1, :, :H, :W])


# ----------------------------------------------------------------------------------- 8. refusals
def test_refusals_reach_no_gpu_call():
    """Each refusal by its message; the models below never get a handle, so no kernel ran for them."""
    fixed = get_model("MLICPP_M_SMALL_DEC").to(DEV).eval()
    vbr = get_model("MLICPP_M_SMALL_DEC_VBR").to(DEV).eval()
    x = torch.zeros(2, 3, 128, 128, device=DEV)
    g = const_plane(2, 128, 128, 1.0)
    for call in (lambda: fixed(x, gain_map=g), lambda: fixed.compress(x, gain_map=g),
                 lambda: fixed.decompress([[b"", b""], [b"", b""]], (2, 2), gain_map=g)):
        with pytest.raises(ValueError, match="fixed-rate"):
            call()
    for bad in (const_plane(2, 128, 192, 1.0), const_plane(1, 128, 128, 1.0), g[0, 0]):
        with pytest.raises(ValueError, match="shape"):
            vbr(x, gain_map=bad)
        with pytest.raises(ValueError, match="shape"):
            vbr.compress(x, gain_map=bad)
        with pytest.raises(ValueError, match="shape"):
            vbr.decompress([[b"", b""], [b"", b""]], (2, 2), gain_map=bad)
    with pytest.raises(ValueError, match="CUDA"):
        vbr(x, gain_map=g.cpu())
    with pytest.raises(ValueError, match="CUDA"):
        vbr.compress(x, gain_map=g.cpu())
    with pytest.raises(ValueError, match="float32"):
        vbr(x, gain_map=g.half())
    with pytest.raises(ValueError, match="batch_stream"):
        vbr.compress(x, gain_map=g, batch_stream=True)
    with pytest.raises(ValueError, match="batch-stream"):
        vbr.decompress([[b"one stream"], [b"", b""]], (2, 2), gain_map=g)
    imgs = torch.zeros(2, 120, 120, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="max_bpp"):
        codec.encode_images(vbr, imgs, roi=torch.ones(2, 120, 120, dtype=torch.uint8), roi_levels=(0, 4), max_bpp=0.5)
    with pytest.raises(ValueError, match="fixed-rate"):
        codec.encode_images(fixed, imgs, roi=torch.ones(2, 120, 120, dtype=torch.uint8), roi_levels=(0, 4))
    assert fixed._handle is None and vbr._handle is None
    # the C ABI's own refusals, before any GPU call: a model that is not *_VBR, a null plane, batch_stream
    # after a plane encode
    lib = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    hf = fixed._ensure_handle(DEV)
    rc = lib.mlic_forward_g(hf, st, x.data_ptr(), 2, 128, 128, None, None, None, g.data_ptr())
    assert rc != 0 and "needs a *_VBR model" in lib.mlic_last_error().decode()
    rc = lib.mlic_compress_g(hf, st, x.data_ptr(), 2, 128, 128, g.data_ptr())
    assert rc != 0 and "needs a *_VBR model" in lib.mlic_last_error().decode()
    net = net_for("MLICPP_M_SMALL_DEC_VBR")
    hv = net._ensure_handle(DEV)
    rc = lib.mlic_forward_g(hv, st, x.data_ptr(), 2, 128, 128, None, None, None, None)
    assert rc != 0 and "null gain plane" in lib.mlic_last_error().decode()
    rc = lib.mlic_compress_g(hv, st, x.data_ptr(), 2, 128, 128, None)
    assert rc != 0 and "null gain plane" in lib.mlic_last_error().decode()
    rc = lib.mlic_decompress_g(hv, st, None, None, None, None, 2, 2, 2, x.data_ptr(), None)
    assert rc != 0 and "null gain plane" in lib.mlic_last_error().decode()
    xs = images(2, 128, 128, 85).to(DEV)
    net.compress(xs, gain_map=g)
    n = C.c_size_t()
    rc = lib.mlic_batch_stream(hv, 0, 2, None, 0, C.byref(n))
    assert rc != 0 and "gain plane" in lib.mlic_last_error().decode()
    net.compress(xs, s=1, batch_stream=True)  # the scalar call's batch stream is untouched
