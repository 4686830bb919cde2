"""Scaled coding on the GPU (DESIGN.md section 5 "Scaled coding"): the fused resample ingest / egress kernels
(csrc/resample.hip) against the fp32 CPU restatement in codec.py, bit for bit, and pixels -> scaled file -> pixels
through codec.py and the two one-image C calls.

Every comparison is exact.  The yardstick is the torch CPU loop `acc = acc + w * view` of codec._resample_cpu
(which tests/test_scaled_cpu.py ties to the float64 oracle); it is computed once per (shape, filter) and shared by
the layouts.  fp32 destinations are NaN-filled between guard words, byte destinations sit inside a 0xA5-filled
allocation that is checked after the call."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from mlic_amd import _lib, bitstream, codec, get_model, synthetic
from resample_oracle import SHAPES

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD, SENT, FSENT = 512, 0xA5, 0x5A5A5A5A
FILTERS = ["lanczos3", "bicubic", "triangle"]


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _pad64(n):
    return (n + 63) // 64 * 64


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def _images(H, W):
    """uint8 [2, H, W, 3] on the CPU: image 0 a ramp through all byte values, image 1 noise with flat 0 / 255 blocks
    (where lanczos and bicubic overshoot and the clamp acts)."""
    r = np.random.default_rng(1000 * H + W)
    a = r.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    a[0] = (np.arange(H * W * 3, dtype=np.int64) * 37).astype(np.uint8).reshape(H, W, 3)
    a[1, : H // 2, : W // 2] = 255
    a[1, H // 2:, W // 2:] = 0
    return torch.from_numpy(a)


def _odd(shape, dtype=torch.uint8):
    n = int(np.prod(shape))
    buf = torch.full((n + 1,), SENT, dtype=dtype, device=DEV)
    assert buf[1:].data_ptr() % 2 == 1
    return buf[1:].view(shape)


def _place(img, variant):
    """-> (device view of the [2,H,W,3] batch laid out as `variant`, layout)."""
    B, H, W, _ = img.shape
    if variant == "hwc":
        t, layout = _odd((B, H, W, 3)), "hwc"
    elif variant == "chw":
        t, layout = _odd((B, 3, H, W)), "chw"
    elif variant == "crop":  # a window of a larger image, at an odd address
        t, layout = _odd((B, H + 3, W + 4, 3))[:, 1:H + 1, 2:W + 2], "hwc"
    elif variant == "batch":  # images further apart than their bytes
        t, layout = _odd((B, H * W * 3 + 7))[:, :H * W * 3].view(B, H, W, 3), "hwc"
        assert not t.is_contiguous()
    else:
        raise AssertionError(variant)
    t.copy_((img if layout == "hwc" else img.permute(0, 3, 1, 2)).to(DEV))
    return t, layout


def _strides4(t, layout):
    s = t.stride()
    return (s[0], s[1], s[2], s[3]) if layout == "hwc" else (s[0], s[2], s[3], s[1])


def run_ingest(t, layout, size, flt):
    """mlic_image_ingest_u8_scaled on a device uint8 view -> fp32 [B,3,Hp,Wp] (NaN-filled before, guards checked)."""
    B = t.size(0)
    H, W = (t.size(1), t.size(2)) if layout == "hwc" else (t.size(2), t.size(3))
    h, w = size
    Hp, Wp = _pad64(h), _pad64(w)
    n = B * 3 * Hp * Wp
    buf = torch.empty(GUARD + n + GUARD, dtype=torch.float32, device=DEV)
    buf.view(torch.int32).fill_(FSENT)
    dst = buf[GUARD:GUARD + n]
    dst.fill_(float("nan"))
    _lib.call("mlic_image_ingest_u8_scaled", _stream(), _p(t), (C.c_int64 * 4)(*_strides4(t, layout)), B, H, W,
              codec.FILTERS.index(flt), h, w, _p(dst), Hp, Wp)
    torch.cuda.synchronize()
    g = buf.view(torch.int32)
    assert bool((g[:GUARD] == FSENT).all()) and bool((g[GUARD + n:] == FSENT).all()), "ingest wrote outside dst"
    return dst.view(B, 3, Hp, Wp).cpu()


@functools.lru_cache(maxsize=None)
def _want_ingest(src, size, flt):
    return codec.ingest_u8_scaled(_images(*src), size, flt, "hwc")


@functools.lru_cache(maxsize=None)
def _source(h, w):
    """fp32 [2,3,Hp,Wp] on the CPU: values around [0, 1] with both clamps hit, a few NaN and infinities inside the
    crop, and NaN all over the padding (a kernel that read it would show)."""
    r = np.random.default_rng(7000 * h + w)
    Hp, Wp = _pad64(h), _pad64(w)
    a = r.uniform(-0.25, 1.25, (2, 3, Hp, Wp)).astype(np.float32)
    a[0, :, : h // 2, : w // 2] = 1.0
    a[0, :, h // 2:h, w // 2:w] = 0.0
    for k, v in enumerate((np.nan, np.inf, -np.inf, -0.0, 1e-40)):
        a[1, k % 3, (k * 5) % h, (k * 11) % w] = v
    a[:, :, h:, :] = np.nan
    a[:, :, :, w:] = np.nan
    return torch.from_numpy(a)


@functools.lru_cache(maxsize=None)
def _want_egress(src, size, flt):
    """(bytes [2,Ho,Wo,3], reference [2,Ho,Wo,3], sq_err list) from the CPU restatement."""
    h, w = src
    img = codec.egress_u8_scaled(_source(h, w), h, w, size, flt, "hwc")
    ref = torch.from_numpy(np.random.default_rng(size[0] * 31 + size[1]).integers(0, 256, tuple(img.shape), dtype=np.uint8))
    d = img.numpy().astype(np.int64) - ref.numpy().astype(np.int64)
    return img, ref, (d * d).reshape(2, -1).sum(1).tolist()


def _dest(B, Ho, Wo, variant):
    """-> (the whole 0xA5-filled allocation, the destination view in it, layout)."""
    if variant == "hwc":
        buf = torch.full((GUARD + B * Ho * Wo * 3 + 1 + GUARD,), SENT, dtype=torch.uint8, device=DEV)
        return buf, buf[GUARD + 1:GUARD + 1 + B * Ho * Wo * 3].view(B, Ho, Wo, 3), "hwc"
    if variant == "chw":
        buf = torch.full((GUARD + B * Ho * Wo * 3 + 1 + GUARD,), SENT, dtype=torch.uint8, device=DEV)
        return buf, buf[GUARD + 1:GUARD + 1 + B * Ho * Wo * 3].view(B, 3, Ho, Wo), "chw"
    if variant == "crop":
        n = B * (Ho + 3) * (Wo + 4) * 3
        buf = torch.full((GUARD + n + 1 + GUARD,), SENT, dtype=torch.uint8, device=DEV)
        return buf, buf[GUARD + 1:GUARD + 1 + n].view(B, Ho + 3, Wo + 4, 3)[:, 1:Ho + 1, 2:Wo + 2], "hwc"
    if variant == "batch":
        n = Ho * Wo * 3
        buf = torch.full((GUARD + B * (n + 7) + 1 + GUARD,), SENT, dtype=torch.uint8, device=DEV)
        return buf, buf[GUARD + 1:GUARD + 1 + B * (n + 7)].view(B, n + 7)[:, :n].view(B, Ho, Wo, 3), "hwc"
    raise AssertionError(variant)


def run_egress(src, h, w, size, flt, variant, ref=None):
    """mlic_image_egress_u8_scaled into a guarded destination -> (bytes as [B,Ho,Wo,3] on the CPU, sq_err or None)."""
    B = src.size(0)
    Ho, Wo = size
    buf, dst, layout = _dest(B, Ho, Wo, variant)
    sq = None
    if ref is not None:
        ref = ref.to(DEV) if layout == "hwc" else ref.permute(0, 3, 1, 2).contiguous().to(DEV)
        sq = torch.full((B,), -1, dtype=torch.int64, device=DEV)
    _lib.call("mlic_image_egress_u8_scaled", _stream(), _p(src), (C.c_int64 * 3)(*src.stride()[:3]), B, h, w,
              codec.FILTERS.index(flt), Ho, Wo, _p(dst), (C.c_int64 * 4)(*_strides4(dst, layout)),
              None if ref is None else _p(ref), None if ref is None else (C.c_int64 * 4)(*_strides4(ref, layout)),
              None if sq is None else _p(sq))
    torch.cuda.synchronize()
    got = (dst if layout == "hwc" else dst.permute(0, 2, 3, 1)).cpu()
    dst.fill_(SENT)
    assert bool((buf == SENT).all()), "egress wrote outside the image's bytes"
    return got, None if sq is None else sq.cpu().tolist()


@pytest.fixture
def forced_path():
    def force(v):
        _lib.call("mlic_set_kernel_option", b"image_io_path", v)
    yield force
    _lib.call("mlic_set_kernel_option", b"image_io_path", -1)


# ------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("flt", FILTERS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_ingest_matches_the_cpu_restatement_bitwise(shape, flt):
    src, size = shape
    want = _want_ingest(src, size, flt)
    assert not torch.isnan(want).any() and float(want.min()) >= 0.0 and float(want.max()) <= 1.0
    for variant in ("hwc", "chw", "crop", "batch"):
        t, layout = _place(_images(*src), variant)
        got = run_ingest(t, layout, size, flt)
        assert not torch.isnan(got).any(), variant
        assert _same_bits(got, want), variant  # bit patterns: the padding is +0.0, not -0.0
        assert int(got[:, :, size[0]:].view(torch.int32).abs().sum()) == 0
        assert int(got[:, :, :, size[1]:].view(torch.int32).abs().sum()) == 0


@pytest.mark.parametrize("flt", FILTERS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_egress_matches_the_cpu_restatement_bitwise(shape, flt, forced_path):
    (h, w), size = shape
    want, ref, want_sq = _want_egress((h, w), size, flt)
    src = _source(h, w).to(DEV)
    for variant in ("hwc", "chw", "crop", "batch"):
        got, _ = run_egress(src, h, w, size, flt, variant)
        assert torch.equal(got, want), variant
        got, sq = run_egress(src, h, w, size, flt, variant, ref=ref)
        assert torch.equal(got, want) and sq == want_sq, variant
    forced_path(0)  # the general-stride form on the canonical layouts: the same bits
    for variant in ("hwc", "chw"):
        got, sq = run_egress(src, h, w, size, flt, variant, ref=ref)
        assert torch.equal(got, want) and sq == want_sq, variant


@pytest.mark.parametrize("flt", FILTERS)
def test_identity_equals_the_plain_kernels(flt):
    H, W = 70, 130
    img = _images(H, W).to(DEV)
    assert _same_bits(codec.ingest_u8_scaled(img, (H, W), flt).cpu(), codec.ingest_u8(img).cpu())
    x = _source(H, W).to(DEV)
    ref = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (2, H, W, 3), dtype=np.uint8)).to(DEV)
    a, sa = codec.egress_u8_scaled(x, H, W, (H, W), flt, ref=ref)
    b, sb = codec.egress_u8(x, H, W, ref=ref)
    assert torch.equal(a, b) and torch.equal(sa, sb)


def test_a_nan_gives_the_bytes_of_zero():
    h, w, size = 37, 53, (19, 27)
    a = _source(h, w).clone()
    a[:, :, :h, :w] = torch.nan_to_num(a[:, :, :h, :w], nan=0.5, posinf=1.0, neginf=0.0)
    b, z = a.clone(), a.clone()
    for k in range(6):
        b[k % 2, k % 3, (7 * k) % h, (13 * k) % w] = float("nan")
        z[k % 2, k % 3, (7 * k) % h, (13 * k) % w] = 0.0
    for flt in FILTERS:
        gb = codec.egress_u8_scaled(b.to(DEV), h, w, size, flt)
        gz = codec.egress_u8_scaled(z.to(DEV), h, w, size, flt)
        ga = codec.egress_u8_scaled(a.to(DEV), h, w, size, flt)
        assert torch.equal(gb, gz) and not torch.equal(gb, ga)


def test_python_layer_on_the_device():
    img = _images(37, 53)
    for layout, t in (("hwc", img), ("chw", img.permute(0, 3, 1, 2).contiguous())):
        got = codec.ingest_u8_scaled(t.to(DEV), (19, 27), "bicubic", layout)
        assert got.is_cuda and _same_bits(got.cpu(), _want_ingest((37, 53), (19, 27), "bicubic"))
    x = _source(19, 27)
    for layout in ("hwc", "chw"):
        want, sq_w = codec.egress_u8_scaled(x, 19, 27, (37, 53), "lanczos3", layout, ref=_images(37, 53) if layout == "hwc"
                                            else _images(37, 53).permute(0, 3, 1, 2))
        got, sq = codec.egress_u8_scaled(x.to(DEV), 19, 27, (37, 53), "lanczos3", layout,
                                         ref=_images(37, 53) if layout == "hwc" else _images(37, 53).permute(0, 3, 1, 2))
        assert torch.equal(got.cpu(), want) and sq.cpu().tolist() == sq_w.tolist()
    canvas = torch.full((2, 50, 60, 3), SENT, dtype=torch.uint8, device=DEV)
    codec.egress_u8_scaled(x.to(DEV), 19, 27, (37, 53), "triangle", out=canvas[:, 3:40, 5:58])
    want = codec.egress_u8_scaled(x, 19, 27, (37, 53), "triangle")
    assert torch.equal(canvas[:, 3:40, 5:58].cpu(), want)
    canvas[:, 3:40, 5:58] = SENT
    assert bool((canvas == SENT).all())
    with pytest.raises(_lib.MlicError, match=r"\[1/8, 8\]"):
        _lib.call("mlic_image_ingest_u8_scaled", _stream(), _p(canvas), (C.c_int64 * 4)(*canvas.stride()), 2, 50, 60, 0, 6,
                  60, _p(canvas), 64, 64)
    with pytest.raises(_lib.MlicError, match="unknown filter"):
        _lib.call("mlic_image_ingest_u8_scaled", _stream(), _p(canvas), (C.c_int64 * 4)(*canvas.stride()), 2, 50, 60, 3, 50,
                  60, _p(canvas), 64, 64)


# --------------------------------------------------------------------------------------- end to end
def _net(name):
    net = get_model(name)
    net.load_state_dict(synthetic.synth_state_dict(name, 0))
    net = net.to(DEV).eval()
    net.update()
    return net


@pytest.fixture(scope="module")
def net_s():
    return _net("MLICPP_S")


@pytest.fixture(scope="module")
def net_vbr():
    return _net("MLICPP_S_VBR")


def _u8_image(H, W, seed):
    x = synthetic.synth_image(_pad64(H), _pad64(W), seed)[0, :, :H, :W]
    return torch.round(x * 255).to(torch.uint8).permute(1, 2, 0).contiguous()


H, W, CODED = 100, 150, (50, 75)


@pytest.mark.parametrize("vbr", [False, True], ids=["fixed", "vbr"])
def test_scaled_file_is_the_header_around_the_coded_image(net_s, net_vbr, vbr):
    net, level = (net_vbr, 3) if vbr else (net_s, None)
    net.range_fallbacks(reset=True)
    img = torch.stack([_u8_image(H, W, 3), _u8_image(H, W, 4)])
    kw = {"level": level} if vbr else {}
    files, info = codec.encode_images(net, img, coded_size=CODED, filter="bicubic", return_info=True, **kw)
    # the model's part: compress of the resampled float image, in the plain container of the coded size
    x = codec.ingest_u8_scaled(img.to(DEV), CODED, "bicubic")
    out = net.compress(x, **({"s": [level] * 2} if vbr else {}))
    for b, f in enumerate(files):
        inner = codec.write_container(CODED[0], CODED[1], out["shape"], out["strings"][0][b], out["strings"][1][b], level)
        head = b"MLS1" + bytes([0, int(vbr), 1, 0]) + H.to_bytes(4, "big") + W.to_bytes(4, "big")
        assert f == head + inner
        assert info[b]["bytes"] == len(f) and info[b]["bpp"] == 8.0 * len(f) / (H * W) and info[b]["coded"] == CODED
        d = codec.peek(f, vbr=vbr)
        assert (d["H"], d["W"], d["coded"], d["filter"], d["level"]) == (H, W, CODED, "bicubic", level)
    assert codec.encode_images(net, img, scale="1/2", filter="bicubic", **kw) == files
    # decode: the model's decompress of the inner file, then the scaled egress
    x_hat = net.decompress(out["strings"], out["shape"], **({"s": [level] * 2} if vbr else {}))["x_hat"]
    want, want_sq = codec.egress_u8_scaled(x_hat, CODED[0], CODED[1], (H, W), "bicubic", ref=img.to(DEV))
    got, dinfo = codec.decode_images(net, files, ref=img)
    assert torch.equal(got, want)
    for b in range(2):
        d = dinfo[b]
        assert d["sq_err"] == int(want_sq[b]) and (d["H"], d["W"], d["display"], d["coded"]) == (H, W, (H, W), CODED)
        assert d["psnr"] == codec.psnr_from_sq_err(d["sq_err"], 3 * H * W) and d["level"] == level
    # the CPU restatement of the egress on the same x_hat gives the same bytes
    assert torch.equal(got.cpu(), codec.egress_u8_scaled(x_hat.cpu(), CODED[0], CODED[1], (H, W), "bicubic"))
    assert not any(net.range_fallbacks(reset=True).values())


def test_out_size_on_a_plain_and_on_a_scaled_file(net_s):
    net = net_s
    net.range_fallbacks(reset=True)
    img = _u8_image(H, W, 5).unsqueeze(0)
    plain = codec.encode_images(net, img)
    c = codec.parse_container(plain[0])
    x_hat = net.decompress([[plain[0][c.y_off:c.y_off + c.y_len]], [plain[0][c.z_off:c.z_off + c.z_len]]],
                           (c.hz, c.wz))["x_hat"]
    thumb, info = codec.decode_images(net, plain, out_size=(25, 38))
    assert torch.equal(thumb, codec.egress_u8_scaled(x_hat, H, W, (25, 38), "lanczos3"))
    assert (info[0]["H"], info[0]["W"], info[0]["coded"], info[0]["bpp"]) == (25, 38, (H, W), 8.0 * len(plain[0]) / (H * W))
    thumb, _ = codec.decode_images(net, plain, out_size=(25, 38), filter="triangle")
    assert torch.equal(thumb, codec.egress_u8_scaled(x_hat, H, W, (25, 38), "triangle"))
    same, _ = codec.decode_images(net, plain, out_size=(H, W))  # the identity tables: the plain decode's bytes
    assert torch.equal(same, codec.decode_images(net, plain)[0])
    scaled = codec.encode_images(net, img, coded_size=CODED)
    s = codec.parse_container_scaled(scaled[0])
    inner = scaled[0][s.inner_off:]
    x_hat = net.decompress([[inner[s.inner.y_off:s.inner.y_off + s.inner.y_len]],
                            [inner[s.inner.z_off:s.inner.z_off + s.inner.z_len]]], (s.inner.hz, s.inner.wz))["x_hat"]
    ref = _u8_image(30, 45, 9).unsqueeze(0)
    thumb, info = codec.decode_images(net, scaled, out_size=(30, 45), ref=ref)
    want, sq = codec.egress_u8_scaled(x_hat, CODED[0], CODED[1], (30, 45), "lanczos3", ref=ref.to(DEV))
    assert torch.equal(thumb, want) and info[0]["sq_err"] == int(sq[0])
    assert info[0]["display"] == (H, W) and info[0]["bpp"] == 8.0 * len(scaled[0]) / (H * W)
    # a plain and a scaled file of one padded size in one call: each at its own display size
    both, info = codec.decode_images(net, [scaled[0], codec.encode_images(net, _u8_image(50, 75, 5).unsqueeze(0))[0]])
    assert tuple(both.shape) == (2, H, W, 3) and (info[1]["H"], info[1]["W"]) == (50, 75)
    assert torch.equal(both[:1], codec.decode_images(net, scaled)[0]) and not bool(both[1, 50:].any())
    assert not any(net.range_fallbacks(reset=True).values())


def test_max_bpp_counts_the_display_pixels_and_the_whole_file(net_s, net_vbr):
    img = _u8_image(H, W, 6).unsqueeze(0)
    free, info = codec.encode_images(net_s, img, coded_size=CODED, return_info=True)
    assert info[0]["passes"] == 0 and info[0]["met"]
    bpp0 = 8.0 * len(free[0]) / (H * W)
    # a budget just under the unconstrained file: at least one filter pass, counted over display pixels
    files, info = codec.encode_images(net_s, img, coded_size=CODED, max_bpp=bpp0 * 0.999, max_passes=2, return_info=True)
    assert info[0]["passes"] >= 1 and info[0]["bpp"] == 8.0 * len(files[0]) / (H * W)
    assert info[0]["met"] == (info[0]["bpp"] <= bpp0 * 0.999)
    # a budget the file meets only because the display has four times the coded pixels
    files, info = codec.encode_images(net_s, img, coded_size=CODED, max_bpp=bpp0 * 1.001, return_info=True)
    assert files == free and info[0]["passes"] == 0 and info[0]["met"]
    assert 8.0 * (len(free[0]) - 16) / (CODED[0] * CODED[1]) > bpp0 * 1.001
    # level="auto": the highest level whose whole scaled file fits the display-pixel budget
    sizes = [len(codec.encode_images(net_vbr, img, coded_size=CODED, level=l)[0]) for l in range(net_vbr.levels)]
    budget = 8.0 * (sizes[2] + 0.5) / (H * W)
    files, info = codec.encode_images(net_vbr, img, coded_size=CODED, level="auto", max_bpp=budget, return_info=True)
    fits = [l for l in range(net_vbr.levels) if 8.0 * sizes[l] / (H * W) <= budget]
    assert info[0]["level"] == max(fits) and len(files[0]) == sizes[max(fits)] and info[0]["met"]


@pytest.mark.parametrize("vbr", [False, True], ids=["fixed", "vbr"])
def test_one_image_c_calls_give_the_python_path_bytes(net_s, net_vbr, vbr):
    net, level = (net_vbr, 2) if vbr else (net_s, -1)
    net.range_fallbacks(reset=True)
    img = _u8_image(H, W, 7)
    gains = [float(net._vbr_scales(1, s=l, coder=True)[0]) for l in range(net.levels)] if vbr else None
    want = codec.encode_images(net, img.unsqueeze(0), coded_size=CODED, filter="lanczos3", **({"level": level} if vbr else {}))[0]
    h = net._handle
    rgb = _odd((H, W * 3 + 5))[:, :W * 3].unflatten(1, (W, 3))
    rgb.copy_(img.to(DEV))
    s3 = (C.c_int64 * 3)(*rgb.stride())
    n = C.c_size_t()
    scale = gains[level] if vbr else 1.0
    with pytest.raises(_lib.MlicError, match=r"\[1/8, 8\]"):
        _lib.call("mlic_encode_image_u8_scaled", h, _stream(), _p(rgb), s3, H, W, 12, 75, 0, scale, level, None, 0, C.byref(n))
    _lib.call("mlic_encode_image_u8_scaled", h, _stream(), _p(rgb), s3, H, W, CODED[0], CODED[1], 0, scale, level, None, 0,
              C.byref(n))
    out = C.create_string_buffer(n.value)
    with pytest.raises(_lib.MlicError, match="buffer too small"):
        _lib.call("mlic_encode_image_u8_scaled", h, _stream(), None, None, 0, 0, 0, 0, 0, 1.0, -1, out, n.value - 1, C.byref(n))
    _lib.call("mlic_encode_image_u8_scaled", h, _stream(), None, None, 0, 0, 0, 0, 0, 1.0, -1, out, n.value, C.byref(n))
    data = C.string_at(out, n.value)
    assert data == want
    # decode: the report-only call, then the display size, then a thumbnail; the plain file likewise
    n_levels = net.levels if vbr else 0
    g = None if gains is None else np.ascontiguousarray(gains, dtype=np.float32)
    gp = None if g is None else C.c_void_p(g.ctypes.data)
    plain = codec.encode_images(net, img.unsqueeze(0), **({"level": level} if vbr else {}))[0]
    for file, coded in ((data, CODED), (plain, (H, W))):
        for out_size in ((0, 0), (30, 45)):
            oh, ow, ol, ch, cw = (C.c_int() for _ in range(5))
            _lib.call("mlic_decode_image_u8_sized", None, None, file, len(file), n_levels, 1 << 28, None, out_size[0],
                      out_size[1], -1, None, None, 0, C.byref(oh), C.byref(ow), C.byref(ol), C.byref(ch), C.byref(cw))
            Ho, Wo = out_size if out_size[0] else (H, W)
            assert (oh.value, ow.value, ol.value, ch.value, cw.value) == (Ho, Wo, level, coded[0], coded[1])
            buf, dst, _ = _dest(1, Ho, Wo, "crop")
            d3 = (C.c_int64 * 3)(*dst[0].stride())
            cap = 1 + (Ho - 1) * dst.stride(1) + (Wo - 1) * dst.stride(2) + 2
            with pytest.raises(_lib.MlicError, match="cap_bytes"):
                _lib.call("mlic_decode_image_u8_sized", h, _stream(), file, len(file), n_levels, 1 << 28, gp, out_size[0],
                          out_size[1], -1, _p(dst), d3, cap - 1, None, None, None, None, None)
            _lib.call("mlic_decode_image_u8_sized", h, _stream(), file, len(file), n_levels, 1 << 28, gp, out_size[0],
                      out_size[1], -1, _p(dst), d3, cap, None, None, None, None, None)
            torch.cuda.synchronize()
            got = dst.cpu()
            dst.fill_(SENT)
            assert bool((buf == SENT).all()), "decode wrote outside the image"
            want_px, _ = codec.decode_images(net, [file], out_size=None if out_size == (0, 0) else out_size)
            assert torch.equal(got, want_px.cpu())
    with pytest.raises(_lib.MlicError, match="out_H, out_W"):
        _lib.call("mlic_decode_image_u8_sized", None, None, data, len(data), n_levels, 1 << 28, None, 30, 0, -1, None, None,
                  0, None, None, None, None, None)
    with pytest.raises(_lib.MlicError, match=r"\[1/8, 8\]"):
        _lib.call("mlic_decode_image_u8_sized", None, None, data, len(data), n_levels, 1 << 28, None, 6, 75, -1, None, None,
                  0, None, None, None, None, None)
    assert not any(net.range_fallbacks(reset=True).values())
