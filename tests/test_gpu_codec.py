"""The uint8 codec path on the GPU: the ingest / egress kernels (csrc/image_io.hip) against the torch
expressions they replace, bit for bit, and pixels -> file bytes -> pixels through codec.py and the C ABI
against the existing compress / write_stream / decompress path.

Every comparison is exact.  The reference of ingest is torch's CPU `u8.float().div(255)` (a true division: it
is what torchvision's ToTensor, which runs on the host, hands the reference's model); ROCm torch's own device
division by a scalar multiplies by the reciprocal and is therefore not the reference (the number of values on
which it differs is printed, not asserted).  Every output is pre-filled with NaN or a sentinel, and every
destination sits between sentinel guard bytes inside one allocation; the guards are checked after each call.
Shapes are the smallest at which these kernels can go wrong: vector tails, odd row starts, padding widths."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

from mlic_amd import _lib, bitstream, codec, get_model, synthetic

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD, SENT = 512, 0xA5
FSENT = 0x5A5A5A5A  # guard word around fp32 destinations
SHAPES = [(1, 1), (1, 67), (63, 65), (64, 64), (65, 127), (130, 70)]


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _images(B, H, W, seed=0):
    """uint8 [B, H, W, 3] on the CPU; image 0 is a ramp (all 256 values once H * W * 3 >= 256)."""
    r = np.random.default_rng(1000 * H + W + seed)
    a = r.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    a[0] = (np.arange(H * W * 3, dtype=np.int64) * 37 + seed).astype(np.uint8).reshape(H, W, 3)
    return torch.from_numpy(a)


def _place(img_hwc, layout, variant):
    """A device tensor of the image batch in `layout` ([B,H,W,3] / [B,3,H,W]) whose memory is arranged as
    `variant`; always starts at an odd address."""
    B, H, W, _ = img_hwc.shape
    src = img_hwc if layout == "hwc" else img_hwc.permute(0, 3, 1, 2)

    def odd(shape):
        n = int(np.prod(shape))
        buf = torch.full((n + 1,), SENT, dtype=torch.uint8, device=DEV)
        return buf[1:].view(shape)

    if variant == "plain":
        t = odd(tuple(src.shape))
    elif variant == "rowpad":  # rows longer than the image's
        t = (odd((B, H, W * 3 + 5))[:, :, :W * 3].unflatten(2, (W, 3)) if layout == "hwc"
             else odd((B, 3, H, W + 3))[..., :W])
    elif variant == "crop":  # a window of a larger image
        t = (odd((B, H + 3, W + 4, 3))[:, 1:H + 1, 2:W + 2] if layout == "hwc"
             else odd((B, 3, H + 3, W + 4))[:, :, 1:H + 1, 2:W + 2])
    elif variant == "rgba":  # four bytes a pixel: neither canonical form
        assert layout == "hwc"
        t = odd((B, H, W, 4))[..., :3]
    elif variant == "transposed":  # column-major pixels: neither canonical form
        t = (odd((B, W, H, 3)).permute(0, 2, 1, 3) if layout == "hwc" else odd((B, 3, W, H)).permute(0, 1, 3, 2))
    else:
        raise AssertionError(variant)
    assert tuple(t.shape) == tuple(src.shape) and (variant != "plain" or t.data_ptr() % 2 == 1)
    t.copy_(src.to(DEV))
    return t


def _strides4(t, layout):
    s = t.stride()
    return (s[0], s[1], s[2], s[3]) if layout == "hwc" else (s[0], s[2], s[3], s[1])


def run_ingest(t, layout, strides=None):
    """mlic_image_ingest_u8 on a device uint8 view -> fp32 [B,3,Hp,Wp] (NaN-filled before, guards checked)."""
    B = t.size(0)
    H, W = (t.size(1), t.size(2)) if layout == "hwc" else (t.size(2), t.size(3))
    Hp, Wp = (H + 63) // 64 * 64, (W + 63) // 64 * 64
    n = B * 3 * Hp * Wp
    buf = torch.empty(GUARD + n + GUARD, dtype=torch.float32, device=DEV)
    buf.view(torch.int32).fill_(FSENT)
    dst = buf[GUARD:GUARD + n]
    dst.fill_(float("nan"))
    s = (C.c_int64 * 4)(*(strides or _strides4(t, layout)))
    _lib.call("mlic_image_ingest_u8", _stream(), _p(t), s, B, H, W, _p(dst), Hp, Wp)
    torch.cuda.synchronize()
    g = buf.view(torch.int32)
    assert bool((g[:GUARD] == FSENT).all()) and bool((g[GUARD + n:] == FSENT).all()), "ingest wrote outside dst"
    return dst.view(B, 3, Hp, Wp).cpu()


def _want_ingest(img_hwc):
    return bitstream.pad64(img_hwc.permute(0, 3, 1, 2).float().div(255)).contiguous()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture
def forced_path():
    def force(v):
        _lib.call("mlic_set_kernel_option", b"image_io_path", v)
    yield force
    _lib.call("mlic_set_kernel_option", b"image_io_path", -1)


# ------------------------------------------------------------------------------------------- ingest
@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("shape", SHAPES)
def test_ingest_matches_float_div_255_bitwise(shape, layout):
    H, W = shape
    for B in (1, 3):
        img = _images(B, H, W)
        if H * W * 3 >= 256:
            assert len(torch.unique(img[0])) == 256
        want = _want_ingest(img)
        assert not torch.isnan(want).any()
        for variant in ("plain", "rowpad", "crop", "transposed") + (("rgba",) if layout == "hwc" else ()):
            got = run_ingest(_place(img, layout, variant), layout)
            assert not torch.isnan(got).any(), (B, variant)
            # bit patterns: the padding is +0.0 (not -0.0), the values are torch's CPU division
            assert _same_bits(got, want), (B, variant)
            assert int(got[:, :, H:].view(torch.int32).abs().sum()) == 0
            assert int(got[:, :, :, W:].view(torch.int32).abs().sum()) == 0


def test_ingest_all_256_values_and_the_reciprocal_product():
    k = torch.arange(256, dtype=torch.uint8)
    img = k.view(1, 1, 256, 1).expand(1, 1, 256, 3).contiguous()
    want = k.float().div(255)
    for layout, t in (("hwc", img), ("chw", img.permute(0, 3, 1, 2).contiguous())):
        got = run_ingest(t.to(DEV), layout)
        for c in range(3):
            assert _same_bits(got[0, c, 0, :256], want)
    dev_div = k.to(DEV).float().div(255).cpu()
    print(f"torch device div(255) differs from the CPU division on "
          f"{int((dev_div.view(torch.int32) != want.view(torch.int32)).sum())} of 256 values (the kernel on 0)")


def test_ingest_forms_agree(forced_path):
    """The general-stride kernel against each canonical form on that form's layout, and all three on a
    one-pixel-wide image, whose memory both canonical stride sets describe."""
    for H, W in ((65, 127), (130, 70)):
        img = _images(3, H, W)
        want = _want_ingest(img)
        for layout in ("hwc", "chw"):
            t = _place(img, layout, "plain")
            out = {}
            for path in (-1, 0, 1 if layout == "hwc" else 2):
                forced_path(path)
                out[path] = run_ingest(t, layout)
                assert _same_bits(out[path], want), (layout, path)
    H, B = 67, 2
    img = _images(B, H, 1)
    t = _place(img, "hwc", "plain")  # bytes r0 g0 b0 r1 g1 b1 ... down the single column
    want = _want_ingest(img)
    for path, strides in ((0, (3 * H, 3, 3, 1)), (1, (3 * H, 3, 3, 1)), (2, (3 * H, 3, 1, 1)), (0, (3 * H, 3, 1, 1))):
        forced_path(path)
        assert _same_bits(run_ingest(t, "hwc", strides), want), (path, strides)


# ------------------------------------------------------------------------------------------- egress
def _special_values():
    k = torch.arange(256, dtype=torch.float32) / 255
    inf = torch.tensor(float("inf"))
    v = [k, torch.nextafter(k, inf), torch.nextafter(k, -inf),
         torch.tensor([-0.0, 0.0, -1.0, -1e-30, 1.0000001, 2.0, 1e30, -1e30, float("inf"), -float("inf"), 0.999999,
                       254.999 / 255, 0.5])]
    return torch.cat(v)


def _egress_source(B, H, W, seed=0):
    """fp32 [B,3,H+3,W+4] on the device: a window of a larger tensor (odd strides, offset start), holding every
    k / 255 with both neighbours, values below 0 and above 1, -0.0 and random values."""
    g = torch.Generator().manual_seed(17 * H + W + seed)
    big = torch.rand(B, 3, H + 5, W + 7, generator=g) * 1.4 - 0.2
    sp = _special_values()
    win = big[:, :, 2:, 3:]
    flat = win[:, :, :H, :W].reshape(B, -1)
    for b in range(B):
        m = min(flat.size(1), sp.numel())
        flat[b, :m] = sp.roll(b * 5)[:m]
    win[:, :, :H, :W] = flat.view(B, 3, H, W)
    bigd = big.to(DEV)
    return bigd[:, :, 2:, 3:], big[:, :, 2:, 3:]


def _dest(B, H, W, layout, variant):
    """(flat sentinel buffer, destination view of shape [B,H,W,3] / [B,3,H,W]) on the device."""
    if variant == "plain":
        shape = (B, H, W, 3) if layout == "hwc" else (B, 3, H, W)
        sl = None
    elif variant == "window":
        shape = (B, H + 3, W + 5, 3) if layout == "hwc" else (B, 3, H + 3, W + 5)
        sl = (slice(None), slice(1, H + 1), slice(2, W + 2)) if layout == "hwc" else \
            (slice(None), slice(None), slice(1, H + 1), slice(2, W + 2))
    elif variant == "rgba":
        shape, sl = (B, H, W, 4), (Ellipsis, slice(0, 3))
    else:
        raise AssertionError(variant)
    n = int(np.prod(shape))
    buf = torch.full((GUARD + 1 + n + GUARD,), SENT, dtype=torch.uint8, device=DEV)
    canvas = buf[GUARD + 1:GUARD + 1 + n].view(shape)
    return buf, canvas if sl is None else canvas[sl]


def run_egress(src, H, W, layout, variant, ref=None):
    """mlic_image_egress_u8 into a guarded destination: (image on the CPU, sq_err list or None); everything
    outside the destination view must still hold the sentinel."""
    B = src.size(0)
    buf, dst = _dest(B, H, W, layout, variant)
    sq = None
    if ref is not None:
        sq = torch.full((B + 2,), -7777, dtype=torch.int64, device=DEV)
    _lib.call("mlic_image_egress_u8", _stream(), _p(src), (C.c_int64 * 3)(*src.stride()[:3]), B, H, W, _p(dst),
              (C.c_int64 * 4)(*_strides4(dst, layout)), None if ref is None else _p(ref),
              None if ref is None else (C.c_int64 * 4)(*_strides4(ref, layout)),
              None if sq is None else C.c_void_p(sq.data_ptr() + 8))
    torch.cuda.synchronize()
    got = dst.cpu()
    dst.fill_(SENT)
    assert bool((buf == SENT).all()), f"egress wrote outside the crop ({layout}, {variant})"
    if sq is not None:
        assert sq[0].item() == -7777 and sq[-1].item() == -7777
        sq = sq[1:-1].tolist()
    return got, sq


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("shape", SHAPES)
def test_egress_matches_to_u8_of_the_crop_bitwise(shape, layout):
    H, W = shape
    for B in (1, 3):
        src, src_cpu = _egress_source(B, H, W)
        assert src.stride(3) == 1 and not src.is_contiguous()
        want = bitstream.to_u8(src_cpu[:, :, :H, :W])
        want = want.permute(0, 2, 3, 1).contiguous() if layout == "hwc" else want.contiguous()
        if H * W * 3 >= 800:
            assert len(torch.unique(want[0])) == 256
        ref_img = _images(B, H, W, seed=3)
        for variant in ("plain", "window") + (("rgba",) if layout == "hwc" else ()):
            got, _ = run_egress(src, H, W, layout, variant)
            assert torch.equal(got, want), (B, variant)
        wsq = ((want.numpy().astype(np.int64) -
                (ref_img if layout == "hwc" else ref_img.permute(0, 3, 1, 2)).numpy().astype(np.int64)) ** 2
               ).reshape(B, -1).sum(1).tolist()
        for rvariant in ("plain", "crop") + (("rgba",) if layout == "hwc" else ()):
            ref = _place(ref_img, layout, rvariant)
            got, sq = run_egress(src, H, W, layout, "window", ref=ref)
            got2, sq2 = run_egress(src, H, W, layout, "plain", ref=ref)
            assert torch.equal(got, want) and torch.equal(got2, want)
            assert sq == wsq and sq2 == wsq, (B, rvariant, sq, sq2, wsq)


def test_egress_forms_agree_and_nan_is_zero(forced_path):
    H, W, B = 65, 127, 3
    src, src_cpu = _egress_source(B, H, W)
    for layout in ("hwc", "chw"):
        want = bitstream.to_u8(src_cpu[:, :, :H, :W])
        want = want.permute(0, 2, 3, 1).contiguous() if layout == "hwc" else want.contiguous()
        ref = _place(_images(B, H, W, seed=3), layout, "plain")
        res = []
        for path in (-1, 0, 1 if layout == "hwc" else 2):
            forced_path(path)
            res.append(run_egress(src, H, W, layout, "window", ref=ref))
            assert torch.equal(res[-1][0], want), (layout, path)
        assert res[0][1] == res[1][1] == res[2][1]
    forced_path(-1)
    x = torch.full((1, 3, 64, 64), float("nan"), device=DEV)
    x[0, 1] = 0.5
    got, _ = run_egress(x, 5, 7, "hwc", "plain")
    assert got[..., 0].eq(0).all() and got[..., 1].eq(127).all() and got[..., 2].eq(0).all()


def test_python_layer_on_the_device():
    """codec.ingest_u8 / egress_u8 on CUDA tensors: the kernels' results, egress(ingest(img)) == img, a strided
    `out`, and sq_err against a reference."""
    for H, W in ((65, 127), (1, 67)):
        img = _images(3, H, W)
        for layout in ("hwc", "chw"):
            t = _place(img, layout, "crop")
            x = codec.ingest_u8(t, layout)
            assert x.is_cuda and x.is_contiguous() and _same_bits(x.cpu(), _want_ingest(img))
            back = codec.egress_u8(x, H, W, layout)
            assert back.is_contiguous() and torch.equal(back, t)
            assert _same_bits(codec.ingest_u8(t[0], layout).cpu(), _want_ingest(img[:1]))
            ref = _place(_images(3, H, W, seed=3), layout, "plain")
            buf, win = _dest(3, H, W, layout, "window")
            out, sq = codec.egress_u8(x, H, W, layout, ref=ref, out=win)
            torch.cuda.synchronize()
            assert out is win and torch.equal(win, t)
            want = ((t.cpu().numpy().astype(np.int64) - ref.cpu().numpy().astype(np.int64)) ** 2).reshape(3, -1).sum(1)
            assert sq.dtype == torch.int64 and sq.tolist() == want.tolist()
            win.fill_(SENT)
            assert bool((buf == SENT).all())


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
    """uint8 [H, W, 3] on the CPU: the synthetic image, cropped from its padded size."""
    x = synthetic.synth_image((H + 63) // 64 * 64, (W + 63) // 64 * 64, seed)[0, :, :H, :W]
    return torch.round(x * 255).to(torch.uint8).permute(1, 2, 0).contiguous()


def _reference_path(net, img_hwc, **kw):
    """The existing path on the float image ToTensor would make of img: (file bytes, uint8 [1,H,W,3])."""
    H, W, _ = img_hwc.shape
    x = bitstream.pad64(img_hwc.permute(2, 0, 1).unsqueeze(0).float().div(255)).to(DEV)
    out = net.compress(x, **kw)
    buf = io.BytesIO()
    bitstream.write_stream(buf, H, W, out["shape"], out["strings"], kw.get("s"))
    x_hat = net.decompress(out["strings"], out["shape"], **kw)["x_hat"]
    return buf.getvalue(), bitstream.to_u8(x_hat[:, :, :H, :W]).permute(0, 2, 3, 1).contiguous().cpu()


def _c_abi_round_trip(net, img_hwc, scale, level, gains):
    """mlic_encode_image_u8 / mlic_decode_image_u8 on one image: (file bytes, uint8 [H,W,3] on the CPU)."""
    H, W, _ = img_hwc.shape
    h = net._handle
    n_levels = 0 if gains is None else len(gains)
    rgb = _place(img_hwc.unsqueeze(0), "hwc", "rowpad")[0]
    s3 = (C.c_int64 * 3)(*rgb.stride())
    n = C.c_size_t()
    _lib.call("mlic_encode_image_u8", h, _stream(), _p(rgb), s3, H, W, scale, level, None, 0, C.byref(n))
    out = C.create_string_buffer(n.value)
    with pytest.raises(_lib.MlicError, match="buffer too small"):
        _lib.call("mlic_encode_image_u8", h, _stream(), None, None, 0, 0, 1.0, -1, out, n.value - 1, C.byref(n))
    _lib.call("mlic_encode_image_u8", h, _stream(), None, None, 0, 0, 1.0, -1, out, n.value, C.byref(n))
    data = C.string_at(out, n.value)
    gh, gw, gl = C.c_int(), C.c_int(), C.c_int()
    g = None if gains is None else np.ascontiguousarray(gains, dtype=np.float32)
    gp = None if g is None else C.c_void_p(g.ctypes.data)
    _lib.call("mlic_decode_image_u8", None, None, data, len(data), n_levels, 1 << 28, None, None, None, 0,
              C.byref(gh), C.byref(gw), C.byref(gl))
    assert (gh.value, gw.value, gl.value) == (H, W, level)
    buf, dst = _dest(1, H, W, "hwc", "window")
    d3 = (C.c_int64 * 3)(*dst[0].stride())
    cap = 1 + (H - 1) * dst.stride(1) + (W - 1) * dst.stride(2) + 2
    with pytest.raises(_lib.MlicError, match="cap_bytes"):
        _lib.call("mlic_decode_image_u8", h, _stream(), data, len(data), n_levels, 1 << 28, gp, _p(dst), d3, cap - 1,
                  C.byref(gh), C.byref(gw), C.byref(gl))
    _lib.call("mlic_decode_image_u8", h, _stream(), data, len(data), n_levels, 1 << 28, gp, _p(dst), d3, cap,
              C.byref(gh), C.byref(gw), C.byref(gl))
    torch.cuda.synchronize()
    px = dst[0].cpu()
    dst.fill_(SENT)
    assert bool((buf == SENT).all()), "decode wrote outside the image"
    return data, px


@pytest.mark.parametrize("size", [(128, 128), (100, 150), (65, 129)])
def test_encode_decode_match_the_existing_path(net_s, size):
    H, W = size
    net = net_s
    net.range_fallbacks(reset=True)
    img = _u8_image(H, W, 3)
    want_bytes, want_px = _reference_path(net, img)
    files = codec.encode_images(net, img)
    assert len(files) == 1 and files[0] == want_bytes
    assert codec.encode_images(net, img.numpy())[0] == want_bytes                                  # a host array
    assert codec.encode_images(net, img.permute(2, 0, 1).contiguous().to(DEV))[0] == want_bytes    # CHW, on the device
    p = codec.peek(files[0])
    assert (p["H"], p["W"], p["level"], p["bytes"]) == (H, W, None, len(want_bytes))
    px, info = codec.decode_images(net, files, ref=img.unsqueeze(0))
    assert px.dtype == torch.uint8 and tuple(px.shape) == (1, H, W, 3) and torch.equal(px.cpu(), want_px)
    sq = int(((want_px.numpy().astype(np.int64) - img.numpy().astype(np.int64)) ** 2).sum())
    assert info[0]["sq_err"] == sq and info[0]["psnr"] == codec.psnr_from_sq_err(sq, 3 * H * W)
    assert (info[0]["H"], info[0]["W"], info[0]["level"], info[0]["bytes"]) == (H, W, None, len(want_bytes))
    assert info[0]["bpp"] == 8.0 * len(want_bytes) / (H * W)
    assert sq > 0 and abs(info[0]["psnr"] - 10 * np.log10(255.0 ** 2 / (sq / (3 * H * W)))) < 1e-9
    plain, _ = codec.decode_images(net, files)
    assert torch.equal(plain, px)
    # the C ABI's one-image calls
    data, cpx = _c_abi_round_trip(net, img, 1.0, -1, None)
    assert data == want_bytes and torch.equal(cpx, want_px[0])
    assert not any(net.range_fallbacks(reset=True).values())


def test_batch_equals_single_calls(net_s):
    net = net_s
    net.range_fallbacks(reset=True)
    H, W = 100, 150
    batch = torch.stack([_u8_image(H, W, 3), _u8_image(H, W, 4)])
    files = codec.encode_images(net, batch)
    singles = [codec.encode_images(net, batch[b])[0] for b in range(2)]
    assert files == singles and files[0] != files[1]
    px, info = codec.decode_images(net, files, ref=batch)
    one = [codec.decode_images(net, [f], ref=batch[b:b + 1]) for b, f in enumerate(files)]
    assert torch.equal(px, torch.cat([o[0] for o in one]))
    assert info == [o[1][0] for o in one]
    # files of one padded size but different H x W: each in the top-left of a zeroed canvas
    small = codec.encode_images(net, batch[1, :90, :131])[0]
    mixed, minfo = codec.decode_images(net, [files[0], small])
    assert tuple(mixed.shape) == (2, H, W, 3) and torch.equal(mixed[0], px[0])
    assert torch.equal(mixed[1, :90, :131], codec.decode_images(net, [small])[0][0])
    assert int(mixed[1, 90:].sum()) == 0 and int(mixed[1, :, 131:].sum()) == 0
    assert (minfo[1]["H"], minfo[1]["W"]) == (90, 131)
    with pytest.raises(ValueError, match="padded size"):
        codec.decode_images(net, [files[0], codec.encode_images(net, batch[0, :64, :64])[0]])
    assert not any(net.range_fallbacks(reset=True).values())


def test_vbr_level_round_trips_in_the_header(net_vbr):
    net = net_vbr
    net.range_fallbacks(reset=True)
    H, W, level = 100, 150, 3
    img = _u8_image(H, W, 5)
    want_bytes, want_px = _reference_path(net, img, s=level)
    files = codec.encode_images(net, img, level=level)
    assert files[0] == want_bytes
    assert codec.peek(files[0], vbr=True, n_levels=net.levels)["level"] == level
    px, info = codec.decode_images(net, files)
    assert torch.equal(px.cpu(), want_px) and info[0]["level"] == level
    with pytest.raises(ValueError):
        codec.encode_images(net, img)  # a VBR file needs its level
    with pytest.raises(_lib.MlicError, match="level"):
        codec.peek(files[0], vbr=True, n_levels=level)
    gains = [float(net._vbr_scales(1, s=l, coder=True)[0]) for l in range(net.levels)]
    data, cpx = _c_abi_round_trip(net, img, gains[level], level, gains)
    assert data == want_bytes and torch.equal(cpx, want_px[0])
    assert not any(net.range_fallbacks(reset=True).values())
