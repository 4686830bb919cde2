"""Rate-constrained encoding on the GPU: the prefilter kernel (csrc/image_io.hip, mlic_image_blur3_pad) against
the CPU restatement bit for bit, and the budget loop of codec.encode_images, the VBR level choice, the C ABI's
mlic_encode_image_u8_budget and bitstream.code_image(max_bpp=) against loops written here from the parts.

Every comparison is exact.  The kernel's destination is pre-filled with NaN and sits between sentinel guard words
inside one allocation; its source carries NaN in the padding, which must not reach the image (a tap outside the
H x W image is 0 whatever the buffer holds there).  Nothing here assumes that filtering lowers the rate of a
synthetic-weight model: whatever the sizes are, the library's loop and the manual one must agree."""
import ctypes as C

import numpy as np
import pytest
import torch

from mlic_amd import _lib, bitstream, codec, get_model, synthetic

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD, FSENT = 512, 0x5A5A5A5A
W9 = [0.05, 0.1, 0.15, 0.2, -0.25, 0.3, 0.35, 0.4, 0.45]  # non-symmetric: a transposed tap order shows


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _pad64(n):
    return (n + 63) // 64 * 64


def _source(B, H, W, seed=0):
    """fp32 [B,3,Hp,Wp] on the CPU: u8 / 255 inside the image, NaN in the padding."""
    r = np.random.default_rng(1000 * H + W + seed)
    u8 = torch.from_numpy(r.integers(0, 256, (B, H, W, 3), dtype=np.uint8))
    x = codec.ingest_u8(u8, "hwc").clone()
    x[:, :, H:] = float("nan")
    x[:, :, :, W:] = float("nan")
    return x


def run_blur(x_cpu, H, W, index=None, w9=None, shift=0):
    """mlic_image_blur3_pad on a device copy of x_cpu -> fp32 [n,3,Hp,Wp] on the CPU.  shift: source and
    destination start this many floats past a 16-byte boundary (0: the float4 form, else the scalar form)."""
    B, _, Hp, Wp = x_cpu.shape
    n = B if index is None else len(index)
    sbuf = torch.empty(x_cpu.numel() + 4, dtype=torch.float32, device=DEV)
    src = sbuf[shift:shift + x_cpu.numel()]
    src.copy_(x_cpu.reshape(-1))
    cnt = n * 3 * Hp * Wp
    buf = torch.empty(GUARD + cnt + GUARD, dtype=torch.float32, device=DEV)
    buf.view(torch.int32).fill_(FSENT)
    dst = buf[GUARD + shift:GUARD + shift + cnt]
    dst.fill_(float("nan"))
    assert src.data_ptr() % 16 == 4 * shift and dst.data_ptr() % 16 == 4 * shift
    ix = None if index is None else torch.tensor(index, dtype=torch.int32, device=DEV)
    w = None if w9 is None else (C.c_float * 9)(*w9)
    _lib.call("mlic_image_blur3_pad", _stream(), _p(src), None if ix is None else _p(ix), n, H, W, Hp, Wp, w, _p(dst))
    torch.cuda.synchronize()
    g = buf.view(torch.int32)
    assert bool((g[:GUARD + shift] == FSENT).all()) and bool((g[GUARD + shift + cnt:] == FSENT).all()), "wrote outside dst"
    return dst.view(n, 3, Hp, Wp).cpu()


def _check(got, x, H, W, index=None, w9=None):
    want = codec.blur3_pad(x, H, W, index=index, weights=w9)
    assert not torch.isnan(want).any()
    assert not torch.isnan(got).any(), "an element was not written, or the padding leaked into the image"
    assert got.shape == want.shape and torch.equal(_bits(got), _bits(want))
    assert int(_bits(got[:, :, H:]).abs().sum()) == 0 and int(_bits(got[:, :, :, W:]).abs().sum()) == 0


# ------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("shape", [(1, 1), (64, 64), (65, 70), (3, 130)] + [(2, w) for w in (1, 2, 3, 4, 5, 63, 64, 65)])
def test_blur_kernel_matches_the_cpu_loop_bitwise(shape):
    H, W = shape
    x = _source(2, H, W)
    for shift in (0, 1):
        _check(run_blur(x, H, W, shift=shift), x, H, W)
        _check(run_blur(x, H, W, w9=W9, shift=shift), x, H, W, w9=W9)


def test_blur_kernel_gathers_duplicates_and_compacts():
    H, W = 130, 257
    x = _source(3, H, W)
    assert tuple(x.shape) == (3, 3, 192, 320)
    for shift in (0, 3):
        got = run_blur(x, H, W, index=[2, 0, 2], shift=shift)
        _check(got, x, H, W, index=[2, 0, 2])
        assert torch.equal(_bits(got[0]), _bits(got[2])) and not torch.equal(got[0], got[1])
    _check(run_blur(x, H, W, index=[1], w9=W9), x, H, W, index=[1], w9=W9)


def test_blur_refuses_overlap_and_launches_nothing():
    H, W, Hp, Wp = 60, 64, 64, 64
    cnt = 2 * 3 * Hp * Wp
    buf = torch.empty(3 * cnt, dtype=torch.float32, device=DEV)
    buf.view(torch.int32).fill_(FSENT)
    for s_off, d_off in ((0, 0), (0, cnt - 4), (cnt - 4, 0), (8, 4)):
        with pytest.raises(_lib.MlicError, match="dst overlaps src"):
            _lib.call("mlic_image_blur3_pad", _stream(), _p(buf[s_off:]), None, 2, H, W, Hp, Wp, None, _p(buf[d_off:]))
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int32) == FSENT).all()), "a refused call wrote"
    # ranges that only touch are fine
    x = _source(2, H, W)
    buf[:cnt].copy_(x.reshape(-1))
    _lib.call("mlic_image_blur3_pad", _stream(), _p(buf), None, 2, H, W, Hp, Wp, None, _p(buf[cnt:]))
    torch.cuda.synchronize()
    _check(buf[cnt:2 * cnt].view(2, 3, Hp, Wp).cpu(), x, H, W)
    assert bool((buf[2 * cnt:].view(torch.int32) == FSENT).all())


def test_python_blur_on_the_device():
    H, W = 65, 70
    x = _source(3, H, W)
    xd = x.to(DEV)
    for index in (None, [2, 0, 2], torch.tensor([1, 1], device=DEV)):
        got = codec.blur3_pad(xd, H, W, index=index)
        assert got.is_cuda and got.is_contiguous()
        _check(got.cpu(), x, H, W, index=index if index is None or isinstance(index, list) else index.tolist())
    # the library's default weights are BLUR3_WEIGHTS
    assert torch.equal(_bits(codec.blur3_pad(xd, H, W, weights=codec.BLUR3_WEIGHTS)), _bits(codec.blur3_pad(xd, H, W)))
    _check(codec.blur3_pad(xd, H, W, weights=W9).cpu(), x, H, W, w9=W9)
    assert torch.equal(_bits(xd.cpu()), _bits(x))  # the source is only read
    with pytest.raises(ValueError):
        codec.blur3_pad(xd, H, W, index=[3])


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
    x = synthetic.synth_image(_pad64(H), _pad64(W), seed)[0, :, :H, :W]
    return torch.round(x * 255).to(torch.uint8).permute(1, 2, 0).contiguous()


def _bpp(f, H, W):
    return 8.0 * len(f) / (H * W)


def _manual_loop(net, img, max_bpp, max_passes, level=None):
    """The loop written from the parts, one image: (file, passes, strings, shape, per-pass sizes)."""
    H, W, _ = img.shape
    kw = {} if level is None else {"s": level}
    x = codec.ingest_u8(img.to(DEV), "hwc")
    k, sizes = 0, []
    while True:
        out = net.compress(x, **kw)
        f = codec.write_container(H, W, out["shape"], out["strings"][0][0], out["strings"][1][0], level)
        sizes.append(len(f))
        if not _bpp(f, H, W) > max_bpp or k >= max_passes:
            return f, k, out["strings"], out["shape"], sizes
        x = codec.blur3_pad(x, H, W)
        k += 1


@pytest.mark.parametrize("size", [(65, 129), (128, 128)])
def test_budget_loop_equals_the_manual_loop(net_s, size):
    H, W = size
    net = net_s
    net.range_fallbacks(reset=True)
    img = _u8_image(H, W, 3)
    plain = codec.encode_images(net, img)
    b0 = _bpp(plain[0], H, W)
    budget = b0 * (1 - 1e-6)
    files, info = codec.encode_images(net, img, max_bpp=budget, max_passes=3, return_info=True)
    f, k, strings, shape, sizes = _manual_loop(net, img, budget, 3)
    print(f"{H} x {W}: file bytes per pass {sizes}")
    assert sizes[0] == len(plain[0])
    assert files == [f] and info[0]["passes"] == k and k >= 1
    assert info[0] == {"bytes": len(f), "bpp": _bpp(f, H, W), "passes": k, "level": None, "met": _bpp(f, H, W) <= budget}
    px, _ = codec.decode_images(net, files)
    want = bitstream.to_u8(net.decompress(strings, shape)["x_hat"][:, :, :H, :W]).permute(0, 2, 3, 1)
    assert torch.equal(px, want)
    assert not any(net.range_fallbacks(reset=True).values())


def test_budget_edges(net_s):
    net = net_s
    net.range_fallbacks(reset=True)
    H, W = 65, 129
    img = _u8_image(H, W, 4)
    plain = codec.encode_images(net, img)
    files, info = codec.encode_images(net, img, max_bpp=1e9, return_info=True)
    assert files == plain and info[0]["passes"] == 0 and info[0]["met"] is True
    files, info = codec.encode_images(net, img, max_bpp=1e-9, max_passes=2, return_info=True)
    assert info[0]["passes"] == 2 and info[0]["met"] is False
    assert files[0] == _manual_loop(net, img, 1e-9, 2)[0]
    p = codec.peek(files[0])
    assert (p["H"], p["W"], p["bytes"]) == (H, W, len(files[0]))
    px, dinfo = codec.decode_images(net, files)
    assert tuple(px.shape) == (1, H, W, 3) and dinfo[0]["bytes"] == len(files[0])
    assert not any(net.range_fallbacks(reset=True).values())


def test_batch_under_one_budget_equals_single_calls(net_s):
    net = net_s
    net.range_fallbacks(reset=True)
    H, W = 100, 150
    batch = torch.stack([_u8_image(H, W, s) for s in (3, 4, 5)])
    plain = [_bpp(f, H, W) for f in codec.encode_images(net, batch)]
    print(f"unconstrained bpp {plain}")
    assert len(set(plain)) > 1
    budget = (min(plain) + max(plain)) / 2  # between their unconstrained sizes
    files, info = codec.encode_images(net, batch, max_bpp=budget, max_passes=2, return_info=True)
    for b in range(3):
        f1, i1 = codec.encode_images(net, batch[b], max_bpp=budget, max_passes=2, return_info=True)
        assert files[b] == f1[0] and info[b] == i1[0], b
    print(f"passes {[i['passes'] for i in info]}, met {[i['met'] for i in info]}")
    assert min(i["passes"] for i in info) == 0 and max(i["passes"] for i in info) >= 1
    assert not any(net.range_fallbacks(reset=True).values())


def test_vbr_level_choice(net_vbr):
    net = net_vbr
    net.range_fallbacks(reset=True)
    H, W = 128, 128
    img = _u8_image(H, W, 5)
    by_level = [codec.encode_images(net, img, level=l)[0] for l in range(net.levels)]
    bpps = [_bpp(f, H, W) for f in by_level]
    print(f"bpp by level {bpps}")
    budget = bpps[2]
    best = max(l for l in range(net.levels) if bpps[l] <= budget)
    files, info = codec.encode_images(net, img, level="auto", max_bpp=budget, return_info=True)
    assert files[0] == by_level[best] and info[0]["level"] == best and info[0]["passes"] == 0 and info[0]["met"]
    assert codec.peek(files[0], vbr=True, n_levels=net.levels)["level"] == best
    # below level 0's size: level 0, and on into the filter loop
    low = bpps[0] * (1 - 1e-6)
    files, info = codec.encode_images(net, img, level="auto", max_bpp=low, max_passes=1, return_info=True)
    assert info[0]["level"] == 0 and info[0]["passes"] == 1
    assert codec.peek(files[0], vbr=True, n_levels=net.levels)["level"] == 0
    assert files[0] == _manual_loop(net, img, low, 1, level=0)[0]
    # an integer level runs the loop at that level
    files, info = codec.encode_images(net, img, level=3, max_bpp=bpps[3] * (1 - 1e-6), max_passes=1, return_info=True)
    assert (info[0]["level"], info[0]["passes"]) == (3, 1)
    assert files[0] == _manual_loop(net, img, bpps[3] * (1 - 1e-6), 1, level=3)[0]
    assert not any(net.range_fallbacks(reset=True).values())


def test_c_abi_budget_encode(net_vbr, net_s):
    for net, level in ((net_s, -1), (net_vbr, 1)):
        net.range_fallbacks(reset=True)
        H, W = 65, 129
        img = _u8_image(H, W, 6)
        lv = None if level < 0 else level
        scale = 1.0 if lv is None else float(net._vbr_scales(1, s=lv, coder=True)[0])
        budget = _bpp(codec.encode_images(net, img, level=lv)[0], H, W) * (1 - 1e-6)
        files, info = codec.encode_images(net, img, level=lv, max_bpp=budget, max_passes=2, return_info=True)
        h = net._handle
        rgb = img.to(DEV)
        s3 = (C.c_int64 * 3)(*rgb.stride())
        n, k = C.c_size_t(), C.c_int(-1)
        _lib.call("mlic_encode_image_u8_budget", h, _stream(), _p(rgb), s3, H, W, scale, level, budget, 2, None, 0,
                  C.byref(n), C.byref(k))
        assert n.value == len(files[0]) and k.value == info[0]["passes"] >= 1
        out = C.create_string_buffer(n.value)
        k2 = C.c_int(-1)
        with pytest.raises(_lib.MlicError, match="buffer too small"):
            _lib.call("mlic_encode_image_u8_budget", h, _stream(), None, None, 0, 0, 1.0, -1, 0.0, 0, out, n.value - 1,
                      C.byref(n), C.byref(k2))
        _lib.call("mlic_encode_image_u8_budget", h, _stream(), None, None, 0, 0, 1.0, -1, 0.0, 0, out, n.value,
                  C.byref(n), C.byref(k2))
        assert C.string_at(out, n.value) == files[0] and k2.value == k.value
        # a budget the first file meets: the plain encode's bytes, no pass
        _lib.call("mlic_encode_image_u8_budget", h, _stream(), _p(rgb), s3, H, W, scale, level, 1e9, 2, None, 0,
                  C.byref(n), C.byref(k))
        out = C.create_string_buffer(n.value)
        _lib.call("mlic_encode_image_u8", h, _stream(), None, None, 0, 0, 1.0, -1, out, n.value, C.byref(n))
        assert k.value == 0 and C.string_at(out, n.value) == codec.encode_images(net, img, level=lv)[0]
        for bad_bpp, bad_passes, word in ((0.0, 2, "max_bpp"), (float("nan"), 2, "max_bpp"), (float("inf"), 2, "max_bpp"),
                                          (1.0, -1, "max_passes")):
            with pytest.raises(_lib.MlicError, match=word):
                _lib.call("mlic_encode_image_u8_budget", h, _stream(), _p(rgb), s3, H, W, scale, level, bad_bpp,
                          bad_passes, None, 0, C.byref(n), C.byref(k))
        assert not any(net.range_fallbacks(reset=True).values())


def test_code_image_budget_agrees_with_encode_images(net_s):
    net = net_s
    net.range_fallbacks(reset=True)
    H, W = 65, 129
    img = _u8_image(H, W, 3)
    x = img.permute(2, 0, 1).unsqueeze(0).float().div(255).contiguous().to(DEV)
    plain = bitstream.code_image(net, x)
    assert set(plain) == {"H", "W", "bytes", "bpp", "psnr", "enc_s", "dec_s", "x_hat"}
    budget = plain["bpp"] * (1 - 1e-6)
    r = bitstream.code_image(net, x, max_bpp=budget, max_passes=3)
    files, info = codec.encode_images(net, img, max_bpp=budget, max_passes=3, return_info=True)
    assert set(r) == set(plain) | {"passes", "met"}
    assert (r["bytes"], r["bpp"], r["passes"], r["met"]) == (len(files[0]), info[0]["bpp"], info[0]["passes"], info[0]["met"])
    assert tuple(r["x_hat"].shape) == (1, 3, H, W)
    assert not any(net.range_fallbacks(reset=True).values())
