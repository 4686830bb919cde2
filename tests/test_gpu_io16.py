"""9..16-bit sample I/O on the GPU: the four kernels of csrc/image_io16.hip against the torch restatements of
codec.py (which tests/test_io16_cpu.py holds to numpy and to the float64 oracle), bit for bit, over depth x sample
alignment x layouts x shapes (and, for Y'CbCr, subsampling x siting with a (matrix, range) pair per combination,
rotating through all six); the stride forms against each other; the words around the destinations; the squared
error, which needs 64 bits from the second sample on; and images -> file bytes -> images through codec.py and the C
ABI's one-image calls.

Every comparison is exact.  Every fp32 destination is NaN-filled between guard words and every sample destination
sits inside a sentinel-filled allocation that is checked after the call.  uint16 tensors are only moved and viewed
on the device: the test handles them as int16 there.  Shapes as in tests/test_gpu_yuv.py."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from mlic_amd import _lib, codec, get_model, synthetic

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD, SENT, FSENT = 512, 0x5AA5, 0x5A5A5A5A
SHAPES = [(1, 1), (2, 2), (3, 5), (37, 51), (6, 259), (5, 513), (70, 130)]
DEPTHS = [8, 10, 12, 16]
SETS = [(m, f) for m in ("bt601", "bt709", "bt2020") for f in (False, True)]
GEOM = [((1, 1), "left"), ((2, 1), "left"), ((2, 1), "centre"), ((2, 2), "left"), ((2, 2), "centre")]
RGB_LAYOUTS = ["hwc", "chw", "rowpad", "crop", "batch"]
YUV_LAYOUTS = ["i420", "nv12", "nv21", "rowpad", "crop", "batch"]


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _i16(t):
    """A uint16 CPU tensor as int16 (the same bits), for the device."""
    return t.view(torch.int16)


def _words(t):
    """An int16 tensor from the device -> int32 word values on the CPU."""
    return t.cpu().to(torch.int32) & 0xFFFF


def _w32(t):
    """A uint16 CPU tensor -> int32 word values."""
    return t.to(torch.int32)


def _rand_words(r, shape, d, msb):
    """uint16 words (numpy) whose samples cover [0, maxv]: MSB-aligned words carry random low bits, LSB-aligned
    ones are above maxv here and there (they read as maxv)."""
    maxv = (1 << d) - 1
    s = r.integers(0, maxv + 1, shape, dtype=np.int64)
    if msb:
        w = (s << (16 - d)) | r.integers(0, 1 << (16 - d), shape, dtype=np.int64)
    else:
        w = np.where(r.random(shape) < 0.05, r.integers(maxv, 65536, shape, dtype=np.int64), s)
    return w.astype(np.uint16)


def _odd(shape):
    """A SENT-filled int16 device tensor of this shape whose first word sits at an address = 2 mod 4, and its whole
    allocation."""
    n = int(np.prod(shape))
    buf = torch.full((n + 1,), SENT, dtype=torch.int16, device=DEV)
    assert buf.data_ptr() % 4 == 0
    return buf[1:].view(shape), buf


def _clean(views, bufs, what):
    for v in views:
        v.fill_(SENT)
    seen = set()
    for b in bufs:
        if b.data_ptr() not in seen:
            seen.add(b.data_ptr())
            assert bool((b == SENT).all()), f"egress wrote outside its destination ({what})"


def _x_hat(B, H, W, seed=0):
    """fp32 [B,3,Hp,Wp] on the CPU: values around [0, 1] with NaN, infinities, signed zeros and the clamp's edges."""
    Hp, Wp = (H + 63) // 64 * 64, (W + 63) // 64 * 64
    r = np.random.default_rng(7000 * H + W + seed)
    x = r.uniform(-0.1, 1.1, (B, 3, Hp, Wp)).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 1.0000001, -1e-7, 0.5], np.float32)
    flat = x.reshape(-1)
    at = r.choice(flat.size, min(flat.size, 4 * special.size), replace=False)
    flat[at] = np.resize(special, at.size)
    x[:, :, H:] = np.nan  # the padding is never read
    x[:, :, :, W:] = np.nan
    return torch.from_numpy(x)


def _fp32_dst(B, H, W):
    Hp, Wp = (H + 63) // 64 * 64, (W + 63) // 64 * 64
    n = B * 3 * Hp * Wp
    buf = torch.empty(GUARD + n + GUARD, dtype=torch.float32, device=DEV)
    buf.view(torch.int32).fill_(FSENT)
    dst = buf[GUARD:GUARD + n]
    dst.fill_(float("nan"))
    return buf, dst, n, Hp, Wp


def _guards_ok(buf, n):
    g = buf.view(torch.int32)
    return bool((g[:GUARD] == FSENT).all()) and bool((g[GUARD + n:] == FSENT).all())


@pytest.fixture
def forced_path():
    def force(v):
        _lib.call("mlic_set_kernel_option", b"image_io_path", v)
    yield force
    _lib.call("mlic_set_kernel_option", b"image_io_path", -1)


# ------------------------------------------------------------------------------------------------------ RGB
def _rgb_alloc(B, H, W, layout):
    """An int16 device view of an image batch arranged as `layout`, the layout name codec uses for it ("hwc" /
    "chw"), and the allocations."""
    if layout == "hwc":
        t, buf = _odd((B, H, W, 3))
        return t, "hwc", [buf]
    if layout == "chw":
        t, buf = _odd((B, 3, H, W))
        return t, "chw", [buf]
    if layout == "rowpad":  # a pitch greater than the width, interleaved
        t, buf = _odd((B, H, W + 3, 3))
        return t[:, :, :W], "hwc", [buf]
    if layout == "crop":  # a planar window whose first sample sits at an address = 2 mod 4
        t, buf = _odd((B, 3, H + 3, W + 4))
        v = t[:, :, 1:H + 1, 2:W + 2]
        if v.data_ptr() % 4 != 2:
            v = t[:, :, 1:H + 1, 1:W + 1]
        assert v.data_ptr() % 4 == 2
        return v, "chw", [buf]
    if layout == "batch":  # the RGB of RGBA words in a batch with a gap: no fast form
        t, buf = _odd((B, 2, H, W, 4))
        return t[:, 1, :, :, :3], "hwc", [buf]
    raise AssertionError(layout)


def _strides4(t, lay):
    s = t.stride()
    return (s[0], s[1], s[2], s[3]) if lay == "hwc" else (s[0], s[2], s[3], s[1])


def _rgb_place(img_hwc, layout):
    """uint16 CPU [B,H,W,3] -> (int16 device view in `layout`, "hwc" / "chw")."""
    B, H, W, _ = img_hwc.shape
    v, lay, _ = _rgb_alloc(B, H, W, layout)
    src = _i16(img_hwc).to(DEV)
    v.copy_(src if lay == "hwc" else src.permute(0, 3, 1, 2))
    return v, lay


def run_ingest_u16(v, lay, d, msb):
    B = v.size(0)
    H, W = (v.size(1), v.size(2)) if lay == "hwc" else (v.size(2), v.size(3))
    buf, dst, n, Hp, Wp = _fp32_dst(B, H, W)
    _lib.call("mlic_image_ingest_u16", _stream(), _p(v), (C.c_int64 * 4)(*_strides4(v, lay)), d, int(msb), B, H, W,
              _p(dst), Hp, Wp)
    torch.cuda.synchronize()
    assert _guards_ok(buf, n), "ingest wrote outside dst"
    return dst.view(B, 3, Hp, Wp).cpu()


def run_egress_u16(x, H, W, d, msb, layout, ref=None):
    """-> (int32 words [B,H,W,3] on the CPU, sq_err list or None)."""
    B = x.size(0)
    v, lay, bufs = _rgb_alloc(B, H, W, layout)
    sq = None if ref is None else torch.full((B,), -1, dtype=torch.int64, device=DEV)
    _lib.call("mlic_image_egress_u16", _stream(), _p(x), (C.c_int64 * 3)(*x.stride()[:3]), B, H, W, d, int(msb), _p(v),
              (C.c_int64 * 4)(*_strides4(v, lay)), None if ref is None else _p(ref[0]),
              None if ref is None else (C.c_int64 * 4)(*_strides4(*ref)), None if sq is None else _p(sq))
    torch.cuda.synchronize()
    out = _words(v if lay == "hwc" else v.permute(0, 2, 3, 1))
    _clean([v], bufs, layout)
    return out, None if sq is None else sq.cpu().tolist()


@pytest.mark.parametrize("d", DEPTHS)
def test_rgb_ingest_kernel_equals_the_restatement_bitwise(d):
    for msb, (H, W) in itertools.product((False, True), SHAPES):
        r = np.random.default_rng(100 * H + W + d)
        img = torch.from_numpy(_rand_words(r, (2, H, W, 3), d, msb))
        want = codec.ingest_u16(img, d, "hwc", msb)
        assert not want.is_cuda
        for layout in RGB_LAYOUTS:
            got = run_ingest_u16(*_rgb_place(img, layout), d, msb)
            assert not torch.isnan(got).any(), (d, msb, H, W, layout)
            assert _same_bits(got, want), (d, msb, H, W, layout)
            assert int(got[:, :, H:].view(torch.int32).abs().sum()) == 0
            assert int(got[:, :, :, W:].view(torch.int32).abs().sum()) == 0


@pytest.mark.parametrize("d", DEPTHS)
def test_rgb_egress_kernel_equals_the_restatement_bitwise_with_sq_err(d):
    for msb, (H, W) in itertools.product((False, True), SHAPES):
        r = np.random.default_rng(300 * H + W + d)
        x = _x_hat(2, H, W)
        ref = torch.from_numpy(_rand_words(r, (2, H, W, 3), d, msb))
        want, wsq = codec.egress_u16(x, H, W, d, "hwc", msb, ref=ref)
        ws = codec.samples_of_words(want, d, msb).to(torch.int64)
        own = ((ws - codec.samples_of_words(ref, d, msb).to(torch.int64)) ** 2).flatten(1).sum(1).tolist()
        assert wsq.tolist() == own
        xd = x.to(DEV)
        for k, layout in enumerate(RGB_LAYOUTS):
            rd = _rgb_place(ref, RGB_LAYOUTS[(k + 1) % len(RGB_LAYOUTS)])  # laid out differently from the output
            got, sq = run_egress_u16(xd, H, W, d, msb, layout, ref=rd)
            assert torch.equal(got, _w32(want)), (d, msb, H, W, layout)
            assert sq == own, (d, msb, H, W, layout)
            plain, none = run_egress_u16(xd, H, W, d, msb, layout)
            assert none is None and torch.equal(plain, got)
            if msb:
                assert int((got & ((1 << (16 - d)) - 1)).sum()) == 0


def test_rgb_sq_err_needs_64_bits_from_the_second_sample():
    # all-65535 against all-0 at depth 16: each squared difference is just under 2^32
    for (H, W), layout in itertools.product([(2, 2), (70, 130)], RGB_LAYOUTS):
        x = torch.ones(2, 3, (H + 63) // 64 * 64, (W + 63) // 64 * 64, device=DEV)
        ref = _rgb_place(torch.zeros(2, H, W, 3, dtype=torch.int16).view(torch.uint16), layout)
        got, sq = run_egress_u16(x, H, W, 16, False, "hwc", ref=ref)
        assert int(got.min()) == 65535
        assert sq == [3 * H * W * 65535 ** 2] * 2, (H, W, layout)


def test_rgb_stride_forms_agree(forced_path):
    for d, msb, (H, W) in [(10, True, (5, 513)), (16, False, (70, 130)), (12, False, (3, 5))]:
        r = np.random.default_rng(H + W)
        img = torch.from_numpy(_rand_words(r, (2, H, W, 3), d, msb))
        x = _x_hat(2, H, W, seed=2).to(DEV)
        ref = _rgb_place(torch.from_numpy(_rand_words(r, (2, H, W, 3), d, msb)), "rowpad")
        for layout, fast in (("hwc", 1), ("rowpad", 1), ("chw", 2), ("crop", 2)):
            placed = _rgb_place(img, layout)
            forced_path(-1)
            a = run_ingest_u16(*placed, d, msb)
            ea, sa = run_egress_u16(x, H, W, d, msb, layout, ref=ref)
            forced_path(fast)  # must be that fast form: refused otherwise
            a2 = run_ingest_u16(*placed, d, msb)
            forced_path(0)  # the general form
            b = run_ingest_u16(*placed, d, msb)
            eb, sb = run_egress_u16(x, H, W, d, msb, layout, ref=ref)
            forced_path(-1)
            assert _same_bits(a, b) and _same_bits(a, a2), (d, H, W, layout)
            assert sa == sb and torch.equal(ea, eb), (d, H, W, layout)
    forced_path(1)
    with pytest.raises(_lib.MlicError, match="column stride 3"):
        run_ingest_u16(*_rgb_place(img, "batch"), d, msb)
    forced_path(2)
    with pytest.raises(_lib.MlicError, match="column stride 1"):
        run_ingest_u16(*_rgb_place(img, "hwc"), d, msb)


# --------------------------------------------------------------------------------------------------- Y'CbCr
def _fmt(sub, site, matrix, full, d, msb):
    """The format of a raw call at depth d (a YuvFormat cannot say BT.2020 at depth 8: the restatements and the C
    calls take the depth as an argument, so a depth-9 format stands in as the descriptor)."""
    if d == 8:
        return codec.YuvFormat(sub=sub, matrix=matrix, full_range=full, site_x=site, depth=9 if matrix == "bt2020" else 8)
    return codec.YuvFormat(sub=sub, matrix=matrix, full_range=full, site_x=site, depth=d, msb=msb)


def _frames(B, H, W, fmt, d, msb, seed=0):
    """(y, cb, cr) uint16 CPU tensors."""
    r = np.random.default_rng(1000 * H + W + seed + d)
    ch, cw = fmt.chroma_size(H, W)
    return tuple(torch.from_numpy(_rand_words(r, s, d, msb)) for s in ((B, H, W), (B, ch, cw), (B, ch, cw)))


def _yuv_alloc(B, H, W, fmt, layout):
    """int16 device views (y, cb, cr) of shapes [B,H,W], [B,ch,cw] x 2 arranged as `layout`, and their allocations
    (tests/test_gpu_yuv.py's _alloc in words)."""
    ch, cw = fmt.chroma_size(H, W)
    if layout == "i420":  # Y, Cb, Cr planes back to back, the first word at an address = 2 mod 4
        n = H * W + 2 * ch * cw
        t, buf = _odd((B, n))
        return (t[:, :H * W].view(B, H, W), t[:, H * W:H * W + ch * cw].view(B, ch, cw),
                t[:, H * W + ch * cw:].view(B, ch, cw)), [buf]
    if layout in ("nv12", "nv21"):  # Y, then interleaved chroma rows: P010 and its swapped twin
        n = H * W + 2 * ch * cw
        t, buf = _odd((B, n))
        uv = t[:, H * W:].view(B, ch, cw, 2)
        a, b = uv[..., 0], uv[..., 1]
        return (t[:, :H * W].view(B, H, W),) + ((a, b) if layout == "nv12" else (b, a)), [buf]
    if layout == "rowpad":  # a pitch greater than the width
        ty, by = _odd((B, H, W + 5))
        tb, bb = _odd((B, ch, cw + 3))
        tr, br = _odd((B, ch, cw + 7))
        return (ty[..., :W], tb[..., :cw], tr[..., :cw]), [by, bb, br]
    if layout == "crop":  # windows of larger planes, starting at an address = 2 mod 4
        out, bufs = [], []
        for h, w in ((H, W), (ch, cw), (ch, cw)):
            t, buf = _odd((B, h + 3, w + 4))
            v = t[:, 1:h + 1, 2:w + 2]
            if v.data_ptr() % 4 != 2:
                v = t[:, 1:h + 1, 1:w + 1]
            assert v.data_ptr() % 4 == 2
            out.append(v)
            bufs.append(buf)
        return tuple(out), bufs
    if layout == "batch":  # a non-contiguous image stride, column stride 3 on Cr (no fast form)
        ty, by = _odd((B, 2, H, W))
        tb, bb = _odd((B, 3, ch, cw))
        tr, br = _odd((B, ch, cw, 3))
        return (ty[:, 1], tb[:, 2], tr[..., 1]), [by, bb, br]
    raise AssertionError(layout)


def _yuv_place(planes, fmt, layout):
    B, H, W = planes[0].shape
    views, _ = _yuv_alloc(B, H, W, fmt, layout)
    for v, p in zip(views, planes):
        assert tuple(v.shape) == tuple(p.shape)
        v.copy_(_i16(p).to(DEV))
    return views


def _plane_args(planes):
    out = []
    for t in planes:
        out += [_p(t), (C.c_int64 * 3)(*t.stride())]
    return out


def run_ingest_yuv16(planes, fmt, d, msb):
    B, H, W = planes[0].shape
    buf, dst, n, Hp, Wp = _fp32_dst(B, H, W)
    desc = fmt.desc()
    _lib.call("mlic_image_ingest_yuv16", _stream(), *_plane_args(planes), C.byref(desc), d, int(msb), B, H, W, _p(dst),
              Hp, Wp)
    torch.cuda.synchronize()
    assert _guards_ok(buf, n), "ingest wrote outside dst"
    return dst.view(B, 3, Hp, Wp).cpu()


def run_egress_yuv16(x, H, W, fmt, d, msb, layout, ref=None):
    """-> ((y, cb, cr) int32 words on the CPU, sq_err list or None)."""
    B = x.size(0)
    views, bufs = _yuv_alloc(B, H, W, fmt, layout)
    sq = None if ref is None else torch.full((B, 3), -1, dtype=torch.int64, device=DEV)
    desc = fmt.desc()
    rargs = [None] * 6 if ref is None else _plane_args(ref)
    _lib.call("mlic_image_egress_yuv16", _stream(), _p(x), (C.c_int64 * 3)(*x.stride()[:3]), B, H, W, C.byref(desc), d,
              int(msb), *_plane_args(views), *rargs, None if sq is None else _p(sq))
    torch.cuda.synchronize()
    out = tuple(_words(v) for v in views)
    _clean(views, bufs, layout)
    return out, None if sq is None else sq.cpu().tolist()


def _cases():
    """(d, msb, shape, (matrix, range)): one pair per combination, rotating through all six."""
    for i, (d, msb, hw) in enumerate(itertools.product(DEPTHS, (False, True), SHAPES)):
        yield d, msb, hw, SETS[i % len(SETS)]


@pytest.mark.parametrize("sub,site", GEOM)
def test_yuv_ingest_kernel_equals_the_restatement_bitwise(sub, site):
    seen = set()
    for d, msb, (H, W), (matrix, full) in _cases():
        seen.add((matrix, full))
        fmt = _fmt(sub, site, matrix, full, d, msb)
        planes = _frames(2, H, W, fmt, d, msb)
        want = codec._ingest_yuv16_cpu(*planes, fmt, d, msb)
        assert not torch.isnan(want).any()
        for layout in YUV_LAYOUTS:
            got = run_ingest_yuv16(_yuv_place(planes, fmt, layout), fmt, d, msb)
            assert not torch.isnan(got).any(), (fmt, d, msb, H, W, layout)
            assert _same_bits(got, want), (fmt, d, msb, H, W, layout)
            assert int(got[:, :, H:].view(torch.int32).abs().sum()) == 0
            assert int(got[:, :, :, W:].view(torch.int32).abs().sum()) == 0
    assert len(seen) == 6


@pytest.mark.parametrize("sub,site", GEOM)
def test_yuv_egress_kernel_equals_the_restatement_bitwise_with_sq_err(sub, site):
    for d, msb, (H, W), (matrix, full) in _cases():
        fmt = _fmt(sub, site, matrix, full, d, msb)
        x = _x_hat(2, H, W)
        ref = _frames(2, H, W, fmt, d, msb, seed=5)
        smp = codec._egress_yuv16_cpu(x[:, :, :H, :W], fmt, d)
        want = [_w32(codec.words_of_samples(s, d, msb)) for s in smp]
        own = torch.stack([((s.to(torch.int64) - codec.samples_of_words(r, d, msb).to(torch.int64)) ** 2).flatten(1).sum(1)
                           for s, r in zip(smp, ref)], 1).tolist()
        xd = x.to(DEV)
        for k, layout in enumerate(YUV_LAYOUTS):
            rd = _yuv_place(ref, fmt, YUV_LAYOUTS[(k + 1) % len(YUV_LAYOUTS)])
            got, sq = run_egress_yuv16(xd, H, W, fmt, d, msb, layout, ref=rd)
            for g, w in zip(got, want):
                assert torch.equal(g, w), (fmt, d, msb, H, W, layout)
            assert sq == own, (fmt, d, msb, H, W, layout)
            plain, none = run_egress_yuv16(xd, H, W, fmt, d, msb, layout)
            assert none is None and all(torch.equal(a, b) for a, b in zip(plain, got))


def test_yuv_sq_err_needs_64_bits_from_the_second_sample():
    fmt = codec.YuvFormat(sub=(2, 2), matrix="bt709", full_range=True, site_x="centre", depth=16)
    for (H, W), layout in itertools.product([(2, 2), (70, 130)], ["i420", "nv12", "batch"]):
        x = torch.ones(2, 3, (H + 63) // 64 * 64, (W + 63) // 64 * 64, device=DEV)  # white: Y = 65535, C = 32768
        ch, cw = fmt.chroma_size(H, W)
        zeros = tuple(torch.zeros(s, dtype=torch.int16).view(torch.uint16) for s in ((2, H, W), (2, ch, cw), (2, ch, cw)))
        got, sq = run_egress_yuv16(x, H, W, fmt, 16, False, layout, ref=_yuv_place(zeros, fmt, layout))
        assert int(got[0].min()) == 65535 and int(got[1].min()) == int(got[2].max()) == 32768
        assert sq == [[H * W * 65535 ** 2, ch * cw * 32768 ** 2, ch * cw * 32768 ** 2]] * 2, (H, W, layout)


@pytest.mark.parametrize("sub,site", GEOM)
def test_yuv_stride_forms_agree(sub, site, forced_path):
    for d, msb, (H, W) in [(10, True, (5, 513)), (16, False, (70, 130)), (12, False, (3, 5))]:
        fmt = _fmt(sub, site, "bt2020", False, d, msb)
        planes = _frames(2, H, W, fmt, d, msb, seed=2)
        x = _x_hat(2, H, W, seed=2).to(DEV)
        ref = _yuv_place(_frames(2, H, W, fmt, d, msb, seed=9), fmt, "rowpad")
        for layout in ("i420", "nv12", "nv21", "rowpad", "crop"):  # each has a fast form
            placed = _yuv_place(planes, fmt, layout)
            forced_path(-1)
            a = run_ingest_yuv16(placed, fmt, d, msb)
            ea, sa = run_egress_yuv16(x, H, W, fmt, d, msb, layout, ref=ref)
            forced_path(2)  # must be a fast form: refused otherwise
            a2 = run_ingest_yuv16(placed, fmt, d, msb)
            forced_path(0)  # the general form
            b = run_ingest_yuv16(placed, fmt, d, msb)
            eb, sb = run_egress_yuv16(x, H, W, fmt, d, msb, layout, ref=ref)
            forced_path(-1)
            assert _same_bits(a, b) and _same_bits(a, a2), (fmt, H, W, layout)
            assert sa == sb and all(torch.equal(p, q) for p, q in zip(ea, eb)), (fmt, H, W, layout)
    forced_path(2)
    with pytest.raises(_lib.MlicError, match="column stride 2"):
        run_ingest_yuv16(_yuv_place(_frames(2, 3, 5, fmt, d, msb), fmt, "batch"), fmt, d, msb)


# ----------------------------------------------------------------------------------------- the Python layer
def test_python_layer_on_the_device_matches_the_cpu_and_honours_out_and_ref():
    d = 12
    H, W = 37, 51
    r = np.random.default_rng(5)
    img = torch.from_numpy(_rand_words(r, (2, H, W, 3), d, False))
    x = codec.ingest_u16(img.to(DEV), d)
    assert x.is_cuda and x.is_contiguous() and _same_bits(x.cpu(), codec.ingest_u16(img, d))
    one = codec.ingest_u16(img[0].permute(2, 0, 1).to(DEV), d, "chw")
    assert _same_bits(one.cpu(), codec.ingest_u16(img[:1], d))
    xh = _x_hat(2, H, W).to(DEV)
    want, wsq = codec.egress_u16(xh.cpu(), H, W, d, ref=img)
    got, sq = codec.egress_u16(xh, H, W, d, ref=img)
    assert got.dtype == torch.uint16 and got.is_cuda and torch.equal(_w32(got.cpu()), _w32(want))
    assert sq.dtype == torch.int64 and sq.cpu().tolist() == wsq.tolist()
    canvas = torch.full((2, H + 2, W + 2, 3), SENT, dtype=torch.int16, device=DEV)
    out = canvas.view(torch.uint16)[:, 1:H + 1, 1:W + 1]
    assert codec.egress_u16(xh, H, W, d, out=out) is out
    torch.cuda.synchronize()
    assert torch.equal(_w32(out.cpu()), _w32(want))
    canvas[:, 1:H + 1, 1:W + 1] = SENT
    assert bool((canvas == SENT).all())
    # Y'CbCr: a P010-style buffer on the device
    fmt = codec.YuvFormat(sub=(2, 2), matrix="bt2020", full_range=False, site_x="left", depth=10, msb=True)
    planes = _frames(2, H, W, fmt, 10, True)
    buf = torch.from_numpy(np.concatenate([planes[0].numpy().reshape(2, -1),
                                           np.stack([planes[1].numpy(), planes[2].numpy()], -1).reshape(2, -1)], 1))
    views = codec.split_yuv(buf.to(DEV), H, W, "nv12", depth=10)
    assert views[1].stride(-1) == 2
    xy = codec.ingest_yuv(*views, fmt)
    assert xy.is_cuda and _same_bits(xy.cpu(), codec.ingest_yuv(*planes, fmt))
    wy = codec.egress_yuv(xh.cpu(), H, W, fmt, ref=planes)
    gy = codec.egress_yuv(xh, H, W, fmt, ref=views)
    assert all(g.dtype == torch.uint16 and torch.equal(_w32(g.cpu()), _w32(w)) for g, w in zip(gy[:3], wy[:3]))
    assert gy[3].cpu().tolist() == wy[3].tolist()
    nv = torch.full((2, codec.yuv_frame_samples(H, W, "nv12") + 4), SENT, dtype=torch.int16, device=DEV)
    outp = codec.split_yuv(nv.view(torch.uint16)[:, :-4], H, W, "nv12", depth=10)
    go = codec.egress_yuv(xh, H, W, fmt, out=outp)
    torch.cuda.synchronize()
    assert all(g is o for g, o in zip(go, outp)) and bool((nv[:, -4:] == SENT).all())
    assert all(torch.equal(_w32(g.cpu()), _w32(w)) for g, w in zip(go, wy[:3]))


# ------------------------------------------------------------------------------------------------ model level
def _net(name):
    net = get_model(name)
    net.load_state_dict(synthetic.synth_state_dict(name, 0))
    net = net.to(DEV).eval()
    net.update()
    return net


@pytest.fixture(scope="module")
def net_s():
    return _net("MLICPP_S")


P010 = codec.YuvFormat(sub=(2, 2), matrix="bt2020", full_range=False, site_x="left", depth=10, msb=True)


def _p010_frame(H, W, seed):
    """One P010 frame buffer (uint16 CPU tensor) made from the synthetic image through the CPU egress."""
    x = synthetic.synth_image((H + 63) // 64 * 64, (W + 63) // 64 * 64, seed).float()
    buf = torch.zeros(codec.yuv_frame_samples(H, W, "nv12"), dtype=torch.int16).view(torch.uint16)
    codec.egress_yuv(x, H, W, P010, out=tuple(v.unsqueeze(0) for v in codec.split_yuv(buf, H, W, "nv12", depth=10)))
    return buf


def test_encode_images_decode_images_at_depth_10_match_the_parts(net_s):
    net = net_s
    H, W = 100, 150
    x0 = synthetic.synth_image(128, 192, 3).float()
    img = codec.egress_u16(x0, H, W, 10)  # uint16 [1,H,W,3], LSB-aligned
    x = codec.ingest_u16(img.to(DEV), 10)
    out = net.compress(x)
    want = codec.write_container(H, W, out["shape"], out["strings"][0][0], out["strings"][1][0])
    files = codec.encode_images(net, img, depth=10)
    assert files == [want]
    assert codec.encode_images(net, img.numpy(), depth=10) == [want]
    assert codec.encode_images(net, img[0].to(DEV), depth=10) == [want]
    x_hat = net.decompress(out["strings"], out["shape"])["x_hat"].float().clone()
    got, info = codec.decode_images(net, files, ref=img, depth=10)
    wimg, wsq = codec.egress_u16(x_hat, H, W, 10, ref=img.to(DEV))
    assert got.dtype == torch.uint16 and torch.equal(_w32(got.cpu()), _w32(wimg.cpu()))
    sq = int(wsq[0])
    assert info[0]["sq_err"] == sq > 0 and info[0]["psnr"] == codec.psnr_from_sq_err(sq, 3 * H * W, 1023)
    assert info[0]["psnr"] == 10.0 * np.log10(1023.0 ** 2 * 3 * H * W / sq)
    msb, _ = codec.decode_images(net, files, depth=10, msb=True)
    assert torch.equal(_w32(msb.cpu()), _w32(wimg.cpu()) << 6)
    # the file does not know its depth: without depth= it decodes to the 8-bit image of the same x_hat
    rgb, _ = codec.decode_images(net, files)
    assert rgb.dtype == torch.uint8 and torch.equal(rgb, codec.egress_u8(x_hat, H, W, "hwc"))


def test_encode_yuv_decode_yuv_on_a_p010_frame_match_the_parts(net_s):
    net = net_s
    H, W = 100, 150
    buf = _p010_frame(H, W, 3)
    planes = tuple(v.unsqueeze(0) for v in codec.split_yuv(buf, H, W, "nv12", depth=10))
    assert planes[1].stride(-1) == 2 and int((_w32(buf) & 63).sum()) == 0
    x = codec.ingest_yuv(*(p.to(DEV) for p in planes), P010)
    out = net.compress(x)
    want = codec.write_container(H, W, out["shape"], out["strings"][0][0], out["strings"][1][0])
    files = codec.encode_yuv(net, *planes, P010)
    assert files == [want]
    assert codec.encode_yuv(net, *(p.numpy() for p in planes), P010) == [want]
    x_hat = net.decompress(out["strings"], out["shape"])["x_hat"].float().clone()
    got, info = codec.decode_yuv(net, files, P010, ref=planes)
    wy, wb, wr, wsq = codec.egress_yuv(x_hat, H, W, P010, ref=planes)
    assert all(a.dtype == torch.uint16 and torch.equal(_w32(a.cpu()), _w32(b.cpu())) for a, b in zip(got, (wy, wb, wr)))
    sq = wsq[0].cpu().tolist()
    own = [int((((_w32(a[0].cpu()) >> 6) - (_w32(b[0]) >> 6)).long() ** 2).sum()) for a, b in zip(got, planes)]
    d = info[0]
    assert d["sq_err"] == sq == own and all(v > 0 for v in sq)
    assert d["psnr_y"] == codec.psnr_from_sq_err(sq[0], H * W, 1023)
    assert d["psnr_u"] == codec.psnr_from_sq_err(sq[1], 50 * 75, 1023)
    assert d["psnr_yuv"] == (6 * d["psnr_y"] + d["psnr_u"] + d["psnr_v"]) / 8
    rgb, _ = codec.decode_images(net, files)
    assert torch.equal(rgb, codec.egress_u8(x_hat, H, W, "hwc"))


def test_c_abi_one_image_yuv16_round_trip_matches_the_python_path(net_s):
    net = net_s
    h = net._handle
    H, W = 100, 150
    buf = _p010_frame(H, W, 5)
    planes = tuple(v.unsqueeze(0) for v in codec.split_yuv(buf, H, W, "nv12", depth=10))
    want = codec.encode_yuv(net, *planes, P010)[0]
    wplanes, _ = codec.decode_yuv(net, [want], P010)
    placed = _yuv_place(planes, P010, "nv12")
    d = P010.desc()
    args = []
    for t in placed:
        args += [_p(t[0]), (C.c_int64 * 2)(*t[0].stride())]
    n = C.c_size_t()
    _lib.call("mlic_encode_image_yuv16", h, _stream(), *args, C.byref(d), 10, 1, H, W, 1.0, -1, None, 0, C.byref(n))
    out = C.create_string_buffer(n.value)
    with pytest.raises(_lib.MlicError, match="buffer too small"):
        _lib.call("mlic_encode_image_yuv16", h, _stream(), None, None, None, None, None, None, None, 0, 0, 0, 0, 1.0, -1,
                  out, n.value - 1, C.byref(n))
    _lib.call("mlic_encode_image_yuv16", h, _stream(), None, None, None, None, None, None, None, 0, 0, 0, 0, 1.0, -1, out,
              n.value, C.byref(n))
    data = C.string_at(out, n.value)
    assert data == want
    # a refused encode, each refusal by its own message, leaves the handle's encoded image as it was
    d3 = P010.desc()
    d3.matrix = 3
    odd = [C.c_void_p(args[0].value + 1)] + args[1:]
    for a, desc, depth, msb, msg in ((args, d, 7, 1, "encode_image_yuv16: depth must be in"),
                                     (args, d, 17, 1, "encode_image_yuv16: depth must be in"),
                                     (args, d, 10, 2, "encode_image_yuv16: msb must be 0"),
                                     (odd, d, 10, 1, "encode_image_yuv16: y must be 2-byte aligned"),
                                     (args, d3, 10, 1, "encode_image_yuv16: matrix must be")):
        with pytest.raises(_lib.MlicError, match=msg):
            _lib.call("mlic_encode_image_yuv16", h, _stream(), *a, C.byref(desc), depth, msb, H, W, 1.0, -1, None, 0,
                      C.byref(n))
        again = C.create_string_buffer(len(want))
        _lib.call("mlic_encode_image_yuv16", h, _stream(), None, None, None, None, None, None, None, 0, 0, 0, 0, 1.0, -1,
                  again, len(want), C.byref(n))
        assert C.string_at(again, n.value) == want
    gh, gw, gl = C.c_int(), C.c_int(), C.c_int()
    _lib.call("mlic_decode_image_yuv16", None, None, data, len(data), 0, 1 << 28, None, None, 0, 0, None, None, 0, None,
              None, 0, None, None, 0, C.byref(gh), C.byref(gw), C.byref(gl))
    assert (gh.value, gw.value, gl.value) == (H, W, -1)
    views, bufs = _yuv_alloc(1, H, W, P010, "rowpad")
    dargs, caps = [], []
    for t in views:
        caps.append(2 * (1 + (t.size(1) - 1) * t.stride(1) + (t.size(2) - 1) * t.stride(2)))  # bytes
    for k, t in enumerate(views):
        dargs += [_p(t[0]), (C.c_int64 * 2)(*t[0].stride()), caps[k]]
    short = list(dargs)
    short[8] = caps[2] - 1
    with pytest.raises(_lib.MlicError, match="cap_bytes"):
        _lib.call("mlic_decode_image_yuv16", h, _stream(), data, len(data), 0, 1 << 28, None, C.byref(d), 10, 1, *short,
                  C.byref(gh), C.byref(gw), C.byref(gl))
    oddd = list(dargs)
    oddd[3] = C.c_void_p(dargs[3].value + 1)
    for a, desc, depth, msb, msg in ((dargs, d, 7, 1, "decode_image_yuv16: depth must be in"),
                                     (dargs, d, 17, 1, "decode_image_yuv16: depth must be in"),
                                     (dargs, d, 10, 2, "decode_image_yuv16: msb must be 0"),
                                     (oddd, d, 10, 1, "decode_image_yuv16: cb must be 2-byte aligned"),
                                     (dargs, d3, 10, 1, "decode_image_yuv16: matrix must be")):
        with pytest.raises(_lib.MlicError, match=msg):
            _lib.call("mlic_decode_image_yuv16", h, _stream(), data, len(data), 0, 1 << 28, None, C.byref(desc), depth, msb,
                      *a, C.byref(gh), C.byref(gw), C.byref(gl))
    torch.cuda.synchronize()
    assert all(bool((b == SENT).all()) for b in bufs), "a refused decode wrote to the planes"
    _lib.call("mlic_decode_image_yuv16", h, _stream(), data, len(data), 0, 1 << 28, None, C.byref(d), 10, 1, *dargs,
              C.byref(gh), C.byref(gw), C.byref(gl))
    torch.cuda.synchronize()
    assert all(torch.equal(_words(v), _w32(w.cpu())) for v, w in zip(views, wplanes))
    _clean(views, bufs, "decode")


def test_tiles_and_code_image_refuse_depths_above_8(net_s):
    from mlic_amd import bitstream
    net = net_s
    img = np.zeros((200, 200, 3), np.uint16)
    with pytest.raises(ValueError, match="blend kernel"):
        codec.encode_tiled(net, img, tile=128, depth=10)
    with pytest.raises(ValueError, match="blend kernel"):
        codec.decode_tiled(net, b"MLT1" + bytes(40), depth=12)
    x = synthetic.synth_image(128, 192, 3)[:, :, :100, :150].contiguous().to(DEV)
    with pytest.raises(ValueError, match="depth 10 is not supported"):
        bitstream.code_image(net, x, yuv=P010)
