"""9..16-bit sample I/O without a GPU: the torch restatements of the four kernels of csrc/image_io16.hip
(codec.ingest_u16 / egress_u16 and codec.ingest_yuv / egress_yuv at depth > 8 on CPU tensors) against numpy and the
float64 oracle of tests/yuv16_oracle.py; the depth-8 and shift identities that tie them to the 8-bit path bit for
bit; split_yuv on uint16 buffers; the command-line tool's 16-bit PPM and high-depth y4m readers / writers; and every
refusal of the C entry points and of the Python layer.

Bounds.  Ingest: |x - x64| <= 1e-6, the 8-bit test's bound: the outputs are in [0, 1] and the count of roundings is
the same at every depth.  Egress: every sample within 1 of the oracle's, and equal to it wherever the oracle's
unrounded t + 0.5 is farther than band(d) = max(1e-3, 2^(d-20)) from an integer (16 fp32 ulps at 2^d against about 8
roundings on the longest path); with x drawn uniformly from [-0.1, 1.1] about 2 band(d) of the samples fall inside the
band, and at most 4 band(d) may (a property of the inputs and the oracle alone, for the seeds committed here)."""
import ctypes as C
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch

import yuv16_oracle as O
from mlic_amd import _lib, codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM = [((1, 1), "left"), ((2, 1), "left"), ((2, 1), "centre"), ((2, 2), "left"), ((2, 2), "centre")]
SETS = [(m, f) for m in ("bt601", "bt709", "bt2020") for f in (False, True)]
SETS8 = [(m, f) for m in ("bt601", "bt709") for f in (False, True)]
DEEP = [10, 12, 16]


def _tool():
    spec = importlib.util.spec_from_file_location("mlic_codec_tool", os.path.join(ROOT, "tools", "mlic_codec.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bits(t):
    return t.contiguous().view(torch.int32)


def _fmt(sub, site, matrix, full, d, msb=False):
    return codec.YuvFormat(sub=sub, matrix=matrix, full_range=full, site_x=site, depth=d, msb=msb)


def _frame(r, H, W, fmt, d, msb=False):
    """uint16 word planes whose samples cover [0, maxv]."""
    ch, cw = fmt.chroma_size(H, W)
    out = []
    for s in ((H, W), (ch, cw), (ch, cw)):
        v = r.integers(0, 1 << d, s, dtype=np.int64)
        if msb:
            v = (v << (16 - d)) | r.integers(0, 1 << (16 - d), s, dtype=np.int64)
        out.append(v.astype(np.uint16))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ 1. RGB
def _all_values(d):
    """Every sample value of depth d as a uint16 [1, n, 3] image (the last pixel padded with zeros)."""
    v = np.zeros(((1 << d) + 2) // 3 * 3, np.uint16)
    v[:1 << d] = np.arange(1 << d)
    return v.reshape(1, -1, 3)


@pytest.mark.parametrize("d", range(8, 17))
def test_rgb_ingest_is_numpys_fp32_division_and_egress_inverts_it_for_every_sample(d):
    img = _all_values(d)
    n = img.shape[1]
    x = codec.ingest_u16(img, d, "hwc")
    assert x.dtype == torch.float32 and tuple(x.shape) == (1, 3, 64, (n + 63) // 64 * 64)
    want = img.astype(np.float32) / np.float32((1 << d) - 1)
    assert np.array_equal(x[0, :, 0, :n].numpy().view(np.int32), want[0].T.view(np.int32))
    assert np.abs(want.astype(np.float64) - O.ingest_rgb(img, d, False)).max() <= 2.0 ** -24
    pad = x.clone()
    pad[:, :, :1, :n] = 0
    assert int(_bits(pad).abs().sum()) == 0  # +0.0 in the padding
    back = codec.egress_u16(x, 1, n, d, "hwc")
    assert back.dtype == torch.uint16 and np.array_equal(back[0].numpy(), img)
    assert np.array_equal(O.egress_rgb(x[0, :, 0, :n].numpy().T, d), img[0].astype(np.int64))
    # LSB-aligned words above maxv read as maxv
    if d < 16:
        over = np.array([[[(1 << d) - 1, 1 << d, 65535]]], np.uint16)
        assert bool((codec.ingest_u16(over, d)[0, :, 0, 0] == 1.0).all())


@pytest.mark.parametrize("d", range(8, 17))
def test_rgb_msb_forms_ignore_input_low_bits_and_write_zero_low_bits(d):
    img = _all_values(d)
    n = img.shape[1]
    r = np.random.default_rng(d)
    low = r.integers(0, 1 << (16 - d), img.shape, dtype=np.int64)
    shifted = ((img.astype(np.int64) << (16 - d)) | low).astype(np.uint16)
    x = codec.ingest_u16(img, d)
    assert torch.equal(_bits(codec.ingest_u16(shifted, d, msb=True)), _bits(x))
    assert np.array_equal(O.samples(shifted, d, True), img.astype(np.int64))
    back = codec.egress_u16(x, 1, n, d, msb=True)[0].numpy().astype(np.int64)
    assert np.array_equal(back, img.astype(np.int64) << (16 - d)) and int((back & ((1 << (16 - d)) - 1)).sum()) == 0
    # sq_err reads the reference by the same rule: the low bits of MSB-aligned reference words do not count
    _, sq = codec.egress_u16(x, 1, n, d, msb=True, ref=shifted)
    assert sq.tolist() == [0]
    ref0 = np.zeros_like(img)
    _, sq = codec.egress_u16(x, 1, n, d, ref=ref0)
    assert sq.dtype == torch.int64 and sq.tolist() == [int((img.astype(np.int64) ** 2).sum())]


def test_rgb_egress_handles_nan_infinities_and_the_clamps_edges():
    x = torch.tensor([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 1.0000001, -1e-7, 0.5, 0.9999999], dtype=torch.float32)
    x = x.view(1, 1, 1, -1).expand(1, 3, 1, -1).contiguous()
    for d in (8, 10, 16):
        m = (1 << d) - 1
        got = codec.egress_u16(x, 1, x.size(3), d)[0, 0, :, 0].tolist()
        assert got == [0, m, 0, 0, 0, m, m, 0, int(np.floor(np.float32(0.5) * np.float32(m))),
                       int(np.floor(np.float32(0.9999999) * np.float32(m)))]


# --------------------------------------------------------------------------------------- 2. depth-8 identities
def test_rgb_at_depth_8_on_widened_bytes_equals_the_8_bit_path_bitwise():
    r = np.random.default_rng(1)
    img8 = r.integers(0, 256, (2, 37, 51, 3), dtype=np.uint8)
    img8[0].reshape(-1)[:256] = np.arange(256)
    x8 = codec.ingest_u8(img8, "hwc")
    assert torch.equal(_bits(codec.ingest_u16(img8.astype(np.uint16), 8, "hwc")), _bits(x8))
    xh = torch.from_numpy(r.uniform(-0.1, 1.1, (2, 3, 64, 64)).astype(np.float32))
    xh[0, 0, 0, :4] = torch.tensor([0.0, 1.0, -0.0, 2.0])
    u8 = codec.egress_u8(xh, 37, 51, "hwc")
    u16 = codec.egress_u16(xh, 37, 51, 8, "hwc")
    assert torch.equal(u16.to(torch.int32), u8.to(torch.int32))
    for layout in ("hwc", "chw"):
        a, sa = codec.egress_u8(xh, 37, 51, layout, ref=torch.from_numpy(img8).permute(0, 3, 1, 2) if layout == "chw" else img8)
        ref16 = torch.from_numpy(img8.astype(np.uint16))
        b, sb = codec.egress_u16(xh, 37, 51, 8, layout, ref=ref16.permute(0, 3, 1, 2) if layout == "chw" else ref16)
        assert torch.equal(a.to(torch.int32), b.to(torch.int32)) and sa.tolist() == sb.tolist()


@pytest.mark.parametrize("sub,site", GEOM)
def test_yuv_at_depth_8_through_the_16_bit_restatement_equals_the_8_bit_restatement(sub, site):
    r = np.random.default_rng(2)
    for matrix, full in SETS8:
        fmt = codec.YuvFormat(sub=sub, matrix=matrix, full_range=full, site_x=site)
        for H, W in [(37, 51), (2, 131)]:
            ch, cw = fmt.chroma_size(H, W)
            p8 = tuple(torch.from_numpy(r.integers(0, 256, s, dtype=np.uint8)) for s in ((1, H, W), (1, ch, cw), (1, ch, cw)))
            p16 = tuple(torch.from_numpy(p.numpy().astype(np.uint16)) for p in p8)
            assert torch.equal(_bits(codec._ingest_yuv16_cpu(*p16, fmt, 8, False)), _bits(codec.ingest_yuv(*p8, fmt)))
            x = torch.from_numpy(r.uniform(-0.1, 1.1, (1, 3, H, W)).astype(np.float32))
            b8 = codec.egress_yuv(x, H, W, fmt)
            s16 = codec._egress_yuv16_cpu(x, fmt, 8)
            assert all(torch.equal(a.to(torch.int32), b) for a, b in zip(b8, s16))


# ------------------------------------------------------------------------------------------ 3. shift identity
@pytest.mark.parametrize("sub,site", GEOM)
def test_limited_range_planes_shifted_up_give_the_8_bit_ingests_bits(sub, site):
    """Limited range: yo, ys, cs and half of depth d are those of depth 8 times 2^(d-8), and so is every sample of
    p8 << (d - 8): every constant and operand differs by an exact power of two, so the fp32 results are equal."""
    r = np.random.default_rng(3)
    for matrix in ("bt601", "bt709"):
        f8 = codec.YuvFormat(sub=sub, matrix=matrix, full_range=False, site_x=site)
        H, W = 37, 51
        ch, cw = f8.chroma_size(H, W)
        p8 = tuple(r.integers(0, 256, s, dtype=np.uint8) for s in ((1, H, W), (1, ch, cw), (1, ch, cw)))
        want = codec.ingest_yuv(*p8, f8)
        for d in DEEP:
            fd = _fmt(sub, site, matrix, False, d)
            pd = tuple((p.astype(np.uint16) << (d - 8)).astype(np.uint16) for p in p8)
            assert torch.equal(_bits(codec.ingest_yuv(*pd, fd)), _bits(want)), (matrix, d)


# ---------------------------------------------------------------------------------- 4. against the float64 oracle
CASES = [(d, sub, site, m, f) for d in DEEP for (sub, site) in GEOM for (m, f) in SETS]


@pytest.mark.parametrize("d,sub,site,matrix,full", CASES)
def test_yuv_ingest_restatement_is_within_1e6_of_the_float64_oracle(d, sub, site, matrix, full):
    r = np.random.default_rng(11 + d)
    worst = 0.0
    for (H, W), msb in [((37, 51), False), ((2, 131), True)]:
        fmt = _fmt(sub, site, matrix, full, d, msb)
        y, cb, cr = _frame(r, H, W, fmt, d, msb)
        x = codec.ingest_yuv(y, cb, cr, fmt)
        assert x.dtype == torch.float32 and tuple(x.shape) == (1, 3, (H + 63) // 64 * 64, (W + 63) // 64 * 64)
        x64 = O.ingest(y, cb, cr, sub, matrix, full, site, d, msb)
        worst = max(worst, float(np.abs(x[0, :, :H, :W].double().numpy() - x64).max()))
        pad = x.clone()
        pad[:, :, :H, :W] = 0
        assert int(_bits(pad).abs().sum()) == 0
    print(f"ingest d={d} {sub} {site} {matrix} full={full}: max |x - x64| = {worst:.3e}")
    assert worst <= 1e-6


def _egress_inputs(r, H, W):
    x = r.uniform(-0.1, 1.1, (3, H, W)).astype(np.float32)
    special = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, np.nextafter(np.float32(1), np.float32(2)),
               -np.float32(1e-7), np.float32(1.0001), np.float32(-0.0001)]
    flat = x.reshape(-1)
    at = r.choice(flat.size, 3 * len(special), replace=False)
    flat[at] = np.tile(np.array(special, np.float32), 3)
    return x


@pytest.mark.parametrize("d,sub,site,matrix,full", CASES)
def test_yuv_egress_restatement_gives_the_oracles_samples_where_they_are_decided(d, sub, site, matrix, full):
    fmt = _fmt(sub, site, matrix, full, d)
    r = np.random.default_rng(23 + d)
    H, W = 64, 66
    x = _egress_inputs(r, H, W)
    got = codec.egress_yuv(torch.from_numpy(x)[None], H, W, fmt)
    want = O.egress_unrounded(x, sub, matrix, full, site, d)
    total = inside = 0
    for g, t in zip(got, want):
        g = g[0].numpy().astype(np.int64)
        assert g.shape == t.shape
        s = O.to_sample(t, d)
        dec = O.decided(t, d)
        assert np.abs(g - s).max() <= 1, fmt
        assert (g[dec] == s[dec]).all(), fmt
        total += dec.size
        inside += int((~dec).sum())
    print(f"egress {fmt!r}: {inside} of {total} samples inside the band ({inside / total:.4f}, band {O.band(d):g})")
    assert inside <= 4 * O.band(d) * total
    # MSB-aligned output: the same samples shifted up
    m = codec.egress_yuv(torch.from_numpy(x)[None], H, W, _fmt(sub, site, matrix, full, d, True))
    assert all(np.array_equal(a.numpy().astype(np.int64), b.numpy().astype(np.int64) << (16 - d)) for a, b in zip(m, got))


# --------------------------------------------------------------------------------------------- 5. constant planes
@pytest.mark.parametrize("d", range(8, 17))
def test_constant_planes_give_the_expected_rgb(d):
    half, maxv, s = 1 << (d - 1), (1 << d) - 1, 1 << (d - 8)
    dt = np.uint8 if d == 8 else np.uint16  # a format of depth 8 is the byte path (and has no BT.2020)
    for (matrix, full), (sub, site) in itertools.product(SETS8 if d == 8 else SETS, GEOM):
        fmt = _fmt(sub, site, matrix, full, d)
        yo, ys = (0, maxv) if full else (16 * s, 219 * s)
        H, W = 5, 7
        ch, cw = fmt.chroma_size(H, W)
        for Y in (yo, yo + ys // 2, yo + ys):
            y = np.full((H, W), Y, dt)
            c = np.full((ch, cw), half, dt)
            if d == 8:  # the 16-bit restatement at depth 8 on the widened bytes gives the same bits
                w = [torch.from_numpy(p.astype(np.uint16))[None] for p in (y, c, c)]
                assert torch.equal(_bits(codec._ingest_yuv16_cpu(*w, fmt, 8, False)), _bits(codec.ingest_yuv(y, c, c, fmt)))
            x = codec.ingest_yuv(y, c, c, fmt)[0, :, :H, :W]
            assert bool((x[0] == x[1]).all()) and bool((x[0] == x[2]).all())  # neutral chroma: R = G = B exactly
            assert abs(float(x[0, 0, 0]) - (Y - yo) / ys) <= 1e-6 and float(x.max()) <= 1.0
            if Y == yo:
                assert int(_bits(x).abs().sum()) == 0  # black is +0.0
            back = codec.egress_yuv(codec.ingest_yuv(y, c, c, fmt), H, W, fmt)
            assert np.array_equal(back[0][0].numpy(), y) and np.array_equal(back[1][0].numpy(), c)


# ------------------------------------------------------------------------------------------------- 6. round trip
@pytest.mark.parametrize("d", DEEP)
@pytest.mark.parametrize("matrix", ["bt601", "bt709", "bt2020"])
def test_444_full_range_round_trip_returns_the_input_samples(d, matrix):
    fmt = _fmt((1, 1), "left", matrix, True, d)
    r = np.random.default_rng(5)
    n = 40000
    y, cb, cr = (r.integers(0, 1 << d, (1, n), dtype=np.int64).astype(np.uint16) for _ in range(3))
    rgb = O.ingest(y, cb, cr, (1, 1), matrix, True, "left", d)  # the filter is on the oracle alone
    keep = ((rgb >= 0.01) & (rgb <= 0.99)).all(0)[0]
    assert keep.sum() > 1000
    y, cb, cr = (p[:, keep] for p in (y, cb, cr))
    W = y.shape[1]
    back = codec.egress_yuv(codec.ingest_yuv(y, cb, cr, fmt), 1, W, fmt)
    for got, want in zip(back, (y, cb, cr)):
        assert np.array_equal(got[0].numpy(), want)


# -------------------------------------------------------------------------------------------------- 7. split_yuv
@pytest.mark.parametrize("layout", ["i420", "yv12", "nv12", "nv21", "i422", "i444"])
@pytest.mark.parametrize("shape", [(4, 6), (5, 7), (1, 1)])
def test_split_yuv_views_uint16_buffers_in_place(layout, shape):
    H, W = shape
    n = codec.yuv_frame_samples(H, W, layout)
    assert codec.yuv_frame_bytes(H, W, layout, 10) == 2 * n == 2 * codec.yuv_frame_bytes(H, W, layout)
    sx, sy = codec._YUV_SUB[layout]
    ch, cw = -(-H // sy), -(-W // sx)
    for make in (lambda a: a, torch.from_numpy):
        for lead in ((), (2,)):
            base = (np.arange(int(np.prod(lead + (n,)))) * 257 % 65536).astype(np.uint16).reshape(lead + (n,))
            y, cb, cr = codec.split_yuv(make(base), H, W, layout, depth=10)
            assert tuple(y.shape) == lead + (H, W) and tuple(cb.shape) == tuple(cr.shape) == lead + (ch, cw)
            yn, bn, rn = (np.asarray(t) for t in (y, cb, cr))
            flat = base.reshape(-1, n)
            for k in range(flat.shape[0]):
                f = flat[k]
                assert np.array_equal(yn.reshape(-1, H, W)[k].reshape(-1), f[:H * W])
                c = f[H * W:]
                if layout in ("nv12", "nv21"):
                    a, b = c[0::2], c[1::2]
                else:
                    a, b = c[:ch * cw], c[ch * cw:]
                first, second = (rn, bn) if layout in ("yv12", "nv21") else (bn, rn)
                assert np.array_equal(first.reshape(-1, ch * cw)[k], a) and np.array_equal(second.reshape(-1, ch * cw)[k], b)
    # P010: interleaved chroma words, column stride 2 elements, and views, not copies
    buf = torch.zeros(n, dtype=torch.int16).view(torch.uint16)
    y, cb, cr = codec.split_yuv(buf, H, W, layout, depth=10)
    assert y.data_ptr() == buf.data_ptr()
    if layout == "nv12":
        assert cb.stride(-1) == 2 and cr.data_ptr() == cb.data_ptr() + 2


def test_split_yuv_refuses_a_wrong_uint16_buffer():
    with pytest.raises(ValueError, match=r"is 36 uint16 words, the buffer has 40"):
        codec.split_yuv(np.zeros(40, np.uint16), 4, 6, "nv12", depth=10)
    with pytest.raises(ValueError, match="depth 8 is a uint8 buffer"):
        codec.split_yuv(np.zeros(36, np.uint16), 4, 6, "nv12")
    with pytest.raises(ValueError, match="depth 10 is a uint16 buffer"):
        codec.split_yuv(np.zeros(36, np.uint8), 4, 6, "nv12", depth=10)
    with pytest.raises(ValueError, match=r"depth must be an integer in \[8, 16\]"):
        codec.split_yuv(np.zeros(36, np.uint16), 4, 6, "nv12", depth=17)
    with pytest.raises(ValueError, match=r"depth must be"):
        codec.yuv_frame_bytes(4, 6, "nv12", 7)


# ---------------------------------------------------------------------------------------------- 8. files: PPM, y4m
@pytest.mark.parametrize("d", [9, 10, 12, 16])
def test_ppm_of_more_than_8_bits_round_trips_big_endian(d, tmp_path):
    tool = _tool()
    r = np.random.default_rng(d)
    img = r.integers(0, 1 << d, (5, 7, 3), dtype=np.int64).astype(np.uint16)
    img[0, 0] = [0, (1 << d) - 1, 258]
    data = tool.write_ppm(img, d)
    head = b"P6\n7 5\n%d\n" % ((1 << d) - 1)
    assert data.startswith(head) and len(data) == len(head) + 5 * 7 * 6
    assert data[len(head) + 4:len(head) + 6] == bytes([1, 2])  # 258, most significant byte first
    got, depth = tool.read_ppm_deep(data)
    assert depth == d and got.dtype == np.uint16 and np.array_equal(got, img)
    p = tmp_path / "a.ppm"
    tool.save_image(str(p), img, d)
    got, depth = tool.load_image(str(p), deep=True)
    assert depth == d and np.array_equal(got, img)
    with pytest.raises(ValueError, match="8-bit image expected"):
        tool.read_ppm(data)  # the 8-bit reader keeps refusing it
    with pytest.raises(ValueError, match="pixel data truncated"):
        tool.read_ppm_deep(data[:-1])
    img8 = r.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    got, depth = tool.read_ppm_deep(tool.write_ppm(img8))
    assert depth == 8 and got.dtype == np.uint8 and np.array_equal(got, img8)


def test_ppm_refuses_a_maxval_that_is_not_a_depth_and_samples_above_it():
    tool = _tool()
    for maxval in (1000, 256, 65534, 254, 65536, 100):
        with pytest.raises(ValueError, match=r"maxval %d is not 2\^d - 1" % maxval):
            tool.read_ppm_deep(b"P6\n2 2\n%d\n" % maxval + bytes(24))
    with pytest.raises(ValueError, match="a sample above maxval 1023"):
        tool.write_ppm(np.full((2, 2, 3), 1024, np.uint16), 10)
    with pytest.raises(ValueError, match="uint16"):
        tool.write_ppm(np.zeros((2, 2, 3), np.uint8), 10)
    with pytest.raises(ValueError, match="depth must be"):
        tool.write_ppm(np.zeros((2, 2, 3), np.uint16), 17)


@pytest.mark.parametrize("tag", ["420p10", "422p10", "444p10", "420p9", "422p12", "444p14", "420p16"])
def test_y4m_of_more_than_8_bits_round_trips_little_endian(tag):
    tool = _tool()
    _, (sx, sy), site, d = tool.y4m_tag(tag)
    assert d == int(tag.split("p")[1]) and site == "left"
    r = np.random.default_rng(d)
    H, W = 5, 7
    ch, cw = -(-H // sy), -(-W // sx)
    frames = [tuple(r.integers(0, 1 << d, s, dtype=np.int64).astype(np.uint16) for s in ((H, W), (ch, cw), (ch, cw)))
              for _ in range(2)]
    frames[0][0][0, 0] = 258
    data = tool.write_y4m(*frames[0], tag)
    body = data.index(b"FRAME\n") + 6
    assert data[body:body + 2] == bytes([2, 1]) and len(data) - body == 2 * (H * W + 2 * ch * cw)
    y, cb, cr, t, params = tool.read_y4m(data, max_depth=16)
    assert t == tag and params == ["F25:1", "Ip", "A1:1"] and y.dtype == np.uint16
    assert all(np.array_equal(a, b) for a, b in zip((y, cb, cr), frames[0]))
    assert tool.write_y4m(y, cb, cr, t, params) == data
    two = data + b"FRAME\n" + b"".join(p.astype("<u2").tobytes() for p in frames[1])
    got = tool.read_y4m(two, 1, max_depth=16)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], frames[1]))
    with pytest.raises(ValueError, match="frame 1 is truncated"):
        tool.read_y4m(two[:-1], 1, max_depth=16)
    with pytest.raises(ValueError, match="frame 0 is truncated"):
        tool.read_y4m(data[:-1], max_depth=16)
    with pytest.raises(ValueError, match=f"C{tag} is {d} bits deep"):
        tool.read_y4m(data)  # the default reader stays an 8-bit reader
    with pytest.raises(ValueError, match=f"uint16 planes .* expected for C{tag} "):
        tool.write_y4m(*(p.astype(np.uint8) for p in frames[0]), tag)
    if d < 16:
        with pytest.raises(ValueError, match="a sample above"):
            tool.write_y4m(np.full((H, W), 1 << d, np.uint16), frames[0][1], frames[0][2], tag)


def test_y4m_refuses_unknown_tags_by_name():
    tool = _tool()
    body = b"FRAME\n" + bytes(2 * (4 * 4 + 2 * 2 * 2))
    for tag in ("420p11", "420p8", "420p010", "411p10", "444alpha", "mono16", "420jpegp10", "440p10"):
        with pytest.raises(ValueError, match="C" + tag + " is not supported"):
            tool.read_y4m(b"YUV4MPEG2 W4 H4 C" + tag.encode() + b"\n" + body, max_depth=16)
        with pytest.raises(ValueError, match="C" + tag + " is not supported"):
            tool.write_y4m(np.zeros((4, 4), np.uint16), np.zeros((2, 2), np.uint16), np.zeros((2, 2), np.uint16), tag)


def test_cli_argument_rules_for_depths_above_8():
    tool = _tool()
    a = tool.parse_args(["encode", "a.yuv", "o.bit", "--synthetic", "1", "--size", "64x48", "--yuv", "nv12", "--depth", "10",
                         "--msb", "--matrix", "2020"])
    assert a.frame_file and a.depth == 10 and a.msb and a.matrix == "2020"
    fmt = tool._yuv_format(a, (2, 2), "left")
    assert fmt == codec.YuvFormat(sub=(2, 2), matrix="bt2020", depth=10, msb=True)
    assert tool._yuv_format(a, (2, 2), "left", depth=12) == codec.YuvFormat(sub=(2, 2), matrix="bt2020", depth=12)
    a = tool.parse_args(["decode", "o.bit", "a.ppm", "--synthetic", "1", "--depth", "12"])
    assert a.depth == 12 and not a.frame_file
    assert tool.parse_args(["decode", "o.bit", "a.y4m", "--synthetic", "1", "--depth", "10", "--ref", "s.y4m"]).depth == 10
    for bad in (["encode", "a.yuv", "o.bit", "--synthetic", "1", "--size", "64x48", "--depth", "17"],
                ["encode", "a.yuv", "o.bit", "--synthetic", "1", "--size", "64x48", "--msb"],
                ["encode", "a.yuv", "o.bit", "--synthetic", "1", "--size", "64x48", "--matrix", "2020"],
                ["encode", "a.ppm", "o.bit", "--synthetic", "1", "--depth", "10"],
                ["encode", "a.ppm", "o.bit", "--synthetic", "1", "--msb"],
                ["decode", "o.bit", "a.ppm", "--synthetic", "1", "--depth", "10", "--region", "0", "0", "8", "8"]):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)
    with pytest.raises(SystemExit, match="matrix must be"):
        tool._yuv_format(tool.parse_args(["decode", "o.bit", "a.y4m", "--synthetic", "1", "--matrix", "2020"]), (2, 2), "left")


def test_cli_raw_yuv_files_of_16_bit_words_load_and_save(tmp_path):
    tool = _tool()
    H, W = 5, 7
    r = np.random.default_rng(9)
    words = (r.integers(0, 1024, codec.yuv_frame_samples(H, W, "nv12"), dtype=np.int64) << 6).astype(np.uint16)
    p = tmp_path / "f.yuv"
    p.write_bytes(bytes(2 * words.size) + words.astype("<u2").tobytes())
    a = tool.parse_args(["encode", str(p), "o.bit", "--synthetic", "1", "--size", "7x5", "--yuv", "nv12", "--depth", "10",
                         "--msb", "--frame", "1"])
    planes, fmt = tool.load_yuv(str(p), a)
    assert fmt.depth == 10 and fmt.msb and planes[0].dtype == np.uint16 and planes[1].strides[-1] == 4
    want = codec.split_yuv(words, H, W, "nv12", depth=10)
    assert all(np.array_equal(g, w) for g, w in zip(planes, want))
    q = tmp_path / "g.yuv"
    tool.save_yuv(str(q), planes, fmt, a)
    assert q.read_bytes() == words.astype("<u2").tobytes()
    a.frame = 2
    with pytest.raises(SystemExit, match="at depth 10 needs"):
        tool.load_yuv(str(p), a)
    # y4m: the tag gives the depth; --depth must agree with it; the writer names the tag from the format
    f10 = codec.YuvFormat(sub=(2, 2), depth=10)
    lsb = tuple(np.ascontiguousarray(v >> 6) for v in want)
    y4 = tmp_path / "h.y4m"
    a = tool.parse_args(["decode", "o.bit", str(y4), "--synthetic", "1", "--depth", "10"])
    tool.save_yuv(str(y4), lsb, f10, a)
    assert b" C420p10\n" in y4.read_bytes()[:64]
    got, gfmt = tool.load_yuv(str(y4), a)
    assert gfmt == f10 and all(np.array_equal(g, w) for g, w in zip(got, lsb))
    a.depth = 12
    with pytest.raises(SystemExit, match="--depth says 12"):
        tool.load_yuv(str(y4), a)
    with pytest.raises(SystemExit, match="LSB-aligned"):
        tool.save_yuv(str(y4), lsb, codec.YuvFormat(sub=(2, 2), depth=10, msb=True), a)


# --------------------------------------------------------------------------------------------------- 9. refusals
P1, P2, P3, PD, PS = 1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 24


def _desc(**kw):
    d = dict(sub_x=2, sub_y=2, matrix=2, full_range=0, site_x=1, reserved=(0, 0, 0))
    d.update(kw)
    return _lib.YuvDesc(d["sub_x"], d["sub_y"], d["matrix"], d["full_range"], d["site_x"], (C.c_int32 * 3)(*d["reserved"]))


def _s(s):
    return None if s is None else (C.c_int64 * len(s))(*s)


def _ingest_u16_rc(src=P1, s=(30000, 300, 3, 1), depth=10, msb=0, B=1, H=100, W=100, dst=PD, Hp=128, Wp=128):
    lib = _lib.lib()
    rc = lib.mlic_image_ingest_u16(None, C.c_void_p(src), _s(s), depth, msb, B, H, W, C.c_void_p(dst), Hp, Wp)
    return rc, lib.mlic_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(src=None), "null argument"), (dict(s=None), "null argument"), (dict(dst=None), "null argument"),
    (dict(B=0), "must be positive"), (dict(H=0), "must be positive"), (dict(W=-1), "must be positive"),
    (dict(Hp=100), "multiples of 64"), (dict(Wp=64), "multiples of 64"),
    (dict(depth=7), "depth must be in [8, 16]"), (dict(depth=17), "depth must be in [8, 16]"),
    (dict(msb=2), "msb must be 0"), (dict(msb=-1), "msb must be 0"),
    (dict(s=(30000, 300, 0, 1)), "zero column or channel stride"), (dict(s=(30000, 300, 3, 0)), "zero column or channel stride"),
    (dict(src=P1 + 1), "src must be 2-byte aligned"), (dict(dst=PD + 2), "dst must be 4-byte aligned"),
])
def test_ingest_u16_refuses_bad_arguments_without_a_device(kw, msg):
    rc, text = _ingest_u16_rc(**kw)
    assert rc != 0 and msg in text and "image_ingest_u16" in text, text


def _egress_u16_rc(src=PD, ss=(49152, 16384, 128), B=1, H=100, W=100, depth=10, msb=0, dst=P1, d=(30000, 300, 3, 1),
                   ref=None, r=None, sq=None):
    lib = _lib.lib()
    rc = lib.mlic_image_egress_u16(None, C.c_void_p(src), _s(ss), B, H, W, depth, msb, C.c_void_p(dst), _s(d),
                                   C.c_void_p(ref), _s(r), C.c_void_p(sq))
    return rc, lib.mlic_last_error().decode()


RREF = dict(ref=P2, r=(30000, 300, 3, 1), sq=PS)


@pytest.mark.parametrize("kw,msg", [
    (dict(src=None), "null argument"), (dict(ss=None), "null argument"), (dict(dst=None), "null argument"),
    (dict(d=None), "null argument"), (dict(B=0), "must be positive"), (dict(H=0), "must be positive"),
    (dict(depth=7), "depth must be in [8, 16]"), (dict(depth=32), "depth must be in [8, 16]"), (dict(msb=3), "msb must be 0"),
    (dict(d=(30000, 300, 0, 1)), "zero column or channel stride (dst)"),
    (dict(ref=P2), "ref and sq_err go together"), (dict(sq=PS), "ref and sq_err go together"),
    ({**RREF, "r": None}, "ref needs strides"), ({**RREF, "r": (30000, 300, 3, 0)}, "ref needs strides"),
    (dict(dst=P1 + 1), "dst must be 2-byte aligned"), ({**RREF, "ref": P2 + 1}, "ref must be 2-byte aligned"),
    (dict(src=PD + 2), "src must be 4-byte"), ({**RREF, "sq": PS + 4}, "sq_err 8-byte aligned"),
])
def test_egress_u16_refuses_bad_arguments_without_a_device(kw, msg):
    rc, text = _egress_u16_rc(**kw)
    assert rc != 0 and msg in text and "image_egress_u16" in text, text


def _ingest_yuv16_rc(y=P1, ys=(10000, 100, 1), cb=P2, bs=(2500, 50, 1), cr=P3, rs=(2500, 50, 1), desc=True, depth=10,
                     msb=1, B=1, H=100, W=100, dst=PD, Hp=128, Wp=128, **dkw):
    lib = _lib.lib()
    d = _desc(**dkw)
    rc = lib.mlic_image_ingest_yuv16(None, C.c_void_p(y), _s(ys), C.c_void_p(cb), _s(bs), C.c_void_p(cr), _s(rs),
                                     C.byref(d) if desc else None, depth, msb, B, H, W, C.c_void_p(dst), Hp, Wp)
    return rc, lib.mlic_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(y=None), "null plane"), (dict(cb=None), "null plane"), (dict(cr=None), "null plane"),
    (dict(dst=None), "null plane or dst"), (dict(ys=None), "null strides"), (dict(bs=None), "null strides"),
    (dict(rs=None), "null strides"), (dict(desc=False), "null mlic_yuv_desc"),
    (dict(B=0), "must be positive"), (dict(H=0), "must be positive"), (dict(W=-1), "must be positive"),
    (dict(Hp=100), "multiples of 64"), (dict(Wp=64), "multiples of 64"), (dict(Hp=64), "multiples of 64"),
    (dict(depth=7), "depth must be in [8, 16]"), (dict(depth=17), "depth must be in [8, 16]"), (dict(msb=2), "msb must be 0"),
    (dict(sub_x=0), "sub_x and sub_y must be 1 or 2"), (dict(sub_y=3), "sub_x and sub_y must be 1 or 2"),
    (dict(sub_x=1, sub_y=2), "4:4:0"), (dict(matrix=3), "matrix must be 0 (BT.601), 1 (BT.709) or 2"),
    (dict(matrix=-1), "matrix must be"), (dict(full_range=2), "full_range must be"), (dict(site_x=2), "site_x must be"),
    (dict(reserved=(0, 1, 0)), "reserved"), (dict(reserved=(10, 0, 0)), "reserved"),
    (dict(ys=(10000, 100, 0)), "zero column stride"), (dict(bs=(2500, 50, 0)), "zero column stride"),
    (dict(y=P1 + 1), "y must be 2-byte aligned"), (dict(cb=P2 + 1), "cb must be 2-byte aligned"),
    (dict(cr=P3 + 3), "cr must be 2-byte aligned"), (dict(dst=PD + 2), "4-byte aligned"),
])
def test_ingest_yuv16_refuses_bad_arguments_without_a_device(kw, msg):
    rc, text = _ingest_yuv16_rc(**kw)
    assert rc != 0 and msg in text and ("image_ingest_yuv16" in text or "mlic_yuv_desc" in text), text


def _egress_yuv16_rc(src=PD, ss=(49152, 16384, 128), B=1, H=100, W=100, desc=True, depth=10, msb=1, y=P1,
                     ys=(10000, 100, 1), cb=P2, bs=(2500, 50, 1), cr=P3, rs=(2500, 50, 1), ry=None, rys=None, rb=None,
                     rbs=None, rr=None, rrs=None, sq=None, **dkw):
    lib = _lib.lib()
    d = _desc(**dkw)
    rc = lib.mlic_image_egress_yuv16(None, C.c_void_p(src), _s(ss), B, H, W, C.byref(d) if desc else None, depth, msb,
                                     C.c_void_p(y), _s(ys), C.c_void_p(cb), _s(bs), C.c_void_p(cr), _s(rs),
                                     C.c_void_p(ry), _s(rys), C.c_void_p(rb), _s(rbs), C.c_void_p(rr), _s(rrs),
                                     C.c_void_p(sq))
    return rc, lib.mlic_last_error().decode()


YREF = dict(ry=P1 + 8, rys=(10000, 100, 1), rb=P2 + 8, rbs=(5000, 100, 2), rr=P2 + 10, rrs=(5000, 100, 2), sq=PS)


@pytest.mark.parametrize("kw,msg", [
    (dict(src=None), "null src or plane"), (dict(y=None), "null src or plane"), (dict(cb=None), "null src or plane"),
    (dict(cr=None), "null src or plane"), (dict(ss=None), "null strides"), (dict(ys=None), "null strides"),
    (dict(desc=False), "null mlic_yuv_desc"), (dict(B=0), "must be positive"), (dict(H=0), "must be positive"),
    (dict(W=0), "must be positive"), (dict(depth=0), "depth must be in [8, 16]"), (dict(msb=7), "msb must be 0"),
    (dict(sub_x=4), "sub_x and sub_y must be 1 or 2"), (dict(sub_x=1, sub_y=2), "4:4:0"), (dict(matrix=7), "matrix must be"),
    (dict(full_range=-1), "full_range must be"), (dict(site_x=-1), "site_x must be"), (dict(reserved=(0, 0, 9)), "reserved"),
    (dict(bs=(2500, 50, 0)), "zero column stride"), (dict(src=PD + 1), "src must be 4-byte aligned"),
    (dict(y=P1 + 1), "y must be 2-byte aligned"), (dict(cr=P3 + 1), "cr must be 2-byte aligned"),
    (dict(sq=PS), "all given or all NULL"), (dict(ry=P1), "all given or all NULL"),
    ({**YREF, "sq": None}, "all given or all NULL"), ({**YREF, "rb": None}, "all given or all NULL"),
    ({**YREF, "rbs": None}, "null ref strides"), ({**YREF, "rrs": (5000, 100, 0)}, "zero column stride (ref)"),
    ({**YREF, "ry": P1 + 7}, "ref_y must be 2-byte aligned"), ({**YREF, "rr": P2 + 9}, "ref_cr must be 2-byte aligned"),
    ({**YREF, "sq": PS + 4}, "sq_err must be 8-byte aligned"),
])
def test_egress_yuv16_refuses_bad_arguments_without_a_device(kw, msg):
    rc, text = _egress_yuv16_rc(**kw)
    assert rc != 0 and msg in text and ("image_egress_yuv16" in text or "mlic_yuv_desc" in text), text


def test_forced_kernel_form_must_fit_the_strides_of_uint16_samples():
    try:
        _lib.call("mlic_set_kernel_option", b"image_io_path", 1)
        rc, msg = _ingest_yuv16_rc()
        assert rc != 0 and "HWC" in msg
        rc, msg = _ingest_u16_rc(s=(40000, 400, 4, 1))
        assert rc != 0 and "column stride 3" in msg
        _lib.call("mlic_set_kernel_option", b"image_io_path", 2)
        rc, msg = _ingest_u16_rc()
        assert rc != 0 and "column stride 1" in msg
        rc, msg = _ingest_yuv16_rc(bs=(2500, 150, 3), rs=(2500, 150, 3))
        assert rc != 0 and "column stride 2" in msg
        rc, msg = _ingest_yuv16_rc(bs=(5000, 100, 2), rs=(5000, 100, 2))  # column stride 2 but not one interleaved plane
        assert rc != 0 and "column stride 2" in msg
    finally:
        _lib.call("mlic_set_kernel_option", b"image_io_path", -1)


def test_one_image_yuv16_entry_points_refuse_without_a_device():
    n, H, W, lv = C.c_size_t(), C.c_int(-5), C.c_int(-5), C.c_int(-5)
    s2 = (C.c_int64 * 2)(100, 1)
    d = _desc()
    with pytest.raises(_lib.MlicError, match="null mlic_model handle"):
        _lib.call("mlic_encode_image_yuv16", None, None, C.c_void_p(P1), s2, C.c_void_p(P2), s2, C.c_void_p(P3), s2,
                  C.byref(d), 10, 1, 100, 100, 1.0, -1, None, 0, C.byref(n))
    data = codec.write_container(100, 150, (2, 3), b"yy", b"z", 3)
    _lib.call("mlic_decode_image_yuv16", None, None, data, len(data), 8, 1 << 28, None, None, 0, 0, None, None, 0, None,
              None, 0, None, None, 0, C.byref(H), C.byref(W), C.byref(lv))
    assert (H.value, W.value, lv.value) == (100, 150, 3)
    with pytest.raises(_lib.MlicError, match="z length runs past the end"):
        _lib.call("mlic_decode_image_yuv16", None, None, data[:-1], len(data) - 1, 8, 1 << 28, None, None, 0, 0, None, None,
                  0, None, None, 0, None, None, 0, C.byref(H), C.byref(W), C.byref(lv))
    with pytest.raises(_lib.MlicError, match="null mlic_model handle"):
        _lib.call("mlic_decode_image_yuv16", None, None, data, len(data), 8, 1 << 28, None, C.byref(d), 10, 1,
                  C.c_void_p(P1), s2, 1 << 20, C.c_void_p(P2), s2, 1 << 20, C.c_void_p(P3), s2, 1 << 20, C.byref(H),
                  C.byref(W), C.byref(lv))


ONE = dict(y=P1, cb=P2, cr=P3, depth=10, msb=1)
ONE_REFUSALS = [
    (dict(depth=7), "depth must be in [8, 16]"), (dict(depth=17), "depth must be in [8, 16]"),
    (dict(msb=2), "msb must be 0"), (dict(msb=-1), "msb must be 0"),
    (dict(y=P1 + 1), "y must be 2-byte aligned"), (dict(cb=P2 + 1), "cb must be 2-byte aligned"),
    (dict(cr=P3 + 1), "cr must be 2-byte aligned"),
    (dict(matrix=3), "matrix must be 0 (BT.601), 1 (BT.709) or 2"), (dict(matrix=-1), "matrix must be"),
    (dict(sub_x=3), "sub_x and sub_y must be 1 or 2"), (dict(sub_x=1, sub_y=2), "4:4:0"),
    (dict(full_range=2), "full_range must be"), (dict(site_x=2), "site_x must be"), (dict(reserved=(0, 0, 1)), "reserved"),
]


@pytest.mark.parametrize("kw,msg", ONE_REFUSALS)
def test_one_image_yuv16_calls_refuse_bad_arguments_before_they_touch_the_handle(kw, msg):
    """Each refusal by its own message, with the call's name in front, and before the handle is looked at: the
    handle here is NULL, which a call that passed its argument checks refuses as such (the test above)."""
    a = {**ONE, **{k: v for k, v in kw.items() if k in ONE}}
    d = _desc(**{k: v for k, v in kw.items() if k not in ONE})
    s2 = (C.c_int64 * 2)(100, 1)
    n, H, W, lv = C.c_size_t(), C.c_int(), C.c_int(), C.c_int()
    lib = _lib.lib()
    rc = lib.mlic_encode_image_yuv16(None, None, C.c_void_p(a["y"]), s2, C.c_void_p(a["cb"]), s2, C.c_void_p(a["cr"]), s2,
                                     C.byref(d), a["depth"], a["msb"], 100, 100, 1.0, -1, None, 0, C.byref(n))
    text = lib.mlic_last_error().decode()
    assert rc != 0 and msg in text and "encode_image_yuv16" in text, text
    data = codec.write_container(100, 150, (2, 3), b"yy", b"z", 3)
    rc = lib.mlic_decode_image_yuv16(None, None, data, len(data), 8, 1 << 28, None, C.byref(d), a["depth"], a["msb"],
                                     C.c_void_p(a["y"]), s2, 1 << 20, C.c_void_p(a["cb"]), s2, 1 << 20,
                                     C.c_void_p(a["cr"]), s2, 1 << 20, C.byref(H), C.byref(W), C.byref(lv))
    text = lib.mlic_last_error().decode()
    assert rc != 0 and msg in text and "decode_image_yuv16" in text, text
    assert (H.value, W.value, lv.value) == (100, 150, 3)  # the file was parsed and reported all the same


def test_one_image_yuv16_calls_refuse_strides_and_caps_before_they_touch_the_handle():
    d = _desc()
    s2, z2 = (C.c_int64 * 2)(100, 1), (C.c_int64 * 2)(100, 0)
    n, H, W, lv = C.c_size_t(), C.c_int(), C.c_int(), C.c_int()
    with pytest.raises(_lib.MlicError, match="encode_image_yuv16: zero column stride"):
        _lib.call("mlic_encode_image_yuv16", None, None, C.c_void_p(P1), s2, C.c_void_p(P2), z2, C.c_void_p(P3), s2,
                  C.byref(d), 10, 1, 100, 100, 1.0, -1, None, 0, C.byref(n))
    with pytest.raises(_lib.MlicError, match="encode_image_yuv16: null chroma plane"):
        _lib.call("mlic_encode_image_yuv16", None, None, C.c_void_p(P1), s2, None, s2, C.c_void_p(P3), s2,
                  C.byref(d), 10, 1, 100, 100, 1.0, -1, None, 0, C.byref(n))
    with pytest.raises(_lib.MlicError, match="null mlic_yuv_desc"):
        _lib.call("mlic_encode_image_yuv16", None, None, C.c_void_p(P1), s2, C.c_void_p(P2), s2, C.c_void_p(P3), s2,
                  None, 10, 1, 100, 100, 1.0, -1, None, 0, C.byref(n))
    data = codec.write_container(100, 150, (2, 3), b"yy", b"z", 3)
    planes = [C.c_void_p(P1), s2, 1 << 20, C.c_void_p(P2), s2, 1 << 20, C.c_void_p(P3), s2, 1 << 20]
    short = list(planes)
    short[2] = 2 * (1 + 99 * 100 + 149) - 1  # one byte less than the Y plane's extent in uint16 words
    with pytest.raises(_lib.MlicError, match="decode_image_yuv16: the file's plane does not fit its cap_bytes"):
        _lib.call("mlic_decode_image_yuv16", None, None, data, len(data), 8, 1 << 28, None, C.byref(d), 10, 1, *short,
                  C.byref(H), C.byref(W), C.byref(lv))
    zero = list(planes)
    zero[4] = z2
    with pytest.raises(_lib.MlicError, match="decode_image_yuv16: strides"):
        _lib.call("mlic_decode_image_yuv16", None, None, data, len(data), 8, 1 << 28, None, C.byref(d), 10, 1, *zero,
                  C.byref(H), C.byref(W), C.byref(lv))
    ok = list(planes)
    ok[2] = 2 * (1 + 99 * 100 + 149)
    with pytest.raises(_lib.MlicError, match="null mlic_model handle"):
        _lib.call("mlic_decode_image_yuv16", None, None, data, len(data), 8, 1 << 28, None, C.byref(d), 10, 1, *ok,
                  C.byref(H), C.byref(W), C.byref(lv))


def test_python_layer_refusals():
    img = np.zeros((4, 6, 3), np.uint16)
    for bad in (7, 17, 10.0, True, None):
        with pytest.raises(ValueError, match=r"depth must be an integer in \[8, 16\]"):
            codec.ingest_u16(img, bad)
    with pytest.raises(ValueError, match="msb must be a bool"):
        codec.ingest_u16(img, 10, msb=1)
    with pytest.raises(ValueError, match="a uint16 array expected, got uint8"):
        codec.ingest_u16(img.astype(np.uint8), 10)
    with pytest.raises(ValueError, match="a uint16 tensor or array expected"):
        codec.ingest_u16(torch.zeros(4, 6, 3, dtype=torch.int16), 10)
    with pytest.raises(ValueError, match="3 channels"):
        codec.ingest_u16(np.zeros((4, 6, 4), np.uint16), 10, "hwc")
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match="fp32"):
        codec.egress_u16(x.double(), 4, 6, 10)
    with pytest.raises(ValueError, match="crop 65 x 6"):
        codec.egress_u16(x, 65, 6, 10)
    with pytest.raises(ValueError, match="out must be uint16"):
        codec.egress_u16(x, 4, 6, 10, out=torch.zeros(1, 4, 6, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="ref must have shape"):
        codec.egress_u16(x, 4, 6, 10, ref=np.zeros((1, 4, 5, 3), np.uint16))
    with pytest.raises(ValueError, match="a uint16 array expected"):
        codec.egress_u16(x, 4, 6, 10, ref=np.zeros((1, 4, 6, 3), np.uint8))
    # encode_images / decode_images
    with pytest.raises(ValueError, match=r"encode_images: depth must be"):
        codec.encode_images(None, img, depth=20)
    with pytest.raises(ValueError, match="a uint16 array expected"):
        codec.encode_images(None, img.astype(np.uint8), depth=10)
    with pytest.raises(ValueError, match="uint8 tensor or array"):
        codec.encode_images(None, img)  # uint16 without depth=
    with pytest.raises(ValueError, match=r"decode_images: depth must be"):
        codec.decode_images(None, [b"x"], depth=3)
    with pytest.raises(ValueError, match="msb must be a bool"):
        codec.decode_images(None, [b"x"], depth=10, msb="yes")
    assert codec.psnr_from_sq_err(4, 2) == codec.psnr_from_sq_err(4, 2, 255) == 10 * np.log10(255.0 ** 2 * 2 / 4)
    assert codec.psnr_from_sq_err(4, 2, 1023) == 10 * np.log10(1023.0 ** 2 * 2 / 4)
    # tiles and code_image: refused by naming the missing piece
    with pytest.raises(ValueError, match="encode_tiled: depth 10 together with tiles is not supported: the blend kernel"):
        codec.encode_tiled(None, np.zeros((200, 200, 3), np.uint16), tile=128, depth=10)
    with pytest.raises(ValueError, match="decode_tiled: depth 16 together with tiles is not supported: the blend kernel"):
        codec.decode_tiled(None, b"MLT1" + bytes(40), depth=16)
    with pytest.raises(ValueError, match=r"depth must be an integer in \[8, 16\]"):
        codec.decode_tiled(None, b"MLT1" + bytes(40), depth=99)
    # depth=8 means uint16 words of 8-bit samples, as in encode_images(depth=8): refused as well, by the same name
    with pytest.raises(ValueError, match="encode_tiled: depth 8 together with tiles is not supported"):
        codec.encode_tiled(None, np.zeros((200, 200, 3), np.uint16), tile=128, depth=8)
    with pytest.raises(ValueError, match="decode_tiled: depth 8 together with tiles is not supported"):
        codec.decode_tiled(None, b"MLT1" + bytes(40), depth=8)
    from mlic_amd import bitstream
    with pytest.raises(ValueError, match="code_image: yuv= at depth 10 is not supported"):
        bitstream.code_image(None, torch.zeros(1, 3, 64, 64), yuv=codec.YuvFormat(depth=10))
    # YuvFormat and the plane checks
    for kw, msg in ((dict(depth=7), "depth must be"), (dict(depth=17), "depth must be"), (dict(depth=10, msb=1), "msb must be"),
                    (dict(msb=True), "msb=True needs depth > 8"), (dict(matrix="bt2020"), "matrix must be"),
                    (dict(matrix="bt2020c", depth=10), "matrix must be")):
        with pytest.raises(ValueError, match=msg):
            codec.YuvFormat(**kw)
    f10 = codec.YuvFormat(depth=10, matrix="bt2020")
    assert f10.desc().matrix == 2 and f10.maxv == 1023 and f10 != codec.YuvFormat(depth=10, matrix="bt2020", msb=True)
    assert "depth=10" in repr(f10) and "depth" not in repr(codec.YuvFormat())
    y, cb, cr = np.zeros((4, 6), np.uint16), np.zeros((2, 3), np.uint16), np.zeros((2, 3), np.uint16)
    with pytest.raises(ValueError, match="y must be a uint16 tensor or array .* depth 10"):
        codec.ingest_yuv(y.astype(np.uint8), cb, cr, f10)
    with pytest.raises(ValueError, match="y must be a uint8 tensor or array"):
        codec.ingest_yuv(y, cb, cr, codec.YuvFormat())
    with pytest.raises(ValueError, match=r"chroma planes \(1, 2, 3\)"):
        codec.ingest_yuv(y, cb, np.zeros((2, 2), np.uint16), f10)
    with pytest.raises(ValueError, match="out must be three uint16 tensors"):
        codec.egress_yuv(x, 4, 6, f10, out=(torch.zeros(1, 4, 6, dtype=torch.uint8),) * 3)
    with pytest.raises(ValueError, match="cb must be a uint16"):
        codec.egress_yuv(x, 4, 6, f10, ref=(y, cb.astype(np.uint8), cr))
    with pytest.raises(ValueError, match="roi= together with Y'CbCr"):
        codec.encode_yuv(None, y, cb, cr, f10, roi=np.ones((4, 6), np.uint8), roi_levels=(0, 1))
    with pytest.raises(ValueError, match="tiles together with Y'CbCr"):
        codec.encode_yuv(None, y, cb, cr, f10, tile=128)
    p = codec.psnr_yuv_from_sq_err([24, 6, 6], 4, 6, f10)
    assert p["psnr_y"] == codec.psnr_from_sq_err(24, 24, 1023) and p["psnr_u"] == codec.psnr_from_sq_err(6, 6, 1023)
