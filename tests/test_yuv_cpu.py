"""Y'CbCr frame I/O without a GPU: the torch restatement of the ingest / egress kernels (codec.ingest_yuv /
egress_yuv on CPU tensors) against the float64 oracle of tests/yuv_oracle.py, the geometry of the chroma filters,
the byte round trip, split_yuv's views, the command-line tool's y4m reader / writer, and every refusal of the C
entry points and of the Python layer.

Bounds.  Ingest: |x - x64| <= 1e-6: at most five fp32 roundings on magnitudes <= 2.2 plus three rounded constants
give < 9e-7.  Egress: a sample is *decided* when the oracle's unrounded t + 0.5 is farther than 1e-3 from an
integer (the fp32 evaluation's error at magnitude 255 is bounded by about 1.2e-4); decided samples must equal the
oracle's byte, undecided ones may be either neighbour, and at most 1 % of the samples may be undecided (a property
of the inputs and the oracle alone)."""
import ctypes as C
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch

import yuv_oracle as O
from mlic_amd import _lib, codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBS = [(1, 1), (2, 1), (2, 2)]
SETS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]
SITES = ["left", "centre"]
ALL = list(itertools.product(SUBS, SETS, SITES))


def _fmt(sub, st, site):
    return codec.YuvFormat(sub=sub, matrix=st[0], full_range=st[1], site_x=site)


def _frame(r, H, W, fmt):
    ch, cw = fmt.chroma_size(H, W)
    return (r.integers(0, 256, (H, W), dtype=np.uint8), r.integers(0, 256, (ch, cw), dtype=np.uint8),
            r.integers(0, 256, (ch, cw), dtype=np.uint8))


def _tool():
    spec = importlib.util.spec_from_file_location("mlic_codec_tool", os.path.join(ROOT, "tools", "mlic_codec.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# --------------------------------------------------------------------------------------- 1. ingest accuracy
@pytest.mark.parametrize("sub,st,site", ALL)
def test_ingest_restatement_is_within_1e6_of_the_float64_oracle(sub, st, site):
    fmt = _fmt(sub, st, site)
    r = np.random.default_rng(11)
    worst = 0.0
    for H, W in [(37, 51), (64, 64), (2, 131)]:
        y, cb, cr = _frame(r, H, W, fmt)
        x = codec.ingest_yuv(y, cb, cr, fmt)
        assert x.dtype == torch.float32 and tuple(x.shape) == (1, 3, (H + 63) // 64 * 64, (W + 63) // 64 * 64)
        x64 = O.ingest(y, cb, cr, sub, st[0], st[1], site)
        worst = max(worst, float(np.abs(x[0, :, :H, :W].double().numpy() - x64).max()))
        pad = x.clone()
        pad[:, :, :H, :W] = 0
        assert int(pad.view(torch.int32).abs().sum()) == 0  # +0.0 in the padding
    print(f"ingest {fmt!r}: max |x - x64| = {worst:.3e}")
    assert worst <= 1e-6


# ---------------------------------------------------------------------------------------- 2. egress bytes
def _egress_inputs(r, H, W):
    x = r.uniform(-0.1, 1.1, (3, H, W)).astype(np.float32)
    special = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, np.nextafter(np.float32(1), np.float32(2)),
               -np.float32(1e-7), np.float32(1.0001), np.float32(-0.0001)]
    flat = x.reshape(-1)
    at = r.choice(flat.size, 3 * len(special), replace=False)
    flat[at] = np.tile(np.array(special, np.float32), 3)
    return x


@pytest.mark.parametrize("sub,st,site", ALL)
def test_egress_restatement_gives_the_oracles_bytes_where_they_are_decided(sub, st, site):
    fmt = _fmt(sub, st, site)
    r = np.random.default_rng(23)
    total = undecided = 0
    for H, W in [(37, 51), (64, 66), (3, 130)]:
        x = _egress_inputs(r, H, W)
        got = codec.egress_yuv(torch.from_numpy(x)[None], H, W, fmt)
        want = O.egress_unrounded(x, sub, st[0], st[1], site)
        for g, t in zip(got, want):
            g = g[0].numpy()
            assert g.shape == t.shape and g.dtype == np.uint8
            d = O.decided(t)
            b = O.to_byte(t)
            assert (g[d] == b[d]).all(), fmt
            lo, hi = O.to_byte(t - 1e-3), O.to_byte(t + 1e-3)
            assert ((g[~d] == lo[~d]) | (g[~d] == hi[~d])).all(), fmt
            total += d.size
            undecided += int((~d).sum())
    print(f"egress {fmt!r}: {undecided} of {total} samples undecided")
    assert undecided <= 0.01 * total


# -------------------------------------------------------------------------------------------- 3. geometry
@pytest.mark.parametrize("site", SITES)
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (2, 1), (3, 5), (4, 6), (7, 8)])
def test_upsampling_map_equals_the_oracle_exactly(shape, sub, site):
    H, W = shape
    fmt = codec.YuvFormat(sub=sub, site_x=site)
    ch, cw = fmt.chroma_size(H, W)
    assert (ch, cw) == (-(-H // sub[1]), -(-W // sub[0]))
    c = ((np.arange(ch * cw) * 7 + 3) % 251).astype(np.uint8).reshape(ch, cw)  # all distinct (ch * cw <= 251)
    assert len(np.unique(c)) == c.size
    got = codec.yuv_upsample16(torch.from_numpy(c)[None], H, W, fmt)[0].numpy()
    want = O.upsample16(c, H, W, sub, site)
    assert got.shape == (H, W) and (got == want).all()
    assert got.min() >= 0 and got.max() <= 4080


@pytest.mark.parametrize("site", SITES)
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (2, 1), (3, 5), (6, 9)])
def test_a_constant_chroma_plane_upsamples_to_itself_and_back(shape, sub, site):
    H, W = shape
    fmt = codec.YuvFormat(sub=sub, site_x=site)
    ch, cw = fmt.chroma_size(H, W)
    for v in (0, 77, 255):
        c = torch.full((1, ch, cw), v, dtype=torch.uint8)
        up = codec.yuv_upsample16(c, H, W, fmt)
        assert bool((up == 16 * v).all())
        t = up.float() / 16 - 128
        down = codec.yuv_downsample(t, fmt) + 128.0
        assert tuple(down.shape) == (1, ch, cw) and bool((down == float(v)).all())
        assert np.array_equal(O.downsample(t[0].double().numpy(), sub, site) + 128.0, np.full((ch, cw), float(v)))


# ------------------------------------------------------------------------------------------ 4. round trip
@pytest.mark.parametrize("st", SETS)
def test_444_round_trip_returns_the_input_bytes(st):
    fmt = _fmt((1, 1), st, "left")
    yo, ys = (0, 255) if st[1] else (16, 219)
    r = np.random.default_rng(5)
    n = 40000
    y, cb, cr = (r.integers(0, 256, (1, n), dtype=np.uint8) for _ in range(3))
    rgb = O.ingest(y, cb, cr, (1, 1), st[0], st[1], "left")  # the filter is on the oracle alone
    keep = ((rgb >= 0.01) & (rgb <= 0.99)).all(0)[0]
    greys = np.arange(yo + 3, yo + ys - 2, dtype=np.uint8)
    y = np.concatenate([y[0][keep], greys])[None]
    cb = np.concatenate([cb[0][keep], np.full(greys.size, 128, np.uint8)])[None]
    cr = np.concatenate([cr[0][keep], np.full(greys.size, 128, np.uint8)])[None]
    assert keep.sum() > 1000
    rgb = O.ingest(y, cb, cr, (1, 1), st[0], st[1], "left")
    assert rgb.min() >= 0.01 and rgb.max() <= 0.99
    W = y.shape[1]
    x = codec.ingest_yuv(y, cb, cr, fmt)
    back = codec.egress_yuv(x, 1, W, fmt)
    for got, want in zip(back, (y, cb, cr)):
        assert np.array_equal(got[0].numpy(), want)


# -------------------------------------------------------------------------------------------- 5. split_yuv
@pytest.mark.parametrize("layout", ["i420", "yv12", "nv12", "nv21", "i422", "i444"])
@pytest.mark.parametrize("shape", [(4, 6), (5, 7), (1, 1)])
def test_split_yuv_returns_views_of_the_buffer(layout, shape):
    H, W = shape
    sx, sy = codec._YUV_SUB[layout]
    ch, cw = -(-H // sy), -(-W // sx)
    n = H * W + 2 * ch * cw
    assert codec.yuv_frame_bytes(H, W, layout) == n
    for batched in (False, True):
        for kind in ("numpy", "torch"):
            buf = np.zeros((2, n) if batched else (n,), np.uint8)
            t = buf if kind == "numpy" else torch.from_numpy(buf)
            y, cb, cr = codec.split_yuv(t, H, W, layout)
            lead = (2,) if batched else ()
            assert tuple(y.shape) == lead + (H, W) and tuple(cb.shape) == tuple(cr.shape) == lead + (ch, cw)
            y[...] = 1
            cb[...] = 2
            cr[...] = 3
            flat = buf.reshape(-1, n)[0]
            assert (flat[:H * W] == 1).all()
            c = flat[H * W:]
            want = {"i420": [2] * (ch * cw) + [3] * (ch * cw), "yv12": [3] * (ch * cw) + [2] * (ch * cw),
                    "nv12": [2, 3] * (ch * cw), "nv21": [3, 2] * (ch * cw)}.get(layout, [2] * (ch * cw) + [3] * (ch * cw))
            assert c.tolist() == want
            if kind == "torch":
                col = cb.stride(-1)
                assert col == (2 if layout in ("nv12", "nv21") else 1) and cr.stride(-1) == col
                if layout == "nv12":
                    assert cr.data_ptr() == cb.data_ptr() + 1
                if layout == "nv21":
                    assert cb.data_ptr() == cr.data_ptr() + 1


def test_split_yuv_refuses_a_wrong_buffer():
    with pytest.raises(ValueError, match=r"is 43 bytes, the buffer has 37"):
        codec.split_yuv(np.zeros(37, np.uint8), 5, 5, "i420")
    with pytest.raises(ValueError, match=r"is 36 bytes, the buffer has 40"):
        codec.split_yuv(torch.zeros(40, dtype=torch.uint8), 4, 6, "nv12")
    with pytest.raises(ValueError, match="layout"):
        codec.split_yuv(np.zeros(36, np.uint8), 4, 6, "p010")
    with pytest.raises(ValueError, match="uint8"):
        codec.split_yuv(np.zeros(36, np.uint16), 4, 6, "i420")
    with pytest.raises(ValueError, match="non-empty"):
        codec.split_yuv(np.zeros(36, np.uint8), 0, 6, "i420")


# ------------------------------------------------------------------------------------------------- 6. y4m
@pytest.mark.parametrize("tag", ["420jpeg", "420mpeg2", "420", "422", "444"])
def test_y4m_round_trips_bytes_and_tags(tag):
    tool = _tool()
    r = np.random.default_rng(3)
    H, W = 5, 7
    sx, sy = tool.Y4M_TAGS[tag][1]
    ch, cw = -(-H // sy), -(-W // sx)
    frames = [(r.integers(0, 256, (H, W), dtype=np.uint8), r.integers(0, 256, (ch, cw), dtype=np.uint8),
               r.integers(0, 256, (ch, cw), dtype=np.uint8)) for _ in range(2)]
    data = tool.write_y4m(*frames[0], tag)
    y, cb, cr, t, params = tool.read_y4m(data)
    assert t == tag and params == ["F25:1", "Ip", "A1:1"]
    assert all(np.array_equal(a, b) for a, b in zip((y, cb, cr), frames[0]))
    assert tool.write_y4m(y, cb, cr, t, params) == data
    two = data + b"FRAME\n" + b"".join(p.tobytes() for p in frames[1])
    got = tool.read_y4m(two, 1)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], frames[1]))
    with pytest.raises(ValueError, match="no frame 2"):
        tool.read_y4m(two, 2)
    with pytest.raises(ValueError, match="frame 1 is truncated"):
        tool.read_y4m(two[:-1], 1)
    with pytest.raises(ValueError, match="frame 0 is truncated"):
        tool.read_y4m(data[:-1])


def test_y4m_default_tag_and_refusals():
    tool = _tool()
    body = b"FRAME\n" + bytes(4 * 4 + 2 * 2 * 2)
    assert tool.read_y4m(b"YUV4MPEG2 W4 H4 F30:1\n" + body)[3] == "420jpeg"
    for tag in ("420p10", "420paldv", "444alpha", "mono", "422p12", "444p16", "411"):
        with pytest.raises(ValueError, match="C" + tag + " "):
            tool.read_y4m(b"YUV4MPEG2 W4 H4 C" + tag.encode() + b"\n" + body)
        with pytest.raises(ValueError, match="C" + tag + " "):
            tool.write_y4m(np.zeros((4, 4), np.uint8), np.zeros((2, 2), np.uint8), np.zeros((2, 2), np.uint8), tag)
    with pytest.raises(ValueError, match="not a YUV4MPEG2"):
        tool.read_y4m(b"P6\n4 4\n255\n" + body)
    with pytest.raises(ValueError, match="positive W and H"):
        tool.read_y4m(b"YUV4MPEG2 W4 C420\n" + body)
    with pytest.raises(ValueError, match="no frame 0"):
        tool.read_y4m(b"YUV4MPEG2 W4 H4 C420\n")


def test_cli_argument_rules_for_frame_files():
    tool = _tool()
    a = tool.parse_args(["encode", "a.yuv", "o.bit", "--synthetic", "1", "--size", "64x48", "--yuv", "nv12"])
    assert a.frame_file and a.size == (64, 48) and a.yuv == "nv12" and a.matrix == "709" and a.range == "limited"
    a = tool.parse_args(["decode", "o.bit", "a.y4m", "--synthetic", "1", "--ref", "src.y4m"])
    assert a.frame_file and a.yuv == "i420" and a.ref == "src.y4m"
    assert not tool.parse_args(["encode", "a.ppm", "o.bit", "--synthetic", "1"]).frame_file
    for bad in (["encode", "a.ppm", "o.bit", "--synthetic", "1", "--yuv", "nv12"],
                ["encode", "a.y4m", "o.bit", "--synthetic", "1", "--tile", "128"],
                ["encode", "a.y4m", "o.bit", "--synthetic", "1", "--roi", "m.ppm", "--roi-levels", "0", "1"],
                ["decode", "o.bit", "a.ppm", "--synthetic", "1", "--ref", "src.y4m"],
                ["encode", "a.yuv", "o.bit", "--synthetic", "1", "--size", "64"]):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)


# ------------------------------------------------------------------------------------------- 7. refusals
P1, P2, P3, PD, PS = 1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 24


def _desc(**kw):
    d = dict(sub_x=2, sub_y=2, matrix=1, full_range=0, site_x=1, reserved=(0, 0, 0))
    d.update(kw)
    return _lib.YuvDesc(d["sub_x"], d["sub_y"], d["matrix"], d["full_range"], d["site_x"], (C.c_int32 * 3)(*d["reserved"]))


def _s3(s):
    return None if s is None else (C.c_int64 * 3)(*s)


def _ingest_rc(y=P1, ys=(10000, 100, 1), cb=P2, bs=(2500, 50, 1), cr=P3, rs=(2500, 50, 1), desc=True, B=1, H=100, W=100,
               dst=PD, Hp=128, Wp=128, **dkw):
    lib = _lib.lib()
    d = _desc(**dkw)
    rc = lib.mlic_image_ingest_yuv8(None, C.c_void_p(y), _s3(ys), C.c_void_p(cb), _s3(bs), C.c_void_p(cr), _s3(rs),
                                    C.byref(d) if desc else None, B, H, W, C.c_void_p(dst), Hp, Wp)
    return rc, lib.mlic_last_error().decode()


INGEST_REFUSALS = [
    (dict(y=None), "null plane"), (dict(cb=None), "null plane"), (dict(cr=None), "null plane"),
    (dict(dst=None), "null plane or dst"), (dict(ys=None), "null strides"), (dict(bs=None), "null strides"),
    (dict(rs=None), "null strides"), (dict(desc=False), "null mlic_yuv_desc"),
    (dict(B=0), "must be positive"), (dict(H=0), "must be positive"), (dict(W=-1), "must be positive"),
    (dict(Hp=100), "multiples of 64"), (dict(Wp=64), "multiples of 64"), (dict(Hp=64), "multiples of 64"),
    (dict(sub_x=0), "sub_x and sub_y must be 1 or 2"), (dict(sub_y=3), "sub_x and sub_y must be 1 or 2"),
    (dict(sub_x=1, sub_y=2), "4:4:0"), (dict(matrix=2), "matrix must be"), (dict(matrix=-1), "matrix must be"),
    (dict(full_range=2), "full_range must be"), (dict(site_x=2), "site_x must be"),
    (dict(reserved=(0, 1, 0)), "reserved"), (dict(ys=(10000, 100, 0)), "zero column stride"),
    (dict(bs=(2500, 50, 0)), "zero column stride"), (dict(rs=(2500, 50, 0)), "zero column stride"),
    (dict(dst=PD + 2), "4-byte aligned"),
]


@pytest.mark.parametrize("kw,msg", INGEST_REFUSALS)
def test_ingest_yuv8_refuses_bad_arguments_without_a_device(kw, msg):
    rc, text = _ingest_rc(**kw)
    assert rc != 0 and msg in text and ("image_ingest_yuv8" in text or "mlic_yuv_desc" in text), text


def _egress_rc(src=PD, ss=(49152, 16384, 128), B=1, H=100, W=100, desc=True, y=P1, ys=(10000, 100, 1), cb=P2,
               bs=(2500, 50, 1), cr=P3, rs=(2500, 50, 1), ry=None, rys=None, rb=None, rbs=None, rr=None, rrs=None, sq=None,
               **dkw):
    lib = _lib.lib()
    d = _desc(**dkw)
    rc = lib.mlic_image_egress_yuv8(None, C.c_void_p(src), _s3(ss), B, H, W, C.byref(d) if desc else None,
                                    C.c_void_p(y), _s3(ys), C.c_void_p(cb), _s3(bs), C.c_void_p(cr), _s3(rs),
                                    C.c_void_p(ry), _s3(rys), C.c_void_p(rb), _s3(rbs), C.c_void_p(rr), _s3(rrs),
                                    C.c_void_p(sq))
    return rc, lib.mlic_last_error().decode()


REF = dict(ry=P1 + 7, rys=(10000, 100, 1), rb=P2 + 7, rbs=(5000, 100, 2), rr=P2 + 8, rrs=(5000, 100, 2), sq=PS)
EGRESS_REFUSALS = [
    (dict(src=None), "null src or plane"), (dict(y=None), "null src or plane"), (dict(cb=None), "null src or plane"),
    (dict(cr=None), "null src or plane"), (dict(ss=None), "null strides"), (dict(ys=None), "null strides"),
    (dict(desc=False), "null mlic_yuv_desc"), (dict(B=0), "must be positive"), (dict(H=0), "must be positive"),
    (dict(W=0), "must be positive"), (dict(sub_x=4), "sub_x and sub_y must be 1 or 2"),
    (dict(sub_x=1, sub_y=2), "4:4:0"), (dict(matrix=7), "matrix must be"), (dict(full_range=-1), "full_range must be"),
    (dict(site_x=-1), "site_x must be"), (dict(reserved=(0, 0, 9)), "reserved"),
    (dict(bs=(2500, 50, 0)), "zero column stride"), (dict(src=PD + 1), "src must be 4-byte aligned"),
    (dict(sq=PS), "all given or all NULL"), (dict(ry=P1), "all given or all NULL"),
    ({**REF, "sq": None}, "all given or all NULL"), ({**REF, "rb": None}, "all given or all NULL"),
    ({**REF, "rbs": None}, "null ref strides"), ({**REF, "rrs": (5000, 100, 0)}, "zero column stride (ref)"),
    ({**REF, "sq": PS + 4}, "sq_err must be 8-byte aligned"),
]


@pytest.mark.parametrize("kw,msg", EGRESS_REFUSALS)
def test_egress_yuv8_refuses_bad_arguments_without_a_device(kw, msg):
    rc, text = _egress_rc(**kw)
    assert rc != 0 and msg in text and ("image_egress_yuv8" in text or "mlic_yuv_desc" in text), text


def test_yuv_forced_kernel_form_must_fit_the_strides():
    try:
        _lib.call("mlic_set_kernel_option", b"image_io_path", 1)
        rc, msg = _ingest_rc()
        assert rc != 0 and "HWC" in msg
        _lib.call("mlic_set_kernel_option", b"image_io_path", 2)
        rc, msg = _ingest_rc(bs=(2500, 150, 3), rs=(2500, 150, 3))
        assert rc != 0 and "column stride 2" in msg
        rc, msg = _ingest_rc(bs=(5000, 100, 2), rs=(5000, 100, 2))  # column stride 2 but not one interleaved plane
        assert rc != 0 and "column stride 2" in msg
    finally:
        _lib.call("mlic_set_kernel_option", b"image_io_path", -1)


def test_one_image_yuv_entry_points_refuse_without_a_device():
    n, H, W, lv = C.c_size_t(), C.c_int(-5), C.c_int(-5), C.c_int(-5)
    s2 = (C.c_int64 * 2)(100, 1)
    d = _desc()
    with pytest.raises(_lib.MlicError, match="null mlic_model handle"):
        _lib.call("mlic_encode_image_yuv8", None, None, C.c_void_p(P1), s2, C.c_void_p(P2), s2, C.c_void_p(P3), s2,
                  C.byref(d), 100, 100, 1.0, -1, None, 0, C.byref(n))
    data = codec.write_container(100, 150, (2, 3), b"yy", b"z", 3)
    _lib.call("mlic_decode_image_yuv8", None, None, data, len(data), 8, 1 << 28, None, None, None, None, 0, None, None, 0,
              None, None, 0, C.byref(H), C.byref(W), C.byref(lv))
    assert (H.value, W.value, lv.value) == (100, 150, 3)
    with pytest.raises(_lib.MlicError, match="z length runs past the end"):
        _lib.call("mlic_decode_image_yuv8", None, None, data[:-1], len(data) - 1, 8, 1 << 28, None, None, None, None, 0,
                  None, None, 0, None, None, 0, C.byref(H), C.byref(W), C.byref(lv))
    with pytest.raises(_lib.MlicError, match="null mlic_model handle"):
        _lib.call("mlic_decode_image_yuv8", None, None, data, len(data), 8, 1 << 28, None, C.byref(d), C.c_void_p(P1), s2,
                  1 << 20, C.c_void_p(P2), s2, 1 << 20, C.c_void_p(P3), s2, 1 << 20, C.byref(H), C.byref(W), C.byref(lv))


def test_python_layer_refusals():
    y, cb, cr = np.zeros((4, 6), np.uint8), np.zeros((2, 3), np.uint8), np.zeros((2, 3), np.uint8)
    fmt = codec.YuvFormat()
    for kw, msg in ((dict(sub=(1, 2)), "sub must be"), (dict(sub=(3, 1)), "sub must be"), (dict(sub=2), "sub must be"),
                    (dict(matrix="bt2020"), "matrix must be"), (dict(full_range=1), "full_range must be a bool"),
                    (dict(site_x="top"), "site_x must be")):
        with pytest.raises(ValueError, match=msg):
            codec.YuvFormat(**kw)
    with pytest.raises(ValueError, match="fmt must be a YuvFormat"):
        codec.ingest_yuv(y, cb, cr, "i420")
    with pytest.raises(ValueError, match=r"chroma planes \(1, 2, 3\)"):
        codec.ingest_yuv(y, cb, np.zeros((2, 2), np.uint8), fmt)
    with pytest.raises(ValueError, match="bit depths above 8"):
        codec.ingest_yuv(y.astype(np.uint16), cb, cr, fmt)
    with pytest.raises(ValueError, match="empty frame"):
        codec.ingest_yuv(np.zeros((0, 6), np.uint8), cb, cr, fmt)
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match="fp32"):
        codec.egress_yuv(x.double(), 4, 6, fmt)
    with pytest.raises(ValueError, match="crop 65 x 6"):
        codec.egress_yuv(x, 65, 6, fmt)
    with pytest.raises(ValueError, match="out must be three uint8 tensors"):
        codec.egress_yuv(x, 4, 6, fmt, out=(torch.zeros(1, 4, 6, dtype=torch.uint8),) * 3)
    with pytest.raises(ValueError, match="chroma planes"):
        codec.egress_yuv(x, 4, 6, fmt, ref=(y, cb, np.zeros((2, 4), np.uint8)))
    with pytest.raises(ValueError, match="ref must be a frame batch"):
        codec.egress_yuv(x, 4, 6, fmt, ref=(np.zeros((6, 6), np.uint8), np.zeros((3, 3), np.uint8), np.zeros((3, 3), np.uint8)))
    with pytest.raises(ValueError, match="roi= together with Y'CbCr"):
        codec.encode_yuv(None, y, cb, cr, fmt, roi=np.ones((4, 6), np.uint8), roi_levels=(0, 1))
    with pytest.raises(ValueError, match="tiles together with Y'CbCr"):
        codec.encode_yuv(None, y, cb, cr, fmt, tile=128)
    with pytest.raises(ValueError, match="needs max_bpp"):
        codec.encode_yuv(None, y, cb, cr, fmt, level="auto")
    with pytest.raises(ValueError, match="max_bpp must be"):
        codec.encode_yuv(None, y, cb, cr, fmt, max_bpp=-1.0)
    with pytest.raises(ValueError, match="no files"):
        codec.decode_yuv(None, [], fmt)
    with pytest.raises(ValueError, match="tiled files together with Y'CbCr"):
        codec.decode_yuv(None, [b"MLT1" + bytes(40)], fmt)


def test_egress_cpu_out_ref_and_psnr_fields():
    fmt = codec.YuvFormat(sub=(2, 2), matrix="bt601", full_range=True, site_x="centre")
    r = np.random.default_rng(9)
    H, W = 5, 7
    x = torch.from_numpy(r.uniform(0, 1, (2, 3, 64, 64)).astype(np.float32))
    planes = codec.egress_yuv(x, H, W, fmt)
    buf = torch.full((2, codec.yuv_frame_bytes(H, W, "nv12") + 3), 0xA5, dtype=torch.uint8)
    out = codec.split_yuv(buf[:, :-3], H, W, "nv12")
    ref = _frame(r, H, W, fmt)
    ref = tuple(torch.from_numpy(np.stack([p, p[::-1].copy()])) for p in ref)
    got = codec.egress_yuv(x, H, W, fmt, ref=ref, out=out)
    assert all(torch.equal(a, b) for a, b in zip(got[:3], planes)) and bool((buf[:, -3:] == 0xA5).all())
    want = [[int(((a[b].long() - q[b].long()) ** 2).sum()) for a, q in zip(planes, ref)] for b in range(2)]
    assert got[3].dtype == torch.int64 and got[3].tolist() == want
    p = codec.psnr_yuv_from_sq_err(want[0], H, W, fmt)
    assert p["sq_err"] == want[0]
    assert p["psnr_y"] == codec.psnr_from_sq_err(want[0][0], H * W)
    assert p["psnr_u"] == codec.psnr_from_sq_err(want[0][1], 3 * 4)
    assert p["psnr_yuv"] == (6 * p["psnr_y"] + p["psnr_u"] + p["psnr_v"]) / 8


def test_constants_are_the_definitions_folded_in_double_and_rounded_once():
    for m, fr in SETS:
        Kr, Kb, Kg, ys, cs, yo = O.params(m, fr)
        k = codec.YuvFormat(matrix=m, full_range=fr).constants()
        want = {"yo": yo, "cy": 1 / ys, "crv": 2 * (1 - Kr) / cs, "cbu": 2 * (1 - Kb) / cs,
                "cgu": 2 * Kb * (1 - Kb) / (Kg * cs), "cgv": 2 * Kr * (1 - Kr) / (Kg * cs),
                "yr": ys * Kr, "yg": ys * Kg, "yb": ys * Kb, "bb": cs / 2, "rr": cs / 2,
                "br": -cs * Kr / (2 * (1 - Kb)), "bg": -cs * Kg / (2 * (1 - Kb)),
                "rg": -cs * Kg / (2 * (1 - Kr)), "rb": -cs * Kb / (2 * (1 - Kr))}
        assert set(k) == set(want)
        for n, v in want.items():
            assert k[n] == float(np.float32(k[n])) and abs(k[n] - v) <= abs(v) * 2.0 ** -24, (m, fr, n)
    k = codec.YuvFormat(matrix="bt709", full_range=True).constants()
    assert k["cy"] == float.fromhex("0x1.010102p-8") and k["bb"] == 127.5  # 1 / 255 and 255 / 2
    assert codec.YuvFormat(matrix="bt601", full_range=False).constants()["rr"] == 112.0
