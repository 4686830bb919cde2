"""The uint8 codec path without a GPU: the library's bitstream container (writer byte-identical to
bitstream.write_stream, validating parser), the argument refusals of the image kernels' entry points, the torch
restatements of ingest / egress, and the command-line tool's PPM reader / writer.  Every comparison is exact."""
import ctypes as C
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

from mlic_amd import _lib, bitstream, codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXPIX = 1 << 28


def _py_file(H, W, y, z, level=None):
    buf = io.BytesIO()
    n = bitstream.write_stream(buf, H, W, ((H + 63) // 64, (W + 63) // 64), [[y], [z]], level)
    assert n == len(buf.getvalue())
    return buf.getvalue()


def _parse(data, vbr, n_levels=8, max_pixels=MAXPIX):
    """(rc, info, message) of mlic_container_parse on exactly these bytes."""
    lib = _lib.lib()
    info = _lib.ContainerInfo()
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(bytes(data) or b"\0")
    rc = lib.mlic_container_parse(buf, len(data), int(vbr), n_levels if vbr else 0, max_pixels, C.byref(info))
    return rc, info, lib.mlic_last_error().decode() if rc else ""


def _cases():
    r = np.random.default_rng(2024)
    out = [(1, 1, None, b"", b""), (64, 64, 0, b"", b"\x07"), (65, 129, None, b"\x01", b"")]
    for _ in range(40):
        H, W = int(r.integers(1, 5000)), int(r.integers(1, 5000))
        level = None if r.integers(0, 2) else int(r.integers(0, 8))
        y = r.integers(0, 256, int(r.integers(0, 400)), dtype=np.uint8).tobytes()
        z = r.integers(0, 256, int(r.integers(0, 60)), dtype=np.uint8).tobytes()
        out.append((H, W, level, y, z))
    return out


def test_writer_is_byte_identical_to_write_stream():
    for H, W, level, y, z in _cases():
        want = _py_file(H, W, y, z, level)
        got = codec.write_container(H, W, ((H + 63) // 64, (W + 63) // 64), y, z, level)
        assert got == want, (H, W, level, len(y), len(z))
        vbr = level is not None
        assert codec.container_bytes(len(y), len(z), vbr) == bitstream.file_bytes(len(y), len(z), vbr) == len(want)


def test_writer_refuses_a_short_buffer_and_answers_a_size_query():
    n = C.c_size_t()
    _lib.call("mlic_container_write", 10, 20, -1, 1, 1, b"abc", 3, b"de", 2, None, 0, C.byref(n))
    assert n.value == bitstream.file_bytes(3, 2)
    buf = C.create_string_buffer(n.value)
    with pytest.raises(_lib.MlicError, match="buffer too small"):
        _lib.call("mlic_container_write", 10, 20, -1, 1, 1, b"abc", 3, b"de", 2, buf, n.value - 1, C.byref(n))
    with pytest.raises(_lib.MlicError, match="null"):
        _lib.call("mlic_container_write", 10, 20, -1, 1, 1, None, 3, b"de", 2, buf, n.value, C.byref(n))


def test_parse_round_trip_returns_exact_offsets():
    for H, W, level, y, z in _cases():
        vbr = level is not None
        data = _py_file(H, W, y, z, level)
        rc, c, msg = _parse(data, vbr)
        assert rc == 0, msg
        hdr = 12 if vbr else 8
        assert (c.H, c.W, c.hz, c.wz) == (H, W, (H + 63) // 64, (W + 63) // 64)
        assert c.level == (level if vbr else -1)
        assert (c.y_off, c.y_len) == (hdr + 12 + 4, len(y))
        assert (c.z_off, c.z_len) == (hdr + 12 + 4 + len(y) + 4, len(z))
        assert c.z_off + c.z_len == len(data)
        # the Python faces of the parser
        assert bitstream.read_stream_checked(data, vbr, 8) == bitstream.read_stream(io.BytesIO(data), vbr)
        assert bitstream.read_stream_checked(io.BytesIO(data), vbr, 8) == bitstream.read_stream(io.BytesIO(data), vbr)
        p = codec.peek(data, vbr, 8)
        assert (p["H"], p["W"], p["level"], p["shape"], p["bytes"]) == (H, W, level, (c.hz, c.wz), len(data))
        assert p["bpp"] == 8.0 * len(data) / (H * W)


def _be(*words):
    return b"".join(int(w).to_bytes(4, "big") for w in words)


MALFORMED = {
    "empty": (b"", False, "truncated"),
    "header cut in H, W": (_be(100)[:3], False, "truncated"),
    "header cut in level": (_be(100, 150) + b"\0\0", True, "truncated"),
    "header cut in h_z, w_z, n": (_be(100, 150, 2, 3)[:-1], False, "truncated"),
    "cut before the y length": (_be(100, 150, 2, 3, 2), False, "truncated"),
    "cut before the z length": (_be(100, 150, 2, 3, 2, 1) + b"y", False, "truncated"),
    "n_strings 1": (_be(100, 150, 2, 3, 1, 0), False, "n_strings"),
    "n_strings 3": (_be(100, 150, 2, 3, 3, 0, 0, 0), False, "n_strings"),
    "y length past the end": (_be(100, 150, 2, 3, 2, 9) + b"y" * 8, False, "y length runs past the end"),
    "y length 2^32 - 1": (_be(100, 150, 2, 3, 2, 0xFFFFFFFF) + b"y" * 8, False, "y length runs past the end"),
    "z length past the end": (_be(100, 150, 2, 3, 2, 1) + b"y" + _be(5) + b"zzzz", False, "z length runs past the end"),
    "bytes left over": (_be(100, 150, 2, 3, 2, 1) + b"y" + _be(1) + b"zX", False, "left over"),
    "H zero": (_be(0, 150, 0, 3, 2, 0, 0), False, "zero"),
    "W zero": (_be(100, 0, 2, 0, 2, 0, 0), False, "zero"),
    "h_z too small": (_be(100, 150, 1, 3, 2, 0, 0), False, "ceil"),
    "h_z too large": (_be(100, 150, 3, 3, 2, 0, 0), False, "ceil"),
    "w_z wrong": (_be(100, 150, 2, 2, 2, 0, 0), False, "ceil"),
    "above max_pixels": (_be(16385, 16384, 257, 256, 2, 0, 0), False, "max_pixels"),
    "huge sides": (_be(0xFFFFFFFF, 0xFFFFFFFF, 1 << 26, 1 << 26, 2, 0, 0), False, "max_pixels"),
    "level == n_levels": (_be(100, 150, 8, 2, 3, 2, 0, 0), True, "level"),
    "level 2^32 - 1": (_be(100, 150, 0xFFFFFFFF, 2, 3, 2, 0, 0), True, "level"),
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_parser_refuses_malformed_input(name):
    data, vbr, word = MALFORMED[name]
    rc, _, msg = _parse(data, vbr)
    assert rc != 0 and msg and word in msg, (name, msg)
    with pytest.raises(_lib.MlicError):
        codec.peek(data, vbr, 8)
    with pytest.raises(_lib.MlicError):
        bitstream.read_stream_checked(data, vbr, 8)


def test_parser_accepts_the_boundaries():
    assert _parse(_be(16384, 16384, 256, 256, 2, 0, 0), False)[0] == 0           # exactly max_pixels
    assert _parse(_be(100, 150, 7, 2, 3, 2, 0, 0), True)[0] == 0                 # the last level
    assert _parse(_be(100, 150, 2, 3, 2, 0, 0), False, max_pixels=128 * 192)[0] == 0
    assert _parse(_be(100, 150, 2, 3, 2, 0, 0), False, max_pixels=128 * 192 - 1)[0] != 0
    with pytest.raises(_lib.MlicError, match="n_levels"):
        _lib.call("mlic_container_parse", b"", 0, 1, 0, MAXPIX, C.byref(_lib.ContainerInfo()))
    with pytest.raises(_lib.MlicError, match="null info"):
        _lib.call("mlic_container_parse", b"", 0, 0, 0, MAXPIX, None)


def _in_bounds(c, n, vbr):
    return (c.y_off + c.y_len <= n and c.z_off + c.z_len == n and c.y_off + c.y_len + 4 == c.z_off
            and c.H > 0 and c.W > 0 and c.hz == (c.H + 63) // 64 and c.wz == (c.W + 63) // 64
            and 4096 * c.hz * c.wz <= MAXPIX and (0 <= c.level < 8 if vbr else c.level == -1))


@pytest.mark.parametrize("vbr", [False, True])
def test_mutation_sweep_is_refused_or_in_bounds(vbr):
    """Every truncation of one valid file, 3000 single-byte and 3000 four-byte overwrites (seeded): each is
    either refused with a message or parsed to offsets inside the input.  tools/container_check.cpp runs the
    same sweep under AddressSanitizer, which also sees the reads."""
    r = np.random.default_rng(7 + vbr)
    y = r.integers(0, 256, 301, dtype=np.uint8).tobytes()
    z = r.integers(0, 256, 17, dtype=np.uint8).tobytes()
    data = _py_file(100, 150, y, z, 3 if vbr else None)
    n = len(data)
    refused = accepted = 0

    def probe(m):
        nonlocal refused, accepted
        rc, c, msg = _parse(m, vbr)
        if rc:
            assert msg
            refused += 1
        else:
            assert _in_bounds(c, len(m), vbr), (bytes(m[:32]), c.y_off, c.y_len, c.z_off, c.z_len)
            accepted += 1

    for k in range(n + 1):
        probe(data[:k])
    assert refused == n and accepted == 1
    for _ in range(3000):
        m = bytearray(data)
        m[int(r.integers(0, n))] = int(r.integers(0, 256))
        probe(m)
    for i in range(3000):
        m = bytearray(data)
        at = int(r.integers(0, n - 3))
        word = int(r.integers(0, 1 << 32)) if i & 1 else int(r.integers(0, 4096))
        m[at:at + 4] = word.to_bytes(4, "big")
        probe(m)
    assert refused > n and accepted > 1


# ------------------------------------------------------------------------- entry points without a device
def _ingest_rc(src=1 << 20, strides=(30000, 300, 3, 1), B=1, H=100, W=100, dst=1 << 21, Hp=128, Wp=128):
    lib = _lib.lib()
    s = None if strides is None else (C.c_int64 * 4)(*strides)
    rc = lib.mlic_image_ingest_u8(None, C.c_void_p(src), s, B, H, W, C.c_void_p(dst), Hp, Wp)
    return rc, lib.mlic_last_error().decode()


@pytest.mark.parametrize("kw", [dict(src=None), dict(dst=None), dict(strides=None), dict(B=0), dict(H=0), dict(W=-1),
                                dict(Hp=100), dict(Wp=192 + 32), dict(Hp=64), dict(Wp=64),
                                dict(strides=(30000, 300, 0, 1)), dict(strides=(30000, 300, 3, 0))])
def test_ingest_refuses_bad_arguments_without_a_device(kw):
    rc, msg = _ingest_rc(**kw)
    assert rc != 0 and "image_ingest_u8" in msg, msg


def _egress_rc(src=1 << 20, ss=(49152, 16384, 128), B=1, H=100, W=100, dst=1 << 21, ds=(30000, 300, 3, 1), ref=None,
               rs=None, sq=None):
    lib = _lib.lib()
    a3 = None if ss is None else (C.c_int64 * 3)(*ss)
    a4 = None if ds is None else (C.c_int64 * 4)(*ds)
    r4 = None if rs is None else (C.c_int64 * 4)(*rs)
    rc = lib.mlic_image_egress_u8(None, C.c_void_p(src), a3, B, H, W, C.c_void_p(dst), a4, C.c_void_p(ref), r4,
                                  C.c_void_p(sq))
    return rc, lib.mlic_last_error().decode()


@pytest.mark.parametrize("kw", [dict(src=None), dict(dst=None), dict(ss=None), dict(ds=None), dict(B=0), dict(H=0),
                                dict(W=0), dict(ds=(30000, 300, 0, 1)), dict(ds=(30000, 300, 3, 0)),
                                dict(ref=1 << 22), dict(sq=1 << 23), dict(ref=1 << 22, sq=1 << 23),
                                dict(ref=1 << 22, sq=1 << 23, rs=(30000, 300, 0, 1))])
def test_egress_refuses_bad_arguments_without_a_device(kw):
    rc, msg = _egress_rc(**kw)
    assert rc != 0 and "image_egress_u8" in msg, msg


def test_forced_kernel_form_must_fit_the_layout():
    try:
        _lib.call("mlic_set_kernel_option", b"image_io_path", 1)
        rc, msg = _ingest_rc(strides=(30000, 100, 1, 10000))
        assert rc != 0 and "HWC" in msg
        _lib.call("mlic_set_kernel_option", b"image_io_path", 2)
        rc, msg = _ingest_rc()
        assert rc != 0 and "CHW" in msg
        with pytest.raises(_lib.MlicError):
            _lib.call("mlic_set_kernel_option", b"image_io_path", 3)
    finally:
        _lib.call("mlic_set_kernel_option", b"image_io_path", -1)


def test_image_codec_entry_points_refuse_without_a_device():
    n, H, W, lv = C.c_size_t(), C.c_int(-5), C.c_int(-5), C.c_int(-5)
    s3 = (C.c_int64 * 3)(300, 3, 1)
    with pytest.raises(_lib.MlicError, match="null mlic_model handle"):
        _lib.call("mlic_encode_image_u8", None, None, C.c_void_p(1 << 20), s3, 100, 100, 1.0, -1, None, 0, C.byref(n))
    # a parse-only decode needs neither a model nor a device, and refuses what the parser refuses
    data = _py_file(100, 150, b"yy", b"z", 3)
    _lib.call("mlic_decode_image_u8", None, None, data, len(data), 8, MAXPIX, None, None, None, 0, C.byref(H),
              C.byref(W), C.byref(lv))
    assert (H.value, W.value, lv.value) == (100, 150, 3)
    data = _py_file(100, 150, b"yy", b"z")
    _lib.call("mlic_decode_image_u8", None, None, data, len(data), 0, MAXPIX, None, None, None, 0, C.byref(H),
              C.byref(W), C.byref(lv))
    assert (H.value, W.value, lv.value) == (100, 150, -1)
    with pytest.raises(_lib.MlicError, match="z length runs past the end"):
        _lib.call("mlic_decode_image_u8", None, None, data[:-1], len(data) - 1, 0, MAXPIX, None, None, None, 0,
                  C.byref(H), C.byref(W), C.byref(lv))
    with pytest.raises(_lib.MlicError, match="max_pixels"):
        _lib.call("mlic_decode_image_u8", None, None, data, len(data), 0, 128 * 192 - 1, None, None, None, 0,
                  C.byref(H), C.byref(W), C.byref(lv))
    # pixels asked for: the handle is checked after the file, before any GPU call
    with pytest.raises(_lib.MlicError, match="null mlic_model handle"):
        _lib.call("mlic_decode_image_u8", None, None, data, len(data), 0, MAXPIX, None, C.c_void_p(1 << 20), s3,
                  1 << 20, C.byref(H), C.byref(W), C.byref(lv))


# --------------------------------------------------------------------------------- CPU restatements
def _ramp_image(H, W, seed=0):
    """uint8 [H, W, 3] holding all 256 values when H * W * 3 >= 256."""
    img = (np.arange(H * W * 3, dtype=np.int64) * 37 + seed).astype(np.uint8).reshape(H, W, 3)
    return torch.from_numpy(img)


@pytest.mark.parametrize("shape", [(1, 1), (63, 65), (64, 64), (65, 127)])
def test_cpu_ingest_is_pad64_of_float_div_255(shape):
    H, W = shape
    img = torch.stack([_ramp_image(H, W, 0), _ramp_image(H, W, 101)])
    want = bitstream.pad64(img.permute(0, 3, 1, 2).float().div(255))
    got = codec.ingest_u8(img, "hwc")
    assert got.dtype == torch.float32 and got.is_contiguous() and got.shape == want.shape
    assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32))
    chw = img.permute(0, 3, 1, 2).contiguous()
    assert torch.equal(codec.ingest_u8(chw, "chw").view(torch.int32), got.view(torch.int32))
    assert torch.equal(codec.ingest_u8(img[0], "hwc"), got[:1])          # one image
    assert torch.equal(codec.ingest_u8(img.numpy(), "hwc"), got)         # a numpy array
    assert got[:, :, H:].abs().sum() == 0 and got[:, :, :, W:].abs().sum() == 0


def test_cpu_true_division_is_not_the_reciprocal_product():
    k = torch.arange(256, dtype=torch.uint8)
    div = k.float().div(255)
    assert int((div != k.float() * torch.tensor(1.0 / 255.0, dtype=torch.float32)).sum()) == 126
    got = codec.ingest_u8(k.view(1, 1, 256, 1).expand(1, 1, 256, 3), "hwc")[0, 0, 0, :256]
    assert torch.equal(got.view(torch.int32), div.view(torch.int32))


@pytest.mark.parametrize("layout", ["hwc", "chw"])
def test_cpu_egress_inverts_ingest_and_counts_squared_errors(layout):
    H, W = 65, 127
    img = torch.stack([_ramp_image(H, W, 0), _ramp_image(H, W, 9)])
    assert len(torch.unique(img[0])) == 256
    src = img if layout == "hwc" else img.permute(0, 3, 1, 2).contiguous()
    x = codec.ingest_u8(src, layout)
    back = codec.egress_u8(x, H, W, layout)
    assert back.dtype == torch.uint8 and torch.equal(back, src)
    r = np.random.default_rng(5)
    noisy = (x + torch.from_numpy(r.normal(0, 0.05, tuple(x.shape)).astype(np.float32)))
    ref = src.flip(0)
    out, sq = codec.egress_u8(noisy, H, W, layout, ref=ref)
    want_img = bitstream.to_u8(noisy[:, :, :H, :W])
    want_img = want_img.permute(0, 2, 3, 1) if layout == "hwc" else want_img
    assert torch.equal(out, want_img)
    want = ((out.numpy().astype(np.int64) - ref.numpy().astype(np.int64)) ** 2).reshape(2, -1).sum(1)
    assert sq.dtype == torch.int64 and sq.tolist() == want.tolist() and want.min() > 0
    # a strided destination: only the crop's bytes change
    canvas = torch.full((2, H + 3, W + 5, 3) if layout == "hwc" else (2, 3, H + 3, W + 5), 0xA5, dtype=torch.uint8)
    win = canvas[:, 1:H + 1, 2:W + 2] if layout == "hwc" else canvas[:, :, 1:H + 1, 2:W + 2]
    codec.egress_u8(noisy, H, W, layout, out=win)
    assert torch.equal(win, want_img)
    mask = torch.ones_like(canvas, dtype=torch.bool)
    (mask[:, 1:H + 1, 2:W + 2] if layout == "hwc" else mask[:, :, 1:H + 1, 2:W + 2]).fill_(False)
    assert bool((canvas[mask] == 0xA5).all())


def test_python_argument_errors():
    with pytest.raises(ValueError):
        codec.ingest_u8(torch.zeros(4, 4, 3))                               # not uint8
    with pytest.raises(ValueError):
        codec.ingest_u8(torch.zeros(4, 4, 4, dtype=torch.uint8), "hwc")     # not 3 channels
    with pytest.raises(ValueError):
        codec.ingest_u8(torch.zeros(4, 4, 3, dtype=torch.uint8), "xyz")
    with pytest.raises(ValueError):
        codec.egress_u8(torch.zeros(1, 3, 64, 64), 65, 64)                  # crop larger than the source
    with pytest.raises(ValueError):
        codec.egress_u8(torch.zeros(1, 3, 64, 64), 64, 64, ref=torch.zeros(1, 60, 64, 3, dtype=torch.uint8))
    assert codec.psnr_from_sq_err(0, 10) == float("inf")
    assert codec.psnr_from_sq_err(3 * 4 * 4, 3 * 4 * 4) == pytest.approx(20 * np.log10(255.0))


# ------------------------------------------------------------------------------------------- the CLI
def _cli():
    spec = importlib.util.spec_from_file_location("mlic_codec_cli", os.path.join(ROOT, "tools", "mlic_codec.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_ppm_round_trip(tmp_path):
    cli = _cli()
    img = _ramp_image(7, 5).numpy()
    data = cli.write_ppm(img)
    assert data.startswith(b"P6\n5 7\n255\n") and len(data) == 11 + 7 * 5 * 3
    assert np.array_equal(cli.read_ppm(data), img)
    # comments and free-form whitespace in the header; pixel bytes that look like whitespace or '#'
    raw = bytes([0x20, 0x0A, 0x23] * 5)
    assert np.array_equal(cli.read_ppm(b"P6 # made by hand\n# again\n5\t1\n255\n" + raw).reshape(-1),
                          np.frombuffer(raw, np.uint8))
    for bad in (b"P5\n5 7\n255\n" + bytes(105), b"P6\n5 7\n65535\n" + bytes(210), b"P6\n5 7\n255\n" + bytes(104),
                b"P6\n5 7\n", b"P6\n0 7\n255\n", b"P6\nfive 7\n255\n" + bytes(105)):
        with pytest.raises(ValueError):
            cli.read_ppm(bad)
    p = tmp_path / "a.ppm"
    cli.save_image(str(p), img)
    assert np.array_equal(cli.load_image(str(p)), img)
