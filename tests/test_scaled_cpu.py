"""Scaled coding without a GPU (DESIGN.md section 5 "Scaled coding"): the library's resampler tables against the
float64 oracle (tests/resample_oracle.py), the oracle against torch and PIL, the fp32 CPU restatement of the two
kernels against the oracle within a bound derived from the tables, the scaled container through the built library,
and the argument policy of encode_images / decode_images."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resample_oracle as ro
from mlic_amd import _lib, codec

FILTERS = ["lanczos3", "bicubic", "triangle"]
U = 2.0 ** -24  # fp32 unit roundoff


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("flt", FILTERS)
def test_tables_match_the_oracle(flt):
    for Li, Lo in ro.axis_pairs():
        start, count, w = codec.resample_table(flt, Li, Lo)
        s2, c2, w2 = ro.table(flt, Li, Lo)
        assert np.array_equal(start, s2) and np.array_equal(count, c2), (Li, Lo)
        assert w.shape == (Lo, int(count.max())) and w.dtype == np.float32
        for o in range(Lo):
            # the double-precision error is far below half an fp32 ulp: only a rounding tie can differ
            assert _ulps(w[o, :count[o]], w2[o].astype(np.float32)).max() <= 1, (Li, Lo, o)
            assert not w[o, count[o]:].any()


@pytest.mark.parametrize("flt", FILTERS)
def test_identity_table_is_exact(flt):
    for L in (1, 7, 130):
        start, count, w = codec.resample_table(flt, L, L)
        assert np.array_equal(start, np.arange(L)) and np.array_equal(count, np.ones(L)) and w.shape == (L, 1)
        assert np.array_equal(w.view(np.int32), np.full((L, 1), np.float32(1.0).view(np.int32)))


def test_tap_bound_holds_at_the_ends_of_the_ratio_range():
    for flt in FILTERS:
        a = ro.RADIUS[flt]
        for Li, Lo in ((8, 1), (800, 100), (797, 100), (1031, 129)):  # 1/8 and just inside it
            _, count, w = codec.resample_table(flt, Li, Lo)
            assert w.shape[1] == count.max() <= 2 * a * 8 + 1 <= 49
        for Li, Lo in ((1, 8), (100, 800), (100, 799)):
            _, count, w = codec.resample_table(flt, Li, Lo)
            assert w.shape[1] == count.max() <= 2 * a + 1
    for Li, Lo in ((100, 801), (801, 100), (1, 9)):
        with pytest.raises(_lib.MlicError, match=r"\[1/8, 8\]"):
            codec.resample_table("lanczos3", Li, Lo)
    with pytest.raises(ValueError, match="filter"):
        codec.resample_table("nearest", 8, 8)
    taps = C.c_int()
    with pytest.raises(_lib.MlicError, match="go together"):
        _lib.call("mlic_resample_table", 0, 8, 4, (C.c_int32 * 4)(), None, None, 0, C.byref(taps))
    with pytest.raises(_lib.MlicError, match="stride"):
        _lib.call("mlic_resample_table", 0, 8, 4, (C.c_int32 * 4)(), (C.c_int32 * 4)(), (C.c_float * 64)(), 2,
                  C.byref(taps))


# ------------------------------------------------------------------------------ oracle cross-checks
def _float_image(H, W, seed=0):
    return np.random.default_rng(seed + 100 * H + W).uniform(0, 1, (2, 3, H, W))


@pytest.mark.parametrize("flt,mode", [("bicubic", "bicubic"), ("triangle", "bilinear")])
def test_oracle_matches_torch_antialias_in_float64(flt, mode):
    for (hi, wi), (ho, wo) in ro.SHAPES:
        if (hi, wi) == (ho, wo):
            continue
        v = _float_image(hi, wi)
        want = F.interpolate(torch.from_numpy(v), size=(ho, wo), mode=mode, antialias=True, align_corners=False).numpy()
        assert np.abs(ro.resample(v, (ho, wo), flt) - want).max() <= 1e-6, ((hi, wi), (ho, wo))


def test_oracle_matches_pil_lanczos():
    Image = pytest.importorskip("PIL.Image")
    for (hi, wi), (ho, wo) in ro.SHAPES:
        if (hi, wi) == (ho, wo):
            continue
        v = _float_image(hi, wi)[0, 0].astype(np.float32)
        want = np.asarray(Image.fromarray(v, mode="F").resize((wo, ho), Image.LANCZOS), dtype=np.float64)
        assert np.abs(ro.resample(v.astype(np.float64), (ho, wo), "lanczos3") - want).max() <= 1e-6, ((hi, wi), (ho, wo))


# --------------------------------------------------------------------------- fp32 CPU restatement
def _bound(flt, src, size):
    """|fp32 two-pass result - float64 oracle| for inputs in [0, 1], from the tables alone.
    Horizontal pass, n_x taps, S_x = max row sum of |w|: the input carries one rounding (byte / 255, relative U),
    each weight one rounding (relative U) and the recursive sum of n products at most gamma_n = n U / (1 - n U)
    relative to sum |w| |v| <= S_x (Higham, Accuracy and Stability, 3.1: n products and n - 1 live additions, the
    first addition to +0 being exact), so |t - t_exact| <= (n_x + 2) U S_x to first order, and |t| <= S_x.  The
    vertical pass multiplies the incoming error by at most S_y and adds (n_y + 1) U S_y max|t|.  Together
    (n_x + n_y + 3) U S_x S_y; the factor 1.01 covers the second-order terms (n U < 3e-6)."""
    (hi, wi), (ho, wo) = src, size
    _, cx, wx = codec.resample_table(flt, wi, wo)
    _, cy, wy = codec.resample_table(flt, hi, ho)
    sx, sy = float(np.abs(wx.astype(np.float64)).sum(1).max()), float(np.abs(wy.astype(np.float64)).sum(1).max())
    assert sx <= 1.56 and sy <= 1.56
    return 1.01 * U * sx * sy * (int(cx.max()) + int(cy.max()) + 3)


@pytest.mark.parametrize("flt", FILTERS)
def test_cpu_ingest_matches_the_oracle_within_the_derived_bound(flt):
    for (hi, wi), (ho, wo) in ro.SHAPES:
        img = torch.from_numpy(np.random.default_rng(hi * 1000 + wi).integers(0, 256, (2, hi, wi, 3), dtype=np.uint8))
        img[1, : hi // 2] = 255  # edges where lanczos and bicubic overshoot: the clamp acts
        img[1, hi // 2:] = 0
        got = codec.ingest_u8_scaled(img, (ho, wo), flt)
        assert tuple(got.shape) == (2, 3, (ho + 63) // 64 * 64, (wo + 63) // 64 * 64) and got.dtype == torch.float32
        assert not got[:, :, ho:].any() and not got[:, :, :, wo:].any()
        want = np.clip(ro.resample(img.permute(0, 3, 1, 2).numpy().astype(np.float64) / 255.0, (ho, wo), flt), 0, 1)
        err = np.abs(got[:, :, :ho, :wo].numpy().astype(np.float64) - want).max()
        assert err <= _bound(flt, (hi, wi), (ho, wo)), ((hi, wi), (ho, wo), err)
        for layout, t in (("chw", img.permute(0, 3, 1, 2)), ("hwc", img[:, :, :, :])):
            assert torch.equal(codec.ingest_u8_scaled(t, (ho, wo), flt, layout), got)
    img = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (70, 130, 3), dtype=np.uint8))
    assert torch.equal(codec.ingest_u8_scaled(img, (70, 130), flt), codec.ingest_u8(img))


@pytest.mark.parametrize("flt", FILTERS)
def test_cpu_egress_matches_the_oracle_within_the_derived_bound(flt):
    for (h, w), (ho, wo) in ro.SHAPES:
        r = np.random.default_rng(h * 1000 + w + 1)
        x = torch.from_numpy(r.uniform(-0.25, 1.25, (2, 3, h + 3, w + 2)).astype(np.float32))
        got, sq = codec.egress_u8_scaled(x, h, w, (ho, wo), flt, ref=torch.zeros(2, ho, wo, 3, dtype=torch.uint8))
        assert tuple(got.shape) == (2, ho, wo, 3) and got.dtype == torch.uint8
        assert sq.tolist() == (got.numpy().astype(np.int64) ** 2).reshape(2, -1).sum(1).tolist()
        v = np.clip(x[:, :, :h, :w].numpy().astype(np.float64), 0, 1)
        want = np.clip(ro.resample(v, (ho, wo), flt), 0, 1) * 255.0
        # floor is discontinuous: the byte may differ by one only where the exact value is within the bound (scaled
        # to bytes, plus the product's own rounding) of an integer
        tol = 255.0 * (_bound(flt, (h, w), (ho, wo)) + U)
        g = got.permute(0, 3, 1, 2).numpy().astype(np.float64)
        lo, hi = np.floor(np.clip(want - tol, 0, 255)), np.floor(np.clip(want + tol, 0, 255))
        assert ((g >= lo) & (g <= hi)).all(), ((h, w), (ho, wo))
        assert (g != np.floor(want)).mean() < 0.01
        assert torch.equal(codec.egress_u8_scaled(x, h, w, (ho, wo), flt, "chw"), got.permute(0, 3, 1, 2))
    x = torch.rand(1, 3, 70, 130)
    x[0, 0, 3, 5] = float("nan")
    assert torch.equal(codec.egress_u8_scaled(x, 70, 130, (70, 130), flt), codec.egress_u8(torch.nan_to_num(x, nan=0.0), 70, 130))
    z = x.clone()
    z[0, 0, 3, 5] = 0.0
    assert torch.equal(codec.egress_u8_scaled(x, 70, 130, (35, 97), flt), codec.egress_u8_scaled(z, 70, 130, (35, 97), flt))


def test_kernel_argument_refusals_on_the_cpu():
    img = torch.zeros(16, 16, 3, dtype=torch.uint8)
    for size, msg in (((1, 16), "ratio range"), ((16, 129), "ratio range"), ((0, 16), "positive"), ((16,), "pair"),
                      ((8.0, 8), "positive integers")):
        with pytest.raises(ValueError, match=msg):
            codec.ingest_u8_scaled(img, size)
    with pytest.raises(ValueError, match="filter"):
        codec.ingest_u8_scaled(img, (8, 8), "cubic")
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match="crop"):
        codec.egress_u8_scaled(x, 65, 64, (64, 64))
    with pytest.raises(ValueError, match="ratio range"):
        codec.egress_u8_scaled(x, 64, 64, (7, 64))
    with pytest.raises(ValueError, match="ref must have shape"):
        codec.egress_u8_scaled(x, 64, 64, (32, 32), ref=torch.zeros(1, 64, 64, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="out must be"):
        codec.egress_u8_scaled(x, 64, 64, (32, 32), out=torch.zeros(1, 64, 64, 3, dtype=torch.uint8))


# --------------------------------------------------------------------------------------- containers
def _inner(h, w, level=None, y=b"0123456789", z=b"abc"):
    return codec.write_container(h, w, ((h + 63) // 64, (w + 63) // 64), y, z, level)


@pytest.mark.parametrize("level", [None, 4])
def test_scaled_container_round_trip(level):
    inner = _inner(50, 75, level)
    for f, name in enumerate(codec.FILTERS):
        data = codec.write_container_scaled(100, 150, inner, name, vbr=level is not None)
        assert data == b"MLS1" + bytes([0, int(level is not None), f, 0]) + (100).to_bytes(4, "big") + \
            (150).to_bytes(4, "big") + inner
        assert codec.is_scaled_file(data) and not codec.is_scaled_file(inner) and not codec.is_tiled_file(data)
        s = codec.parse_container_scaled(data, n_levels=6)
        assert (s.H, s.W, s.filter, bool(s.vbr), s.inner_off, s.inner_len) == (100, 150, f, level is not None, 16, len(inner))
        c = s.inner
        assert (c.H, c.W, c.hz, c.wz, c.level) == (50, 75, 1, 2, -1 if level is None else level)
        assert data[16 + c.y_off:16 + c.y_off + c.y_len] == b"0123456789" and data[16 + c.z_off:][:c.z_len] == b"abc"
        d = codec.peek(data)
        assert d == {"scaled": True, "H": 100, "W": 150, "coded": (50, 75), "filter": name, "vbr": level is not None,
                     "level": level, "shape": (1, 2), "Hp": 64, "Wp": 128, "y_len": 10, "z_len": 3, "bytes": len(data),
                     "bpp": 8.0 * len(data) / 15000}
        # the plain parsers refuse it, as they refuse a tiled file (read as H, W the header is 1.3e9 x at most 65795)
        for vbr in (False, True):
            with pytest.raises(_lib.MlicError, match="max_pixels|h_z, w_z|H or W is zero"):
                codec.parse_container(data, vbr=vbr)
        with pytest.raises(_lib.MlicError, match="magic"):
            codec.parse_container_tiled(data)


def test_scaled_container_refusals_each_with_its_own_message():
    inner = _inner(50, 75, 3)
    data = codec.write_container_scaled(100, 150, inner, "lanczos3", vbr=True)

    def mutated(at, value):
        m = bytearray(data)
        m[at:at + len(value)] = value
        return bytes(m)

    cases = [(data[:15], "container_parse_scaled: truncated header"), (mutated(0, b"X"), "bad magic"),
             (mutated(4, b"\x01"), "unknown version"), (mutated(5, b"\x03"), "unknown flags"),
             (mutated(6, b"\x03"), "unknown filter"), (mutated(7, b"\x01"), "reserved byte"),
             (mutated(8, bytes(4)), "container_parse_scaled: H or W is zero"),
             (mutated(12, bytes(4)), "container_parse_scaled: H or W is zero"),
             (mutated(8, (401).to_bytes(4, "big")), "ratio"), (mutated(12, (9).to_bytes(4, "big")), "ratio"),
             (data[:16], "container_parse: truncated header"), (data[:-1], "runs past the end"),
             (data + b"\0", "left over"), (mutated(16, bytes(4)), "container_parse: H or W is zero"),
             (mutated(24, (6).to_bytes(4, "big")), "level is not below n_levels"),
             (mutated(5, b"\x00"), "container_parse"), (mutated(28, (2).to_bytes(4, "big")), "h_z, w_z")]
    seen = set()
    for bad, msg in cases:
        with pytest.raises(_lib.MlicError, match=msg) as e:
            codec.parse_container_scaled(bad, n_levels=6)
        seen.add(str(e.value))
    assert len(seen) >= 14  # the refusals have their own messages
    with pytest.raises(_lib.MlicError, match="image exceeds max_pixels"):
        codec.parse_container_scaled(data, n_levels=6, max_pixels=100 * 150 - 1)
    assert codec.parse_container_scaled(mutated(8, (400).to_bytes(4, "big")), 6).H == 400  # ratio 8 is legal
    n = C.c_size_t()
    for args, msg in (((0, 150, 1, 0, inner, len(inner)), "H or W is zero"), ((100, 150, 1, 3, inner, len(inner)), "filter"),
                      ((100, 150, 1, 0, inner, 0), "empty inner"), ((100, 150, 1, -1, inner, len(inner)), "negative filter")):
        with pytest.raises(_lib.MlicError, match=msg):
            _lib.call("mlic_container_write_scaled", *args, C.create_string_buffer(64), 64, C.byref(n))
    with pytest.raises(_lib.MlicError, match="buffer too small"):
        _lib.call("mlic_container_write_scaled", 100, 150, 1, 0, inner, len(inner), C.create_string_buffer(20), 20, C.byref(n))
    assert n.value == 16 + len(inner)


def test_scaled_container_mutation_sweep_through_the_library():
    """Every truncation is refused; a seeded sweep of overwrites is refused with a message or parses to fields inside
    the file and inside the ratio range (the stand-alone tools/container_scaled_check.cpp runs the same sweep under
    the sanitizers)."""
    r = np.random.default_rng(0)
    for level in (None, 2):
        data = codec.write_container_scaled(100, 150, _inner(50, 75, level, bytes(r.integers(0, 256, 37, dtype=np.uint8))),
                                            "bicubic", vbr=level is not None)
        for n in range(len(data)):
            with pytest.raises(_lib.MlicError):
                codec.parse_container_scaled(data[:n], 6)
        refused = accepted = 0
        for i in range(3000):
            m = bytearray(data)
            at = int(r.integers(0, min(len(m), 56) if i & 3 else len(m)))
            if i & 1:
                m[at] = int(r.integers(0, 256))
            else:
                m[at:at + 4] = int(r.integers(0, 4096 if i & 4 else 1 << 32)).to_bytes(4, "big")
                m = m[:len(data)]
            try:
                s = codec.parse_container_scaled(bytes(m), 6)
            except _lib.MlicError as e:
                assert len(str(e)) > 10
                refused += 1
                continue
            accepted += 1
            c, n = s.inner, len(m) - 16
            assert s.inner_off == 16 and s.inner_len == n and s.filter <= 2 and s.H * s.W <= codec.MAX_PIXELS
            assert c.y_off + c.y_len <= n and c.z_off + c.z_len <= n
            assert c.H <= 8 * s.H and s.H <= 8 * c.H and c.W <= 8 * s.W and s.W <= 8 * c.W
        assert refused > 100 and accepted > 100


# ------------------------------------------------------------------------------------------- policy
def test_the_scale_to_coded_size_rule():
    # per axis max(1, floor(L * scale + 1/2)): round to nearest in exact arithmetic, a tie goes up
    assert codec.coded_size(100, 150, Fraction(1, 2)) == (50, 75)
    assert codec.coded_size(101, 151, Fraction(1, 2)) == (51, 76)  # 50.5 and 75.5: ties go up
    assert codec.coded_size(5, 7, Fraction(1, 2)) == (3, 4)        # 2.5 -> 3 (round() would give 2)
    assert codec.coded_size(1080, 1920, "1/2") == (540, 960) and codec.coded_size(1080, 1920, "2/3") == (720, 1280)
    assert codec.coded_size(3, 1000, Fraction(1, 8)) == (1, 125)   # 0.375 -> 0 -> at least 1
    assert codec.coded_size(10, 10, 2) == (20, 20) and codec.coded_size(10, 10, 0.5) == (5, 5)
    assert codec.coded_size(7, 9, Fraction(1, 3)) == (2, 3)
    for bad in (0, -1, "x", None, True, Fraction(0)):
        with pytest.raises(ValueError, match="scale"):
            codec.coded_size(10, 10, bad)


class _Net:
    """A model that must not be reached: the refusals come before any device work."""
    device = torch.device("cpu")

    def compress(self, *a, **k):
        raise AssertionError("compress reached")

    decompress = compress


class _VbrNet(_Net):
    levels = 6


def test_encode_images_argument_refusals():
    img = torch.zeros(2, 64, 96, 3, dtype=torch.uint8)
    net = _Net()
    for kw, msg in (({"coded_size": (32, 48), "scale": Fraction(1, 2)}, "pass one"),
                    ({"coded_size": (32, 48), "filter": "nearest"}, "filter must be one of"),
                    ({"coded_size": (32,)}, "pair"), ({"coded_size": (0, 48)}, "positive integers"),
                    ({"coded_size": (7, 48)}, "ratio range"), ({"coded_size": (32, 769)}, "ratio range"),
                    ({"scale": Fraction(1, 9)}, "ratio range"), ({"scale": 9}, "ratio range"), ({"scale": 0}, "scale"),
                    ({"scale": Fraction(1, 2), "depth": 10}, "together with depth="),
                    ({"scale": Fraction(1, 2), "max_bpp": -1.0}, "max_bpp")):
        with pytest.raises(ValueError, match=msg):
            codec.encode_images(net, img, **kw)
    with pytest.raises(ValueError, match="together with roi="):
        codec.encode_images(_VbrNet(), img, scale=Fraction(1, 2), roi=torch.ones(2, 64, 96, dtype=torch.uint8), roi_levels=(0, 3))
    with pytest.raises(ValueError, match="variable-rate model needs level"):
        codec.encode_images(_VbrNet(), img, scale=Fraction(1, 2))
    with pytest.raises(ValueError, match="together with tiles"):
        codec.encode_tiled(net, img[0], scale=Fraction(1, 2))
    with pytest.raises(ValueError, match="together with tiles"):
        codec.encode_tiled(net, img[0], coded_size=(32, 48))
    y, c = torch.zeros(1, 64, 96, dtype=torch.uint8), torch.zeros(1, 32, 48, dtype=torch.uint8)
    with pytest.raises(ValueError, match="together with Y'CbCr"):
        codec.encode_yuv(net, y, c, c, codec.YuvFormat(), scale=Fraction(1, 2))


def test_decode_images_argument_refusals():
    net = _Net()
    plain = _inner(50, 75)
    scaled = codec.write_container_scaled(100, 150, plain)
    for kw, msg in (({"out_size": (50,)}, "pair"), ({"out_size": (0, 5)}, "positive integers"),
                    ({"out_size": (6, 75)}, "ratio range"), ({"out_size": (50, 601)}, "ratio range"),
                    ({"out_size": (50, 75), "filter": "nearest"}, "filter must be one of"),
                    ({"out_size": (50, 75), "depth": 10}, "together with depth=")):
        with pytest.raises(ValueError, match=msg):
            codec.decode_images(net, [plain], **kw)
    with pytest.raises(ValueError, match="filter= given"):
        codec.decode_images(net, [plain], filter="bicubic")
    with pytest.raises(ValueError, match="together with depth="):
        codec.decode_images(net, [scaled], depth=10)
    with pytest.raises(ValueError, match="ref must be uint8"):
        codec.decode_images(_Decodes(), [scaled], ref=torch.zeros(1, 50, 75, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="has no level word, the model is variable-rate"):
        codec.decode_images(_VbrNet(), [scaled])
    with pytest.raises(ValueError, match="carries a level word, the model is fixed-rate"):
        codec.decode_images(net, [codec.write_container_scaled(100, 150, _inner(50, 75, 2), vbr=True)])
    with pytest.raises(ValueError, match="share one padded"):
        codec.decode_images(net, [scaled, codec.write_container_scaled(100, 150, _inner(100, 150))])
    with pytest.raises(ValueError, match="together with tiles"):
        codec.decode_tiled(net, scaled)
    with pytest.raises(ValueError, match="together with tiles"):
        codec.decode_tiled(net, b"MLT1", out_size=(10, 10))
    with pytest.raises(ValueError, match="together with Y'CbCr"):
        codec.decode_yuv(net, [scaled], codec.YuvFormat())
    with pytest.raises(ValueError, match="together with Y'CbCr"):
        codec.decode_yuv(net, [plain], codec.YuvFormat(), out_size=(10, 10))
    roi = codec.write_container_roi(50, 75, (1, 2), b"0123", b"ab", 3, np.array([[1, 3]]))
    with pytest.raises(ValueError, match="together with ROI files"):
        codec.decode_images(_VbrNet(), [roi], out_size=(25, 38))


class _Decodes(_Net):
    """decompress gives a fixed x_hat: the CPU egress runs, so the whole decode path of a scaled file does."""

    def decompress(self, strings, shape, **kw):
        g = torch.Generator().manual_seed(3)
        return {"x_hat": torch.rand(len(strings[0]), 3, 64 * shape[0], 64 * shape[1], generator=g)}


def test_decode_images_of_a_scaled_file_on_the_cpu():
    net = _Decodes()
    scaled = codec.write_container_scaled(100, 150, _inner(50, 75), "bicubic")
    x_hat = net.decompress([[b""]], (1, 2))["x_hat"]
    ref = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (1, 100, 150, 3), dtype=np.uint8))
    img, info = codec.decode_images(net, [scaled], ref=ref)
    want, sq = codec.egress_u8_scaled(x_hat, 50, 75, (100, 150), "bicubic", ref=ref)
    assert torch.equal(img, want)
    assert info[0] == {"H": 100, "W": 150, "display": (100, 150), "coded": (50, 75), "filter": "bicubic", "level": None,
                       "bytes": len(scaled), "bpp": 8.0 * len(scaled) / 15000, "sq_err": int(sq[0]),
                       "psnr": codec.psnr_from_sq_err(int(sq[0]), 45000)}
    thumb, info = codec.decode_images(net, [scaled], out_size=(20, 30), filter="triangle")
    assert torch.equal(thumb, codec.egress_u8_scaled(x_hat, 50, 75, (20, 30), "triangle"))
    assert (info[0]["H"], info[0]["W"], info[0]["display"], info[0]["bpp"]) == (20, 30, (100, 150), 8.0 * len(scaled) / 15000)
    thumb, info = codec.decode_images(net, [_inner(50, 75)], out_size=(20, 30))
    assert torch.equal(thumb, codec.egress_u8_scaled(x_hat, 50, 75, (20, 30), "lanczos3"))
    assert info[0]["display"] == (50, 75) and info[0]["filter"] == "lanczos3"


# ---------------------------------------------------------------------------------------------- CLI
def test_cli_arguments():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "mlic_codec.py")
    spec = importlib.util.spec_from_file_location("mlic_codec_cli_scaled", path)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["--model", "MLICPP_S", "--synthetic", "0"]
    a = cli.parse_args(["encode", "a.ppm", "a.bit", "--scale", "1/2", "--filter", "bicubic"] + base)
    assert a.scale == Fraction(1, 2) and a.filter == "bicubic" and a.coded_size is None
    a = cli.parse_args(["encode", "a.ppm", "a.bit", "--coded-size", "960x540"] + base)
    assert a.coded_size == (960, 540) and a.scale is None
    a = cli.parse_args(["decode", "a.bit", "a.ppm", "--out-size", "240x135", "--filter", "triangle"] + base)
    assert a.out_size == (240, 135)
    for bad in (["encode", "a.ppm", "a.bit", "--scale", "1/2", "--coded-size", "9x9"],
                ["encode", "a.ppm", "a.bit", "--scale", "1/9"], ["encode", "a.ppm", "a.bit", "--scale", "x"],
                ["encode", "a.ppm", "a.bit", "--scale", "1/2", "--tile", "128"],
                ["encode", "a.ppm", "a.bit", "--scale", "1/2", "--roi", "m.ppm", "--roi-levels", "0", "3"],
                ["encode", "a.y4m", "a.bit", "--scale", "1/2"], ["encode", "a.ppm", "a.bit", "--out-size", "9x9"],
                ["encode", "a.ppm", "a.bit", "--filter", "bicubic"], ["decode", "a.bit", "a.ppm", "--scale", "1/2"],
                ["decode", "a.bit", "a.ppm", "--out-size", "9x9", "--depth", "10"],
                ["decode", "a.bit", "a.ppm", "--out-size", "9x9", "--region", "0", "0", "8", "8"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad + base)
