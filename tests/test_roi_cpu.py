"""ROI coding, the parts that need no GPU: the container's third string (writer, validating parser, every
refusal by its message, truncation at every offset), the CPU restatements of the mask kernels, the Python argument
checks of encode_images(roi=...) / code_image(roi=...) against a stub model, the CLI flags, and the test-side
oracle's own pin (a constant plane is the scalar VBR oracle, bit for bit).  tools/container_roi_check.cpp runs the
container through AddressSanitizer + UBSan as a stand-alone program."""
import ctypes as C
import importlib.util
import os
import struct

import numpy as np
import pytest
import torch

from mlic_amd import _lib, bitstream, codec, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NLEV = 6


# ---------------------------------------------------------------------------------------- container
def _levels(hz, wz, seed=0, top=NLEV - 1):
    return np.random.default_rng(seed).integers(0, top + 1, (hz, wz)).astype(np.uint8)


def _file(H=120, W=200, y=b"\x01\x02\x03\x04\x05", z=b"\xaa\xbb", level=5, lv=None):
    hz, wz = (H + 63) // 64, (W + 63) // 64
    lv = _levels(hz, wz) if lv is None else lv
    return codec.write_container_roi(H, W, (hz, wz), y, z, level, lv), lv


def _packed(lv):
    flat = [int(v) for v in lv.reshape(-1)] + [0]
    return bytes([0] + [(flat[k] << 4) | flat[k + 1] for k in range(0, lv.size, 2)])


@pytest.mark.parametrize("H,W", [(120, 200), (64, 64), (129, 65), (1080, 1920), (512, 768)])
def test_container_roi_roundtrip(H, W):
    hz, wz = (H + 63) // 64, (W + 63) // 64
    y, z = bytes(range(37)), bytes(range(5))
    f, lv = _file(H, W, y, z, 5)
    # the layout: the VBR file with n_strings = 3 and the map as the third string
    plain = codec.write_container(H, W, (hz, wz), y, z, 5)
    mp = _packed(lv)
    assert len(mp) == 1 + (hz * wz + 1) // 2
    assert f == plain[:20] + struct.pack(">I", 3) + plain[24:] + struct.pack(">I", len(mp)) + mp
    c, back = codec.parse_container_roi(f, NLEV)
    assert (c.H, c.W, c.hz, c.wz, c.level) == (H, W, hz, wz, 5)
    assert f[c.y_off:c.y_off + c.y_len] == y and f[c.z_off:c.z_off + c.z_len] == z
    assert back.dtype == np.uint8 and np.array_equal(back, lv)
    d = codec.peek(f, vbr=True, n_levels=NLEV)
    assert np.array_equal(d["roi_levels"], lv) and d["level"] == 5 and d["bytes"] == len(f)
    assert len(f) - len(plain) == 4 + len(mp)


def test_map_bytes_per_file():
    """The map's cost: 1 + ceil(hz * wz / 2) bytes and its length word."""
    for (H, W), cost in (((1080, 1920), 4 + 256), ((512, 768), 4 + 49)):
        f, _ = _file(H, W)
        hz, wz = (H + 63) // 64, (W + 63) // 64
        assert len(f) - len(codec.write_container(H, W, (hz, wz), b"\x01\x02\x03\x04\x05", b"\xaa\xbb", 5)) == cost


def test_two_string_file_parses_with_empty_map():
    plain = codec.write_container(120, 200, (2, 4), b"abc", b"de", 3)
    c, lv = codec.parse_container_roi(plain, NLEV)
    assert lv is None and (c.H, c.W, c.level, c.y_len, c.z_len) == (120, 200, 3, 3, 2)
    assert "roi_levels" not in codec.peek(plain, vbr=True, n_levels=NLEV)


def test_container_parse_still_refuses_roi_files():
    f, _ = _file()
    with pytest.raises(_lib.MlicError, match="n_strings"):
        codec.parse_container(f, True, NLEV)
    with pytest.raises(_lib.MlicError, match="n_strings"):
        bitstream.read_stream_checked(f, vbr=True, n_levels=NLEV)


def _refused(data, word, n_levels=NLEV, max_pixels=codec.MAX_PIXELS):
    with pytest.raises(_lib.MlicError, match=word):
        codec.parse_container_roi(bytes(data), n_levels, max_pixels)


def test_container_roi_refusals():
    f, lv = _file()  # 120 x 200: 2 x 4 cells, a 5-byte map at the end
    map_at = len(f) - 5
    m = bytearray(f); m[map_at] = 1
    _refused(m, "version byte")
    m = bytearray(f); m[map_at + 2] = (NLEV << 4) | (m[map_at + 2] & 15)
    _refused(m, "level of the map")
    m = bytearray(f); m[map_at + 4] = (m[map_at + 4] & 0xF0) | NLEV
    _refused(m, "level of the map")
    _refused(f, "level", n_levels=int(lv.max()))  # the header's level word / the map against a smaller table
    for delta in (-1, 1, 200):
        m = bytearray(f); m[map_at - 4:map_at] = struct.pack(">I", 5 + delta)
        _refused(m, "map length")
    _refused(f + b"\x00", "left over")
    _refused(f, "above 16", n_levels=17)
    _refused(f, "n_levels", n_levels=0)
    for n in (0, 1, 4):
        m = bytearray(f); m[20:24] = struct.pack(">I", n)
        _refused(m, "n_strings")
    # an odd cell count: the last low nibble is padding and must be 0
    g, _ = _file(64, 129, lv=_levels(1, 3))
    m = bytearray(g); m[-1] |= 1
    _refused(m, "padding nibble")
    # and everything container_parse refuses
    m = bytearray(f); m[0:4] = struct.pack(">I", 0)
    _refused(m, "H or W is zero")
    m = bytearray(f); m[8:12] = struct.pack(">I", NLEV)
    _refused(m, "level is not below n_levels")
    m = bytearray(f); m[12:16] = struct.pack(">I", 3)
    _refused(m, "h_z, w_z")
    _refused(f, "max_pixels", max_pixels=128 * 256 - 1)
    m = bytearray(f); m[24:28] = struct.pack(">I", 1 << 20)
    _refused(m, "y length")
    # the writer's own refusals
    with pytest.raises(ValueError):
        codec.write_container_roi(120, 200, (2, 4), b"", b"", 5, np.full((2, 4), 16))
    with pytest.raises(ValueError):
        codec.write_container_roi(120, 200, (2, 4), b"", b"", 5, np.zeros((2, 3), np.uint8))
    n = C.c_size_t()
    rc = _lib.lib().mlic_container_write_roi(120, 200, -1, 2, 4, b"", 0, b"", 0, None, None, 0, C.byref(n))
    assert rc != 0 and "VBR" in _lib.lib().mlic_last_error().decode()


def test_container_roi_truncation_every_offset():
    f, _ = _file(64, 129, y=b"\x07" * 9, z=b"\x09" * 3, lv=_levels(1, 3))
    codec.parse_container_roi(f, NLEV)
    for n in range(len(f)):
        with pytest.raises(_lib.MlicError):
            codec.parse_container_roi(f[:n], NLEV)  # a bytes object of exactly n bytes


# ------------------------------------------------------------------------------ CPU restatements
def _np_levels(mask, lo, hi):
    """The cell rule, restated: level = lo + ceil((hi - lo) * count / area) in integers."""
    B, H, W = mask.shape
    hz, wz = -(-H // 64), -(-W // 64)
    out = np.zeros((B, hz, wz), np.uint8)
    for b in range(B):
        for i in range(hz):
            for j in range(wz):
                cell = mask[b, 64 * i:64 * i + 64, 64 * j:64 * j + 64]
                count, area = int(np.count_nonzero(cell)), cell.size
                out[b, i, j] = lo + -(-(hi - lo) * count // area)
    return out


def test_roi_levels_cpu_rule():
    r = np.random.default_rng(3)
    m = (r.random((2, 120, 200)) < 0.3).astype(np.uint8) * 200
    m[0, :, 100:] = 1
    m[1, :64, :64] = 0
    m[1, 100, 150] = 7  # one pixel lifts its cell above lo
    for lo, hi in ((0, 5), (2, 2), (1, 4), (0, 255)):
        got = codec.roi_levels(torch.from_numpy(m), lo, hi)
        assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), _np_levels(m, lo, hi))
    assert codec.roi_levels(torch.zeros(70, 70, dtype=torch.bool), 1, 4).tolist() == [[[1, 1], [1, 1]]]
    assert codec.roi_levels(torch.ones(70, 70, dtype=torch.bool), 1, 4).tolist() == [[[4, 4], [4, 4]]]
    for bad in ((3, 2), (-1, 2), (0, 256), (0.0, 2)):
        with pytest.raises(ValueError, match="lo <= hi"):
            codec.roi_levels(torch.zeros(8, 8, dtype=torch.uint8), *bad)
    with pytest.raises(ValueError, match="mask"):
        codec.roi_levels(torch.zeros(8, 8), 0, 1)


def test_sq_err_roi_cpu():
    r = np.random.default_rng(4)
    a = r.integers(0, 256, (2, 30, 50, 3)).astype(np.uint8)
    b = r.integers(0, 256, (2, 30, 50, 3)).astype(np.uint8)
    m = (r.random((2, 30, 50)) < 0.4)
    got = codec.sq_err_roi(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(m)).numpy()
    sq = ((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum(-1)
    exp = np.stack([(sq * m).sum((1, 2)), m.sum((1, 2)), (sq * ~m).sum((1, 2)), (~m).sum((1, 2))], 1)
    assert np.array_equal(got, exp)
    p = codec.psnr_roi(torch.from_numpy(a), torch.from_numpy(a), torch.from_numpy(np.ones((2, 30, 50), bool)))
    assert p[0]["psnr_roi"] == float("inf") and p[0]["psnr_bg"] is None and p[0]["n_roi"] == 1500


# ------------------------------------------------------------------------------------------- policy
GAINS = [0.1, 0.2, 0.4, 0.6, 0.8, 1.0]


class StubRoiNet:
    """compress / decompress as the VBR models have them (s= or gain_map=), on the CPU: the y string is the
    plane's bytes, so a test can see which plane the codec handed over."""
    device = torch.device("cpu")

    def __init__(self, vbr=True):
        if vbr:
            self.levels = len(GAINS)
            self.Gain = -torch.tensor(GAINS)  # the coder paths use |Gain|
        self.calls = []

    def compress(self, x, s=None, gain_map=None):
        B, _, Hp, Wp = x.shape
        self.calls.append(("compress", s, gain_map))
        assert gain_map is None or tuple(gain_map.shape) == (B, 1, Hp // 16, Wp // 16)
        ys = [b"" if gain_map is None else gain_map[b].numpy().tobytes() for b in range(B)]
        return {"strings": [ys, [b"z"] * B], "shape": (Hp // 64, Wp // 64)}

    def decompress(self, strings, shape, s=None, gain_map=None):
        self.calls.append(("decompress", s, gain_map))
        return {"x_hat": torch.full((len(strings[1]), 3, 64 * shape[0], 64 * shape[1]), 0.5)}


def _images(B=2, H=120, W=200):
    return torch.from_numpy(np.random.default_rng(9).integers(0, 256, (B, H, W, 3)).astype(np.uint8))


def _masks(B=2, H=120, W=200):
    m = torch.zeros(B, H, W, dtype=torch.uint8)
    m[0, :, W // 2:] = 1
    if B > 1:
        m[1, 70:90, 10:20] = 255
    return m


def test_encode_decode_roi_with_stub():
    net, imgs, masks = StubRoiNet(), _images(), _masks()
    files, info = codec.encode_images(net, imgs, roi=masks, roi_levels=(1, 4), return_info=True)
    lmap = codec.roi_levels(masks, 1, 4)
    plane = net.calls[0][2]
    assert net.calls[0][1] is None and torch.equal(plane, codec.gain_plane(net, lmap))
    assert torch.equal(plane[0, 0, ::4, ::4], torch.tensor(GAINS)[lmap[0].long()])  # |Gain|, nearest expansion
    assert plane.shape == (2, 1, 8, 16) and torch.equal(plane[:, :, 1::4, 3::4], plane[:, :, ::4, ::4])
    for b, f in enumerate(files):
        d = codec.peek(f, vbr=True, n_levels=net.levels)
        assert np.array_equal(d["roi_levels"], lmap[b].numpy()) and d["level"] == 4 and (d["H"], d["W"]) == (120, 200)
        assert np.array_equal(info[b]["roi_levels"], lmap[b].numpy()) and info[b]["bytes"] == len(f)
        c, _ = codec.parse_container_roi(f, net.levels)
        assert f[c.y_off:c.y_off + c.y_len] == plane[b].numpy().tobytes()
    # the decoder rebuilds the same plane from the file alone; a plain VBR file beside an ROI file decodes
    # through the constant map of its level
    plain = codec.encode_images(net, imgs[:1], level=2)[0]
    img, dinfo = codec.decode_images(net, [files[1], plain])
    call = net.calls[-1]
    assert call[0] == "decompress" and call[1] is None
    assert torch.equal(call[2][0], plane[1]) and torch.equal(call[2][1], torch.full((1, 8, 16), GAINS[2]))
    assert np.array_equal(dinfo[0]["roi_levels"], lmap[1].numpy()) and "roi_levels" not in dinfo[1]
    assert img.shape == (2, 120, 200, 3)
    # without an ROI file nothing changes: the level goes through s=
    codec.decode_images(net, [plain])
    assert net.calls[-1][1] == [2] and net.calls[-1][2] is None


def test_roi_argument_refusals():
    imgs, masks = _images(), _masks()
    with pytest.raises(ValueError, match="max_bpp"):
        codec.encode_images(StubRoiNet(), imgs, roi=masks, roi_levels=(0, 5), max_bpp=0.5)
    with pytest.raises(ValueError, match="go together"):
        codec.encode_images(StubRoiNet(), imgs, roi=masks)
    with pytest.raises(ValueError, match="go together"):
        codec.encode_images(StubRoiNet(), imgs, level=1, roi_levels=(0, 5))
    with pytest.raises(ValueError, match="level="):
        codec.encode_images(StubRoiNet(), imgs, level=1, roi=masks, roi_levels=(0, 5))
    with pytest.raises(ValueError, match="fixed-rate"):
        codec.encode_images(StubRoiNet(vbr=False), imgs, roi=masks, roi_levels=(0, 5))
    for bad in ((3, 2), (0, 6), (-1, 2), (0, 1, 2), 3, (0.0, 1)):
        with pytest.raises(ValueError, match="roi_levels"):
            codec.encode_images(StubRoiNet(), imgs, roi=masks, roi_levels=bad)
    with pytest.raises(ValueError, match="shape"):
        codec.encode_images(StubRoiNet(), imgs, roi=masks[:, :100], roi_levels=(0, 5))
    with pytest.raises(ValueError, match="mask"):
        codec.encode_images(StubRoiNet(), imgs, roi=masks.float(), roi_levels=(0, 5))
    with pytest.raises(ValueError, match="VBR"):
        codec.gain_plane(StubRoiNet(vbr=False), torch.zeros(1, 2, 2, dtype=torch.uint8))
    with pytest.raises(ValueError, match="levels in"):
        codec.gain_plane(StubRoiNet(), torch.full((1, 2, 2), 6, dtype=torch.uint8))
    # no refusal reached the model
    net = StubRoiNet()
    with pytest.raises(ValueError):
        codec.encode_images(net, imgs, roi=masks, roi_levels=(0, 9))
    assert net.calls == []


def test_code_image_roi_fields():
    net = StubRoiNet()
    x = _images(1).permute(0, 3, 1, 2).contiguous().float().div(255)
    mask = _masks(1)[0]
    plain = bitstream.code_image(net, x, s=3)
    assert "psnr_roi" not in plain and "psnr_bg" not in plain
    r = bitstream.code_image(net, x, roi=mask, roi_levels=(0, 5))
    assert set(r) == set(plain) | {"psnr_roi", "psnr_bg", "roi_levels"}
    assert np.array_equal(r["roi_levels"], codec.roi_levels(mask, 0, 5)[0].numpy())
    u, h = bitstream.to_u8(x), bitstream.to_u8(r["x_hat"])
    sq = ((u.long() - h.long()) ** 2).sum(1)[0]
    inside = mask != 0
    exp = codec.psnr_from_sq_err(int(sq[inside].sum()), 3 * int(inside.sum()))
    assert r["psnr_roi"] == exp and r["psnr_bg"] == codec.psnr_from_sq_err(int(sq[~inside].sum()), 3 * int((~inside).sum()))
    assert r["bytes"] == 12 + 12 + 4 + 4 * 8 * 16 + 4 + 1 + 4 + 5
    with pytest.raises(ValueError, match="roi"):
        bitstream.code_image(net, x, roi=mask, roi_levels=(0, 5), max_bpp=1.0)
    with pytest.raises(ValueError, match="roi"):
        bitstream.code_image(net, x, roi=mask, roi_levels=(0, 5), s=2)
    with pytest.raises(ValueError, match="go together"):
        bitstream.code_image(net, x, roi=mask)


def test_model_gain_map_refusals_without_a_gpu():
    """Every gain_map refusal is a ValueError raised before anything touches the GPU (this test has none)."""
    from mlic_amd import get_model
    vbr = get_model("MLICPP_M_SMALL_DEC_VBR")
    fixed = get_model("MLICPP_M_SMALL_DEC")
    x = torch.zeros(2, 3, 128, 192)
    g = torch.ones(2, 1, 8, 12)
    with pytest.raises(ValueError, match="fixed-rate"):
        fixed(x, gain_map=g)
    with pytest.raises(ValueError, match="fixed-rate"):
        fixed.compress(x, gain_map=g)
    with pytest.raises(ValueError, match="shape"):
        vbr(x, gain_map=torch.ones(2, 1, 8, 8))
    with pytest.raises(ValueError, match="shape"):
        vbr.compress(x, gain_map=torch.ones(1, 8, 12))
    with pytest.raises(ValueError, match="float32"):
        vbr(x, gain_map=g.double())
    with pytest.raises(ValueError, match="CUDA"):
        vbr(x, gain_map=g)  # a CPU plane
    with pytest.raises(ValueError, match="CUDA"):
        vbr.decompress([[b"", b""], [b"", b""]], (2, 3), gain_map=g[:, 0])
    with pytest.raises(ValueError, match="shape"):
        vbr.decompress([[b"", b""], [b"", b""]], (2, 3), gain_map=torch.ones(2, 8, 8))


# ---------------------------------------------------------------------------------------------- CLI
def _cli():
    spec = importlib.util.spec_from_file_location("mlic_codec_cli_roi", os.path.join(ROOT, "tools", "mlic_codec.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_roi_flags(capsys, tmp_path):
    cli = _cli()
    base = ["encode", "a.ppm", "a.bit", "--synthetic", "0", "--model", "MLICPP_L_VBR"]
    a = cli.parse_args(base)
    assert (a.roi, a.roi_levels) == (None, None)
    a = cli.parse_args(base + ["--roi", "m.ppm", "--roi-levels", "0", "5"])
    assert (a.roi, a.roi_levels) == ("m.ppm", [0, 5])
    for bad in (["--roi", "m.ppm"], ["--roi-levels", "0", "5"], ["--roi", "m.ppm", "--roi-levels", "5", "0"],
                ["--roi", "m.ppm", "--roi-levels", "0"], ["--roi", "m.ppm", "--roi-levels", "0", "5", "--level", "3"],
                ["--roi", "m.ppm", "--roi-levels", "0", "5", "--max-bpp", "0.3"]):
        with pytest.raises(SystemExit):
            cli.parse_args(base + bad)
    with pytest.raises(SystemExit):
        cli.parse_args(["decode", "a.bit", "a.ppm", "--synthetic", "0", "--roi", "m.ppm", "--roi-levels", "0", "5"])
    with pytest.raises(SystemExit):
        cli.parse_args(["encode", "a.ppm", "--synthetic", "0"])  # no destination
    with pytest.raises(SystemExit):
        cli.parse_args(["encode", "a.ppm", "a.bit"])  # no weights
    capsys.readouterr()
    # info needs neither weights nor a GPU: it prints what the file says, and the map of an ROI file
    f, lv = _file(120, 200, level=5)
    path = tmp_path / "a.bit"
    path.write_bytes(f)
    cli.main(["info", str(path), "--model", "MLICPP_L_VBR"])
    out = capsys.readouterr().out
    assert "120 x 200" in out and "level 5" in out and "level map" in out
    assert [ln.split() for ln in out.strip().splitlines()[-2:]] == [[f"{v:x}" for v in row] for row in lv]


# ------------------------------------------------------------------------------------------- oracle
def test_oracle_constant_plane_is_the_scalar_oracle():
    """tests/roi_oracle.py restates RefMLIC._slice_loop; with a constant plane it must be that loop, bit for
    bit: x_hat, likelihoods and the coder lists."""
    import mlic_ref_cpu as ref
    import roi_oracle
    name, H, W, s = "MLICPP_M_SMALL_DEC_VBR", 64, 128, 3
    sd = synthetic.synth_state_dict(name, rate=1)
    x = synthetic.synth_image(H, W, 2)
    o = roi_oracle.RefMLICRoi(name, sd)
    gain = float(sd["Gain"][s])
    assert gain > 0
    rec = {}
    got = o.forward_g(x, torch.full((1, 1, H // 16, W // 16), gain), record=lambda ph, a, b: rec.__setitem__(ph, (a, b)))
    exp = ref.RefMLIC(name, sd).compress_streams(x, s=s, likelihoods=True)
    assert torch.equal(got["y_hat"], exp["y_hat"])
    assert torch.equal(got["likelihoods"]["y_likelihoods"], exp["likelihoods"]["y_likelihoods"])
    assert torch.equal(got["likelihoods"]["z_likelihoods"], exp["likelihoods"]["z_likelihoods"])
    assert len(rec) == len(exp["phases"])
    for ph, (sym, idx) in enumerate(exp["phases"]):
        assert torch.equal(rec[ph][0], sym) and torch.equal(rec[ph][1], idx)
    lv = torch.tensor([[[0, 4]]])
    g = roi_oracle.expand_levels(lv, sd["Gain"].abs())
    assert g.shape == (1, 1, 4, 8) and float(g[0, 0, 3, 3]) == float(sd["Gain"][0].abs())
    assert float(g[0, 0, 0, 4]) == float(sd["Gain"][4].abs())
