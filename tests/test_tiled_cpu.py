"""Tiled coding, the parts that need no GPU: the tile grid (the C and the Python definition), the torch restatement
of the blend against a float64 loop oracle written here, the tiled container (round trip, every refusal by its own
message, tools/container_tiled_check.cpp under AddressSanitizer + UBSan as a stand-alone program), and the policy of
encode_tiled / decode_tiled with a stub model: tile order, chunking, which tiles a region decode touches, and the
combinations that are refused."""
import ctypes as C
import importlib.util
import math
import os
import shutil
import struct
import subprocess
import warnings

import numpy as np
import pytest
import torch

from mlic_amd import _lib, bitstream, codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGAL = [(T, V) for T in (128, 192, 256) for V in (0, 16, 32, 64)]


# --------------------------------------------------------------------------------------------- grid
def _c_grid(H, W, T, V):
    ny, nx = C.c_uint32(), C.c_uint32()
    _lib.call("mlic_tile_grid", H, W, T, V, C.byref(ny), C.byref(nx), None, 0)
    rects = (C.c_uint32 * (4 * ny.value * nx.value))()
    _lib.call("mlic_tile_grid", H, W, T, V, C.byref(ny), C.byref(nx), rects, ny.value * nx.value)
    return ny.value, nx.value, [tuple(rects[4 * k:4 * k + 4]) for k in range(ny.value * nx.value)]


@pytest.mark.parametrize("T, V", LEGAL)
def test_grid_properties_and_weights(T, V):
    S = T - V
    for L in range(1, 701):
        g = codec.tile_grid(L, 1, T, V)
        axis, n = g["ys"], g["ny"]
        assert n == (1 if L <= T else -(-(L - V) // S)) and len(axis) == n
        assert axis == [(k * S, min(T, L - k * S)) for k in range(n)]
        assert axis[0][0] == 0 and axis[-1][0] + axis[-1][1] == L and all(e >= 1 for _, e in axis)  # covers [0, L)
        assert n == 1 or axis[-1][1] > V
        cover = np.zeros(L, np.int64)
        w32 = np.zeros(L, np.float32)
        w64 = np.zeros(L, np.float64)
        for k, (s, e) in enumerate(axis):
            w = codec.tile_weights(L, T, V, k)
            assert w.dtype == torch.float32 and w.shape == (e,)
            cover[s:s + e] += 1
            w32[s:s + e] += w.numpy()
            w64[s:s + e] += w.double().numpy()
            if k + 1 < n:  # the strip shared with tile k + 1 is [(k + 1) S, k S + T), V wide
                nxt = axis[k + 1][0]
                assert (nxt, s + e) == ((k + 1) * S, k * S + T) and s + e - nxt == V
                later = codec.tile_weights(L, T, V, k + 1)[:V].double().numpy()
                assert np.array_equal(later, (2 * np.arange(V) + 1) / (2 * V)) if V else later.size == 0
                assert np.array_equal(w.double().numpy()[S:], 1 - later)
        assert cover.min() >= 1 and cover.max() <= 2
        assert np.all(w32 == np.float32(1)) and np.all(w64 == 1.0)  # exactly 1, in fp32 and in double
        assert (_c_grid(L, 1, T, V)[0], [(r[0], r[2]) for r in _c_grid(L, 1, T, V)[2]]) == (n, axis)  # C == Python


def test_grid_2d_c_and_python_agree():
    for H, W, T, V in [(200, 330, 128, 32), (100, 90, 128, 32), (128, 224, 128, 32), (700, 513, 192, 64),
                       (1080, 1920, 512, 16), (4096, 4096, 1024, 0), (1, 1, 128, 64), (129, 128, 128, 0)]:
        g = codec.tile_grid(H, W, T, V)
        assert (g["ny"], g["nx"], g["rects"]) == _c_grid(H, W, T, V)
        assert len({(h, w) for _, _, h, w in g["rects"]}) <= 4  # interior, right column, bottom row, corner
    assert codec.tile_grid(200, 330, 128, 32)["xs"] == [(0, 128), (96, 128), (192, 128), (288, 42)]
    assert (codec.tile_grid(128, 224, 128, 32)["ny"], codec.tile_grid(128, 224, 128, 32)["nx"]) == (1, 2)


@pytest.mark.parametrize("T, V", [(0, 0), (64, 0), (100, 0), (130, 0), (65536, 0), (128, 8), (128, 48), (192, 128),
                                  (128.0, 0), (True, 0)])
def test_grid_refuses_bad_parameters(T, V):
    with pytest.raises(ValueError):
        codec.tile_grid(100, 100, T, V)
    if isinstance(T, int) and not isinstance(T, bool):
        ny, nx = C.c_uint32(), C.c_uint32()
        assert _lib.lib().mlic_tile_grid(100, 100, T & 0xffffffff, V, C.byref(ny), C.byref(nx), None, 0) != 0
        assert "tile grid" in _lib.lib().mlic_last_error().decode()


def test_grid_refuses_empty_images_and_small_buffers():
    with pytest.raises(ValueError):
        codec.tile_grid(0, 10, 128, 0)
    ny, nx = C.c_uint32(), C.c_uint32()
    lib = _lib.lib()
    assert lib.mlic_tile_grid(0, 10, 128, 0, C.byref(ny), C.byref(nx), None, 0) != 0
    rects = (C.c_uint32 * 8)()
    assert lib.mlic_tile_grid(300, 300, 128, 0, C.byref(ny), C.byref(nx), rects, 2) != 0
    assert "rects buffer too small" in lib.mlic_last_error().decode()


# -------------------------------------------------------------------------------------------- blend
def _random_tiles(H, W, T, V, seed, device="cpu"):
    """fp32 tiles [3, pad64(h), pad64(w)] with values in about [-0.5, 1.5], some huge, +-inf and NaN; the padding
    holds NaN (it must never be read)."""
    r = np.random.default_rng(seed)
    tiles = []
    for _, _, h, w in codec.tile_grid(H, W, T, V)["rects"]:
        a = np.full((3, -(-h // 64) * 64, -(-w // 64) * 64), np.nan, np.float32)
        v = r.uniform(-0.5, 1.5, (3, h, w)).astype(np.float32)
        m = r.random((3, h, w))
        v[m < 0.01] = np.nan
        v[(m >= 0.01) & (m < 0.02)] = np.inf
        v[(m >= 0.02) & (m < 0.03)] = -np.inf
        v[(m >= 0.03) & (m < 0.04)] = 3.0e38
        v[(m >= 0.04) & (m < 0.05)] = -0.0
        a[:, :h, :w] = v
        tiles.append(torch.from_numpy(a).to(device))
    return tiles


def blend_oracle(tiles, H, W, T, V, region=None):
    """The definition, one value at a time in Python floats (IEEE double): acc = 0.0; acc += (wy * wx) * x_hat over
    the covering tiles, tile row then tile column; then float32, NaN -> 0, clamp, * 255 in fp32, floor.
    -> uint8 numpy [h, w, 3] and the per-pixel count of covering tiles."""
    S = T - V
    ys = [(k * S, min(T, H - k * S)) for k in range(1 if H <= T else -(-(H - V) // S))]
    xs = [(k * S, min(T, W - k * S)) for k in range(1 if W <= T else -(-(W - V) // S))]
    y0, x0, h, w = region or (0, 0, H, W)
    lists = [t.tolist() for t in tiles]

    def weight(p, k, axis):
        s, e = axis[k]
        if k > 0 and p - s < V:
            return (2 * (p - s) + 1) / (2 * V)
        if k + 1 < len(axis) and p >= axis[k + 1][0]:
            return 1.0 - (2 * (p - axis[k + 1][0]) + 1) / (2 * V)
        return 1.0

    acc = np.zeros((h, w, 3), np.float64)
    cover = np.zeros((h, w), np.int64)
    for y in range(y0, y0 + h):
        kys = [k for k, (s, e) in enumerate(ys) if s <= y < s + e]
        for x in range(x0, x0 + w):
            kxs = [k for k, (s, e) in enumerate(xs) if s <= x < s + e]
            cover[y - y0, x - x0] = len(kys) * len(kxs)
            for c in range(3):
                a = 0.0
                for ky in kys:
                    for kx in kxs:
                        a += (weight(y, ky, ys) * weight(x, kx, xs)) * lists[ky * len(xs) + kx][c][y - ys[ky][0]][x - xs[kx][0]]
                acc[y - y0, x - x0, c] = a
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        v = acc.astype(np.float32)
        v = np.where(np.isnan(v), np.float32(0), v)
        u = np.floor(np.clip(v, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)
    return u, cover


BLEND_CASES = [(150, 170, 128, 32, None), (150, 170, 128, 32, (95, 93, 37, 41)), (100, 300, 128, 64, None),
               (140, 150, 128, 16, (3, 5, 131, 140)), (130, 140, 128, 0, None), (100, 90, 128, 32, None)]


@pytest.mark.parametrize("H, W, T, V, region", BLEND_CASES)
def test_blend_restatement_against_the_loop_oracle(H, W, T, V, region):
    tiles = _random_tiles(H, W, T, V, seed=H + W + V)
    before = [t.clone() for t in tiles]
    want, cover = blend_oracle(tiles, H, W, T, V, region)
    got = codec.blend_tiles(tiles, H, W, T, V, region=region)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(tiles, before))
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want)
    assert want.min() == 0 and want.max() == 255 and 0 < np.count_nonzero((want > 0) & (want < 255))
    # the planar layout, a strided destination that keeps its surroundings, and sq_err
    chw = codec.blend_tiles(tiles, H, W, T, V, region=region, layout="chw")
    assert np.array_equal(chw.permute(1, 2, 0).numpy(), want)
    h, w = want.shape[:2]
    canvas = torch.full((h + 2, w + 3, 4), 0xA5, dtype=torch.uint8)
    ref = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (h, w, 3), dtype=np.uint8))
    out, sq = codec.blend_tiles(tiles, H, W, T, V, region=region, out=canvas[1:h + 1, 2:w + 2, :3], ref=ref)
    assert np.array_equal(canvas[1:h + 1, 2:w + 2, :3].numpy(), want)
    rest = canvas.clone()
    rest[1:h + 1, 2:w + 2, :3] = 0xA5
    assert bool((rest == 0xA5).all())
    assert sq.dtype == torch.int64 and int(sq[0]) == int(((want.astype(np.int64) - ref.numpy().astype(np.int64)) ** 2).sum())
    # where one tile covers a pixel the result is egress_u8 of that tile (a NaN is 0 in both)
    y0, x0 = (region or (0, 0))[:2]
    g = codec.tile_grid(H, W, T, V)
    seen = 0
    for k, (ty, tx, th, tw) in enumerate(g["rects"]):
        clean = torch.where(torch.isnan(tiles[k]), torch.zeros_like(tiles[k]), tiles[k])
        e = codec.egress_u8(clean.unsqueeze(0), th, tw, "hwc")[0].numpy()
        for y in range(max(ty, y0), min(ty + th, y0 + h)):
            row = cover[y - y0]
            for x in range(max(tx, x0), min(tx + tw, x0 + w)):
                if row[x - x0] == 1:
                    seen += 1
                    assert np.array_equal(want[y - y0, x - x0], e[y - ty, x - tx]), (k, y, x)
    assert seen == int((cover == 1).sum()) and seen > 0
    if V and g["ny"] * g["nx"] > 1:
        assert int((cover > 1).sum()) > 0


def test_blend_refusals():
    H, W, T, V = 150, 170, 128, 32
    tiles = [torch.zeros(3, 128, 128), torch.zeros(3, 128, 128), torch.zeros(3, 64, 128), torch.zeros(3, 64, 128)]
    codec.blend_tiles(tiles, H, W, T, V)
    with pytest.raises(ValueError, match="missing"):
        codec.blend_tiles([tiles[0], None, tiles[2], tiles[3]], H, W, T, V)
    # a region that tile 1 does not cover needs no tile 1; a dict names the tiles it has
    assert codec.blend_tiles([tiles[0], None, tiles[2], None], H, W, T, V, region=(0, 0, 150, 96)).shape == (150, 96, 3)
    assert codec.blend_tiles({0: tiles[0]}, H, W, T, V, region=(10, 10, 50, 60)).shape == (50, 60, 3)
    for bad in (dict(region=(0, 0, 151, 10)), dict(region=(0, -1, 10, 10)), dict(region=(5, 5, 0, 3)),
                dict(region=(1, 2, 3)), dict(layout="nhwc"), dict(out=torch.zeros(150, 170, 3)),
                dict(ref=torch.zeros(150, 169, 3, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            codec.blend_tiles(tiles, H, W, T, V, **bad)
    with pytest.raises(ValueError, match="entries"):
        codec.blend_tiles(tiles[:3], H, W, T, V)
    with pytest.raises(ValueError, match="fp32"):
        codec.blend_tiles([tiles[0], tiles[1], tiles[2], torch.zeros(3, 64, 64)], H, W, T, V)


def _blend_rc(**kw):
    """mlic_image_tile_blend_u8 with made-up pointers that are never dereferenced: every refusal comes before any
    GPU call, so this runs without a device."""
    a = dict(dev=0x10000, H=150, W=170, T=128, V=32, y0=0, x0=0, h=150, w=170, dst=0x20000, d=(510, 3, 1), ref=0, r=None,
             sq=0, tiles=(0x100000, 0x200000, 0x300000, 0x400000))
    a.update(kw)
    lib = _lib.lib()
    host = (C.c_void_p * len(a["tiles"]))(*[p or None for p in a["tiles"]])
    rc = lib.mlic_image_tile_blend_u8(None, C.c_void_p(a["dev"]), host, a["H"], a["W"], a["T"], a["V"], a["y0"], a["x0"],
                                      a["h"], a["w"], C.c_void_p(a["dst"]), (C.c_int64 * 3)(*a["d"]),
                                      C.c_void_p(a["ref"]), None if a["r"] is None else (C.c_int64 * 3)(*a["r"]),
                                      C.c_void_p(a["sq"]))
    return rc, lib.mlic_last_error().decode() if rc else ""


@pytest.mark.parametrize("kw, word", [
    (dict(dev=0), "null argument"), (dict(dst=0), "null argument"), (dict(H=0), "H, W in"), (dict(W=(1 << 24) + 1), "H, W in"),
    (dict(T=100), "multiple of 64"), (dict(V=8), "0, 16, 32 or 64"), (dict(T=-128), "negative"),
    (dict(h=0), "inside the image"), (dict(y0=1), "inside the image"), (dict(x0=-1), "inside the image"),
    (dict(w=171), "inside the image"), (dict(d=(510, 0, 1)), "zero column or channel stride"),
    (dict(ref=0x30000, r=(510, 3, 1)), "go together"), (dict(sq=0x40000), "go together"),
    (dict(ref=0x30000, sq=0x40000), "ref needs strides"), (dict(dev=0x10004), "8-byte aligned"),
    (dict(tiles=(0x100000, 0, 0x300000, 0x400000)), "covers the region is null"),
    (dict(tiles=(0x100000, 0x200002, 0x300000, 0x400000)), "4-byte aligned"),
])
def test_blend_entry_point_refuses_without_a_device(kw, word):
    rc, msg = _blend_rc(**kw)
    assert rc != 0 and "image_tile_blend_u8" in msg and word in msg, msg


# ---------------------------------------------------------------------------------------- container
def _tile_files(H, W, T, V, level=None, seed=0):
    r = np.random.default_rng(seed)
    out = []
    for _, _, h, w in codec.tile_grid(H, W, T, V)["rects"]:
        y, z = r.bytes(int(r.integers(0, 40))), r.bytes(int(r.integers(0, 9)))
        out.append(codec.write_container(h, w, (-(-h // 64), -(-w // 64)), y, z, level))
    return out


@pytest.mark.parametrize("H, W, T, V, level", [(200, 330, 128, 32, None), (100, 90, 128, 0, 3), (128, 224, 128, 32, 5),
                                               (700, 650, 192, 64, None)])
def test_container_tiled_roundtrip(H, W, T, V, level):
    files = _tile_files(H, W, T, V, level)
    data = codec.write_container_tiled(H, W, T, V, files, vbr=level is not None)
    g = codec.tile_grid(H, W, T, V)
    n = len(files)
    head = struct.pack(">4sBBIIHHII", b"MLT1", 0, int(level is not None), H, W, T, V, g["ny"], g["nx"])
    offs = np.concatenate([[0], np.cumsum([len(f) for f in files])])
    assert data == head + b"".join(struct.pack(">Q", int(o)) for o in offs) + b"".join(files)
    assert codec.is_tiled_file(data) and not codec.is_tiled_file(files[0])
    t = codec.parse_container_tiled(data)
    assert (t.H, t.W, t.T, t.V, t.ny, t.nx, bool(t.vbr)) == (H, W, T, V, g["ny"], g["nx"], level is not None)
    assert (t.table_off, t.payload_off, t.payload_len) == (26, 26 + 8 * (n + 1), sum(len(f) for f in files))
    for k, f in enumerate(files):
        off, ln = codec.tiled_tile(data, t, k)
        assert data[off:off + ln] == f
    with pytest.raises(_lib.MlicError, match="outside the grid"):
        codec.tiled_tile(data, t, n)
    d = codec.peek(data, n_levels=6)
    assert d["tiled"] and (d["H"], d["W"], d["tile"], d["overlap"], d["grid"]) == (H, W, T, V, (g["ny"], g["nx"]))
    assert [x["bytes"] for x in d["tiles"]] == [len(f) for f in files] and d["level"] == level
    assert [(x["y0"], x["x0"], x["H"], x["W"]) for x in d["tiles"]] == g["rects"]
    assert d["bytes"] == len(data) and d["bpp"] == 8.0 * len(data) / (H * W)
    # the per-image parsers keep refusing it, and decode_images names decode_tiled
    for vbr in (False, True):
        with pytest.raises(_lib.MlicError):
            codec.parse_container(data, vbr, 6)
    with pytest.raises(_lib.MlicError):
        codec.parse_container_roi(data, 6)
    with pytest.raises(ValueError, match="decode_tiled"):
        codec.decode_images(StubNet(), [data])


def test_container_tiled_refusals_each_with_its_own_message():
    H, W, T, V = 200, 330, 128, 32
    files = _tile_files(H, W, T, V)
    data = codec.write_container_tiled(H, W, T, V, files)
    tab, last = 26, 26 + 8 * len(files)

    def refused(mut, word, max_pixels=codec.MAX_IMAGE_PIXELS):
        m = bytearray(data)
        mut(m)
        with pytest.raises(_lib.MlicError, match=word):
            codec.parse_container_tiled(bytes(m), max_pixels)

    def put(at, fmt, *v):
        return lambda m: m.__setitem__(slice(at, at + struct.calcsize(fmt)), struct.pack(fmt, *v))

    refused(lambda m: m.__delitem__(slice(25, None)), "truncated header")
    refused(put(0, ">4s", b"MLT2"), "bad magic")
    refused(put(4, ">B", 1), "unknown version")
    refused(put(5, ">B", 2), "unknown flags")
    refused(put(14, ">H", 129), "multiple of 64")
    refused(put(14, ">H", 64), "at least 128")
    refused(put(16, ">H", 8), "0, 16, 32 or 64")
    refused(put(6, ">I", 0), "H or W is zero")
    refused(put(10, ">I", 0), "H or W is zero")
    refused(lambda m: None, "exceeds max_pixels", H * W - 1)
    codec.parse_container_tiled(data, H * W)
    refused(put(18, ">I", 3), "not the grid")
    refused(put(22, ">I", 5), "not the grid")
    big = 0xffffff00  # H * W = 2^32 - 256 pixels passes max_pixels; its table cannot fit in the file
    refused(put(6, ">IIHHII", big, 1, T, V, -(-(big - V) // (T - V)), 1), "offset table does not fit")
    refused(put(tab, ">Q", 1), "first offset is not 0")
    refused(lambda m: m.__setitem__(slice(tab + 16, tab + 24), m[tab + 8:tab + 16]), "not strictly increasing")
    refused(put(tab + 8, ">Q", 1 << 63), "not strictly increasing|last offset")
    refused(put(last, ">Q", len(b"".join(files)) + 1), "last offset is not the payload's length")
    refused(lambda m: m.append(0), "last offset is not the payload's length")
    for n in range(len(data)):  # truncated anywhere
        with pytest.raises(_lib.MlicError):
            codec.parse_container_tiled(data[:n])
    # the writer: a file count off the grid, an empty tile, bad parameters
    with pytest.raises(_lib.MlicError, match="ny \\* nx"):
        codec.write_container_tiled(H, W, T, V, files[:-1])
    with pytest.raises(_lib.MlicError, match="empty tile"):
        codec.write_container_tiled(H, W, T, V, files[:-1] + [b""])
    with pytest.raises(_lib.MlicError, match="multiple of 64"):
        codec.write_container_tiled(H, W, 100, V, files)
    # a tile whose own header disagrees with the grid
    wrong = list(files)
    wrong[3] = codec.write_container(128, 43, (2, 1), b"", b"")
    with pytest.raises(_lib.MlicError, match="tile 3 says 128 x 43, the grid 128 x 42"):
        codec.peek(codec.write_container_tiled(H, W, T, V, wrong))


def test_container_tiled_check_program_under_sanitizers(tmp_path):
    """tools/container_tiled_check.cpp with container.cpp, AddressSanitizer + UBSan, as a stand-alone program (no
    sanitizer runtime comes near Python): the grid sweep, round trips, refusals, truncations and mutations.  The
    sanitizer runtimes are linked statically (g++ needs the two flags, clang does it by default), so the program
    starts in whatever environment the suite runs in, which is passed on unchanged."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed for the container's sanitizer check"
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / "container_tiled_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static + [
           "-I" + os.path.join(ROOT, "mlic_amd", "csrc"), os.path.join(ROOT, "tools", "container_tiled_check.cpp"),
           os.path.join(ROOT, "mlic_amd", "csrc", "container.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-300:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("container_tiled_check ok"), r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------- policy
class StubNet:
    """A lossless 'model' on the CPU: the y string is the tile's padded uint8 pixels, the z string names the level.
    calls records (kind, batch size, padded shape, levels)."""
    device = torch.device("cpu")

    def __init__(self, vbr=False):
        if vbr:
            self.levels = 6
        self.calls = []

    def compress(self, x, s=None):
        B, _, Hp, Wp = x.shape
        assert Hp % 64 == 0 and Wp % 64 == 0 and x.is_contiguous() and x.dtype == torch.float32
        assert (s is None) == (not hasattr(self, "levels")) and (s is None or len(s) == B)
        self.calls.append(("compress", B, (Hp, Wp), None if s is None else list(s)))
        ys = [bitstream.to_u8(x[b]).numpy().tobytes() for b in range(B)]
        return {"strings": [ys, [b"z" if s is None else bytes([s[b]]) for b in range(B)]], "shape": (Hp // 64, Wp // 64)}

    def decompress(self, strings, shape, s=None):
        B = len(strings[0])
        assert (s is None) == (not hasattr(self, "levels")) and (s is None or len(s) == B)
        self.calls.append(("decompress", B, (64 * shape[0], 64 * shape[1]), None if s is None else list(s)))
        x = [torch.from_numpy(np.frombuffer(y, np.uint8).reshape(3, 64 * shape[0], 64 * shape[1]).copy()) for y in strings[0]]
        return {"x_hat": torch.stack(x).float().div(255)}


def _image(H, W, seed=7):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8))


@pytest.mark.parametrize("V", [0, 32])
@pytest.mark.parametrize("layout", ["hwc", "chw"])
def test_tiles_are_row_major_crops_and_the_decode_is_the_image(V, layout):
    H, W, T = 200, 330, 128
    img = _image(H, W)
    g = codec.tile_grid(H, W, T, V)
    net = StubNet()
    src = img if layout == "hwc" else img.permute(2, 0, 1).contiguous()
    data, info = codec.encode_tiled(net, src, tile=T, overlap=V, return_info=True)
    t = codec.parse_container_tiled(data)
    for k, (ty, tx, th, tw) in enumerate(g["rects"]):
        off, ln = codec.tiled_tile(data, t, k)
        assert data[off:off + ln] == codec.encode_images(StubNet(), img[ty:ty + th, tx:tx + tw])[0], k
    n, grid = len(g["rects"]), (g["ny"], g["nx"])
    assert grid == ((2, 4) if V else (2, 3))
    assert info["tile_bytes"] == [codec.tiled_tile(data, t, k)[1] for k in range(n)] and info["grid"] == grid
    assert (info["H"], info["W"], info["tile"], info["overlap"], info["bytes"], info["level"]) == (H, W, T, V, len(data), None)
    # one call per shape group (interior, right column, bottom row, corner), in order of first appearance
    shapes = [(h, w) for _, _, h, w in g["rects"]]
    groups = list(dict.fromkeys(shapes))
    assert len(groups) == 4
    assert [c[1:3] for c in net.calls] == [(shapes.count(s), (-(-s[0] // 64) * 64, -(-s[1] // 64) * 64)) for s in groups]
    out, dinfo = codec.decode_tiled(net, data, ref=img)
    assert torch.equal(out, img) and dinfo["sq_err"] == 0 and dinfo["psnr"] == float("inf")
    assert dinfo["tiles_decoded"] == list(range(n)) and dinfo["grid"] == grid and dinfo["region"] == (0, 0, H, W)
    assert (dinfo["H"], dinfo["W"], dinfo["tile"], dinfo["overlap"], dinfo["bytes"]) == (H, W, T, V, len(data))
    assert dinfo["bpp"] == 8.0 * len(data) / (H * W)
    # a non-contiguous source (a window of a larger canvas, RGBA) is read in place and gives the same file
    canvas = torch.zeros(H + 5, W + 7, 4, dtype=torch.uint8)
    canvas[2:H + 2, 3:W + 3, :3] = img
    view = canvas[2:H + 2, 3:W + 3, :3]
    assert codec.encode_tiled(StubNet(), view if layout == "hwc" else view.permute(2, 0, 1), tile=T, overlap=V) == data
    assert codec.encode_tiled(StubNet(), img.numpy(), tile=T, overlap=V) == data


def test_tile_batch_is_invisible_in_the_file():
    H, W, T, V = 300, 330, 128, 32  # 3 x 4 tiles: six interior tiles in two tile rows
    img = _image(H, W, 8)
    want = None
    for tb in (1, 2, 4, 5, 8, 100):
        net = StubNet()
        data = codec.encode_tiled(net, img, tile=T, overlap=V, tile_batch=tb)
        want = want or data
        assert data == want and max(c[1] for c in net.calls) <= tb
        assert sum(c[1] for c in net.calls) == 12
        dnet = StubNet()
        out, info = codec.decode_tiled(dnet, data, tile_batch=tb)
        assert torch.equal(out, img) and max(c[1] for c in dnet.calls) <= tb and sum(c[1] for c in dnet.calls) == 12
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="tile_batch"):
            codec.encode_tiled(StubNet(), img, tile=T, overlap=V, tile_batch=bad)
        with pytest.raises(ValueError, match="tile_batch"):
            codec.decode_tiled(StubNet(), want, tile_batch=bad)


@pytest.mark.parametrize("region, tiles", [
    ((40, 40, 50, 50), [0]),                    # inside tile 0's interior
    ((0, 0, 200, 96), [0, 4]),                  # the first column, left of every strip
    ((100, 100, 10, 10), [0, 1, 4, 5]),         # inside the corner four tiles share
    ((96, 96, 1, 1), [0, 1, 4, 5]),
    ((128, 127, 72, 203), [4, 5, 6, 7]),        # below the first row's extent
    ((0, 288, 96, 42), [2, 3]),
    ((0, 320, 96, 10), [3]),
    ((199, 329, 1, 1), [7]),
    (None, list(range(8))),
])
def test_region_decode_touches_exactly_the_intersecting_tiles(region, tiles):
    H, W, T, V = 200, 330, 128, 32
    img = _image(H, W, 9)
    data = codec.encode_tiled(StubNet(), img, tile=T, overlap=V)
    net = StubNet()
    out, info = codec.decode_tiled(net, data, region=region)
    y0, x0, h, w = region or (0, 0, H, W)
    assert torch.equal(out, img[y0:y0 + h, x0:x0 + w]) and info["tiles_decoded"] == tiles
    assert sum(c[1] for c in net.calls) == len(tiles) and all(c[0] == "decompress" for c in net.calls)
    assert info["region"] == (y0, x0, h, w)


def test_vbr_level_is_one_level_for_the_image():
    img = _image(150, 170, 10)
    net = StubNet(vbr=True)
    data, info = codec.encode_tiled(net, img, tile=128, overlap=16, level=4, return_info=True)
    assert info["level"] == 4 and all(c[3] == [4] * c[1] for c in net.calls)
    t = codec.parse_container_tiled(data)
    assert t.vbr == 1 and codec.peek(data, n_levels=6)["level"] == 4
    assert all(x["level"] == 4 for x in codec.peek(data, n_levels=6)["tiles"])
    out, dinfo = codec.decode_tiled(net, data)
    assert torch.equal(out, img) and dinfo["level"] == 4 and all(c[3] == [4] * c[1] for c in net.calls)
    with pytest.raises(_lib.MlicError, match="level"):
        codec.peek(data, n_levels=4)
    with pytest.raises(ValueError, match="level word"):
        codec.decode_tiled(StubNet(), data)
    with pytest.raises(ValueError, match="level word"):
        codec.decode_tiled(net, codec.encode_tiled(StubNet(), img, tile=128))
    with pytest.raises(ValueError, match="needs level"):
        codec.encode_tiled(net, img, tile=128)
    with pytest.raises(ValueError, match="fixed-rate"):
        codec.encode_tiled(StubNet(), img, tile=128, level=2)


def test_out_of_scope_combinations_are_refused():
    img = _image(150, 170, 11)
    vnet = StubNet(vbr=True)
    mask = torch.ones(150, 170, dtype=torch.uint8)
    for kw, word in ((dict(max_bpp=1.0, level=2), "max_bpp"), (dict(level="auto"), "auto"),
                     (dict(roi=mask, roi_levels=(0, 3)), "roi"), (dict(roi_levels=(0, 3)), "roi"),
                     (dict(level=[1, 2, 3, 4]), "per-tile levels"), (dict(level=(2,)), "per-tile levels"),
                     (dict(level=np.array([1, 2])), "per-tile levels")):
        with pytest.raises(ValueError, match=word):
            codec.encode_tiled(vnet, img, tile=128, **kw)
    assert vnet.calls == []
    with pytest.raises(ValueError, match="one image"):
        codec.encode_tiled(StubNet(), torch.stack([img, img]), tile=128)
    for bad in (dict(tile=100), dict(tile=64), dict(tile=128, overlap=8), dict(tile=128, overlap=128)):
        with pytest.raises(ValueError):
            codec.encode_tiled(StubNet(), img, **bad)
    data = codec.encode_tiled(StubNet(), img, tile=128)
    for region in ((0, 0, 151, 10), (-1, 0, 5, 5), (0, 0, 0, 5), (1, 2, 3)):
        with pytest.raises(ValueError, match="region"):
            codec.decode_tiled(StubNet(), data, region=region)
    with pytest.raises(ValueError, match="ref must be"):
        codec.decode_tiled(StubNet(), data, region=(0, 0, 10, 10), ref=img)
    with pytest.raises(ValueError, match="not a tiled file"):
        codec.decode_tiled(StubNet(), codec.encode_images(StubNet(), img)[0])
    with pytest.raises(_lib.MlicError, match="max_pixels"):
        codec.decode_tiled(StubNet(), data, max_pixels=150 * 170 - 1)
    # bitstream.code_image: tile= is off by default and goes with the level alone
    x = img.permute(2, 0, 1).unsqueeze(0).float().div(255)
    for kw in (dict(max_bpp=1.0), dict(roi=mask, roi_levels=(0, 3))):
        with pytest.raises(ValueError, match="tile="):
            bitstream.code_image(StubNet(), x, tile=128, **kw)


def test_code_image_tile_record():
    img = _image(150, 170, 12)
    x = img.permute(2, 0, 1).unsqueeze(0).float().div(255)
    r = bitstream.code_image(StubNet(), x, tile=128, overlap=16)
    data = codec.encode_tiled(StubNet(), img, tile=128, overlap=16)
    assert (r["H"], r["W"], r["bytes"], r["tile"], r["overlap"], r["grid"]) == (150, 170, len(data), 128, 16, (2, 2))
    assert r["bpp"] == 8.0 * len(data) / (150 * 170) and r["psnr"] == float("inf") and len(r["tile_bytes"]) == 4
    assert torch.equal(bitstream.to_u8(r["x_hat"])[0].permute(1, 2, 0), img)
    plain = bitstream.code_image(StubNet(), x)
    assert "tile" not in plain and set(plain) == {"H", "W", "bytes", "bpp", "psnr", "enc_s", "dec_s", "x_hat"}


def _cli():
    spec = importlib.util.spec_from_file_location("mlic_codec_tiled_cli", os.path.join(ROOT, "tools", "mlic_codec.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_tile_flags(capsys, tmp_path):
    cli = _cli()
    a = cli.parse_args(["encode", "a.ppm", "a.bit", "--synthetic", "1", "--tile", "256"])
    assert (a.tile, a.overlap, a.tile_batch, a.region) == (256, 32, 8, None)
    a = cli.parse_args(["decode", "a.bit", "a.ppm", "--synthetic", "1", "--region", "1", "2", "3", "4"])
    assert a.region == [1, 2, 3, 4] and a.tile is None
    for bad in (["encode", "a", "b", "--synthetic", "1", "--tile", "100"],
                ["encode", "a", "b", "--synthetic", "1", "--tile", "128", "--overlap", "8"],
                ["encode", "a", "b", "--synthetic", "1", "--overlap", "16"],
                ["encode", "a", "b", "--synthetic", "1", "--tile", "128", "--max-bpp", "1"],
                ["encode", "a", "b", "--synthetic", "1", "--tile", "128", "--roi", "m.ppm", "--roi-levels", "0", "3"],
                ["encode", "a", "b", "--synthetic", "1", "--tile", "128", "--tile-batch", "0"],
                ["encode", "a", "b", "--synthetic", "1", "--region", "0", "0", "1", "1"],
                ["decode", "a", "b", "--synthetic", "1", "--tile", "128"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    capsys.readouterr()
    # info on a tiled file needs no device: the grid and the per-tile sizes
    img = _image(150, 170, 13)
    data = codec.encode_tiled(StubNet(), img, tile=128, overlap=16)
    p = tmp_path / "t.bit"
    p.write_bytes(data)
    cli.main(["info", str(p), "--model", "MLICPP_S"])
    out = capsys.readouterr().out
    assert "150 x 170" in out and "tile 128, overlap 16, grid 2 x 2" in out and out.count("\n  tile ") == 4
    assert "at (112, 112), 38 x 58" in out
    # the file's flag is checked against the model before any tile is parsed: a message about the level word
    v = tmp_path / "v.bit"
    v.write_bytes(codec.encode_tiled(StubNet(vbr=True), img, tile=128, overlap=16, level=2))
    with pytest.raises(SystemExit, match="carry a level word, MLICPP_S is fixed-rate"):
        cli.main(["info", str(v), "--model", "MLICPP_S"])
    with pytest.raises(SystemExit, match="have no level word, MLICPP_S_VBR is variable-rate"):
        cli.main(["info", str(p), "--model", "MLICPP_S_VBR"])
    cli.main(["info", str(v), "--model", "MLICPP_S_VBR"])
    assert "level 2" in capsys.readouterr().out


def test_peek_honours_an_explicit_max_pixels():
    img = _image(150, 170, 14)
    data = codec.encode_tiled(StubNet(), img, tile=128, overlap=16)
    assert codec.peek(data)["tiled"] and codec.peek(data, max_pixels=150 * 170)["tiled"]
    for bound in (150 * 170 - 1, 1):
        with pytest.raises(_lib.MlicError, match="max_pixels"):
            codec.peek(data, max_pixels=bound)
    # a caller's 1 << 28 is a bound on a tiled file too, not a stand-in for the default
    big = bytearray(codec.write_container_tiled(200, 330, 128, 32, _tile_files(200, 330, 128, 32)))
    codec.parse_container_tiled(bytes(big), codec.MAX_PIXELS)
    huge = struct.pack(">II", 1 << 15, 1 << 14)  # 2^29 pixels: refused at 1 << 28 whatever else the file says
    big[6:14] = huge
    with pytest.raises(_lib.MlicError, match="max_pixels"):
        codec.peek(bytes(big), max_pixels=codec.MAX_PIXELS)
    with pytest.raises(_lib.MlicError, match="not the grid"):
        codec.peek(bytes(big))  # within the default whole-image bound: the next check speaks
    plain = codec.encode_images(StubNet(), img)[0]
    assert codec.peek(plain)["H"] == 150
    with pytest.raises(_lib.MlicError, match="max_pixels"):
        codec.peek(plain, max_pixels=1)
