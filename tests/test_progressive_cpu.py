"""Progressive coding, the parts that need no GPU: the layered container (round trip through the C and the Python
writer, the truncation sweep against the layout, every refusal by its own message, tools/container_layered_check.cpp
under AddressSanitizer + UBSan as a stand-alone program), and the policy of encode_images(layered=) /
decode_images(slices=) / decode_progressive with a stub model: grouping by (kind, K), what slices=None means on a
truncated file, and the argument refusals, which reach no library call."""
import importlib.util
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from mlic_amd import _lib, bitstream, codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layers(S, lens=(0, 1, 5, 9)):
    return [bytes((17 * k + i + 1) & 255 for i in range(lens[k % len(lens)])) for k in range(S)]


def _layout(z_len, layers, vbr):
    """(end of z, end of each layer) from the format's definition."""
    z_end = 16 + (4 if vbr else 0) + 8 + 4 + z_len
    ends, at = [], z_end
    for l in layers:
        at += 4 + len(l)
        ends.append(at)
    return z_end, ends


# ---------------------------------------------------------------------------------------- container
@pytest.mark.parametrize("S", [1, 4, 10])
@pytest.mark.parametrize("level", [None, 3])
def test_container_round_trip(S, level):
    H, W, z = 120, 200, b"\xa0\xa1\xa2"
    for layers in (_layers(S), [b""] * S, _layers(S, (7,))):
        data = codec.write_container_layered(H, W, (2, 4), z, layers, level)
        assert data == codec._write_container_layered_c(H, W, (2, 4), z, layers, level)
        assert len(data) == codec.container_layered_bytes(len(z), [len(l) for l in layers], level is not None)
        assert len(data) == _layout(len(z), layers, level is not None)[1][-1]
        assert data[:4] == b"MLL1" and data[4:8] == bytes([0, int(level is not None), S, 0])
        assert codec.is_layered_file(data) and not codec.is_tiled_file(data) and not codec.is_scaled_file(data)
        for trunc in (False, True):
            c = codec.parse_container_layered(data, 6, allow_truncated=trunc)
            assert (c.H, c.W, c.hz, c.wz, c.S, c.layers_present) == (H, W, 2, 4, S, S)
            assert c.level == (-1 if level is None else level)
            assert data[c.z_off:c.z_off + c.z_len] == z and codec._layers(data, c) == layers
        d = codec.peek(data, n_levels=6)
        assert d["layered"] and d["layer_bytes"] == [len(l) for l in layers] and d["layers_present"] == d["slices"] == S
        assert d["level"] == level and d["vbr"] == (level is not None) and d["shape"] == (2, 4)
        assert d["header_bytes"] + d["z_len"] + sum(d["layer_bytes"]) + 4 * S == d["bytes"] == len(data)


def test_truncation_sweep():
    layers, z = _layers(4), b"zzz"
    assert [len(l) for l in layers] == [0, 1, 5, 9]
    for level in (None, 2):
        data = codec.write_container_layered(120, 200, (2, 4), z, layers, level)
        z_end, ends = _layout(len(z), layers, level is not None)
        for n in range(len(data) + 1):
            want = sum(e <= n for e in ends)
            if n < z_end:
                with pytest.raises(_lib.MlicError, match="truncated|runs past the end"):
                    codec.parse_container_layered(data[:n], 6, allow_truncated=True)
            else:
                c = codec.parse_container_layered(data[:n], 6, allow_truncated=True)
                assert c.layers_present == want and codec._layers(data[:n], c) == layers[:want]
                assert codec.peek(data[:n], n_levels=6)["layers_present"] == want
            if n < len(data):
                with pytest.raises(_lib.MlicError):
                    codec.parse_container_layered(data[:n], 6)
        assert codec.parse_container_layered(data, 6).layers_present == 4
        for K in range(5):
            cut = codec.truncate_layered(data, K)
            assert cut == data[:z_end if K == 0 else ends[K - 1]]
            assert codec.parse_container_layered(cut, 6, allow_truncated=True).layers_present == K
            # a truncated file truncates further, never back
            assert codec.truncate_layered(cut, K) == cut
            with pytest.raises(ValueError, match="truncate_layered: K must be in"):
                codec.truncate_layered(cut, K + 1)
        with pytest.raises(ValueError, match="truncate_layered"):
            codec.truncate_layered(data, -1)


def _put32(data, at, v):
    return data[:at] + struct.pack(">I", v) + data[at + 4:]


def test_parser_refusals_each_by_its_message():
    layers, z = _layers(4), b"zzz"
    data = codec.write_container_layered(120, 200, (2, 4), z, layers, 3)
    z_end, ends = _layout(len(z), layers, True)

    def refused(bad, match, trunc=True, n_levels=6, max_pixels=codec.MAX_PIXELS):
        with pytest.raises(_lib.MlicError, match=match):
            codec.parse_container_layered(bad, n_levels, max_pixels, allow_truncated=trunc)

    refused(b"MLX1" + data[4:], "bad magic")
    refused(data[:4] + b"\x01" + data[5:], "unknown version")
    refused(data[:5] + b"\x03" + data[6:], "unknown flags")
    refused(data[:6] + b"\x00" + data[7:], "S is not in 1..32")
    refused(data[:6] + b"\x21" + data[7:], "S is not in 1..32")
    refused(data[:7] + b"\x01" + data[8:], "reserved byte is not 0")
    refused(data[:10], "truncated header")
    refused(data[:18], r"truncated header \(level\)")
    refused(data[:25], r"truncated header \(h_z, w_z\)")
    refused(data[:30], "truncated before the z length")
    refused(data[:z_end - 1], "the z length runs past the end")
    refused(_put32(data, 8, 0), "H or W is zero")
    refused(_put32(data, 16, 6), "level is not below n_levels")
    refused(_put32(data, 20, 3), "h_z, w_z are not")
    refused(data, "exceeds max_pixels", max_pixels=128 * 256 - 1)
    refused(_put32(data, z_end, 1 << 30), "a layer length runs past the end", trunc=False)
    refused(data[:ends[1] + 2], "truncated before a layer length", trunc=False)
    refused(data + b"\x00", "bytes left over after the last layer")
    refused(data + b"\x00", "bytes left over after the last layer", trunc=False)
    # the writer's own
    with pytest.raises(ValueError, match="1..32 layers"):
        codec.write_container_layered(64, 64, (1, 1), b"", [], None)
    with pytest.raises(ValueError, match="1..32 layers"):
        codec.write_container_layered(64, 64, (1, 1), b"", [b""] * 33, None)
    with pytest.raises(_lib.MlicError, match="S must be in 1..32"):
        codec._write_container_layered_c(64, 64, (1, 1), b"", [b""] * 33, None)
    with pytest.raises(_lib.MlicError, match="S must be in 1..32"):
        codec.container_layered_bytes(0, [0] * 33)


def test_other_parsers_refuse_a_layered_file():
    for level in (None, 3):
        data = codec.write_container_layered(120, 200, (2, 4), b"zzz", _layers(4), level)
        for vbr in (False, True):
            with pytest.raises(_lib.MlicError, match="container_parse"):
                codec.parse_container(data, vbr, 6)
        with pytest.raises(_lib.MlicError, match="container_parse"):
            codec.parse_container_roi(data, 6)
        with pytest.raises(_lib.MlicError, match="bad magic"):
            codec.parse_container_tiled(data)
        with pytest.raises(_lib.MlicError, match="bad magic"):
            codec.parse_container_scaled(data, 6)


def test_container_layered_check_program_under_sanitizers(tmp_path):
    """tools/container_layered_check.cpp with container.cpp, AddressSanitizer + UBSan, as a stand-alone program (no
    sanitizer runtime comes near Python): round trips, the truncation sweep, refusals and the header's bit-flip and
    overwrite sweep.  Skipped where the compiler cannot link the sanitizer runtimes."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed for the container's sanitizer check"
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run([cxx] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if p.returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed: " + p.stderr[-200:])
    exe = str(tmp_path / "container_layered_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g"] + san + [
           "-I" + os.path.join(ROOT, "mlic_amd", "csrc"), os.path.join(ROOT, "tools", "container_layered_check.cpp"),
           os.path.join(ROOT, "mlic_amd", "csrc", "container.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-300:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("container_layered_check ok"), \
        r.stdout[-2000:] + r.stderr[-2000:]


def test_phase_fill_entry_refuses_without_a_device():
    """mlic_phase_fill_run checks its descriptor before any HIP call (the pointers are never dereferenced); it asks
    for neither symbols nor gains."""
    import ctypes as C
    n = 3 * 4 * 6
    base = dict(params=64, params_bs=2 * n, yh=64, yh_bs=n, ntable=64, table=64, phase=1, vbr=1, B=2, C=3, H=4, W=6)
    for kw, msg in (({"yh": None}, "null tensor"), ({"params": None}, "null tensor"), ({"W": 7}, "W must be even"),
                    ({"phase": 2}, "phase must be"), ({"yh_bs": n - 1}, "yh_bs smaller"),
                    ({"params_bs": 2 * n - 1}, "params_bs smaller"), ({"B": 0}, "B must be"), ({"C": 0}, "C must be"),
                    ({"H": -2}, "H, W must be"), ({"vbr": 0, "rsp": 64}, "gain planes need vbr")):
        with pytest.raises(_lib.MlicError, match=msg):
            _lib.call("mlic_phase_fill_run", None, C.byref(_lib.QuantDesc(**{**base, **kw})))
    with pytest.raises(_lib.MlicError, match="null descriptor"):
        _lib.call("mlic_phase_fill_run", None, None)


# ------------------------------------------------------------------------------------------- policy
S_STUB = 4


class StubNet:
    """A 'model' on the CPU with 4 slices.  Layer k of an image is one byte, k + 16 * image mean's top nibble; z
    names the level.  A decode paints every pixel (10 * K + fill code + level) / 255, so the image says which call
    made it.  calls records (kind, batch size, z grid, K, fill, levels)."""
    device = torch.device("cpu")
    slice_num = S_STUB

    def __init__(self, vbr=False):
        if vbr:
            self.levels = 6
        self.calls = []

    def compress(self, x, s=None, layered=False):
        B, _, Hp, Wp = x.shape
        assert (s is None) == (not hasattr(self, "levels"))
        self.calls.append(("compress", B, (Hp // 64, Wp // 64), None, layered, s))
        tag = [int(x[b].mean() * 15) for b in range(B)]
        out = {"strings": [[bytes([tag[b]] * 5) for b in range(B)], [bytes([0 if s is None else s[b]]) for b in range(B)]],
               "shape": (Hp // 64, Wp // 64)}
        if layered:
            out["layers"] = [[bytes([16 * tag[b] + k]) * (k + 1) for k in range(S_STUB)] for b in range(B)]
        return out

    def _paint(self, kind, B, shape, K, fill, s):
        self.calls.append((kind, B, tuple(shape), K, fill, s))
        lv = [0] * B if s is None else list(s)
        v = torch.tensor([10 * K + (fill == "zero") + 2 * lv[b] for b in range(B)], dtype=torch.float32) / 255
        return {"x_hat": v.view(B, 1, 1, 1).expand(B, 3, 64 * shape[0], 64 * shape[1]).contiguous() + 0.001}

    def decompress(self, strings, shape, s=None, slices=None, fill="mean"):
        assert all(len(y) == 5 for y in strings[0])
        return self._paint("plain", len(strings[1]), shape, S_STUB if slices is None else slices, fill, s)

    def decompress_layers(self, layers, zs, shape, s=None, slices=None, fill="mean"):
        assert len({len(l) for l in layers}) == 1
        for l in layers:
            assert [len(x) for x in l] == list(range(1, len(l) + 1))
        K = len(layers[0]) if slices is None else slices
        assert K <= len(layers[0])
        return self._paint("layers", len(zs), shape, K, fill, s)


def _images(B=3, H=70, W=100):
    g = torch.Generator().manual_seed(5)
    return torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)


@pytest.mark.parametrize("vbr", [False, True])
def test_encode_layered_writes_layered_files(vbr):
    imgs, net = _images(), StubNet(vbr)
    level = [1, 4, 2] if vbr else None
    files, info = codec.encode_images(net, imgs, level=level, layered=True, return_info=True)
    assert net.calls == [("compress", 3, (2, 2), None, True, level)]
    for b, f in enumerate(files):
        c = codec.parse_container_layered(f, 6 if vbr else None)
        assert (c.H, c.W, c.hz, c.wz, c.S, c.layers_present) == (70, 100, 2, 2, S_STUB, S_STUB)
        assert c.level == (level[b] if vbr else -1)
        assert info[b]["layer_bytes"] == [1, 2, 3, 4] == codec.peek(f, n_levels=6)["layer_bytes"]
        assert info[b]["bytes"] == len(f)
    # without layered= nothing changes: a plain file, and compress is not asked for layers
    net = StubNet(vbr)
    plain = codec.encode_images(net, imgs, level=level)
    assert net.calls == [("compress", 3, (2, 2), None, False, level)] and not codec.is_layered_file(plain[0])


def test_decode_groups_by_kind_and_k():
    imgs, net = _images(4), StubNet()
    lay = codec.encode_images(net, imgs, layered=True)
    plain = codec.encode_images(net, imgs)
    files = [lay[0], codec.truncate_layered(lay[1], 2), plain[2], codec.truncate_layered(lay[3], 2), lay[2],
             codec.truncate_layered(lay[0], 0)]
    net.calls.clear()
    img, info = codec.decode_images(net, files)
    # slices=None: every layer present, file by file; the plain file beside them decodes whole
    assert [d["slices"] for d in info] == [4, 2, None, 2, 4, 0]
    assert [d.get("layers_present") for d in info] == [4, 2, None, 2, 4, 0]
    assert net.calls == [("layers", 2, (2, 2), 4, "mean", None), ("layers", 2, (2, 2), 2, "mean", None),
                         ("plain", 1, (2, 2), 4, "mean", None), ("layers", 1, (2, 2), 0, "mean", None)]
    assert img.shape == (6, 70, 100, 3)
    assert [int(img[b, 0, 0, 0]) for b in range(6)] == [40, 20, 40, 20, 40, 0]  # each from its own group, in order
    # slices=K on all of them: two groups, one per kind
    net.calls.clear()
    img, info = codec.decode_images(net, files[:5], slices=1, fill="zero")
    assert [d["slices"] for d in info] == [1] * 5
    assert net.calls == [("layers", 4, (2, 2), 1, "zero", None), ("plain", 1, (2, 2), 1, "zero", None)]
    assert [int(img[b, 0, 0, 0]) for b in range(5)] == [11] * 5
    # K above what a truncated file holds
    with pytest.raises(ValueError, match="slices=3, but the file holds 2 whole layers"):
        codec.decode_images(net, files, slices=3)
    # a cut in the middle of a layer is the file up to the layer before
    cut = lay[1][:len(codec.truncate_layered(lay[1], 3)) - 1]
    net.calls.clear()
    _, info = codec.decode_images(net, [cut])
    assert info[0]["slices"] == 2 and net.calls == [("layers", 1, (2, 2), 2, "mean", None)]


def test_decode_vbr_levels_ride_with_their_group():
    imgs, net = _images(3), StubNet(vbr=True)
    lay = codec.encode_images(net, imgs, level=[1, 4, 2], layered=True)
    files = [lay[0], codec.truncate_layered(lay[1], 1), lay[2]]
    net.calls.clear()
    img, info = codec.decode_images(net, files, ref=imgs)
    assert net.calls == [("layers", 2, (2, 2), 4, "mean", [1, 2]), ("layers", 1, (2, 2), 1, "mean", [4])]
    assert [d["level"] for d in info] == [1, 4, 2] and all("psnr" in d for d in info)
    assert [int(img[b, 0, 0, 0]) for b in range(3)] == [42, 18, 44]


def test_decode_progressive_steps():
    imgs, net = _images(1), StubNet()
    data = codec.encode_images(net, imgs, layered=True)[0]
    net.calls.clear()
    steps = codec.decode_progressive(net, data, ref=imgs[0])
    assert [s["slices"] for s in steps] == [1, 2, 4]  # (1, 2, 4, S) with S = 4
    assert [c[3] for c in net.calls] == [1, 2, 4] and all(c[0] == "layers" and c[1] == 1 for c in net.calls)
    assert [s["bytes"] for s in steps] == [len(codec.truncate_layered(data, k)) for k in (1, 2, 4)]
    for s in steps:
        one, info = codec.decode_images(net, [data], ref=imgs[:1], slices=s["slices"])
        assert torch.equal(s["image"], one[0]) and s["sq_err"] == info[0]["sq_err"] and s["psnr"] == info[0]["psnr"]
    # a truncated file: the steps it still has; a plain file: no byte counts
    assert [s["slices"] for s in codec.decode_progressive(net, codec.truncate_layered(data, 2))] == [1, 2]
    plain = codec.encode_images(net, imgs)[0]
    steps = codec.decode_progressive(net, plain, steps=(0, 3), fill="zero")
    assert [(s["slices"], s["bytes"]) for s in steps] == [(0, None), (3, None)]
    for bad in ((), (2, 1), (1, 1), (5,), (-1,), (True,), (1.0,)):
        with pytest.raises(ValueError, match="steps must be strictly increasing"):
            codec.decode_progressive(net, data, steps=bad)
    with pytest.raises(ValueError, match="holds 0 whole layers"):
        codec.decode_progressive(net, codec.truncate_layered(data, 0), steps=(1, 2))


class NoCallNet(StubNet):
    def compress(self, *a, **k):
        raise AssertionError("compress reached")

    def decompress(self, *a, **k):
        raise AssertionError("decompress reached")

    decompress_layers = decompress


def test_argument_refusals_reach_no_library_call(monkeypatch):
    imgs = _images(2)
    net = StubNet(vbr=True)
    lay = codec.encode_images(net, imgs, level=2, layered=True)
    plain = codec.encode_images(net, imgs, level=2)
    roi_file = codec.write_container_roi(70, 100, (2, 2), b"yyyyy", b"\x02", 2, np.zeros((2, 2), np.uint8))
    scaled = codec.write_container_scaled(70, 100, plain[0], vbr=True)
    tiled = codec.write_container_tiled(192, 192, 128, 0, [codec.write_container(128, 128, (2, 2), b"y", b"z", 2),
                                                           codec.write_container(128, 64, (2, 1), b"y", b"z", 2),
                                                           codec.write_container(64, 128, (1, 2), b"y", b"z", 2),
                                                           codec.write_container(64, 64, (1, 1), b"y", b"z", 2)], vbr=True)

    def boom(name, *a):
        raise AssertionError(f"library call {name} reached")
    monkeypatch.setattr(_lib, "call", boom)
    no = NoCallNet(vbr=True)
    mask = torch.ones(2, 70, 100, dtype=torch.uint8)
    enc = [(dict(roi=mask, roi_levels=(1, 3)), "layered=True together with roi"),
           (dict(max_bpp=0.5, level=2), "layered=True together with max_bpp"),
           (dict(max_bpp=0.5, level="auto"), "layered=True together with max_bpp"),
           (dict(level="auto"), "layered=True together with level='auto'"),
           (dict(scale=0.5, level=2), "layered=True together with scale"),
           (dict(coded_size=(35, 50), level=2), "layered=True together with coded_size")]
    for kw, match in enc:
        with pytest.raises(ValueError, match=match):
            codec.encode_images(no, imgs, layered=True, **kw)
    with pytest.raises(ValueError, match="encode_tiled: layered=True together with tiles"):
        codec.encode_tiled(no, imgs[0], tile=128, level=2, layered=True)
    fmt = codec.YuvFormat()
    planes = (torch.zeros(1, 64, 64, dtype=torch.uint8), torch.zeros(1, 32, 32, dtype=torch.uint8),
              torch.zeros(1, 32, 32, dtype=torch.uint8))
    with pytest.raises(ValueError, match="encode_yuv: layered=True together with Y'CbCr frames"):
        codec.encode_yuv(no, *planes, fmt, level=2, layered=True)
    with pytest.raises(ValueError, match="decode_yuv: slices= / layered files together with Y'CbCr"):
        codec.decode_yuv(no, [plain[0]], fmt, slices=1)
    with pytest.raises(ValueError, match="decode_yuv: slices= / layered files together with Y'CbCr"):
        codec.decode_yuv(no, [lay[0]], fmt)
    dec = [(dict(files=[lay[0]], slices=5), r"slices must be an integer in \[0, 4\]"),
           (dict(files=[lay[0]], slices=-1), r"slices must be an integer in \[0, 4\]"),
           (dict(files=[lay[0]], slices=True), r"slices must be an integer in \[0, 4\]"),
           (dict(files=[lay[0]], slices=1.0), r"slices must be an integer in \[0, 4\]"),
           (dict(files=[lay[0]], slices=1, fill="median"), "fill must be 'mean' or 'zero'"),
           (dict(files=[plain[0]], fill="zero"), "fill= goes with slices= or layered files"),
           (dict(files=[lay[0]], slices=1, out_size=(35, 50)), "together with out_size= are not supported"),
           (dict(files=[lay[0]], out_size=(35, 50)), "together with out_size= are not supported"),
           (dict(files=[plain[0]], slices=1, filter="bicubic"), "filter= goes with scaled files"),
           (dict(files=[scaled], slices=1), "slices= on a scaled file is not supported"),
           (dict(files=[tiled], slices=1), "slices= on a tiled file is not supported")]
    for kw, match in dec:
        with pytest.raises(ValueError, match=match):
            codec.decode_images(no, kw.pop("files"), **kw)
    with pytest.raises(ValueError, match="decode_tiled: slices= on a tiled file is not supported"):
        codec.decode_tiled(no, tiled, slices=1)
    with pytest.raises(ValueError, match="fill must be 'mean' or 'zero'"):
        codec.decode_progressive(no, lay[0], fill="none")
    monkeypatch.undo()
    # these go through the validating parsers (library calls, on the host), and still never reach the model
    with pytest.raises(ValueError, match="slices= on an ROI file is not supported"):
        codec.decode_images(no, [roi_file], slices=1)
    with pytest.raises(ValueError, match="the layered file has no level word, the model is variable-rate"):
        codec.decode_images(no, [codec.write_container_layered(70, 100, (2, 2), b"z", [b"a"] * 4, None)])
    with pytest.raises(ValueError, match="the layered file has 3 layers, the model has 4 slices"):
        codec.decode_images(no, [codec.write_container_layered(70, 100, (2, 2), b"z", [b"a"] * 3, 2)])
    with pytest.raises(ValueError, match="the layered file carries a level word, the model is fixed-rate"):
        codec.decode_images(NoCallNet(), [lay[0]])
    with pytest.raises(_lib.MlicError, match="truncated"):
        codec.decode_images(no, [lay[0][:20]])
    with pytest.raises(ValueError, match="must share one padded size"):
        codec.decode_images(no, [lay[0], codec.write_container_layered(64, 64, (1, 1), b"z", [b"a"] * 4, 2)])


def test_code_image_progressive_fields():
    class Net(StubNet):
        def decompress_layers(self, layers, zs, shape, **kw):
            K = len(layers[0])
            self.calls.append(("layers", K))
            return {"x_hat": torch.full((1, 3, 64 * shape[0], 64 * shape[1]), 0.1 * K)}

    x = _images(1)[0:1].permute(0, 3, 1, 2).contiguous().float().div(255)
    net = Net()
    r = bitstream.code_image(net, x, progressive=True)
    assert r["layer_bytes"] == [1, 2, 3, 4] and len(r["prefix_psnr"]) == S_STUB + 1
    assert r["prefix_psnr"][-1] == r["psnr"]
    assert [c for c in net.calls if c[0] == "layers"] == [("layers", 4)] + [("layers", k) for k in range(4)]
    assert r["bytes"] == 16 + 8 + 4 + 1 + sum(4 + n for n in r["layer_bytes"])
    assert "layer_bytes" not in bitstream.code_image(_PlainNet(), x)
    for kw in (dict(tile=128), dict(max_bpp=0.5), dict(roi=torch.ones(70, 100), roi_levels=(0, 1)),
               dict(batch_stream=True)):
        with pytest.raises(ValueError, match="progressive=True together with"):
            bitstream.code_image(NoCallNet(), x, progressive=True, **kw)


class _PlainNet(StubNet):
    def decompress(self, strings, shape, **kw):
        return {"x_hat": torch.full((1, 3, 64 * shape[0], 64 * shape[1]), 0.5)}


# ---------------------------------------------------------------------------------------------- CLI
def _cli():
    spec = importlib.util.spec_from_file_location("mlic_codec_cli", os.path.join(ROOT, "tools", "mlic_codec.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flags_and_truncate(tmp_path, capsys):
    cli = _cli()
    a = cli.parse_args(["encode", "a.ppm", "a.bit", "--synthetic", "0", "--layered"])
    assert a.layered and a.slices is None
    a = cli.parse_args(["decode", "a.bit", "a.ppm", "--synthetic", "0", "--slices", "3", "--fill", "zero"])
    assert (a.slices, a.fill) == (3, "zero")
    assert not cli.parse_args(["encode", "a.ppm", "a.bit", "--synthetic", "0"]).layered
    bad = [["encode", "a.ppm", "a.bit", "--synthetic", "0", "--layered", "--max-bpp", "0.5"],
           ["encode", "a.ppm", "a.bit", "--synthetic", "0", "--layered", "--tile", "128"],
           ["encode", "a.ppm", "a.bit", "--synthetic", "0", "--layered", "--scale", "1/2"],
           ["encode", "a.y4m", "a.bit", "--synthetic", "0", "--layered"],
           ["decode", "a.bit", "a.ppm", "--synthetic", "0", "--layered"],
           ["encode", "a.ppm", "a.bit", "--synthetic", "0", "--slices", "2"],
           ["decode", "a.bit", "a.ppm", "--synthetic", "0", "--slices", "-1"],
           ["decode", "a.bit", "a.ppm", "--synthetic", "0", "--slices", "2", "--out-size", "10x10"],
           ["decode", "a.bit", "a.y4m", "--synthetic", "0", "--slices", "2"],
           ["decode", "a.bit", "a.ppm", "--synthetic", "0", "-k", "2"],
           ["truncate", "a.bit", "-k", "2"], ["truncate", "a.bit", "-o", "b.bit"],
           ["truncate", "a.bit", "b.bit", "-k", "2", "-o", "c.bit"],
           ["truncate", "a.bit", "-k", "-1", "-o", "b.bit"],
           ["truncate", "a.bit", "-k", "1", "-o", "b.bit", "--level", "2"]]
    for argv in bad:
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
    capsys.readouterr()
    data = codec.write_container_layered(120, 200, (2, 4), b"zzz", _layers(4), None)
    src, dst = tmp_path / "a.bit", tmp_path / "b.bit"
    src.write_bytes(data)
    cli.main(["truncate", str(src), "-k", "2", "-o", str(dst)])
    assert dst.read_bytes() == codec.truncate_layered(data, 2)
    assert "2 layers" in capsys.readouterr().out
    cli.main(["info", str(dst), "--model", "MLICPP_L"])
    out = capsys.readouterr().out
    assert "layered: 2 of 4 layers (truncated)" in out and "layer 1: 1 B" in out
    with pytest.raises(SystemExit, match="K must be in"):
        cli.main(["truncate", str(dst), "-k", "3", "-o", str(tmp_path / "c.bit")])
    plain = tmp_path / "p.bit"
    plain.write_bytes(codec.write_container(64, 64, (1, 1), b"y", b"z"))
    with pytest.raises(SystemExit, match="not a layered file"):
        cli.main(["truncate", str(plain), "-k", "1", "-o", str(tmp_path / "c.bit")])
