"""Residual coding, the parts that need no GPU: the integer definitions through their NumPy restatement (the bound
over all 256 x 256 x 128 cases, the class sizes, the digest), the tables and the rANS round trip with escapes, the
residual container (round trip, the truncation sweep against the layout, every refusal by its own message, the other
parsers refusing it, tools/container_residual_check.cpp under AddressSanitizer + UBSan as a stand-alone program),
the kernel entries' argument refusals (made before any GPU call), and the policy of encode_images(max_error=) /
decode_images with a stub model: the CPU path end to end and every refusal by name."""
import ctypes as C
import importlib.util
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from mlic_amd import _lib, bitstream, codec, entropy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------ definitions
def test_bound_for_every_sample_base_and_tau():
    """|x - rec| <= tau, rec = x at tau 0 and |q| <= 255, for all 256 x 256 x 128 (x, base, tau)."""
    x, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    for tau in range(128):
        q, rec = codec._quantise_np(x, b, tau)
        assert np.abs(x - rec).max() <= tau, tau
        assert np.abs(q).max() <= 255 and rec.min() >= 0 and rec.max() <= 255
        if tau == 0:
            assert (rec == x).all() and (q == x - b).all()


def test_restatements_use_the_definition():
    """front's sym / max_err and apply's out are the quantiser above, in the canonical order, in both layouts."""
    g = torch.Generator().manual_seed(3)
    base = torch.randint(0, 256, (2, 6, 9, 3), dtype=torch.uint8, generator=g)
    x = torch.randint(0, 256, (2, 6, 9, 3), dtype=torch.uint8, generator=g)
    for tau in (0, 1, 5, 127):
        f = codec._residual_front_cpu(base, x, tau)
        q, rec = codec._quantise_np(x.permute(0, 3, 1, 2).numpy().astype(np.int64),
                                    base.permute(0, 3, 1, 2).numpy().astype(np.int64), tau)
        assert (f["sym"].numpy() == q).all() and f["sym"].dtype == torch.int16
        assert f["max_err"].tolist() == [int(np.abs(x[i].permute(2, 0, 1).numpy() - rec[i]).max()) for i in range(2)]
        out, sq, me = codec._residual_apply_cpu(base, f["sym"], tau, ref=x)
        assert (out.permute(0, 3, 1, 2).numpy() == rec).all() and int(me.max()) <= tau
        assert sq.tolist() == [int(((x[i].numpy().astype(np.int64) - out[i].numpy()) ** 2).sum()) for i in range(2)]
        # the other layout: the same canonical planes
        f2 = codec._residual_front_cpu(base.permute(0, 3, 1, 2).contiguous(), x, tau, "chw", "hwc")
        for k in f:
            assert torch.equal(f[k], f2[k]), k
        # front without x: the shared outputs
        f3 = codec._residual_front_cpu(base, None, tau)
        assert set(f3) == {"ctx", "ctx_count", "digest"} and all(torch.equal(f3[k], f[k]) for k in f3)


def test_class_sizes_and_contexts():
    sizes = np.bincount(codec._CLASS_OF, minlength=8)
    assert sizes.tolist() == [2, 2, 4, 8, 16, 32, 64, 128]
    assert all(codec._CLASS_OF[a] == (0 if a < 2 else int(np.floor(np.log2(a)))) for a in range(256))
    # a 1 x 2 image with values (0, a): both samples see max - min = a, in each channel's own context block
    for a in (0, 1, 2, 3, 4, 127, 128, 255):
        img = torch.tensor([[[0, 0, 0], [a, a, a]]], dtype=torch.uint8)
        f = codec._residual_front_cpu(img)
        want = [8 * c + int(codec._CLASS_OF[a]) for c in range(3)]
        assert f["ctx"][0, :, 0, :].tolist() == [[w, w] for w in want]
        assert f["ctx_count"][0].tolist() == [2 if k in want else 0 for k in range(24)]
    # edge replication: a step edge one pixel from the border leaves the far side flat
    img = torch.zeros(1, 5, 7, 3, dtype=torch.uint8)
    img[:, :, 1:] = 200
    ctx = codec._residual_front_cpu(img)["ctx"][0, 0]
    assert (ctx[:, :2] == 7).all() and (ctx[:, 2:] == 0).all()


def test_digest_changes_with_every_single_byte():
    g = torch.Generator().manual_seed(7)
    img = torch.randint(0, 256, (1, 5, 7, 3), dtype=torch.uint8, generator=g)
    d0 = int(codec._residual_front_cpu(img)["digest"][0]) & M64
    flat = img.permute(0, 3, 1, 2).reshape(-1).tolist()
    assert d0 == sum((v + 1) * (((i + 1) * 0x9E3779B97F4A7C15) & M64) for i, v in enumerate(flat)) & M64
    # every other value of every byte: one batch of 255 changed images per position
    for y in range(5):
        for x in range(7):
            for c in range(3):
                m = img.repeat(255, 1, 1, 1)
                m[:, y, x, c] = torch.tensor([v for v in range(256) if v != int(img[0, y, x, c])], dtype=torch.uint8)
                d = codec._residual_front_cpu(m)["digest"]
                assert not bool((d == codec._residual_front_cpu(img)["digest"][0]).any()), (y, x, c)


# ---------------------------------------------------------------------------------------------- tables
def _hist():
    h = np.zeros((24, 128), np.int64)
    h[0, 63] = 1000                      # q = 0 only: m = 0
    h[1, 63 - 5], h[1, 63 + 2], h[1, 127] = 3, 900, 7   # m = 5, with escapes
    h[2, 127] = 11                       # escapes only: m = 0
    h[9, 0], h[9, 126], h[9, 63] = 1, 1, 1 << 20  # m = 63, a steep histogram: the rare symbols keep frequency 1
    h[23, 63 - 1:63 + 2] = (5, 6, 7)     # m = 1
    return h


def test_tables_from_a_histogram():
    h = _hist()
    t = codec.residual_tables(h)
    want_m = {0: 0, 1: 5, 2: 0, 9: 63, 23: 1}
    for k in range(24):
        if k not in want_m:
            assert t["m"][k] == 0xFF and t["length"][k] == 0 and not t["freq"][k].any()
            continue
        m = want_m[k]
        n = 2 * m + 2
        assert t["m"][k] == m and t["length"][k] == n + 1 and t["offset"][k] == -m
        f = t["freq"][k].astype(np.int64)
        assert f[:n].sum() == 65536 and f[:n].min() >= 1 and not f[n:].any()
        assert (t["cdf"][k, :n + 1] == np.concatenate([[0], np.cumsum(f[:n])])).all() and not t["cdf"][k, n + 1:].any()
        # the library's own quantiser on count / total as float32, the escape's count last
        pmf = np.concatenate([h[k, 63 - m:63 + m + 1], h[k, 127:]]).astype(np.float32) / np.float32(h[k].sum())
        assert (entropy.pmf_to_quantized_cdf(pmf) == t["cdf"][k, :n + 1]).all()
    assert t["freq"][9, 0] == 1 and t["freq"][9, 126] == 1
    t2 = codec._tables_of_freq(t["m"], t["freq"])
    assert all((t2[k] == t[k]).all() for k in ("m", "cdf", "length", "offset"))
    with pytest.raises(ValueError, match="residual_tables"):
        codec.residual_tables(np.zeros((24, 127)))
    with pytest.raises(_lib.MlicError, match="null hist"):
        _lib.call("mlic_residual_tables", None, None, None, None, None, None)


def test_rans_round_trip_with_escapes_and_an_m0_context():
    t = codec.residual_tables(_hist())
    sym = np.array([0, 0, 0, 2, -5, 64, -64, 255, -255, 6, 0, 17, -200, 1, -1, 0, 63, -63, 100], np.int32)
    ctx = np.array([0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 23, 23, 23, 9, 9, 9], np.int32)
    tabs = codec._coder_tables(t)
    data = entropy.rans_encode(sym, ctx, *tabs)
    assert (entropy.rans_decode(data, ctx, *tabs) == sym).all()
    # an m = 0 context codes 0 in its table and everything else through the escape
    assert t["m"][0] == 0 and t["m"][2] == 0
    z = np.array([0, 1, -1, 64, -255, 255, 0], np.int32)
    data = entropy.rans_encode(z, np.zeros(7, np.int32), *tabs)
    assert (entropy.rans_decode(data, np.zeros(7, np.int32), *tabs) == z).all()


# ------------------------------------------------------------------------------------------- container
def _file(level=None, tau=3, res=b"\x01\x02\x03\x04\x05", H=120, W=200):
    t = codec.residual_tables(_hist())
    inner = codec.write_container(H, W, ((H + 63) // 64, (W + 63) // 64), b"yyyyyyy", b"zzz", level)
    return codec.write_container_residual(H, W, inner, res, tau, 0x0123456789ABCDEF, t["m"], t["freq"],
                                          vbr=level is not None), inner, t


def _table_bytes(t):
    return sum(1 + (0 if m == 0xFF else 2 * (2 * int(m) + 2)) for m in t["m"])


@pytest.mark.parametrize("level", [None, 3])
def test_container_round_trip(level):
    for tau, res in ((0, b""), (3, b"\x01\x02\x03"), (127, bytes(range(200)))):
        data, inner, t = _file(level, tau, res)
        assert data[:8] == b"MLR1" + bytes([0, int(level is not None), tau, 24])
        assert data[8:24] == struct.pack(">IIQ", 120, 200, 0x0123456789ABCDEF)
        assert len(data) == 24 + _table_bytes(t) + 4 + len(inner) + 4 + len(res)
        assert codec.is_residual_file(data) and not codec.is_scaled_file(data) and not codec.is_layered_file(data) \
            and not codec.is_tiled_file(data)
        s = codec.parse_container_residual(data, 6)
        assert (s.H, s.W, s.tau, bool(s.vbr), s.digest) == (120, 200, tau, level is not None, 0x0123456789ABCDEF)
        assert data[s.inner_off:s.inner_off + s.inner_len] == inner == codec.strip_residual(data)
        assert data[s.res_off:s.res_off + s.res_len] == res
        assert list(s.m) == t["m"].tolist() and s.inner.level == (-1 if level is None else level)
        t2 = codec._file_tables(data, s)
        assert all((t2[k] == t[k]).all() for k in ("m", "cdf", "length", "offset"))
        d = codec.peek(data, n_levels=6)
        assert d["residual"] and d["max_error"] == tau and d["level"] == level and d["shape"] == (2, 4)
        assert (d["base_bytes"], d["residual_bytes"]) == (len(inner), len(res))
        assert d["header_bytes"] + d["base_bytes"] + d["residual_bytes"] == d["bytes"] == len(data)


def test_truncation_sweep():
    for level in (None, 2):
        data, inner, t = _file(level)
        head = 24 + _table_bytes(t)
        for n in range(len(data)):
            with pytest.raises(_lib.MlicError, match="truncated|runs past the end|bad magic"):
                codec.parse_container_residual(data[:n], 6)
        for n, msg in ((23, "truncated header"), (24, "truncated before a table's m"), (head - 1, "truncated inside a table"),
                       (head + 3, "truncated before the inner length"), (head + 4, "the inner length runs past the end"),
                       (head + 4 + len(inner) + 3, "truncated before the residual length"),
                       (len(data) - 1, "the residual length runs past the end")):
            with pytest.raises(_lib.MlicError, match=msg):
                codec.parse_container_residual(data[:n], 6)
        codec.parse_container_residual(data, 6)


def _put(data, at, raw):
    return data[:at] + raw + data[at + len(raw):]


def test_parser_refusals_each_by_its_message():
    data, inner, t = _file(3)
    head = 24 + _table_bytes(t)
    first = 24  # context 0 is present: its m byte, then 2 frequencies
    assert t["m"][0] == 0
    cases = [(_put(data, 0, b"MLS1"), "bad magic"), (_put(data, 4, b"\x01"), "unknown version"),
             (_put(data, 5, b"\x03"), "unknown flags"), (_put(data, 6, b"\x80"), "tau above 127"),
             (_put(data, 7, b"\x17"), "n_ctx is not 24"), (_put(data, 8, struct.pack(">I", 0)), "H or W is zero"),
             (_put(data, 12, struct.pack(">I", 0)), "H or W is zero"), (_put(data, first, b"\x40"), "an m outside 0..63"),
             (_put(data, first, b"\xfe"), "an m outside 0..63"), (_put(data, first + 1, b"\x00\x00"), "a zero frequency"),
             (_put(data, first + 1, b"\x00\x01"), "do not sum to 65536"),
             (_put(data, head, struct.pack(">I", len(data))), "the inner length runs past the end"),
             (_put(data, head, struct.pack(">I", 0)), "an empty inner file"),
             (_put(data, head + 4 + len(inner), struct.pack(">I", 6)), "the residual length runs past the end"),
             (data + b"\x00", "bytes left over"),
             (_put(data, 5, b"\x00"), "container_parse"),  # the flag no longer matches the inner file
             (_put(data, head + 4, struct.pack(">I", 0)), "container_parse: H or W is zero"),
             (_put(data, head + 4 + 8, struct.pack(">I", 6)), "level is not below n_levels"),
             (_put(data, head + 4 + 4, struct.pack(">I", 199)), "the inner file's H x W is not the outer one"),
             (_put(data, head + 4, struct.pack(">I", 121)), "the inner file's H x W is not the outer one")]
    for bad, msg in cases:
        with pytest.raises(_lib.MlicError, match=msg):
            codec.parse_container_residual(bad, 6)
    with pytest.raises(_lib.MlicError, match="image exceeds max_pixels"):
        codec.parse_container_residual(data, 6, max_pixels=120 * 200 - 1)
    with pytest.raises(_lib.MlicError, match="null info"):
        _lib.call("mlic_container_parse_residual", data, len(data), 6, 1 << 28, None)
    # the writer's refusals
    for kw, msg in (({"H": 0}, "H or W is zero"), ({"tau": 128}, "tau above 127"), ({"inner": b""}, "an empty inner file")):
        a = {"H": 120, "W": 200, "inner": inner, "res": b"r", "tau": 3, "digest": 1, "m": t["m"], "freq": t["freq"], **kw}
        with pytest.raises(_lib.MlicError, match=msg):
            codec.write_container_residual(**a)
    m = t["m"].copy()
    m[0] = 64
    with pytest.raises(_lib.MlicError, match="an m outside 0..63"):
        codec.write_container_residual(120, 200, inner, b"", 3, 1, m, t["freq"])
    f = t["freq"].copy()
    f[0, 0] = 0
    with pytest.raises(_lib.MlicError, match="a zero frequency"):
        codec.write_container_residual(120, 200, inner, b"", 3, 1, t["m"], f)
    f[0, 0] = t["freq"][0, 0] - 1
    with pytest.raises(_lib.MlicError, match="do not sum to 65536"):
        codec.write_container_residual(120, 200, inner, b"", 3, 1, t["m"], f)


def test_other_parsers_refuse_a_residual_file():
    for level in (None, 3):
        data, _, _ = _file(level)
        for vbr in (False, True):
            with pytest.raises(_lib.MlicError):
                codec.parse_container(data, vbr, 6)
        with pytest.raises(_lib.MlicError):
            codec.parse_container_roi(data, 6)
        with pytest.raises(_lib.MlicError, match="bad magic"):
            codec.parse_container_tiled(data)
        with pytest.raises(_lib.MlicError, match="bad magic"):
            codec.parse_container_scaled(data, 6)
        for trunc in (False, True):
            with pytest.raises(_lib.MlicError, match="bad magic"):
                codec.parse_container_layered(data, 6, allow_truncated=trunc)
        plain = codec.strip_residual(data)
        with pytest.raises(_lib.MlicError, match="bad magic"):
            codec.parse_container_residual(plain, 6)


def test_container_residual_check_program_under_sanitizers(tmp_path):
    """tools/container_residual_check.cpp with container.cpp, AddressSanitizer + UBSan, as a stand-alone program (no
    sanitizer runtime comes near Python): round trips, every truncation, refusals, the seeded overwrite sweep and
    the exhaustive sweeps of residual.h.  Skipped where the compiler cannot link the sanitizer runtimes."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed for the container's sanitizer check"
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run([cxx] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if p.returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed: " + p.stderr[-200:])
    exe = str(tmp_path / "container_residual_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g"] + san + [
           "-I" + os.path.join(ROOT, "mlic_amd", "csrc"), os.path.join(ROOT, "tools", "container_residual_check.cpp"),
           os.path.join(ROOT, "mlic_amd", "csrc", "container.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-300:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("container_residual_check ok"), \
        r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------ the entries' refusals
def test_kernel_entries_refuse_bad_arguments_before_any_gpu_call():
    """Every argument is checked before any HIP call: the pointers (small fake addresses) are never dereferenced."""
    s4 = (C.c_int64 * 4)(300, 30, 3, 1)
    z4 = (C.c_int64 * 4)(300, 30, 0, 1)
    front = dict(base=64, bs=s4, x=64, xs=s4, B=1, H=4, W=5, tau=1, ctx=64, count=64, digest=64, sym=64, hist=64, merr=64)
    order = ("base", "bs", "x", "xs", "B", "H", "W", "tau", "ctx", "count", "digest", "sym", "hist", "merr")
    for kw, msg in (({"base": None}, "null base"), ({"bs": None}, "null base strides"), ({"B": 0}, "B must be positive"),
                    ({"H": 0}, "H and W must be positive"), ({"W": -1}, "H and W must be positive"),
                    ({"tau": -1}, "tau must be in 0..127"), ({"tau": 128}, "tau must be in 0..127"),
                    ({"bs": z4}, r"zero column or channel stride \(base\)"), ({"ctx": None}, "null ctx"),
                    ({"count": None}, "null ctx_count"), ({"digest": None}, "null digest"),
                    ({"digest": 68}, "digest 8-byte aligned"), ({"count": 66}, "ctx_count must be 4-byte"),
                    ({"xs": None}, "x needs strides"), ({"xs": z4}, r"zero column or channel stride \(x\)"),
                    ({"sym": None}, "with x, sym, hist and max_err are all needed"),
                    ({"hist": None}, "with x, sym, hist and max_err are all needed"),
                    ({"merr": None}, "with x, sym, hist and max_err are all needed"),
                    ({"sym": 65}, "sym must be 2-byte"), ({"hist": 66}, "hist and max_err 4-byte aligned"),
                    ({"x": None, "xs": None}, "sym, hist and max_err go with x"),
                    ({"B": 1 << 30, "H": 1 << 20}, "batch too large")):
        a = {**front, **kw}
        with pytest.raises(_lib.MlicError, match=msg):
            _lib.call("mlic_image_residual_front_u8", None, *[a[k] for k in order])
    apply = dict(base=64, bs=s4, sym=64, B=1, H=4, W=5, tau=1, out=64, os=s4, ref=64, rs=s4, sq=64, merr=64)
    order = ("base", "bs", "sym", "B", "H", "W", "tau", "out", "os", "ref", "rs", "sq", "merr")
    for kw, msg in (({"base": None}, "null base"), ({"bs": None}, "null base strides"), ({"sym": None}, "null sym"),
                    ({"out": None}, "null out or out strides"), ({"os": None}, "null out or out strides"),
                    ({"B": 0}, "B must be positive"), ({"H": 0}, "H and W must be positive"),
                    ({"tau": 128}, "tau must be in 0..127"), ({"tau": -3}, "tau must be in 0..127"),
                    ({"bs": z4}, r"zero column or channel stride \(base\)"),
                    ({"os": z4}, r"zero column or channel stride \(out\)"), ({"sym": 65}, "sym must be 2-byte aligned"),
                    ({"sq": None}, "ref without sq_err"), ({"merr": None}, "ref without max_err"),
                    ({"ref": None, "rs": None}, "sq_err and max_err go with ref"),
                    ({"rs": None}, "ref needs strides"), ({"rs": z4}, "ref needs strides"),
                    ({"sq": 68}, "sq_err must be 8-byte"), ({"merr": 66}, "max_err 4-byte aligned"),
                    ({"B": 1 << 30, "H": 1 << 20, "ref": None, "rs": None, "sq": None, "merr": None}, "batch too large")):
        a = {**apply, **kw}
        with pytest.raises(_lib.MlicError, match=msg):
            _lib.call("mlic_image_residual_apply_u8", None, *[a[k] for k in order])


# ---------------------------------------------------------------------------------------------- policy
class StubNet:
    """A 'model' on the CPU.  compress keeps a coarse picture of each image (its 8 x 8 block means, one byte each,
    as the y string); decompress paints it back, so the base image is a real, lossy picture of the input and is
    bit-identical from call to call.  calls records (kind, batch size)."""
    device = torch.device("cpu")
    slice_num = 4

    def __init__(self, vbr=False, drift=0.0):
        if vbr:
            self.levels = 6
        self.calls, self.drift = [], drift

    def compress(self, x, s=None, layered=False, gain_map=None):
        B, _, Hp, Wp = x.shape
        assert (s is None) == (not hasattr(self, "levels"))
        self.calls.append(("compress", B))
        m = torch.nn.functional.avg_pool2d(x, 8)
        ys = [bytes((m[b] * 255).round().to(torch.uint8).reshape(-1).tolist()) for b in range(B)]
        return {"strings": [ys, [bytes([0 if s is None else s[b]]) for b in range(B)]], "shape": (Hp // 64, Wp // 64)}

    def decompress(self, strings, shape, s=None, **kw):
        B = len(strings[0])
        assert (s is None) == (not hasattr(self, "levels"))
        self.calls.append(("decompress", B))
        h, w = 8 * shape[0], 8 * shape[1]
        m = torch.stack([torch.tensor(list(y), dtype=torch.float32).view(3, h, w) for y in strings[0]]) / 255
        x = torch.nn.functional.interpolate(m, scale_factor=8, mode="nearest")
        return {"x_hat": (x + self.drift).contiguous()}


def _images(B=3, H=70, W=100):
    g = torch.Generator().manual_seed(5)
    smooth = torch.nn.functional.interpolate(torch.rand(B, 3, 5, 6, generator=g), size=(H, W), mode="bilinear")
    noise = torch.randint(-6, 7, (B, 3, H, W), generator=g)
    return (smooth * 255 + noise).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("vbr", [False, True])
@pytest.mark.parametrize("tau", [0, 1, 3])
def test_cpu_path_end_to_end(vbr, tau):
    imgs, net = _images(), StubNet(vbr)
    level = [1, 4, 2] if vbr else None
    files, info = codec.encode_images(net, imgs, level=level, max_error=tau, return_info=True)
    plain = codec.encode_images(net, imgs, level=level)
    assert [codec.strip_residual(f) for f in files] == plain and all(codec.is_residual_file(f) for f in files)
    for b, f in enumerate(files):
        d = codec.peek(f, n_levels=6)
        assert info[b]["bytes"] == len(f) == info[b]["base_bytes"] + info[b]["residual_bytes"] + d["header_bytes"]
        assert (info[b]["max_error"], info[b]["base_bytes"], info[b]["level"]) == (tau, len(plain[b]), level and level[b])
    out, dinfo = codec.decode_images(net, files, ref=imgs)
    err = (out.to(torch.int16) - imgs.to(torch.int16)).abs()
    assert int(err.max()) <= tau and (tau > 0 or torch.equal(out, imgs))
    base, binfo = codec.decode_images(net, plain)
    for b in range(3):
        assert dinfo[b]["max_abs_err"] == int(err[b].max()) and dinfo[b]["max_error"] == tau
        assert dinfo[b]["sq_err"] == int((err[b].to(torch.int64) ** 2).sum()) and dinfo[b]["bytes"] == len(files[b])
        assert dinfo[b]["residual_bytes"] == info[b]["residual_bytes"]
    # the output is the restatement applied to the plain decode
    f = codec._residual_front_cpu(base, imgs, tau)
    assert torch.equal(out, codec._residual_apply_cpu(base, f["sym"], tau))
    # enhance=False: the base picture; a batch is the files of single calls
    only, oinfo = codec.decode_images(net, files, enhance=False)
    assert torch.equal(only, base) and oinfo[0]["enhanced"] is False and oinfo[0]["max_error"] == tau
    assert [codec.encode_images(net, imgs[b], level=level and level[b], max_error=tau)[0] for b in range(3)] == files


def test_mixed_sizes_and_taus_in_one_decode():
    net = StubNet()
    a, b = _images(1, 70, 100), _images(1, 100, 75)
    fa = codec.encode_images(net, a, max_error=2)[0]
    fb = codec.encode_images(net, b, max_error=0)[0]
    out, info = codec.decode_images(net, [fa, fb])
    assert tuple(out.shape) == (2, 100, 100, 3) and [d["max_error"] for d in info] == [2, 0]
    assert int((out[0, :70].to(torch.int16) - a[0].to(torch.int16)).abs().max()) <= 2
    assert torch.equal(out[1, :, :75], b[0]) and not out[0, 70:].any() and not out[1, :, 75:].any()


def test_digest_mismatch_raises_and_names_the_knobs():
    imgs = _images(2)
    files = codec.encode_images(StubNet(), imgs, max_error=1)
    # a decoder whose synthesis differs: the base image is not the encoder's
    with pytest.raises(RuntimeError, match="digest.*set_synthesis_precision.*precision mode"):
        codec.decode_images(StubNet(drift=0.02), files)
    # an altered digest field: nothing faults, the comparison fails (after one more decode of the file alone)
    net = StubNet()
    bad = files[1][:16] + bytes([files[1][16] ^ 1]) + files[1][17:]
    with pytest.raises(RuntimeError, match="file 1: the digest"):
        codec.decode_images(net, [files[0], bad])
    assert net.calls == [("decompress", 2), ("decompress", 1)]
    out, _ = codec.decode_images(net, [bad], enhance=False)  # the base picture needs no digest
    assert tuple(out.shape) == (1, 70, 100, 3)


def test_a_context_without_a_table_is_refused():
    imgs = _images(1)
    net = StubNet()
    f = codec.encode_images(net, imgs, max_error=1)[0]
    s = codec.parse_container_residual(f)
    k = next(k for k in range(24) if s.m[k] != 0xFF)
    at = s.freq_off[k] - 1
    cut = f[:at] + b"\xff" + f[at + 1 + 2 * (2 * s.m[k] + 2):]
    with pytest.raises(ValueError, match=rf"contexts \[{k}\] occur in the base image but the file has no table"):
        codec.decode_images(net, [cut])


def test_python_refusals_each_by_name():
    imgs, net, vnet = _images(2), StubNet(), StubNet(vbr=True)
    mask = torch.ones(2, 70, 100, dtype=torch.uint8)
    for kw, name in (({"roi": mask, "roi_levels": (1, 3)}, "roi="), ({"max_bpp": 0.5}, "max_bpp="),
                     ({"max_bpp": 0.5, "level": "auto"}, "max_bpp="), ({"level": "auto"}, "level='auto'"),
                     ({"depth": 10}, "depth="), ({"scale": "1/2"}, "scale="), ({"coded_size": (35, 50)}, "coded_size="),
                     ({"layered": True}, "layered=")):
        with pytest.raises(ValueError, match=f"max_error= .residual coding. together with {name}"):
            codec.encode_images(vnet, imgs, max_error=1, **kw)
    for bad in (-1, 128, 1.0, True, "0"):
        with pytest.raises(ValueError, match="max_error must be an integer in"):
            codec.encode_images(net, imgs, max_error=bad)
    with pytest.raises(ValueError, match="encode_tiled: max_error= .residual coding. together with tiles"):
        codec.encode_tiled(net, imgs[0], tile=128, max_error=0)
    y = torch.zeros(1, 70, 100, dtype=torch.uint8)
    c = torch.zeros(1, 35, 50, dtype=torch.uint8)
    with pytest.raises(ValueError, match="encode_yuv: max_error= .residual coding. together with Y'CbCr frames"):
        codec.encode_yuv(net, y, c, c, codec.YuvFormat(), max_error=0)
    with pytest.raises(ValueError, match="rate_map: rate maps together with max_error= .residual coding."):
        codec.rate_map(net, imgs, max_error=0)
    with pytest.raises(ValueError, match="code_image: max_error= together with batch_stream="):
        bitstream.code_image(net, torch.zeros(1, 3, 70, 100), max_error=0, batch_stream=True)
    for kw in ({"tile": 128}, {"max_bpp": 0.5}, {"progressive": True}, {"scale": "1/2"}, {"depth": 10},
               {"roi": mask[0], "roi_levels": (1, 2)}, {"yuv": codec.YuvFormat()}):
        with pytest.raises(ValueError, match=f"code_image: max_error= together with {next(iter(kw))}="):
            bitstream.code_image(net, torch.zeros(1, 3, 70, 100), max_error=0, **kw)
    assert net.calls == [] and vnet.calls == []
    files = codec.encode_images(net, imgs, max_error=1)
    plain = codec.encode_images(net, imgs)
    net.calls.clear()
    for kw, name in (({"slices": 2}, "slices="), ({"out_size": (35, 50)}, "out_size="), ({"filter": "bicubic"}, "filter="),
                     ({"depth": 10}, "depth=")):
        with pytest.raises(ValueError, match=f"decode_images: {name} on a residual file"):
            codec.decode_images(net, files, **kw)
    with pytest.raises(ValueError, match="residual files .MLR1. and other files in one call"):
        codec.decode_images(net, [files[0], plain[1]])
    with pytest.raises(ValueError, match="decode_tiled: a residual file .MLR1."):
        codec.decode_tiled(net, files[0])
    with pytest.raises(ValueError, match="inner file has no level word, the model is variable-rate"):
        codec.decode_images(vnet, files)
    assert net.calls == [] and vnet.calls == []


def test_code_image_residual_fields():
    net = StubNet()
    img = _images(1).permute(0, 3, 1, 2).float().div(255)
    r0 = bitstream.code_image(net, img)
    assert "residual_bytes" not in r0 and "max_abs_err" not in r0
    for tau in (0, 2):
        r = bitstream.code_image(net, img, max_error=tau)
        assert r["max_abs_err"] <= tau and r["residual_bytes"] > 0 and r["bytes"] == r0["bytes"]


def _cli():
    spec = importlib.util.spec_from_file_location("mlic_codec_cli", os.path.join(ROOT, "tools", "mlic_codec.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flags_and_strip(tmp_path, capsys):
    cli = _cli()
    a = cli.parse_args(["encode", "a.ppm", "a.bit", "--synthetic", "0", "--max-error", "3"])
    assert a.max_error == 3 and not a.base_only
    assert cli.parse_args(["encode", "a.ppm", "a.bit", "--synthetic", "0", "--lossless"]).max_error == 0
    assert cli.parse_args(["encode", "a.ppm", "a.bit", "--synthetic", "0"]).max_error is None
    assert cli.parse_args(["decode", "a.bit", "a.ppm", "--synthetic", "0", "--base-only"]).base_only
    bad = [["encode", "a.ppm", "a.bit", "--synthetic", "0", "--max-error", "128"],
           ["encode", "a.ppm", "a.bit", "--synthetic", "0", "--max-error", "1", "--lossless"],
           ["encode", "a.ppm", "a.bit", "--synthetic", "0", "--lossless", "--max-bpp", "0.5"],
           ["encode", "a.ppm", "a.bit", "--synthetic", "0", "--lossless", "--tile", "128"],
           ["encode", "a.ppm", "a.bit", "--synthetic", "0", "--lossless", "--layered"],
           ["encode", "a.ppm", "a.bit", "--synthetic", "0", "--lossless", "--scale", "1/2"],
           ["encode", "a.y4m", "a.bit", "--synthetic", "0", "--lossless"],
           ["decode", "a.bit", "a.ppm", "--synthetic", "0", "--lossless"],
           ["decode", "a.bit", "a.ppm", "--synthetic", "0", "--base-only", "--slices", "2"],
           ["encode", "a.ppm", "a.bit", "--synthetic", "0", "--base-only"],
           ["strip", "a.bit"], ["strip", "a.bit", "-o", "b.bit", "--level", "2"]]
    for argv in bad:
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
    capsys.readouterr()
    data, inner, _ = _file()
    src, dst = tmp_path / "a.bit", tmp_path / "b.bit"
    src.write_bytes(data)
    cli.main(["strip", str(src), "-o", str(dst)])
    assert dst.read_bytes() == inner and "the base file" in capsys.readouterr().out
    cli.main(["info", str(src), "--model", "MLICPP_L"])
    out = capsys.readouterr().out
    assert "residual: max error 3" in out and f"base {len(inner)} B" in out and "residual 5 B" in out
    with pytest.raises(SystemExit, match="not a residual file"):
        cli.main(["strip", str(dst), "-o", str(src)])
