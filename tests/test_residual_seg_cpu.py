"""Segmented residual strings without a GPU: the host segment coder against entropy.rans_encode, the final-state
check, the "MLR2" container, the stand-alone sanitizer program, the device entries' argument refusals (before any
GPU call), the CPU end-to-end path and the Python / CLI surface.

The end-to-end tests run on a CPU stand-in model (the StubNet of tests/test_residual_cpu.py, restated here): the
MLIC++ networks themselves only run on the GPU, where tests/test_gpu_residual_seg.py codes synthetic MLICPP_S and
MLICPP_S_VBR."""
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


# --------------------------------------------------------------------------------------- the host coder
def _tables(present, m_of):
    """Tables with the given contexts present: m_of[k] symbols each side, a flat histogram with a rare escape."""
    hist = np.zeros((24, 128), np.int64)
    for k in present:
        mk = m_of.get(k, 5)
        hist[k, 63 - mk:63 + mk + 1] = np.arange(1, 2 * mk + 2)[::-1] * 7
        hist[k, 127] = 3
    return codec.residual_tables(hist)


def _symbols(N, t, seed):
    """sym int16 / ctx uint8 [1,3,H,W]-shaped data as flat arrays: contexts among the present ones, symbols inside
    the tables, at +-255, just beyond m, and with raw escape values of one, two and three nibbles."""
    rng = np.random.default_rng(seed)
    present = np.flatnonzero(t["m"] != 0xFF)
    ctx = present[rng.integers(0, len(present), N)].astype(np.uint8)
    m = t["m"][ctx].astype(np.int64)
    sym = np.rint(rng.normal(0, 2, N)).astype(np.int64).clip(-m, m)
    kind = rng.integers(0, 12, N)
    sym = np.where(kind == 0, m + 1, sym)   # just beyond m: raw 0, no nibble
    sym = np.where(kind == 1, -m - 1, sym)  # raw 1: one nibble
    sym = np.where(kind == 2, m + 9, sym)   # raw 16: two nibbles
    sym = np.where(kind == 3, 255, sym)     # three nibbles under a small m
    sym = np.where(kind == 4, -255, sym)
    return sym.astype(np.int16), ctx


def _shape(N):
    assert N % 3 == 0
    return (1, 3, 1, N // 3)


@pytest.mark.parametrize("L", [256, 257, 4096])
def test_host_segments_are_rans_encode_of_their_slices(L):
    t = _tables([0, 3, 8, 17, 23], {0: 0, 3: 63, 8: 1, 17: 5, 23: 20})  # an m = 0 context, absent contexts
    assert t["m"][0] == 0 and (t["m"] == 0xFF).sum() == 19
    cdf, length, offset = codec._coder_tables(t)
    for N in (3, 255, 2 * L - (2 * L) % 3 + 3, 3 * L, 3 * L + 30):  # N < L, short last segments, N a multiple of L
        sym, ctx = _symbols(N, t, N + L)
        s_t, c_t = torch.from_numpy(sym).view(_shape(N)), torch.from_numpy(ctx).view(_shape(N))
        (data, segb), = codec.residual_encode_segments(s_t, c_t, t, L)
        n_seg = -(-N // L)
        assert segb.dtype == np.uint32 and segb.shape == (n_seg,) and int(segb.sum()) == len(data)
        off = 0
        for k in range(n_seg):
            sl = slice(k * L, min((k + 1) * L, N))
            want = entropy.rans_encode(sym[sl].astype(np.int32), ctx[sl].astype(np.int32), cdf, length, offset)
            assert data[off:off + segb[k]] == want, (N, k)
            assert segb[k] % 4 == 0 and 8 <= segb[k] <= 4 * (sl.stop - sl.start + 2)
            off += int(segb[k])
        back = codec.residual_decode_segments([data], [segb], c_t, t, L)
        assert back.dtype == torch.int16 and torch.equal(back, s_t)
        assert codec.residual_encode_segments(s_t, c_t, t, L, "host")[0][0] == data  # "device" on CPU is the host entry
    # the escape path took every nibble count
    m = t["m"][ctx].astype(np.int64)
    v = sym.astype(np.int64) + m
    raw = np.where(v < 0, -2 * v - 1, 2 * (v - (2 * m + 1)))[(v < 0) | (v >= 2 * m + 1)]
    assert {(int(r).bit_length() + 3) // 4 for r in raw} == {0, 1, 2, 3} and raw.max() <= 510


def test_final_state_check_names_the_segment():
    L, N = 256, 256 * 12
    t = _tables([1, 2], {1: 4, 2: 9})
    sym, ctx = _symbols(N, t, 5)
    sym[:] = np.clip(sym, -3, 3)  # equal statistics, so that two segments have one length
    s_t, c_t = torch.from_numpy(sym).view(_shape(N)), torch.from_numpy(ctx).view(_shape(N))
    (data, segb), = codec.residual_encode_segments(s_t, c_t, t, L)
    off = np.concatenate([[0], np.cumsum(segb)]).astype(int)
    for seg in range(12):
        for at in (off[seg], off[seg] + 4, off[seg + 1] - 1):  # the flush, and the last word read
            bad = bytearray(data)
            bad[at] ^= 0x04
            with pytest.raises(codec.ResidualSegmentError, match=f"image 0, segment {seg}: ") as e:
                codec.residual_decode_segments([bytes(bad)], [segb], c_t, t, L)
            assert e.value.segment == seg and e.value.image == 0
    pairs = [(a, b) for a in range(12) for b in range(a + 1, 12) if segb[a] == segb[b]]
    assert pairs, segb
    a, b = pairs[0]
    sa, sb = data[off[a]:off[a + 1]], data[off[b]:off[b + 1]]
    assert sa != sb
    swapped = data[:off[a]] + sb + data[off[a + 1]:off[b]] + sa + data[off[b + 1]:]
    with pytest.raises(codec.ResidualSegmentError, match=f"image 0, segment {a}: "):
        codec.residual_decode_segments([swapped], [segb], c_t, t, L)
    # what the tables cannot code is refused on the way in, by segment
    far = sym.copy()
    far[700] = 256
    with pytest.raises(codec.ResidualSegmentError, match=r"segment 2: a symbol outside \[-255, 255\]"):
        codec.residual_encode_segments(torch.from_numpy(far).view(_shape(N)), c_t, t, L)
    other = ctx.copy()
    other[300] = 5
    with pytest.raises(codec.ResidualSegmentError, match="segment 1: a context without a table"):
        codec.residual_encode_segments(s_t, torch.from_numpy(other).view(_shape(N)), t, L)
    with pytest.raises(codec.ResidualSegmentError, match="segment 1: a context without a table"):
        codec.residual_decode_segments([data], [segb], torch.from_numpy(other).view(_shape(N)), t, L)


# ------------------------------------------------------------------------------------------- container
def _hist():
    h = np.zeros((24, 128), np.int64)
    h[0, 63] = 1000
    h[1, 60:67] = (3, 40, 300, 900, 280, 50, 2)
    h[1, 127] = 4
    h[9, 0:127] = 5
    h[9, 127] = 90
    return h


def _file(level=None, tau=3, H=40, W=50, L=256, seed=1):
    t = codec.residual_tables(_hist())
    rng = np.random.default_rng(seed)
    n_seg = -(-3 * H * W // L)
    segb = (8 + 4 * rng.integers(0, 20, n_seg)).astype(np.uint32)
    segs = rng.integers(0, 256, int(segb.sum()), dtype=np.uint8).tobytes()
    inner = codec.write_container(H, W, ((H + 63) // 64, (W + 63) // 64), b"yyyyyyy", b"zzz", level)
    data = codec.write_container_residual_seg(H, W, inner, segs, segb, L, tau, 0x0123456789ABCDEF, t["m"], t["freq"],
                                              vbr=level is not None)
    return data, inner, t, segb, segs


def _table_bytes(t):
    return sum(1 + (0 if m == 0xFF else 2 * (2 * int(m) + 2)) for m in t["m"])


@pytest.mark.parametrize("level", [None, 3])
def test_container_round_trip(level):
    for tau, L in ((0, 256), (3, 257), (127, 65536)):
        data, inner, t, segb, segs = _file(level, tau, L=L)
        n_seg = len(segb)
        assert data[:8] == b"MLR2" + bytes([0, int(level is not None), tau, 24])
        assert data[8:24] == struct.pack(">IIQ", 40, 50, 0x0123456789ABCDEF)
        head = 24 + _table_bytes(t)
        assert data[head:head + 12] == struct.pack(">III", L, n_seg, len(inner))
        assert len(data) == head + 12 + len(inner) + 4 + 4 * n_seg + len(segs)
        assert codec.is_residual_file(data) and codec.is_residual_seg_file(data) and not codec.is_scaled_file(data) \
            and not codec.is_layered_file(data) and not codec.is_tiled_file(data)
        s = codec.parse_container_residual_seg(data, 6)
        assert (s.H, s.W, s.tau, bool(s.vbr), s.digest) == (40, 50, tau, level is not None, 0x0123456789ABCDEF)
        assert (s.seg_len, s.n_seg, s.res_len, s.data_len) == (L, n_seg, 4 * n_seg + len(segs), len(segs))
        assert data[s.inner_off:s.inner_off + s.inner_len] == inner == codec.strip_residual(data)
        assert data[s.res_off - 4:s.res_off] == struct.pack(">I", s.res_len) and s.index_off == s.res_off
        assert (np.frombuffer(data, ">u4", n_seg, s.index_off) == segb).all()
        assert data[s.data_off:s.data_off + s.data_len] == segs and s.data_off + s.data_len == len(data)
        t2 = codec._file_tables(data, s)
        assert all((t2[k] == t[k]).all() for k in ("m", "freq", "cdf", "length", "offset"))
        d = codec.peek(data, n_levels=6)
        assert d["residual"] and d["max_error"] == tau and d["level"] == level and d["shape"] == (1, 1)
        assert (d["residual_segment"], d["segments"]) == (L, n_seg)
        assert (d["base_bytes"], d["residual_bytes"]) == (len(inner), 4 * n_seg + len(segs))
        assert d["header_bytes"] + d["base_bytes"] + d["residual_bytes"] == d["bytes"] == len(data)


def test_truncation_sweep():
    for level in (None, 2):
        data, inner, t, segb, segs = _file(level)
        head = 24 + _table_bytes(t)
        for n in range(len(data)):
            with pytest.raises(_lib.MlicError, match="truncated|runs past the end|bad magic"):
                codec.parse_container_residual_seg(data[:n], 6)
        for n, msg in ((23, "truncated header"), (24, "truncated before a table's m"), (26, "truncated inside a table"),
                       (head - 1, "truncated before a table's m"),
                       (head + 7, "truncated before seg_len, n_seg"), (head + 11, "truncated before the inner length"),
                       (head + 12, "the inner length runs past the end"),
                       (head + 12 + len(inner) + 3, "truncated before the residual length"),
                       (head + 12 + len(inner) + 4 + 2, "the residual length runs past the end"),
                       (len(data) - 1, "the residual length runs past the end")):
            with pytest.raises(_lib.MlicError, match=msg):
                codec.parse_container_residual_seg(data[:n], 6)
        codec.parse_container_residual_seg(data, 6)


def _put(data, at, raw):
    return data[:at] + raw + data[at + len(raw):]


def test_parser_refusals_each_by_its_message():
    data, inner, t, segb, segs = _file(3)
    head = 24 + _table_bytes(t)
    first = 24
    assert t["m"][0] == 0
    inner_at = head + 12
    res_at = inner_at + len(inner)
    idx = res_at + 4
    u32 = lambda v: struct.pack(">I", v)  # noqa: E731
    cases = [(_put(data, 0, b"MLR1"), "bad magic"), (_put(data, 4, b"\x01"), "unknown version"),
             (_put(data, 5, b"\x03"), "unknown flags"), (_put(data, 6, b"\x80"), "tau above 127"),
             (_put(data, 7, b"\x17"), "n_ctx is not 24"), (_put(data, 8, u32(0)), "H or W is zero"),
             (_put(data, 12, u32(0)), "H or W is zero"), (_put(data, first, b"\x40"), "an m outside 0..63"),
             (_put(data, first + 1, b"\x00\x00"), "a zero frequency"),
             (_put(data, first + 1, b"\x00\x01"), "do not sum to 65536"),
             (_put(data, head, u32(255)), "seg_len outside 256..65536"),
             (_put(data, head, u32(65537)), "seg_len outside 256..65536"),
             (_put(data, head, u32(512)), "n_seg is not ceil"),
             (_put(data, head + 4, u32(len(segb) - 1)), "n_seg is not ceil"),
             (_put(data, head + 8, u32(len(data))), "the inner length runs past the end"),
             (_put(data, head + 8, u32(0)), "an empty inner file"),
             (_put(data, res_at, u32(4 * len(segb) + len(segs) + 1)), "the residual length runs past the end"),
             (_put(data, res_at, u32(4 * len(segb) - 4)), "the residual length is below its index"),
             (_put(data, idx, u32(int(segb[0]) + 1)), "a segment length that is not a multiple of 4"),
             (_put(data, idx + 4, u32(4)), "a segment length below 8"),
             (_put(data, idx + 8, u32(4 * (256 + 4) + 4)), "a segment length above the capacity bound"),
             (_put(data, idx + 4 * (len(segb) - 1), u32(4 * (3 * 40 * 50 % 256 + 4) + 4)), "above the capacity bound"),
             (_put(data, idx, u32(int(segb[0]) + 4)), "is not 4 n_seg \\+ the segment lengths"),
             (_put(data, 5, b"\x00"), "container_parse"),
             (_put(data, inner_at, u32(0)), "container_parse: H or W is zero"),
             (_put(data, inner_at + 8, u32(6)), "level is not below n_levels"),
             (_put(data, inner_at + 4, u32(49)), "the inner file's H x W is not the outer one")]
    for bad, msg in cases:
        with pytest.raises(_lib.MlicError, match=msg):
            codec.parse_container_residual_seg(bad, 6)
    with pytest.raises(_lib.MlicError, match="bytes left over after the segments"):
        codec.parse_container_residual_seg(data + b"\x00", 6)
    with pytest.raises(_lib.MlicError, match="image exceeds max_pixels"):
        codec.parse_container_residual_seg(data, 6, max_pixels=40 * 50 - 1)
    with pytest.raises(_lib.MlicError, match="null info"):
        _lib.call("mlic_container_parse_residual_seg", data, len(data), 6, 1 << 28, None)
    # the writer's refusals
    ok = {"H": 40, "W": 50, "inner": inner, "segs": segs, "seg_bytes": segb, "segment": 256, "tau": 3, "digest": 1,
          "m": t["m"], "freq": t["freq"]}
    short = segb.copy()
    short[0] = 4
    odd = segb.copy()
    odd[1] += 2
    big = segb.copy()
    big[2] = 4 * 261
    for kw, msg in (({"H": 0}, "H or W is zero"), ({"tau": 128}, "tau above 127"), ({"inner": b""}, "an empty inner file"),
                    ({"segment": 255}, "seg_len outside 256..65536"), ({"segment": 512}, "n_seg is not ceil"),
                    ({"seg_bytes": short}, "a segment length below 8"), ({"seg_bytes": odd}, "not a multiple of 4"),
                    ({"seg_bytes": big}, "above the capacity bound"), ({"segs": segs + b"\0\0\0\0"}, "do not sum to the data length")):
        with pytest.raises(_lib.MlicError, match=msg):
            codec.write_container_residual_seg(**{**ok, **kw})


def test_parsers_tell_the_kinds_apart():
    for level in (None, 3):
        data, inner, t, segb, segs = _file(level)
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
        with pytest.raises(_lib.MlicError, match="bad magic .not a residual file"):
            codec.parse_container_residual(data, 6)
        mlr1 = codec.write_container_residual(40, 50, inner, b"abcd", 3, 1, t["m"], t["freq"], vbr=level is not None)
        for other in (mlr1, inner):
            with pytest.raises(_lib.MlicError, match="bad magic .not a segmented residual file"):
                codec.parse_container_residual_seg(other, 6)


def test_container_residual_seg_check_program_under_sanitizers(tmp_path):
    """tools/container_residual_seg_check.cpp with container.cpp and rans.cpp, AddressSanitizer + UBSan, as a
    stand-alone program (no sanitizer runtime comes near Python): the parser on mutated files and the capacity bound
    over adversarial segments.  Skipped where the compiler cannot link the sanitizer runtimes."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed for the container's sanitizer check"
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run([cxx] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if p.returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed: " + p.stderr[-200:])
    exe = str(tmp_path / "container_residual_seg_check")
    csrc = os.path.join(ROOT, "mlic_amd", "csrc")
    cmd = [cxx, "-std=c++17", "-O1", "-g"] + san + [
           "-I" + csrc, os.path.join(ROOT, "tools", "container_residual_seg_check.cpp"),
           os.path.join(csrc, "container.cpp"), os.path.join(csrc, "rans.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-300:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("container_residual_seg_check ok"), \
        r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------ the entries' refusals
def test_device_entries_refuse_bad_arguments_before_any_gpu_call():
    """Every argument is checked before any HIP call: the device pointers (small fake addresses) are never
    dereferenced, and no GPU is needed."""
    t = codec.residual_tables(_hist())
    m = np.ascontiguousarray(t["m"])
    freq = np.ascontiguousarray(t["freq"])
    H, W, L = 16, 24, 256
    n_seg = -(-3 * H * W // L)  # 5
    lens = (C.c_uint64 * 1)()
    enc = dict(sym=64, ctx=64, B=1, H=H, W=W, m=m.ctypes.data, freq=freq.ctypes.data, L=L, n_seg=n_seg, out=64, cap=4096,
               segb=64, lens=lens, scratch=256, scratch_bytes=1 << 20, status=None)
    order = ("sym", "ctx", "B", "H", "W", "m", "freq", "L", "n_seg", "out", "cap", "segb", "lens", "scratch",
             "scratch_bytes", "status")
    bad_m = m.copy()
    bad_m[0] = 64
    zero_f = freq.copy()
    zero_f[0, 0] = 0
    off_f = freq.copy()
    off_f[1, 0] += 1
    for kw, msg in (({"sym": None}, "null sym"), ({"ctx": None}, "null ctx"), ({"out": None}, "null out"),
                    ({"segb": None}, "null seg_bytes"), ({"lens": None}, "null len"), ({"scratch": None}, "null scratch"),
                    ({"m": None}, "null m"), ({"freq": None}, "null frequencies"), ({"B": 0}, "B must be positive"),
                    ({"H": 0}, "H and W must be positive"), ({"L": 255}, "segment length 255 is outside 256..65536"),
                    ({"L": 65537}, "is outside 256..65536"), ({"n_seg": n_seg + 1}, "n_seg 6 is not ceil"),
                    ({"H": 1 << 14, "W": 1 << 14, "n_seg": 1}, "more than 2\\^29 samples"),
                    ({"m": bad_m.ctypes.data}, "an m outside 0..63"), ({"freq": zero_f.ctypes.data}, "a zero frequency"),
                    ({"freq": off_f.ctypes.data}, "do not sum to 65536"), ({"cap": 4098}, "multiple of 4"),
                    ({"cap": 8 * n_seg - 4}, "capacity is too small"), ({"scratch_bytes": 64}, "scratch too small"),
                    ({"sym": 65}, "sym must be 2-byte"), ({"out": 66}, "out and seg_bytes 4-byte"),
                    ({"scratch": 264}, "scratch 16-byte aligned")):
        a = {**enc, **kw}
        with pytest.raises(_lib.MlicError, match=msg):
            _lib.call("mlic_residual_encode_segments", None, *[a[k] for k in order])
    segb = np.array([40, 8, 1028, 12, 16], np.uint32)
    dlen = (C.c_uint64 * 1)(int(segb.sum()))
    dec = dict(data=64, stride=2048, dlen=dlen, segb=segb.ctypes.data, ctx=64, B=1, H=H, W=W, m=m.ctypes.data,
               freq=freq.ctypes.data, L=L, n_seg=n_seg, sym=64, scratch=256, scratch_bytes=1 << 20, status=None)
    order = ("data", "stride", "dlen", "segb", "ctx", "B", "H", "W", "m", "freq", "L", "n_seg", "sym", "scratch",
             "scratch_bytes", "status")
    arr = lambda *v: np.array(v, np.uint32)  # noqa: E731
    keep = []
    for kw, msg in (({"data": None}, "null data"), ({"ctx": None}, "null ctx"), ({"sym": None}, "null sym"),
                    ({"scratch": None}, "null scratch"), ({"segb": None}, "null segment lengths"),
                    ({"dlen": None}, "null data lengths"), ({"L": 100}, "is outside 256..65536"),
                    ({"n_seg": 4}, "n_seg 4 is not ceil"), ({"stride": 2050}, "stride must be a multiple of 4"),
                    ({"segb": arr(42, 8, 1028, 12, 16)}, "segment 0: a length that is not a multiple of 4"),
                    ({"segb": arr(40, 4, 1028, 12, 16)}, "segment 1: a length below 8"),
                    ({"segb": arr(40, 8, 1044, 12, 16)}, "segment 2: a length above the capacity bound"),
                    ({"segb": arr(40, 8, 1028, 12, 4 * (3 * H * W % L + 4) + 4)}, "segment 4: a length above the capacity"),
                    ({"segb": arr(40, 8, 1028, 12, 20)}, "lengths sum to 1108, the data length is 1104"),
                    ({"stride": 1100}, "data length exceeds the stride"), ({"scratch_bytes": 64}, "scratch too small"),
                    ({"data": 66}, "data 4-byte"), ({"sym": 65}, "sym must be 2-byte")):
        a = {**dec, **kw}
        if isinstance(a["segb"], np.ndarray):
            keep.append(a["segb"])
            a["segb"] = a["segb"].ctypes.data
        with pytest.raises(_lib.MlicError, match=msg):
            _lib.call("mlic_residual_decode_segments", None, *[a[k] for k in order])
    n = C.c_size_t()
    _lib.call("mlic_residual_segments_scratch_bytes", 2, 10, C.byref(n))
    assert n.value >= 2 * 48 * 1024 and n.value % 16 == 0
    with pytest.raises(_lib.MlicError, match="n_seg"):
        _lib.call("mlic_residual_segments_scratch_bytes", 1, 0, C.byref(n))


# ---------------------------------------------------------------------------------------------- policy
class StubNet:
    """A 'model' on the CPU (tests/test_residual_cpu.py's): compress keeps the 8 x 8 block means of each image as
    the y string, decompress paints them back, so the base image is a real, lossy, repeatable picture."""
    device = torch.device("cpu")
    slice_num = 4

    def __init__(self, vbr=False):
        if vbr:
            self.levels = 6
        self.calls = []

    def compress(self, x, s=None, layered=False, gain_map=None):
        B, _, Hp, Wp = x.shape
        assert (s is None) == (not hasattr(self, "levels"))
        self.calls.append(("compress", B))
        m = torch.nn.functional.avg_pool2d(x, 8)
        ys = [bytes((m[b] * 255).round().to(torch.uint8).reshape(-1).tolist()) for b in range(B)]
        return {"strings": [ys, [bytes([0 if s is None else s[b]]) for b in range(B)]], "shape": (Hp // 64, Wp // 64)}

    def decompress(self, strings, shape, s=None, **kw):
        B = len(strings[0])
        self.calls.append(("decompress", B))
        h, w = 8 * shape[0], 8 * shape[1]
        m = torch.stack([torch.tensor(list(y), dtype=torch.float32).view(3, h, w) for y in strings[0]]) / 255
        return {"x_hat": torch.nn.functional.interpolate(m, scale_factor=8, mode="nearest").contiguous()}


def _images(B=3, H=64, W=64, seed=5):
    g = torch.Generator().manual_seed(seed)
    smooth = torch.nn.functional.interpolate(torch.rand(B, 3, 5, 6, generator=g), size=(H, W), mode="bilinear")
    noise = torch.randint(-6, 7, (B, 3, H, W), generator=g)
    return (smooth * 255 + noise).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("vbr", [False, True])
@pytest.mark.parametrize("tau", [0, 1, 3])
def test_cpu_path_end_to_end(vbr, tau):
    imgs, net = _images(), StubNet(vbr)
    level = [1, 4, 2] if vbr else None
    files, info = codec.encode_images(net, imgs, level=level, max_error=tau, residual_segment=256, return_info=True)
    host = codec.encode_images(net, imgs, level=level, max_error=tau, residual_segment=256, residual_coder="host")
    plain = codec.encode_images(net, imgs, level=level)
    assert files == host and all(f[:4] == b"MLR2" for f in files)
    assert [codec.strip_residual(f) for f in files] == plain
    n_seg = -(-3 * 64 * 64 // 256)
    for b, f in enumerate(files):
        d = codec.peek(f, n_levels=6)
        assert info[b]["bytes"] == len(f) == info[b]["base_bytes"] + info[b]["residual_bytes"] + d["header_bytes"]
        assert (info[b]["max_error"], info[b]["residual_segment"], info[b]["segments"]) == (tau, 256, n_seg)
        assert (d["residual_segment"], d["segments"], d["base_bytes"]) == (256, n_seg, len(plain[b]))
    base, _ = codec.decode_images(net, plain)
    f0 = codec._residual_front_cpu(base, imgs, tau)
    for coder in ("device", "host"):  # "device" on a CPU model falls to the host entry
        out, dinfo = codec.decode_images(net, files, ref=imgs, residual_coder=coder)
        err = (out.to(torch.int16) - imgs.to(torch.int16)).abs()
        assert int(err.max()) <= tau and (tau > 0 or torch.equal(out, imgs))
        assert torch.equal(out, codec._residual_apply_cpu(base, f0["sym"], tau))
        for b in range(3):
            assert dinfo[b]["max_abs_err"] == int(err[b].max()) and dinfo[b]["max_error"] == tau
            assert dinfo[b]["segments"] == n_seg and dinfo[b]["residual_bytes"] == info[b]["residual_bytes"]
    only, oinfo = codec.decode_images(net, files, enhance=False)
    assert torch.equal(only, base) and oinfo[0]["enhanced"] is False
    single = [codec.encode_images(net, imgs[b], level=level and level[b], max_error=tau, residual_segment=256)[0]
              for b in range(3)]
    assert single == files
    # the segments are the serial file's symbols: an MLR1 and an MLR2 file of one image decode to the same pixels
    serial = codec.encode_images(net, imgs, level=level, max_error=tau)
    both, binfo = codec.decode_images(net, [serial[2], files[2]])
    assert torch.equal(both[0], both[1]) and "segments" not in binfo[0] and binfo[1]["segments"] == n_seg


class BatchDriftNet(StubNet):
    """StubNet whose decompress of two or more images returns image 1 perturbed, while a single image comes back
    exact: the batch's base then differs from the file's own, as after the range guard's fp32 re-run of a lane."""

    def decompress(self, strings, shape, s=None, **kw):
        out = super().decompress(strings, shape, s=s, **kw)
        if len(strings[0]) >= 2:
            x = out["x_hat"][1]
            out["x_hat"][1] = torch.where(x > 0.5, x - 0.03, x + 0.03)  # about 8 of 255: no sample stays as it was
        return out


def _same(a, b):
    if torch.is_tensor(a):
        return a.dtype == b.dtype and torch.equal(a.view(torch.int16) if a.dtype == torch.uint16 else a,
                                                  b.view(torch.int16) if b.dtype == torch.uint16 else b)
    return len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))


def test_a_batch_whose_base_drifts_is_repaired_by_the_decode_alone():
    """The successful branch of the decoder's retry, for the three kinds of picture through the one driver: the
    digest of the batch's base differs from the file's, the file decoded alone has the file's digest, that base is
    pasted in, and the call returns exactly what decoding each file alone returns."""
    imgs, clean, drift = _images(2), StubNet(), BatchDriftNet()
    deep = (imgs.to(torch.int32) * 4 + 1).to(torch.uint16)  # 10-bit samples
    fmt = codec.YuvFormat((2, 2), "bt709", False, "left", 8)
    planes = codec.egress_yuv(imgs.permute(0, 3, 1, 2).float() / 255, 64, 64, fmt)
    cases = {
        b"MLR2": (codec.encode_images(clean, imgs, max_error=1, residual_segment=256), imgs,
                  lambda net, files, **kw: codec.decode_images(net, files, **kw)),
        b"MLR3": (codec.encode_residual16(clean, deep, 10, max_error=1, residual_segment=256, shift=1), deep,
                  lambda net, files, **kw: codec.decode_images(net, files, **kw)),
        b"MLR4": (codec.encode_residual_yuv(clean, *planes, fmt, max_error=1, residual_segment=256), planes,
                  lambda net, files, **kw: codec.decode_yuv(net, files, fmt, **kw))}
    for magic, (files, orig, decode) in cases.items():
        assert len(files) == 2 and all(f[:4] == magic for f in files)
        plain = [codec.strip_residual(f) for f in files]
        own = [decode(clean, [f])[0] for f in plain]  # each file's own base
        batch = decode(drift, plain)[0]
        pick = (lambda t, b: t[b:b + 1]) if torch.is_tensor(batch) else (lambda t, b: tuple(p[b:b + 1] for p in t))
        assert _same(pick(batch, 0), own[0]) and not _same(pick(batch, 1), own[1])  # the drift is real
        alone = [decode(clean, [f], ref=pick(orig, b)) for b, f in enumerate(files)]
        drift.calls.clear()
        out, info = decode(drift, files, ref=orig)
        # the batch, then file 1 alone (file 0's digest agreed)
        assert [c for c in drift.calls if c[0] == "decompress"] == [("decompress", 2), ("decompress", 1)]
        for b in range(2):
            assert _same(pick(out, b), alone[b][0])
            assert info[b] == alone[b][1][0] and info[b]["max_abs_err"] <= 1
        assert _same(decode(drift, files)[0], out)


def test_without_a_segment_the_file_is_the_serial_one_byte_for_byte():
    """encode_images(max_error=) without residual_segment= still writes the "MLR1" file: here it is rebuilt by hand
    from the base picture, residual_front's symbols, entropy.rans_encode and write_container_residual."""
    imgs, net = _images(2, 70, 100), StubNet()
    for tau in (0, 2):
        files = codec.encode_images(net, imgs, max_error=tau)
        plain = codec.encode_images(net, imgs)
        base, _ = codec.decode_images(net, plain)
        f = codec._residual_front_cpu(base, imgs, tau)
        for b in range(2):
            t = codec.residual_tables(f["hist"][b])
            res = entropy.rans_encode(f["sym"][b].reshape(-1).numpy().astype(np.int32),
                                      f["ctx"][b].reshape(-1).numpy().astype(np.int32), *codec._coder_tables(t))
            want = codec.write_container_residual(70, 100, plain[b], res, tau, int(f["digest"][b]), t["m"], t["freq"])
            assert files[b] == want and files[b][:4] == b"MLR1"


def test_mixed_kinds_sizes_and_taus_in_one_decode():
    net = StubNet()
    a, b = _images(1, 70, 100), _images(1, 100, 75, seed=6)
    fa = codec.encode_images(net, a, max_error=2, residual_segment=300)[0]
    fb = codec.encode_images(net, b, max_error=0)[0]
    fc = codec.encode_images(net, a, max_error=0, residual_segment=4096)[0]
    out, info = codec.decode_images(net, [fa, fb, fc])
    assert tuple(out.shape) == (3, 100, 100, 3) and [d["max_error"] for d in info] == [2, 0, 0]
    assert [d.get("residual_segment") for d in info] == [300, None, 4096]
    assert int((out[0, :70].to(torch.int16) - a[0].to(torch.int16)).abs().max()) <= 2
    assert torch.equal(out[1, :, :75], b[0]) and torch.equal(out[2, :70], a[0]) and not out[0, 70:].any()


def test_a_corrupt_segment_names_the_file_and_the_segment():
    net = StubNet()
    imgs = _images(2)
    files = codec.encode_images(net, imgs, max_error=1, residual_segment=256)
    s = codec.parse_container_residual_seg(files[1])
    lens = np.frombuffer(files[1], ">u4", s.n_seg, s.index_off)
    at = s.data_off + int(lens[:7].sum()) + 5
    bad = files[1][:at] + bytes([files[1][at] ^ 0x10]) + files[1][at + 1:]
    for coder in ("device", "host"):
        with pytest.raises(ValueError, match="decode_images: file 1: segment 7 of the residual string is corrupt"):
            codec.decode_images(net, [files[0], bad], residual_coder=coder)
    k = next(k for k in range(24) if s.m[k] != 0xFF)
    cut_at = s.freq_off[k] - 1
    cut = files[1][:cut_at] + b"\xff" + files[1][cut_at + 1 + 2 * (2 * s.m[k] + 2):]
    with pytest.raises(ValueError, match=rf"contexts \[{k}\] occur in the base image but the file has no table"):
        codec.decode_images(net, [cut])


def test_python_refusals_each_by_name():
    imgs, net = _images(2), StubNet()
    with pytest.raises(ValueError, match="encode_images: residual_segment= needs max_error="):
        codec.encode_images(net, imgs, residual_segment=4096)
    for bad in (255, 65537, 1024.0, True, "4096"):
        with pytest.raises(ValueError, match="residual_segment must be an integer in \\[256, 65536\\]"):
            codec.encode_images(net, imgs, max_error=1, residual_segment=bad)
    for fn in (lambda c: codec.encode_images(net, imgs, max_error=1, residual_segment=256, residual_coder=c),
               lambda c: codec.decode_images(net, [b"MLR2"], residual_coder=c)):
        with pytest.raises(ValueError, match="residual_coder must be 'device' or 'host'"):
            fn("gpu")
    mask = torch.ones(2, 64, 64, dtype=torch.uint8)
    vnet = StubNet(vbr=True)
    for kw, name in (({"roi": mask, "roi_levels": (1, 3)}, "roi="), ({"max_bpp": 0.5}, "max_bpp="),
                     ({"depth": 10}, "depth="), ({"scale": "1/2"}, "scale="), ({"layered": True}, "layered=")):
        with pytest.raises(ValueError, match=f"max_error= .residual coding. together with {name}"):
            codec.encode_images(vnet, imgs, max_error=1, residual_segment=256, **kw)
    with pytest.raises(ValueError, match="code_image: residual_segment= needs max_error="):
        bitstream.code_image(net, torch.zeros(1, 3, 64, 64), residual_segment=256)
    assert net.calls == [] and vnet.calls == []
    files = codec.encode_images(net, imgs, max_error=1, residual_segment=256)
    plain = codec.encode_images(net, imgs)
    net.calls.clear()
    for kw, name in (({"slices": 2}, "slices="), ({"out_size": (35, 50)}, "out_size="), ({"filter": "bicubic"}, "filter="),
                     ({"depth": 10}, "depth=")):
        with pytest.raises(ValueError, match=f"decode_images: {name} on a residual file .MLR2."):
            codec.decode_images(net, files, **kw)
    with pytest.raises(ValueError, match="residual files .MLR1. and other files in one call"):
        codec.decode_images(net, [files[0], plain[1]])
    with pytest.raises(ValueError, match="decode_tiled: a residual file"):
        codec.decode_tiled(net, files[0])
    with pytest.raises(ValueError, match="inner file has no level word, the model is variable-rate"):
        codec.decode_images(vnet, files)
    assert net.calls == [] and vnet.calls == []
    sym = torch.zeros(1, 3, 4, 5, dtype=torch.int16)
    ctx = torch.zeros(1, 3, 4, 5, dtype=torch.uint8)
    t = codec.residual_tables(_hist())
    with pytest.raises(ValueError, match="sym must be an int16 tensor"):
        codec.residual_encode_segments(sym.int(), ctx, t, 256)
    with pytest.raises(ValueError, match="ctx must be a uint8 tensor"):
        codec.residual_encode_segments(sym, sym, t, 256)
    with pytest.raises(ValueError, match="1 images but 2 table sets"):
        codec.residual_encode_segments(sym, ctx, [t, t], 256)
    with pytest.raises(ValueError, match="1 segment lengths per image expected"):
        codec.residual_decode_segments([b"12345678"], [np.array([8, 8])], ctx, t, 256)


def test_code_image_passes_the_segment_through():
    net = StubNet()
    img = _images(1).permute(0, 3, 1, 2).float().div(255)
    r1 = bitstream.code_image(net, img, max_error=2)
    r2 = bitstream.code_image(net, img, max_error=2, residual_segment=1024)
    assert r1["residual_kind"] == "MLR1" and "segments" not in r1
    assert r2["residual_kind"] == "MLR2" and (r2["residual_segment"], r2["segments"]) == (1024, 12)
    assert r2["max_abs_err"] <= 2 and r2["bytes"] == r1["bytes"]
    assert 0 < r2["residual_bytes"] - r1["residual_bytes"] < 12 * 12  # below the flush and the index entry per segment


def _cli():
    spec = importlib.util.spec_from_file_location("mlic_codec_cli", os.path.join(ROOT, "tools", "mlic_codec.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flags(tmp_path, capsys):
    cli = _cli()
    enc = ["encode", "a.ppm", "a.bit", "--synthetic", "0"]
    a = cli.parse_args(enc + ["--max-error", "3", "--residual-segment", "1024"])
    assert (a.max_error, a.residual_segment, a.residual_coder) == (3, 1024, None)
    a = cli.parse_args(enc + ["--lossless", "--residual-segment", "256", "--residual-coder", "host"])
    assert (a.max_error, a.residual_segment, a.residual_coder) == (0, 256, "host")
    assert cli.parse_args(enc + ["--lossless"]).residual_segment is None
    assert cli.parse_args(["decode", "a.bit", "a.ppm", "--synthetic", "0", "--residual-coder", "host"]).residual_coder == "host"
    for argv in (enc + ["--residual-segment", "1024"], enc + ["--lossless", "--residual-segment", "255"],
                 enc + ["--lossless", "--residual-segment", "65537"], enc + ["--lossless", "--residual-coder", "host"],
                 enc + ["--lossless", "--residual-segment", "256", "--residual-coder", "gpu"],
                 ["decode", "a.bit", "a.ppm", "--synthetic", "0", "--residual-segment", "256"],
                 ["info", "a.bit", "--synthetic", "0", "--residual-coder", "host"]):
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
    capsys.readouterr()
    data, inner, t, segb, segs = _file()
    src, dst = tmp_path / "a.bit", tmp_path / "b.bit"
    src.write_bytes(data)
    cli.main(["strip", str(src), "-o", str(dst)])
    assert dst.read_bytes() == inner
    capsys.readouterr()
    cli.main(["info", str(src), "--model", "MLICPP_L"])
    out = capsys.readouterr().out
    assert "residual: max error 3" in out and f"in {len(segb)} segments of 256" in out and f"base {len(inner)} B" in out
