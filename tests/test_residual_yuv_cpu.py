"""Residual coding of Y'CbCr frames without a GPU: the integer definitions (tests/residual_yuv_oracle.py against
codec.py's restatement, the existing RGB definitions and the library's shift rule), the host segment coders for a
given N, the "MLR4" container, the stand-alone sanitizer program, the entries' refusals before any GPU call, the codec
end to end on a CPU stand-in model (the StubNet of tests/test_residual_cpu.py, restated here) and the command line's
flags.  tests/test_gpu_residual_yuv.py runs the kernels and synthetic MLICPP_S."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import residual16_oracle as orc16
import residual_yuv_oracle as orc
from mlic_amd import _lib, codec
from mlic_amd.codec import YuvFormat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBS = [(2, 2), (2, 1), (1, 1)]


def _fmt(sub, d, msb=False):
    return YuvFormat(sub, "bt709", False, "left", d, msb)


def _frame(H, W, sub, d, msb, seed, B=1, near=False):
    """(base, x): two lists of three word planes [B,h,w] over the full word range (near: x a noisy copy of base)."""
    rng = np.random.default_rng(seed)
    hc, wc = orc.chroma_size(H, W, sub)
    dt, top = (np.uint8, 255) if d == 8 else (np.uint16, 65535)
    shapes = [(B, H, W), (B, hc, wc), (B, hc, wc)]
    base = [rng.integers(0, top + 1, s).astype(dt) for s in shapes]
    if not near:
        return base, [rng.integers(0, top + 1, s).astype(dt) for s in shapes]
    maxv = (1 << d) - 1
    x = [orc.words(np.clip(orc.samples(v, d, msb) + rng.integers(-9, 10, v.shape), 0, maxv), d, msb) for v in base]
    return base, x


def _smp(planes, d, msb, b=0):
    return [orc.samples(v[b], d, msb) for v in planes]


# ------------------------------------------------------------------------------------------ the integers
@pytest.mark.parametrize("d,msb", [(8, False), (10, False), (10, True), (16, False)])
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (5, 70), (19, 131)])
def test_codec_restatement_is_the_oracle(H, W, sub, d, msb):
    fmt = _fmt(sub, d, msb)
    base, x = _frame(H, W, sub, d, msb, 1000 * H + W + d, B=2)
    for tau in (0, 2, 127):
        for s in ([0] if d == 8 else [0, 2, d - 7]):
            got = codec._residual_front_yuv_cpu(tuple(torch.from_numpy(v) for v in base),
                                                tuple(torch.from_numpy(v) for v in x), fmt, tau, s)
            st = codec._residual_front_yuv_cpu(tuple(torch.from_numpy(v) for v in base),
                                               tuple(torch.from_numpy(v) for v in x), fmt, tau, 0, stats=True)
            assert set(st) == {"max_abs_q", "sum_abs_q"}
            for b in range(2):
                want = orc.front(_smp(base, d, msb, b), _smp(x, d, msb, b), d, tau, s)
                assert want["max_err"] <= tau
                assert np.array_equal(got["ctx"][b].numpy(), want["ctx"])
                assert np.array_equal(got["ctx_count"][b].numpy(), want["ctx_count"])
                assert int(got["digest"][b]) & orc.MASK == want["digest"]
                assert np.array_equal(got["sym"][b].numpy(), want["sym"])
                assert np.array_equal(got["plane"][b].numpy().view(np.uint64), want["plane"])
                assert np.array_equal(got["hist"][b].numpy(), want["hist"])
                assert int(got["max_err"][b]) == want["max_err"]
                assert int(got["max_abs_q"][b]) == int(st["max_abs_q"][b]) == want["max_abs_q"]
                assert int(got["sum_abs_q"][b]) == int(st["sum_abs_q"][b]) == want["sum_abs_q"]
            if d > 8 and not all(orc.fits(int(v), s) for v in got["max_abs_q"]):
                continue  # symbols outside +-255: the apply pass refuses them (below)
            ref = tuple(torch.from_numpy(v) for v in x)
            out = codec._residual_apply_yuv_cpu(tuple(torch.from_numpy(v) for v in base), got["sym"], got["plane"], fmt,
                                                tau, s, ref, None)
            for b in range(2):
                want = orc.front(_smp(base, d, msb, b), _smp(x, d, msb, b), d, tau, s)
                ap = orc.apply(_smp(base, d, msb, b), want["sym"], want["plane"], d, tau, s, ref=_smp(x, d, msb, b))
                assert not ap["bad"]
                for o, r, w in zip(out[:3], ap["rec"], want["rec"]):
                    assert np.array_equal(r, w) and np.array_equal(o[b].numpy(), orc.words(r, d, msb))
                assert out[3][b].tolist() == ap["sq_err"] and int(out[4][b]) == ap["max_err"] <= tau


def test_the_plane_is_packed_bit_by_bit():
    rng = np.random.default_rng(3)
    for shapes in ([(3, 70), (2, 35), (2, 35)], [(1, 1)] * 3, [(2, 64), (2, 64), (2, 64)], [(2, 129), (1, 65), (1, 65)]):
        for s in (1, 3, 9):
            lo = [rng.integers(0, 1 << s, sh) for sh in shapes]
            a, b = orc.pack_plane(lo, s), orc.pack_plane_bitwise(lo, s)
            assert np.array_equal(a, b) and a.size == s * sum(h * -(-w // 64) for h, w in shapes)
            back = orc.unpack_plane(a, shapes, s)
            assert all(np.array_equal(u, v) for u, v in zip(back, lo))
            for (h, w), v in zip(shapes, lo):  # bits beyond the plane's width are zero
                if w % 64:
                    words = orc.pack_plane([v], s).reshape(h, -(-w // 64), s)
                    assert not (words[:, -1, :] >> np.uint64(w % 64)).any()


@pytest.mark.parametrize("d", [10, 16])
def test_444_planes_of_an_rgb_image_give_the_deep_layers_outputs(d):
    H, W, tau, s = 9, 70, 1, 3
    rng = np.random.default_rng(d)
    base = rng.integers(0, 1 << d, (3, H, W)).astype(np.uint16)
    x = rng.integers(0, 1 << d, (3, H, W)).astype(np.uint16)
    want = orc16.front(base.astype(np.int64), x.astype(np.int64), d, tau, s)
    got = codec._residual_front_yuv_cpu(tuple(torch.from_numpy(base[c][None]) for c in range(3)),
                                        tuple(torch.from_numpy(x[c][None]) for c in range(3)), _fmt((1, 1), d), tau, s)
    assert np.array_equal(got["ctx"][0].numpy(), want["ctx"].reshape(-1))
    assert np.array_equal(got["sym"][0].numpy(), want["sym"].reshape(-1))
    assert np.array_equal(got["plane"][0].numpy().view(np.uint64), want["plane"])
    assert np.array_equal(got["hist"][0].numpy(), want["hist"])
    assert int(got["digest"][0]) & orc.MASK == want["digest"]
    mine = orc.front([v.astype(np.int64) for v in base], [v.astype(np.int64) for v in x], d, tau, s)
    assert np.array_equal(mine["plane"], want["plane"]) and mine["digest"] == want["digest"]


def test_444_planes_of_an_rgb_image_give_the_8_bit_layers_outputs():
    H, W, tau = 9, 70, 2
    rng = np.random.default_rng(8)
    base = rng.integers(0, 256, (1, 3, H, W)).astype(np.uint8)
    x = rng.integers(0, 256, (1, 3, H, W)).astype(np.uint8)
    want = codec._residual_front_cpu(torch.from_numpy(base), torch.from_numpy(x), tau, "chw", "chw")
    got = codec._residual_front_yuv_cpu(tuple(torch.from_numpy(base[:, c]) for c in range(3)),
                                        tuple(torch.from_numpy(x[:, c]) for c in range(3)), _fmt((1, 1), 8), tau, 0)
    for k in ("ctx", "sym"):
        assert torch.equal(got[k], want[k].reshape(1, -1)), k
    for k in ("ctx_count", "hist", "digest", "max_err"):
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("d", [8, 10, 16])
@pytest.mark.parametrize("tau", [0, 1, 2, 127])
def test_the_bound_holds_over_the_full_word_range(d, tau):
    for msb in ([False] if d == 8 else [False, True]):
        base, x = _frame(31, 67, (2, 2), d, msb, 7 * d + tau)
        b, v = _smp(base, d, msb), _smp(x, d, msb)
        for p in range(3):
            edge = np.array([0, 1, tau, 2 * tau + 1, (1 << d) - 2, (1 << d) - 1])
            xs = np.concatenate([v[p].reshape(-1), np.repeat(edge, edge.size)])
            bs = np.concatenate([b[p].reshape(-1), np.tile(edge, edge.size)])
            q = orc.quantise(xs, bs, tau)
            rec = orc.reconstruct(bs, q, tau, d)
            assert int(np.abs(xs - rec).max()) <= tau and (tau or np.array_equal(rec, xs))
            assert rec.min() >= 0 and rec.max() <= (1 << d) - 1 and int(np.abs(q).max()) <= (1 << d) - 1
        got = codec._residual_front_yuv_cpu(tuple(torch.from_numpy(t) for t in base), tuple(torch.from_numpy(t) for t in x),
                                            _fmt((2, 2), d, msb), tau, 0 if d == 8 else d - 7)
        assert int(got["max_err"][0]) <= tau


def test_the_shift_rule_and_the_plane_word_count_against_brute_force():
    rng = np.random.default_rng(5)
    for d in (9, 10, 12, 16):
        for _ in range(60):
            H, W = int(rng.integers(1, 300)), int(rng.integers(1, 300))
            sub = SUBS[int(rng.integers(0, 3))]
            n = orc.n_samples(H, W, sub)
            assert n == codec.residual_yuv_samples(H, W, sub) == codec.residual_yuv_geom(H, W, sub)["N"]
            mq = int(rng.integers(0, 1 << d))
            sq = int(rng.integers(0, mq * n + 1))
            assert codec.residual_shift(d, n, mq, sq) == orc.shift_rule(d, n, mq, sq)
            for s in range(0, d - 6):
                assert codec.residual_yuv_plane_words(H, W, sub, s) == orc.plane_words(H, W, sub, s) == \
                    codec.residual_yuv_geom(H, W, sub)["groups"] * s
    assert orc.shift_rule(8, 100, 255, 25500) == 0 and orc.max_shift(8) == 0 and orc.max_shift(10) == 3
    for bad, word in (((0, 4, 2, 2), "H and W must be positive"), ((4, 4, 1, 2), "must be one of"),
                      ((4, 4, 3, 1), "must be one of"), ((1 << 15, 1 << 15, 1, 1), "more than 2\\^29 samples")):
        with pytest.raises(_lib.MlicError, match="residual_yuv_samples: .*" + word):
            _lib.call("mlic_residual_yuv_samples", *bad, C.byref(C.c_uint64()))
    with pytest.raises(_lib.MlicError, match="residual_yuv_plane_words: shift must be in 0..9"):
        _lib.call("mlic_residual_yuv_plane_words", 4, 4, 2, 2, 10, C.byref(C.c_uint64()))


# ------------------------------------------------------------------------- the segment coders for a given N
def _tables_and_symbols(N, seed):
    rng = np.random.default_rng(seed)
    sym = rng.integers(-70, 71, N).astype(np.int16)
    ctx = rng.integers(0, 24, N).astype(np.uint8)
    hist = orc.histogram(sym.astype(np.int64), ctx)
    return sym, ctx, codec.residual_tables(hist)


def test_host_n_at_3hw_is_the_hw_entry_byte_for_byte():
    H, W, L = 7, 45, 256
    sym, ctx, t = _tables_and_symbols(3 * H * W, 1)
    a = codec.residual_encode_segments(torch.from_numpy(sym.reshape(1, 3, H, W)), torch.from_numpy(ctx.reshape(1, 3, H, W)),
                                       [t], L, "host")
    b = codec.residual_encode_segments(torch.from_numpy(sym[None]), torch.from_numpy(ctx[None]), [t], L, "host")
    assert a[0][0] == b[0][0] and np.array_equal(a[0][1], b[0][1])
    back = codec.residual_decode_segments([b[0][0]], [b[0][1]], torch.from_numpy(ctx[None]), [t], L, "host")
    assert tuple(back.shape) == (1, 3 * H * W) and np.array_equal(back[0].numpy(), sym)


@pytest.mark.parametrize("N,n_seg,last", [(3, 1, 3), (6 * 256 + 1, 7, 1), (orc.n_samples(19, 261, (2, 2)), 30, 155)])
def test_host_n_codes_strings_that_are_no_rgb_image(N, n_seg, last):
    L = 256
    sym, ctx, t = _tables_and_symbols(N, N)
    (data, segb), = codec.residual_encode_segments(torch.from_numpy(sym[None]), torch.from_numpy(ctx[None]), [t], L, "host")
    assert len(segb) == n_seg == -(-N // L) and N - (n_seg - 1) * L == last and int(segb.sum()) == len(data)
    # each segment is rans_encode of its slice
    from mlic_amd import entropy
    at = 0
    for k in range(n_seg):
        sl = slice(k * L, min((k + 1) * L, N))
        want = entropy.rans_encode(sym[sl].astype(np.int32), ctx[sl].astype(np.int32), *codec._coder_tables(t))
        assert data[at:at + int(segb[k])] == want
        at += int(segb[k])
    back = codec.residual_decode_segments([data], [segb], torch.from_numpy(ctx[None]), [t], L, "host")
    assert np.array_equal(back[0].numpy(), sym)


def test_the_n_entries_refuse_bad_sizes_before_anything_else():
    m = np.zeros((1, 24), np.uint8)
    freq = np.zeros((1, 24, 128), np.uint16)
    freq[:, :, 0], freq[:, :, 1] = 65535, 1
    sym, ctx = np.zeros(1000, np.int16), np.zeros(1000, np.uint8)
    segb = np.zeros(8, np.uint32)
    lens = (C.c_uint64 * 1)()

    def enc(N=1000, L=256, n_seg=4, B=1):
        _lib.call("mlic_residual_encode_segments_host_n", sym.ctypes.data, ctx.ctypes.data, B, N, m.ctypes.data,
                  freq.ctypes.data, L, n_seg, None, 0, segb.ctypes.data, lens)

    enc()
    for kw, word in ((dict(N=0), "N must be positive"), (dict(N=(1 << 29) + 1, n_seg=2097153), "N is above 2\\^29"),
                     (dict(L=255), "outside 256..65536"), (dict(n_seg=3), r"n_seg 3 is not ceil\(N / seg_len\) = 4"),
                     (dict(B=0), "B must be positive")):
        with pytest.raises(_lib.MlicError, match="residual_encode_segments_host_n: .*" + word):
            enc(**kw)
    n = C.c_size_t()
    _lib.call("mlic_residual_segments_scratch_bytes_n", 2, 1000, 256, C.byref(n))
    old = C.c_size_t()
    _lib.call("mlic_residual_segments_scratch_bytes", 2, 4, C.byref(old))
    assert n.value == old.value > 0
    with pytest.raises(_lib.MlicError, match="residual_segments_scratch_bytes_n: "):
        _lib.call("mlic_residual_segments_scratch_bytes_n", 2, 0, 256, C.byref(n))
    p = lambda v: C.c_void_p(v)  # noqa: E731
    for name, args in (("mlic_residual_encode_segments_n",
                        (None, p(64), p(128), 1, 1000, m.ctypes.data, freq.ctypes.data, 256, 5, p(256), 4096, p(512), lens,
                         p(1024), 1 << 20, None)),
                       ("mlic_residual_decode_segments_n",
                        (None, p(64), 4096, lens, segb.ctypes.data, p(128), 1, 1000, m.ctypes.data, freq.ctypes.data, 256, 5,
                         p(256), p(1024), 1 << 20, None))):
        with pytest.raises(_lib.MlicError, match=name[5:] + r": n_seg 5 is not ceil\(N / seg_len\) = 4"):
            _lib.call(name, *args)  # refused before any HIP call: the fake device pointers are never used


# ------------------------------------------------------------------------------------------ the container
def _parts(depth=10, shift=3, sub=(2, 2), matrix="bt709", full_range=False, site_x="left", vbr=False, H=17, W=70, L=256):
    rng = np.random.default_rng(depth * 31 + shift)
    hist = np.zeros((24, 128), np.int64)
    hist[:, 60:67] = rng.integers(1, 50, (24, 7))
    hist[5] = 0
    hist[7, 127] = 3
    t = codec.residual_tables(hist)
    fmt = YuvFormat(sub, matrix, full_range, site_x, depth)
    n_seg = -(-orc.n_samples(H, W, sub) // L)
    seg_bytes = (8 + 4 * rng.integers(0, 20, n_seg)).astype(np.uint32)
    segs = rng.integers(0, 256, int(seg_bytes.sum()), dtype=np.uint8).tobytes()
    inner = codec.write_container(H, W, (-(-H // 64), -(-W // 64)), b"\x01\x02\x03", b"\x09", 2 if vbr else None)
    low = rng.integers(0, 256, 8 * orc.plane_words(H, W, sub, shift), dtype=np.uint8).tobytes()
    return dict(H=H, W=W, inner=inner, segs=segs, seg_bytes=seg_bytes, segment=L, tau=3, fmt=fmt, shift=shift, low=low,
                digest=0x0123456789ABCDEF, m=t["m"], freq=t["freq"], vbr=vbr)


def _python_writer(p):
    """The "MLR4" file written out from its layout (include/mlic_hip.h), big-endian."""
    fmt = p["fmt"]
    out = b"MLR4" + bytes([0, int(p["vbr"]), p["tau"], 24]) + struct.pack(">IIQ", p["H"], p["W"], p["digest"])
    for k in range(24):
        mk = int(p["m"][k])
        out += bytes([mk])
        if mk != 0xFF:
            out += struct.pack(f">{2 * mk + 2}H", *[int(v) for v in p["freq"][k, :2 * mk + 2]])
    out += bytes([fmt.depth, p["shift"], fmt.sub[0], fmt.sub[1], {"bt601": 0, "bt709": 1, "bt2020": 2}[fmt.matrix],
                  int(fmt.full_range) | (int(fmt.site_x == "left") << 1)])
    out += struct.pack(">III", p["segment"], len(p["seg_bytes"]), len(p["inner"])) + p["inner"]
    out += struct.pack(">I", 4 * len(p["seg_bytes"]) + len(p["segs"]))
    out += struct.pack(f">{len(p['seg_bytes'])}I", *[int(v) for v in p["seg_bytes"]]) + p["segs"]
    return out + struct.pack(">I", len(p["low"])) + p["low"]


@pytest.mark.parametrize("vbr", [False, True])
@pytest.mark.parametrize("depth,shift,sub,matrix,full_range,site_x", [
    (8, 0, (2, 2), "bt601", True, "centre"), (10, 3, (2, 2), "bt2020", False, "left"), (16, 9, (2, 1), "bt709", False, "left"),
    (12, 0, (1, 1), "bt709", True, "left")])
def test_container_round_trips_and_the_python_writer_is_the_c_writer(depth, shift, sub, matrix, full_range, site_x, vbr):
    p = _parts(depth, shift, sub, matrix, full_range, site_x, vbr)
    f = codec.write_container_residual_yuv(**p)
    assert f == _python_writer(p)
    s = codec.parse_container_residual_yuv(f, n_levels=6)
    assert f[:4] == b"MLR4" and codec.is_residual_yuv_file(f) and not codec.is_residual_file(f)
    assert not codec.is_residual_deep_file(f)
    assert (s.H, s.W, s.tau, bool(s.vbr), s.digest, s.depth, s.shift) == (17, 70, 3, vbr, p["digest"], depth, shift)
    assert (s.sub_x, s.sub_y, s.matrix, bool(s.full_range), bool(s.site_x)) == \
        (sub[0], sub[1], {"bt601": 0, "bt709": 1, "bt2020": 2}[matrix], full_range, site_x == "left")
    assert (s.seg_len, s.n_seg, s.lo_len) == (256, len(p["seg_bytes"]), len(p["low"]))
    assert f[s.inner_off:s.inner_off + s.inner_len] == p["inner"] == codec.strip_residual(f, n_levels=6)
    assert f[s.data_off:s.data_off + s.data_len] == p["segs"] and f[s.lo_off:s.lo_off + s.lo_len] == p["low"]
    assert np.array_equal(np.frombuffer(f, ">u4", s.n_seg, s.index_off), p["seg_bytes"])
    assert s.lo_off + s.lo_len == len(f) and list(s.m) == list(p["m"])
    d = codec.peek(f, n_levels=6)
    assert (d["depth"], d["shift"], d["low_bytes"], d["max_error"], d["segments"]) == (depth, shift, len(p["low"]), 3, s.n_seg)
    assert (d["sub"], d["matrix"], d["full_range"], d["site_x"]) == (sub, matrix, full_range, site_x)
    assert d["bytes"] == len(f) == d["base_bytes"] + d["residual_bytes"] + d["low_bytes"] + d["header_bytes"]
    assert codec.residual_yuv_format(f, n_levels=6) == p["fmt"]


def test_container_refusals_each_have_their_own_message():
    p = _parts()
    f = codec.write_container_residual_yuv(**p)
    s = codec.parse_container_residual_yuv(f)
    ds = s.inner_off - 18  # depth, shift, sub_x, sub_y, matrix, flags | seg_len, n_seg, inner_len
    put = lambda at, b: f[:at] + bytes(b) + f[at + len(b):]  # noqa: E731
    u32 = lambda v: int(v).to_bytes(4, "big")  # noqa: E731
    cases = [(put(3, b"3"), "bad magic"), (put(4, [1]), "unknown version"), (put(5, [2]), "unknown flags"),
             (put(6, [128]), "tau above 127"), (put(7, [23]), "n_ctx is not 24"), (put(8, u32(0)), "H or W is zero"),
             (put(24, [64]), "an m outside 0..63"), (put(ds, [7]), "depth outside 8..16"), (put(ds, [17]), "depth outside 8..16"),
             (put(ds, [8]), "shift must be 0 at depth 8"), (put(ds + 1, [4]), "shift outside 0..depth - 7"),
             (put(ds + 1, [2]), "lo_len is not"), (put(ds + 2, [1]), "sub_x, sub_y is not one of"),
             (put(ds + 3, [3]), "sub_x, sub_y is not one of"), (put(ds + 4, [3]), "matrix outside 0..2"),
             (put(ds + 5, [6]), "reserved flag bits are set"), (put(ds + 5, [0x80]), "reserved flag bits are set"),
             (put(ds + 6, u32(255)), "seg_len outside 256..65536"), (put(ds + 10, u32(s.n_seg + 1)), "n_seg is not ceil(N / seg_len)"),
             (put(ds + 3, [1]), "n_seg is not ceil(N / seg_len)"),  # 4:2:2 has other N
             (put(ds + 14, u32(0)), "an empty inner file"), (put(s.index_off, u32(6)), "not a multiple of 4"),
             (put(s.index_off, u32(4)), "a segment length below 8"),
             (put(s.index_off, u32(int(p["seg_bytes"][0]) + 4)), "not 4 n_seg + the segment lengths"),
             (put(s.lo_off - 4, u32(s.lo_len + 8)), "lo_len is not"), (f[:-1], "truncated inside the low-bit plane"),
             (f[:s.lo_off - 2], "truncated before the low-bit plane's length"),
             (f[:ds + 3], "truncated before depth, shift and the frame's fields"),
             (f + b"\0", "bytes left over after the low-bit plane"), (f[:10], "truncated header")]
    seen = set()
    for bad, word in cases:
        with pytest.raises(_lib.MlicError, match="container_parse_residual_yuv: .*" + re.escape(word)) as e:
            codec.parse_container_residual_yuv(bad)
        seen.add(str(e.value).split(" [")[0])
    assert len(seen) == len({w for _, w in cases})
    p8 = _parts(depth=8, shift=0)
    f8 = codec.write_container_residual_yuv(**p8)
    s8 = codec.parse_container_residual_yuv(f8)
    at = s8.inner_off - 18 + 4
    with pytest.raises(_lib.MlicError, match=r"container_parse_residual_yuv: matrix 2 \(BT.2020\) at depth 8"):
        codec.parse_container_residual_yuv(f8[:at] + bytes([2]) + f8[at + 1:])
    with pytest.raises(_lib.MlicError, match="exceeds max_pixels"):
        codec.parse_container_residual_yuv(f, max_pixels=17 * 70 - 1)
    for n in range(0, len(f), 7):  # truncations (the check program takes every byte)
        with pytest.raises(_lib.MlicError):
            codec.parse_container_residual_yuv(f[:n])
    for kw, word in ((dict(shift=4), "shift outside 0..depth - 7"), (dict(low=p["low"] + bytes(8)), "lo_len is not"),
                     (dict(tau=128), "tau above 127"), (dict(seg_bytes=p["seg_bytes"][:-1]), "n_seg is not ceil(N / seg_len)")):
        with pytest.raises(_lib.MlicError, match="container_write_residual_yuv: " + re.escape(word)):
            codec.write_container_residual_yuv(**{**p, **kw})
    with pytest.raises(_lib.MlicError, match="container_write_residual_yuv: shift must be 0 at depth 8"):
        codec.write_container_residual_yuv(**{**p8, "shift": 1})
    args = [17, 70, 0, 3, 8, 0, 2, 2, 2, 0, 1, 1, p8["m"].ctypes.data, p8["freq"].ctypes.data, 256, len(p8["seg_bytes"]),
            p8["seg_bytes"].ctypes.data, p8["inner"], len(p8["inner"]), p8["segs"], len(p8["segs"]), None, 0, None, 0,
            C.byref(C.c_size_t())]
    with pytest.raises(_lib.MlicError, match=r"container_write_residual_yuv: matrix 2 \(BT.2020\) at depth 8"):
        _lib.call("mlic_container_write_residual_yuv", *args)
    args[8:11] = [1, 2, 1]
    with pytest.raises(_lib.MlicError, match="container_write_residual_yuv: full_range must be 0 or 1"):
        _lib.call("mlic_container_write_residual_yuv", *args)


def test_the_other_parsers_refuse_an_mlr4_file_and_this_one_theirs():
    p = _parts()
    f = codec.write_container_residual_yuv(**p)
    for parse in (codec.parse_container, codec.parse_container_residual, codec.parse_container_residual_seg,
                  codec.parse_container_residual_deep, codec.parse_container_scaled, codec.parse_container_layered,
                  codec.parse_container_tiled, lambda d: codec.parse_container(d, True, 6),
                  lambda d: codec.parse_container_roi(d, 6)):
        with pytest.raises(_lib.MlicError):
            parse(f)
    n3 = -(-3 * 17 * 70 // 256)
    sb3 = np.full(n3, 8, np.uint32)
    seg = codec.write_container_residual_seg(17, 70, p["inner"], bytes(8 * n3), sb3, 256, 3, 1, p["m"], p["freq"])
    deep = codec.write_container_residual_deep(17, 70, p["inner"], bytes(8 * n3), sb3, 256, 3, 10, 0, b"", 1, p["m"], p["freq"])
    for other in (seg, deep, p["inner"]):
        with pytest.raises(_lib.MlicError, match="bad magic|truncated header"):
            codec.parse_container_residual_yuv(other)
    assert codec.parse_container_residual_seg(seg).n_seg == n3  # the MLR2 and MLR3 parsers are unchanged
    assert codec.parse_container_residual_deep(deep).n_seg == n3


def test_container_residual_yuv_check_program_under_sanitizers(tmp_path):
    """tools/container_residual_yuv_check.cpp with container.cpp, rans.cpp and residual_seg.cpp, AddressSanitizer +
    UBSan, as a stand-alone program (no sanitizer runtime comes near Python): the geometry and the bound swept, the
    writer and the parser with every refusal and truncations at every byte, and the host coders for a given N on
    all-escape segments.  Skipped where the compiler cannot link the sanitizer runtimes."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed for the container's sanitizer check"
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    pr = subprocess.run([cxx] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if pr.returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed: " + pr.stderr[-200:])
    exe = str(tmp_path / "container_residual_yuv_check")
    csrc = os.path.join(ROOT, "mlic_amd", "csrc")
    cmd = [cxx, "-std=c++17", "-O1", "-g"] + san + [
           "-I" + csrc, os.path.join(ROOT, "tools", "container_residual_yuv_check.cpp"),
           os.path.join(csrc, "container.cpp"), os.path.join(csrc, "rans.cpp"), os.path.join(csrc, "residual_seg.cpp"),
           "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-300:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("container_residual_yuv_check ok"), \
        r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------ the entries' refusals
def test_device_entries_refuse_bad_arguments_before_any_gpu_call():
    """Every argument is checked before any HIP call: the device pointers (small fake addresses) are never
    dereferenced, and no GPU is needed."""
    p = lambda v: C.c_void_p(v)  # noqa: E731
    st = (C.c_int64 * 3)(64, 8, 1)
    zero = (C.c_int64 * 3)(64, 8, 0)
    good = _lib.YuvDesc(2, 2, 1, 0, 1, (C.c_int32 * 3)(0, 0, 0))

    def planes(a, s=st, first=None, first_s=None):
        return [p(a if first is None else first) if (a or first) else None, s if first_s is None else first_s,
                p(a + 64) if a else None, s, p(a + 128) if a else None, s]

    def front16(base=1024, bs=st, x=4096, desc=good, d=10, msb=0, B=1, H=4, W=8, tau=0, s=2, ctx=256, cnt=512, dg=8192,
                sym=2048, lo=16384, hist=32768, me=65536, mq=131072, sq=262144, b0=None, b0s=None, x0=None):
        _lib.call("mlic_image_residual_front_yuv16", None, *planes(base, bs, b0, b0s), *planes(x, st, x0),
                  C.byref(desc) if desc is not None else None, d, msb, B, H, W, tau, s, p(ctx), p(cnt), p(dg), p(sym),
                  p(lo), p(hist), p(me), p(mq), p(sq))

    def desc(**kw):
        f = dict(sub_x=2, sub_y=2, matrix=1, full_range=0, site_x=1)
        f.update(kw)
        return _lib.YuvDesc(f["sub_x"], f["sub_y"], f["matrix"], f["full_range"], f["site_x"],
                            (C.c_int32 * 3)(0, 0, f.get("reserved", 0)))

    cases = ((dict(B=0), "B must be positive"), (dict(W=0), "H and W must be positive"),
             (dict(W=(1 << 24) + 1), "frame side above 2\\^24"), (dict(d=8), "depth must be in 9..16"),
             (dict(d=17), "depth must be in 9..16"), (dict(msb=2), "msb must be 0 or 1"), (dict(desc=None), "null mlic_yuv_desc"),
             (dict(desc=desc(sub_x=3)), "sub_x and sub_y must be 1 or 2"), (dict(desc=desc(sub_x=1)), "4:4:0"),
             (dict(desc=desc(matrix=3)), "matrix must be 0"), (dict(desc=desc(full_range=2)), "full_range must be 0 or 1"),
             (dict(desc=desc(site_x=2)), "site_x must be 0"), (dict(desc=desc(reserved=1)), "reserved fields must be 0"),
             (dict(tau=128), "tau must be in 0..127"), (dict(bs=zero), "zero column stride \\(base"),
             (dict(b0=1025), "base planes must be 2-byte aligned"), (dict(ctx=None), "null ctx"),
             (dict(dg=8196), "digest 8-byte aligned"), (dict(x0=4097), "x planes must be 2-byte aligned"),
             (dict(s=4), "shift must be in 0..depth - 7"), (dict(s=-1), "shift must be in 0..depth - 7"),
             (dict(sym=None), "are all needed"), (dict(mq=None), "are all needed"),
             (dict(lo=None), "lo_plane goes with a shift above 0"), (dict(s=0), "lo_plane goes with a shift above 0"),
             (dict(lo=16388), "8-byte aligned"), (dict(x=0), "go with x"))
    for kw, word in cases:
        with pytest.raises(_lib.MlicError, match="image_residual_front_yuv16: .*" + word):
            front16(**kw)
    with pytest.raises(_lib.MlicError, match="image_residual_front_yuv16: null base plane \\(y\\)"):
        _lib.call("mlic_image_residual_front_yuv16", None, None, st, p(64), st, p(128), st, *([None] * 6), C.byref(good), 10,
                  0, 1, 4, 8, 0, 0, p(256), p(512), p(8192), None, None, None, None, None, None)
    with pytest.raises(_lib.MlicError, match="image_residual_front_yuv16: x needs three planes with strides"):
        _lib.call("mlic_image_residual_front_yuv16", None, *planes(1024), p(4096), st, None, None, p(4224), st,
                  C.byref(good), 10, 0, 1, 4, 8, 0, 0, p(256), p(512), p(8192), p(2048), None, p(32768), p(65536), p(131072),
                  p(262144))

    def front8(s=0, lo=None, desc_=good, tau=0):
        _lib.call("mlic_image_residual_front_yuv8", None, *planes(1024), *planes(4096), C.byref(desc_), 1, 4, 8, tau, s,
                  p(256), p(512), p(8192), p(2048), p(lo) if lo else None, p(32768), p(65536), p(131072), p(262144))

    for kw, word in ((dict(s=1), "shift must be 0 at depth 8"), (dict(lo=16384), "lo_plane must be null at depth 8"),
                     (dict(desc_=desc(matrix=2)), "matrix must be 0 \\(BT.601\\) or 1 \\(BT.709\\)"), (dict(tau=-1), "tau must be")):
        with pytest.raises(_lib.MlicError, match="image_residual_front_yuv8: .*" + word):
            front8(**kw)

    def stats(x=4096, d=10, mq=131072, sq=262144, tau=0):
        _lib.call("mlic_image_residual_stats_yuv16", None, *planes(1024), *planes(x), C.byref(good), d, 0, 1, 4, 8, tau,
                  p(mq), p(sq))

    for kw, word in ((dict(x=0), "x needs three planes"), (dict(d=8), "depth must be"), (dict(mq=None), "null max_abs_q"),
                     (dict(sq=262148), "sum_abs_q 8-byte aligned"), (dict(tau=-1), "tau must be")):
        with pytest.raises(_lib.MlicError, match="image_residual_stats_yuv16: .*" + word):
            stats(**kw)

    def apply(sym=2048, lo=16384, d=10, s=2, out=4096, os_=st, ref=0, sq=None, me=None, status=256):
        _lib.call("mlic_image_residual_apply_yuv16", None, *planes(1024), p(sym), p(lo), C.byref(good), d, 0, 1, 4, 8, 0, s,
                  *planes(out, os_), *planes(ref), p(sq), p(me), p(status))

    for kw, word in ((dict(sym=None), "null sym"), (dict(out=0), "out needs three planes"), (dict(status=None), "null status"),
                     (dict(s=4), "shift must be"), (dict(lo=None), "lo_plane goes with"), (dict(os_=zero), "zero column stride \\(out\\)"),
                     (dict(out=4097), "out planes must be 2-byte aligned"), (dict(ref=512), "ref without sq_err"),
                     (dict(ref=512, sq=1024), "ref without max_err"), (dict(sq=1024), "go with ref"), (dict(d=20), "depth must be")):
        with pytest.raises(_lib.MlicError, match="image_residual_apply_yuv16: .*" + word):
            apply(**kw)


# ---------------------------------------------------------------------------------------------- policy
class StubNet:
    """A 'model' on the CPU (tests/test_residual_cpu.py's): compress keeps the 8 x 8 block means of each image as
    the y string, decompress paints them back, so the base picture is a real, lossy, repeatable picture."""
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


H2, W2 = 70, 66
FORMATS = {"i420": ("i420", YuvFormat((2, 2), "bt709", False, "left", 8)),
           "nv12": ("nv12", YuvFormat((2, 2), "bt601", True, "centre", 8)),
           "i422p10": ("i422", YuvFormat((2, 1), "bt709", False, "left", 10)),
           "p010": ("nv12", YuvFormat((2, 2), "bt2020", False, "left", 10, True))}


def _frames(name, B=3, seed=5):
    layout, fmt = FORMATS[name]
    g = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.interpolate(torch.rand(B, 3, 5, 6, generator=g), size=(H2, W2), mode="bilinear")
    x = (x + 0.04 * torch.randn(B, 3, H2, W2, generator=g)).clamp(0, 1)
    y, cb, cr = codec.egress_yuv(x, H2, W2, fmt)
    buf = np.zeros((B, codec.yuv_frame_samples(H2, W2, layout)), np.uint8 if fmt.depth == 8 else np.uint16)
    py, pcb, pcr = codec.split_yuv(buf, H2, W2, layout, fmt.depth)
    py[...], pcb[...], pcr[...] = y.numpy(), cb.numpy(), cr.numpy()
    if fmt.depth == 8 and not fmt.full_range:
        py[:, 0, :8] = [0, 1, 15, 236, 254, 255, 3, 250]  # outside the legal range: they come back exactly all the same
    return codec.split_yuv(buf, H2, W2, layout, fmt.depth), fmt


@pytest.mark.parametrize("vbr", [False, True])
@pytest.mark.parametrize("tau", [0, 2])
@pytest.mark.parametrize("name", list(FORMATS))
def test_cpu_path_end_to_end(name, tau, vbr):
    planes, fmt = _frames(name)
    net = StubNet(vbr)
    level = [1, 4, 2] if vbr else None
    files, info = codec.encode_residual_yuv(net, *planes, fmt, max_error=tau, level=level, residual_segment=300,
                                            residual_coder="host", return_info=True)
    plain = codec.encode_yuv(net, *planes, fmt, level=level)
    assert all(f[:4] == b"MLR4" for f in files) and [codec.strip_residual(f, n_levels=6) for f in files] == plain
    assert files == codec.encode_residual_yuv(net, *planes, fmt, max_error=tau, level=level, residual_segment=300)
    N = orc.n_samples(H2, W2, fmt.sub)
    base, _ = codec.decode_yuv(net, plain, fmt)
    for b, f in enumerate(files):
        pk = codec.peek(f, n_levels=6)
        assert info[b]["bytes"] == len(f) == info[b]["base_bytes"] + info[b]["residual_bytes"] + info[b]["low_bytes"] + pk["header_bytes"]
        assert (info[b]["max_error"], info[b]["depth"], info[b]["sub"], info[b]["segments"]) == (tau, fmt.depth, fmt.sub, -(-N // 300))
        assert info[b]["low_bytes"] == 8 * orc.plane_words(H2, W2, fmt.sub, info[b]["shift"])
        st = codec.residual_stats_yuv(tuple(t[b] for t in base), tuple(p[b] for p in planes), fmt, tau)
        assert info[b]["shift"] == orc.shift_rule(fmt.depth, N, int(st["max_abs_q"][0]), int(st["sum_abs_q"][0]))
    for coder in ("device", "host"):  # "device" on a CPU model falls to the host entry
        out, dinfo = codec.decode_yuv(net, files, fmt, ref=planes, residual_coder=coder)
        for o, src in zip(out, planes):
            got, want = orc.samples(o.numpy(), fmt.depth, fmt.msb), orc.samples(src, fmt.depth, fmt.msb)
            assert o.dtype == fmt.dtype and int(np.abs(got - want).max()) <= tau and (tau or np.array_equal(got, want))
            if fmt.msb:
                assert not (o.numpy() & 63).any()
        for b in range(3):
            assert dinfo[b]["max_abs_err"] <= tau == dinfo[b]["max_error"] and len(dinfo[b]["sq_err"]) == 3
            assert tau or dinfo[b]["sq_err"] == [0, 0, 0]
            assert "psnr_y" in dinfo[b] and "psnr_yuv" in dinfo[b]
    only, oinfo = codec.decode_yuv(net, files, fmt, enhance=False)
    assert all(torch.equal(a, b) for a, b in zip(only, base)) and oinfo[0]["enhanced"] is False
    single = [codec.encode_residual_yuv(net, *(p[b] for p in planes), fmt, max_error=tau, level=level and level[b],
                                        residual_segment=300)[0] for b in range(3)]
    assert single == files


def test_refusals_by_name():
    net = StubNet()
    planes, fmt = _frames("i422p10", B=2)
    files = codec.encode_residual_yuv(net, *planes, fmt, max_error=1)
    plain = codec.encode_yuv(net, *planes, fmt)
    with pytest.raises(ValueError, match=r"encode_yuv: max_error= \(residual coding\) together with Y'CbCr frames is not supported"):
        codec.encode_yuv(net, *planes, fmt, max_error=0)
    for kw, word in ((dict(max_bpp=0.5), "max_bpp="), (dict(roi=np.ones((H2, W2), np.uint8)), "roi="), (dict(tile=128), "tiles"),
                     (dict(scale=0.5), "scaled coding"), (dict(coded_size=(32, 32)), "scaled coding"), (dict(layered=True), "layered=")):
        with pytest.raises(ValueError, match=f"encode_residual_yuv: residual coding of Y'CbCr frames together with {word} is not supported"):
            codec.encode_residual_yuv(net, *planes, fmt, **kw)
    with pytest.raises(ValueError, match="together with level='auto' is not supported"):
        codec.encode_residual_yuv(net, *planes, fmt, level="auto")
    for kw, word in ((dict(max_error=128), "max_error must be"), (dict(residual_shift=4), "shift must be an integer in \\[0, 3\\]"),
                     (dict(residual_segment=100), "residual_segment must be"), (dict(residual_coder="gpu"), "residual_coder must be")):
        with pytest.raises(ValueError, match="encode_residual_yuv: " + word):
            codec.encode_residual_yuv(net, *planes, fmt, **kw)
    p8, f8 = _frames("i420", B=1)
    with pytest.raises(ValueError, match="encode_residual_yuv: shift must be an integer in \\[0, 0\\] at depth 8"):
        codec.encode_residual_yuv(net, *p8, f8, residual_shift=1)
    with pytest.raises(ValueError, match="must be a uint16 tensor or array"):
        codec.encode_residual_yuv(net, *p8, fmt)
    with pytest.raises(ValueError, match=r"YuvFormat: sub must be \(1, 1\), \(2, 1\) or \(2, 2\)"):
        YuvFormat((1, 2))
    other = {"depth": YuvFormat(fmt.sub, fmt.matrix, fmt.full_range, fmt.site_x, 12),
             "sub": YuvFormat((2, 2), fmt.matrix, fmt.full_range, fmt.site_x, fmt.depth),
             "matrix": YuvFormat(fmt.sub, "bt601", fmt.full_range, fmt.site_x, fmt.depth),
             "full_range": YuvFormat(fmt.sub, fmt.matrix, True, fmt.site_x, fmt.depth),
             "site_x": YuvFormat(fmt.sub, fmt.matrix, fmt.full_range, "centre", fmt.depth)}
    for field, wrong in other.items():
        with pytest.raises(ValueError, match=rf"decode_yuv: file 0 \(MLR4\) was written with {field}="):
            codec.decode_yuv(net, files, wrong)
    with pytest.raises(ValueError, match=r"residual \(MLR4\) and plain files cannot be mixed"):
        codec.decode_yuv(net, [files[0], plain[1]], fmt)
    with pytest.raises(ValueError, match=r"decode_images: a Y'CbCr residual file \(MLR4\) holds planes, not RGB: decode_yuv decodes it"):
        codec.decode_images(net, files)
    with pytest.raises(ValueError, match="out_size= / slices= together with residual"):
        codec.decode_yuv(net, files, fmt, slices=2)
    with pytest.raises(ValueError, match="model is variable-rate"):
        codec.decode_yuv(StubNet(True), files, fmt)
    # an explicit shift that fits, and one that does not
    base, _ = codec.decode_yuv(net, plain, fmt)
    mq = int(codec.residual_stats_yuv(base, planes, fmt, 0)["max_abs_q"].max())
    smin = codec.residual_min_shift(10, mq)
    fa = codec.encode_residual_yuv(net, *planes, fmt, residual_shift=3)
    assert codec.peek(fa[0])["shift"] == 3
    out, _ = codec.decode_yuv(net, fa, fmt)
    assert all(np.array_equal(o.numpy(), np.asarray(p)) for o, p in zip(out, planes))
    if smin > 0:
        with pytest.raises(ValueError, match=rf"residual_shift=0 does not fit frame \d .*the smallest shift that fits is \d$"):
            codec.encode_residual_yuv(net, *planes, fmt, residual_shift=0)
    # a corrupt file: the digest, a padding bit, a segment -- each refused by a check
    f = fa[1]
    s = codec.parse_container_residual_yuv(f)
    with pytest.raises(RuntimeError, match="the digest of the decoded base image"):
        codec.decode_yuv(net, [fa[0], f[:16] + bytes([f[16] ^ 1]) + f[17:]], fmt)
    at = s.lo_off + 8 * (1 * s.shift) + 7  # luma row 0, group 1 (W = 66: two columns), bit plane 0, bits 56..63
    with pytest.raises(ValueError, match="file 1: the low-bit plane has bits set beyond column 66 of plane 0"):
        codec.decode_yuv(net, [fa[0], f[:at] + bytes([f[at] | 0x80]) + f[at + 1:]], fmt)
    lens = np.frombuffer(f, ">u4", s.n_seg, s.index_off)
    at = s.data_off + int(lens[:1].sum()) + int(lens[1]) // 2
    with pytest.raises(ValueError, match="decode_yuv: file 1: segment 1 of the residual string is corrupt"):
        codec.decode_yuv(net, [fa[0], f[:at] + bytes([f[at] ^ 0x08]) + f[at + 1:]], fmt)


# ------------------------------------------------------------------------------------------ the command line
def _cli():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import mlic_codec
    finally:
        sys.path.pop(0)
    return mlic_codec


def test_cli_flags_for_frame_residuals():
    cli = _cli()
    enc = ["encode", "a.y4m", "a.bit", "--synthetic", "0"]
    a = cli.parse_args(enc + ["--frame-lossless"])
    assert a.frame_max_error == 0 and a.max_error is None and a.frame_file and a.residual_segment is None
    a = cli.parse_args(enc + ["--frame-max-error", "2", "--residual-segment", "512", "--residual-coder", "host",
                              "--residual-shift", "3", "--level", "1"])
    assert (a.frame_max_error, a.residual_segment, a.residual_coder, a.residual_shift) == (2, 512, "host", 3)
    assert cli.parse_args(enc + ["--frame-lossless", "--residual-coder", "host"]).residual_coder == "host"
    raw = ["encode", "a.yuv", "a.bit", "--synthetic", "0", "--size", "64x48", "--yuv", "nv12", "--depth", "10", "--msb"]
    assert cli.parse_args(raw + ["--frame-lossless"]).frame_max_error == 0
    d = cli.parse_args(["decode", "a.bit", "a.y4m", "--synthetic", "0", "--base-only"])
    assert d.base_only and d.frame_file
    for argv in (enc + ["--frame-max-error", "1", "--frame-lossless"], enc + ["--frame-max-error", "128"],
                 enc + ["--frame-lossless", "--max-bpp", "0.5"], enc + ["--frame-lossless", "--level", "auto", "--max-bpp", "1"],
                 enc + ["--frame-lossless", "--scale", "1/2"], enc + ["--frame-lossless", "--layered"],
                 enc + ["--frame-lossless", "--tile", "128"], enc + ["--frame-lossless", "--lossless"],
                 enc + ["--frame-lossless", "--residual-segment", "255"], enc + ["--frame-lossless", "--residual-shift", "10"],
                 ["encode", "a.ppm", "a.bit", "--synthetic", "0", "--frame-lossless"],
                 ["decode", "a.bit", "a.y4m", "--synthetic", "0", "--frame-lossless"],
                 enc + ["--lossless"], enc + ["--residual-segment", "512"], enc + ["--residual-shift", "2"],
                 enc + ["--residual-coder", "host"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(argv)
        assert e.value.code == 2, argv
