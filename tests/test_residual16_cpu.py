"""Residual coding of 9..16-bit samples without a GPU: the integer definitions (tests/residual16_oracle.py against
codec.py's restatement and the library's shift rule), the "MLR3" container, the stand-alone sanitizer program, the
entries' refusals before any GPU call, and the codec end to end on a CPU stand-in model (the StubNet of
tests/test_residual_cpu.py, restated here).  tests/test_gpu_residual16.py runs the kernels and synthetic MLICPP_S."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import residual16_oracle as orc
from mlic_amd import _lib, codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ the integers
def _bound(x, b, tau, d):
    q = orc.quantise(x, b, tau)
    rec = orc.reconstruct(b, q, tau, d)
    assert int(np.abs(x - rec).max()) <= tau and int(np.abs(q).max()) <= (1 << d) - 1
    if tau == 0:
        assert np.array_equal(rec, x)


@pytest.mark.parametrize("tau", [0, 1, 2, 127])
def test_the_bound_holds_exhaustively_at_depth_9(tau):
    x, b = np.meshgrid(np.arange(512, dtype=np.int64), np.arange(512, dtype=np.int64))
    _bound(x, b, tau, 9)


@pytest.mark.parametrize("d", [10, 12, 16])
def test_the_bound_holds_on_edge_pairs_and_random_pairs(d):
    maxv = (1 << d) - 1
    rng = np.random.default_rng(d)
    for tau in (0, 1, 2, 63, 127):
        edge = np.array([0, 1, tau, 2 * tau + 1, maxv // 2, maxv - 1, maxv], np.int64)
        x, b = np.meshgrid(edge, edge)
        _bound(x, b, tau, d)
        _bound(rng.integers(0, maxv + 1, 100000), rng.integers(0, maxv + 1, 100000), tau, d)


@pytest.mark.parametrize("d", [9, 10, 12, 16])
def test_split_then_join_is_the_identity_and_hi_stays_within_255_exactly_when_the_shift_fits(d):
    maxv = (1 << d) - 1
    q = np.arange(-maxv, maxv + 1, dtype=np.int64)
    for s in range(d - 6):
        hi, lo = orc.split(q, s)
        assert lo.min() >= 0 and lo.max() <= (1 << s) - 1 and np.array_equal(orc.join(hi, lo, s), q)
        assert np.array_equal(hi, q >> s)
        # for every bound M on |q|: all |hi| <= 255 exactly when M fits
        worst = np.maximum.accumulate(np.abs(orc.split(-np.arange(maxv + 1), s)[0]))
        fit = np.array([orc.fits(m, s) for m in range(0, maxv + 1, 7)])
        assert np.array_equal(worst[::7] <= 255, fit)
        assert all(codec.residual_shift_fits(m, s) == orc.fits(m, s) for m in (0, 255, 256, 255 << s, (255 << s) + 1, maxv))
    assert orc.fits(maxv, d - 7) and codec.residual_min_shift(d, maxv) <= d - 7


def test_the_shift_rule_on_hand_computed_cases():
    N = 3 * 100 * 100
    cases = [(10, N, 0, 0, 0),            # a perfect base
             (10, N, 255, 8 * N, 0),      # both conditions with equality at 0
             (10, N, 256, 8 * N, 1),      # (256 + 1) >> 1 = 128
             (10, N, 255, 8 * N + 1, 1),  # the sum alone pushes it to 1
             (12, N, 4095, 40 * N, 5),    # (4095 + 15) >> 4 = 256 does not fit, (4095 + 31) >> 5 = 128 does
             (16, N, 65535, 600 * N, 9),  # only d - 7 fits the largest q
             (16, N, 2000, 600 * N, 7),   # fits from 3; 8 * 2^7 = 1024 >= 600 > 512
             (16, N, 4100, 4100 * N, 9),  # nothing fits the sum (8 * 2^9 = 4096): d - 7
             (9, N, 511, 511 * N, 2)]     # d - 7 = 2 and 8 * 4 = 32 < 511: d - 7
    for d, n, mq, sq, want in cases:
        assert codec.residual_shift(d, n, mq, sq) == want == orc.shift_rule(d, n, mq, sq), (d, mq, sq)
    rng = np.random.default_rng(3)
    for _ in range(300):
        d = int(rng.integers(9, 17))
        mq = int(rng.integers(0, 1 << d))
        sq = int(rng.integers(0, mq * N + 1))
        assert codec.residual_shift(d, N, mq, sq) == orc.shift_rule(d, N, mq, sq)
    for bad in ((8, N, 0, 0), (17, N, 0, 0), (10, 0, 0, 0), (10, N, 1024, 0), (10, N, 5, 5 * N + 1)):
        with pytest.raises((_lib.MlicError, ValueError)):
            codec.residual_shift(*bad)


@pytest.mark.parametrize("W", [1, 63, 64, 65, 130])
def test_plane_packing(W):
    H, s = 3, 5
    rng = np.random.default_rng(W)
    lo = rng.integers(0, 1 << s, (3, H, W)).astype(np.int64)
    want = orc.pack_plane(lo, s)
    G = -(-W // 64)
    assert want.size == 3 * H * G * s == codec.residual_plane_words(H, W, s)
    got = codec._pack_plane_np(lo[None], s)[0]
    assert np.array_equal(got, want)
    assert np.array_equal(codec._unpack_plane_np(got[None], H, W, s)[0], lo)
    # by hand: bit x mod 64 of word ((c H + y) G + x / 64) s + j
    for c, y, x, j in ((0, 0, 0, 0), (2, H - 1, W - 1, s - 1), (1, 1, W // 2, 2)):
        assert (int(want[((c * H + y) * G + x // 64) * s + j]) >> (x % 64)) & 1 == (int(lo[c, y, x]) >> j) & 1
    if W % 64:  # bits beyond column W are zero
        assert not (want.reshape(3 * H, G, s)[:, -1, :] >> np.uint64(W % 64)).any()
    assert codec._pack_plane_np(lo[None], 0).size == 0


@pytest.mark.parametrize("d,tau,H,W", [(9, 0, 5, 7), (10, 1, 19, 70), (12, 127, 9, 65), (16, 3, 8, 130)])
def test_codec_restatement_is_the_oracle(d, tau, H, W):
    rng = np.random.default_rng(H * W)
    maxv = (1 << d) - 1
    base = rng.integers(0, min(65535, maxv + 9) + 1, (2, H, W, 3)).astype(np.uint16)
    x = np.clip(base.astype(np.int64) + rng.integers(-900, 901, base.shape), 0, 65535).astype(np.uint16)
    st = codec.residual_stats16(base, x, d, tau)
    for s in sorted({0, d - 7, codec.residual_min_shift(d, int(st["max_abs_q"].max()))}):
        chw = np.ascontiguousarray(base.transpose(0, 3, 1, 2))
        got = codec.residual_front16(chw, x, d, tau, s, "chw", "hwc")
        for b in range(2):
            sm = lambda a: np.minimum(a[b].astype(np.int64), maxv).transpose(2, 0, 1)  # noqa: E731
            want = orc.front(sm(base), sm(x), d, tau, s)
            assert np.array_equal(got["ctx"][b].numpy(), want["ctx"]) and int(got["digest"][b]) & orc.MASK == want["digest"]
            assert np.array_equal(got["ctx_count"][b].numpy(), want["ctx_count"])
            assert np.array_equal(got["sym"][b].numpy(), want["sym"]) and np.array_equal(got["hist"][b].numpy(), want["hist"])
            assert np.array_equal(got["plane"][b].numpy().view(np.uint64), want["plane"])
            assert (int(got["max_err"][b]), int(got["max_abs_q"][b]), int(got["sum_abs_q"][b])) == \
                (want["max_err"], want["max_abs_q"], want["sum_abs_q"]) == \
                (want["max_err"], int(st["max_abs_q"][b]), int(st["sum_abs_q"][b]))
            if codec.residual_shift_fits(want["max_abs_q"], s):
                out, sq, me = codec.residual_apply16(base[b], got["sym"][b:b + 1], got["plane"][b:b + 1], d, tau, s, ref=x[b])
                assert np.array_equal(out[0].numpy(), want["rec"].transpose(1, 2, 0)) and int(me[0]) == want["max_err"] <= tau
                assert int(sq[0]) == int(((want["rec"] - sm(x)) ** 2).sum())


# ------------------------------------------------------------------------------------------ the container
def _parts(H=17, W=70, L=256, depth=10, shift=3, vbr=False):
    rng = np.random.default_rng(H * W + shift)
    hist = np.zeros((24, 128), np.int64)
    for k in (0, 3, 9, 17):
        hist[k, 63 - k:63 + k + 1] = 5
        hist[k, 127] = 1
    t = codec.residual_tables(hist)
    n_seg = -(-3 * H * W // L)
    seg_bytes = (8 + 4 * rng.integers(0, 20, n_seg)).astype(np.uint32)
    segs = rng.integers(0, 256, int(seg_bytes.sum()), dtype=np.uint8).tobytes()
    inner = codec.write_container(H, W, (-(-H // 64), -(-W // 64)), b"\x01\x02\x03", b"\x09", 2 if vbr else None)
    low = rng.integers(0, 256, 8 * codec.residual_plane_words(H, W, shift), dtype=np.uint8).tobytes()
    return dict(H=H, W=W, inner=inner, segs=segs, seg_bytes=seg_bytes, segment=L, tau=3, depth=depth, shift=shift,
                low=low, digest=0x0123456789ABCDEF, m=t["m"], freq=t["freq"], vbr=vbr)


@pytest.mark.parametrize("vbr", [False, True])
@pytest.mark.parametrize("depth,shift", [(9, 0), (10, 3), (16, 9)])
def test_container_round_trips(depth, shift, vbr):
    p = _parts(depth=depth, shift=shift, vbr=vbr)
    f = codec.write_container_residual_deep(**p)
    s = codec.parse_container_residual_deep(f, n_levels=6)
    assert f[:4] == b"MLR3" and codec.is_residual_deep_file(f) and not codec.is_residual_file(f)
    assert (s.H, s.W, s.tau, bool(s.vbr), s.digest, s.depth, s.shift) == (17, 70, 3, vbr, p["digest"], depth, shift)
    assert (s.seg_len, s.n_seg, s.lo_len) == (256, len(p["seg_bytes"]), len(p["low"]))
    assert f[s.inner_off:s.inner_off + s.inner_len] == p["inner"] == codec.strip_residual(f, n_levels=6)
    assert f[s.data_off:s.data_off + s.data_len] == p["segs"] and f[s.lo_off:s.lo_off + s.lo_len] == p["low"]
    assert np.array_equal(np.frombuffer(f, ">u4", s.n_seg, s.index_off), p["seg_bytes"])
    assert s.lo_off + s.lo_len == len(f) and list(s.m) == list(p["m"])
    d = codec.peek(f, n_levels=6)
    assert (d["depth"], d["shift"], d["low_bytes"], d["max_error"], d["segments"]) == (depth, shift, len(p["low"]), 3, s.n_seg)
    assert d["bytes"] == len(f) == d["base_bytes"] + d["residual_bytes"] + d["low_bytes"] + d["header_bytes"]


def test_container_refusals_each_have_their_own_message():
    p = _parts()
    f = codec.write_container_residual_deep(**p)
    s = codec.parse_container_residual_deep(f)
    ds = s.inner_off - 14
    put = lambda at, b: f[:at] + bytes(b) + f[at + len(b):]  # noqa: E731
    u32 = lambda v: int(v).to_bytes(4, "big")  # noqa: E731
    cases = [(put(3, b"2"), "bad magic"), (put(4, [1]), "unknown version"), (put(5, [2]), "unknown flags"),
             (put(6, [128]), "tau above 127"), (put(7, [23]), "n_ctx is not 24"), (put(8, u32(0)), "H or W is zero"),
             (put(24, [64]), "an m outside 0..63"), (put(ds, [8]), "depth outside 9..16"), (put(ds, [17]), "depth outside 9..16"),
             (put(ds + 1, [4]), "shift outside 0..depth - 7"), (put(ds + 1, [2]), "lo_len is not"),
             (put(ds + 2, u32(255)), "seg_len outside 256..65536"), (put(ds + 6, u32(s.n_seg + 1)), "n_seg is not ceil"),
             (put(ds + 10, u32(0)), "an empty inner file"), (put(s.index_off, u32(6)), "not a multiple of 4"),
             (put(s.index_off, u32(4)), "a segment length below 8"),
             (put(s.index_off, u32(int(p["seg_bytes"][0]) + 4)), "not 4 n_seg + the segment lengths"),
             (put(s.lo_off - 4, u32(s.lo_len + 8)), "lo_len is not"), (f[:-1], "truncated inside the low-bit plane"),
             (f[:s.lo_off - 2], "truncated before the low-bit plane's length"), (f[:ds + 1], "truncated before depth, shift"),
             (f + b"\0", "bytes left over after the low-bit plane"), (f[:10], "truncated header")]
    seen = set()
    for bad, word in cases:
        with pytest.raises(_lib.MlicError, match="container_parse_residual_deep: .*" + re.escape(word)) as e:
            codec.parse_container_residual_deep(bad)
        seen.add(str(e.value).split(" [")[0])
    assert len(seen) == len({w for _, w in cases})
    with pytest.raises(_lib.MlicError, match="exceeds max_pixels"):
        codec.parse_container_residual_deep(f, max_pixels=17 * 70 - 1)
    for n in range(0, len(f), 7):  # truncations (the check program takes every byte)
        with pytest.raises(_lib.MlicError):
            codec.parse_container_residual_deep(f[:n])
    for kw, word in ((dict(depth=8), "depth outside 9..16"), (dict(shift=4), "shift outside 0..depth - 7"),
                     (dict(low=p["low"] + bytes(8)), "lo_len is not"), (dict(tau=128), "tau above 127")):
        with pytest.raises(_lib.MlicError, match="container_write_residual_deep: " + re.escape(word)):
            codec.write_container_residual_deep(**{**p, **kw})


def test_the_other_parsers_refuse_an_mlr3_file_and_this_one_theirs():
    p = _parts()
    f = codec.write_container_residual_deep(**p)
    for parse in (codec.parse_container, codec.parse_container_residual, codec.parse_container_residual_seg,
                  codec.parse_container_scaled, codec.parse_container_layered, codec.parse_container_tiled,
                  lambda d: codec.parse_container(d, True, 6), lambda d: codec.parse_container_roi(d, 6)):
        with pytest.raises(_lib.MlicError):
            parse(f)
    seg = codec.write_container_residual_seg(p["H"], p["W"], p["inner"], p["segs"], p["seg_bytes"], 256, 3, 1, p["m"], p["freq"])
    for other in (seg, p["inner"]):
        with pytest.raises(_lib.MlicError, match="bad magic|truncated header"):
            codec.parse_container_residual_deep(other)
    assert codec.parse_container_residual_seg(seg).n_seg == len(p["seg_bytes"])  # the MLR2 parser is unchanged


def test_container_residual_deep_check_program_under_sanitizers(tmp_path):
    """tools/container_residual_deep_check.cpp with container.cpp and rans.cpp, AddressSanitizer + UBSan, as a
    stand-alone program (no sanitizer runtime comes near Python): the division, the bound, the split and the shift
    rule swept, and the parser on truncations at every byte and corrupted headers.  Skipped where the compiler
    cannot link the sanitizer runtimes."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed for the container's sanitizer check"
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run([cxx] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if p.returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed: " + p.stderr[-200:])
    exe = str(tmp_path / "container_residual_deep_check")
    csrc = os.path.join(ROOT, "mlic_amd", "csrc")
    cmd = [cxx, "-std=c++17", "-O1", "-g"] + san + [
           "-I" + csrc, os.path.join(ROOT, "tools", "container_residual_deep_check.cpp"),
           os.path.join(csrc, "container.cpp"), os.path.join(csrc, "rans.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-300:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("container_residual_deep_check ok"), \
        r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------ the entries' refusals
def test_device_entries_refuse_bad_arguments_before_any_gpu_call():
    """Every argument is checked before any HIP call: the device pointers (small fake addresses) are never
    dereferenced, and no GPU is needed."""
    p = lambda v: C.c_void_p(v)  # noqa: E731
    st = (C.c_int64 * 4)(3 * 8 * 4, 3 * 8, 3, 1)
    zero = (C.c_int64 * 4)(96, 24, 0, 1)

    def front(base=64, bs=st, x=128, xs=st, B=1, H=4, W=8, d=10, tau=0, s=2, ctx=256, cnt=512, dg=1024, sym=2048,
              lo=4096, hist=8192, me=16384, mq=32768, sq=65536):
        _lib.call("mlic_image_residual_front_u16", None, p(base), bs, p(x), xs, B, H, W, d, tau, s, p(ctx), p(cnt), p(dg),
                  p(sym), p(lo), p(hist), p(me), p(mq), p(sq))

    for kw, word in ((dict(base=None), "null base"), (dict(B=0), "B must be positive"), (dict(W=0), "H and W"),
                     (dict(d=8), "depth must be in 9..16"), (dict(d=17), "depth must be in 9..16"),
                     (dict(tau=128), "tau must be in 0..127"), (dict(bs=zero), "zero column or channel stride \\(base\\)"),
                     (dict(base=65), "base must be 2-byte aligned"), (dict(ctx=None), "null ctx"),
                     (dict(dg=1028), "digest 8-byte aligned"), (dict(xs=zero), "zero column or channel stride \\(x\\)"),
                     (dict(x=129), "x must be 2-byte aligned"), (dict(s=4), "shift must be in 0..depth - 7"),
                     (dict(s=-1), "shift must be in 0..depth - 7"), (dict(sym=None), "are all needed"),
                     (dict(mq=None), "are all needed"), (dict(lo=None), "lo_plane goes with a shift above 0"),
                     (dict(s=0), "lo_plane goes with a shift above 0"), (dict(lo=4100), "8-byte aligned"),
                     (dict(x=None), "go with x")):
        with pytest.raises(_lib.MlicError, match="image_residual_front_u16: .*" + word):
            front(**kw)

    def stats(base=64, x=128, B=1, d=10, tau=0, mq=32768, sq=65536):
        _lib.call("mlic_image_residual_stats_u16", None, p(base), st, p(x), st, B, 4, 8, d, tau, p(mq), p(sq))

    for kw, word in ((dict(x=None), "null x"), (dict(d=8), "depth must be"), (dict(mq=None), "null max_abs_q"),
                     (dict(sq=65540), "sum_abs_q 8-byte aligned"), (dict(tau=-1), "tau must be")):
        with pytest.raises(_lib.MlicError, match="image_residual_stats_u16: .*" + word):
            stats(**kw)

    def apply(base=64, sym=2048, lo=4096, B=1, d=10, tau=0, s=2, out=128, os_=st, ref=None, rs=None, sq=None, me=None,
              status=256):
        _lib.call("mlic_image_residual_apply_u16", None, p(base), st, p(sym), p(lo), B, 4, 8, d, tau, s, p(out), os_,
                  p(ref), rs, p(sq), p(me), p(status))

    for kw, word in ((dict(sym=None), "null sym"), (dict(out=None), "null out"), (dict(status=None), "null status"),
                     (dict(s=4), "shift must be"), (dict(lo=None), "lo_plane goes with"), (dict(os_=zero), "\\(out\\)"),
                     (dict(out=129), "2-byte"), (dict(ref=512), "ref without sq_err"), (dict(sq=1024), "go with ref"),
                     (dict(ref=512, sq=1024, me=2048), "ref needs strides"), (dict(d=20), "depth must be")):
        with pytest.raises(_lib.MlicError, match="image_residual_apply_u16: .*" + word):
            apply(**kw)


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


def _images(B, H, W, d, seed=5, noise=40):
    g = torch.Generator().manual_seed(seed)
    maxv = (1 << d) - 1
    smooth = torch.nn.functional.interpolate(torch.rand(B, 3, 5, 6, generator=g), size=(H, W), mode="bilinear")
    n = torch.randint(-noise, noise + 1, (B, 3, H, W), generator=g)
    return (smooth * maxv + n).clamp(0, maxv).to(torch.int32).to(torch.uint16).permute(0, 2, 3, 1).contiguous()


def _err(a, b):
    return (a.to(torch.int32) - b.to(torch.int32)).abs()


@pytest.mark.parametrize("vbr", [False, True])
@pytest.mark.parametrize("tau", [0, 3])
@pytest.mark.parametrize("d", [10, 16])
def test_cpu_path_end_to_end(d, tau, vbr):
    imgs, net = _images(3, 70, 100, d), StubNet(vbr)
    level = [1, 4, 2] if vbr else None
    files, info = codec.encode_residual16(net, imgs, d, max_error=tau, level=level, residual_segment=300,
                                          residual_coder="host", return_info=True)
    plain = codec.encode_images(net, imgs, level=level, depth=d)
    assert all(f[:4] == b"MLR3" for f in files) and [codec.strip_residual(f, n_levels=6) for f in files] == plain
    assert files == codec.encode_residual16(net, imgs, d, max_error=tau, level=level, residual_segment=300)
    n_seg = -(-3 * 70 * 100 // 300)
    for b, f in enumerate(files):
        pk = codec.peek(f, n_levels=6)
        assert info[b]["bytes"] == len(f) == info[b]["base_bytes"] + info[b]["residual_bytes"] + info[b]["low_bytes"] + pk["header_bytes"]
        assert (info[b]["max_error"], info[b]["depth"], info[b]["residual_segment"], info[b]["segments"]) == (tau, d, 300, n_seg)
        assert (pk["depth"], pk["shift"], pk["base_bytes"]) == (d, info[b]["shift"], len(plain[b]))
        assert info[b]["low_bytes"] == 8 * codec.residual_plane_words(70, 100, info[b]["shift"])
    base, _ = codec.decode_images(net, plain, depth=d)
    for coder in ("device", "host"):  # "device" on a CPU model falls to the host entry
        out, dinfo = codec.decode_images(net, files, ref=imgs, residual_coder=coder)
        err = _err(out, imgs)
        assert out.dtype == torch.uint16 and int(err.max()) <= tau and (tau > 0 or torch.equal(out, imgs))
        for b in range(3):
            assert dinfo[b]["max_abs_err"] == int(err[b].max()) and dinfo[b]["max_error"] == tau
            assert dinfo[b]["sq_err"] == int((err[b].to(torch.int64) ** 2).sum()) and dinfo[b]["depth"] == d
            assert dinfo[b]["psnr"] == codec.psnr_from_sq_err(dinfo[b]["sq_err"], 3 * 70 * 100, (1 << d) - 1)
            # the shift is the rule's, from the statistics of the image against its base
            st = codec.residual_stats16(base[b], imgs[b], d, tau)
            assert dinfo[b]["shift"] == orc.shift_rule(d, 3 * 70 * 100, int(st["max_abs_q"][0]), int(st["sum_abs_q"][0]))
    assert torch.equal(codec.decode_images(net, files, depth=d)[0], out)
    only, oinfo = codec.decode_images(net, files, enhance=False)
    assert torch.equal(only, base) and oinfo[0]["enhanced"] is False and oinfo[0]["depth"] == d
    single = [codec.encode_residual16(net, imgs[b], d, max_error=tau, level=level and level[b], residual_segment=300)[0]
              for b in range(3)]
    assert single == files


def test_explicit_shift_and_mixed_files_in_one_decode():
    net = StubNet()
    a, b = _images(1, 70, 100, 12), _images(1, 100, 75, 10, seed=6)
    c = _images(1, 70, 100, 12, seed=9, noise=3)
    auto, info = codec.encode_residual16(net, a, 12, return_info=True)
    s0 = info[0]["shift"]
    base, _ = codec.decode_images(net, codec.encode_images(net, a, depth=12), depth=12)
    smin = codec.residual_min_shift(12, int(codec.residual_stats16(base, a, 12, 0)["max_abs_q"][0]))
    assert 1 <= smin <= s0
    other = next(s for s in range(smin, 6) if s != s0)  # any shift that fits may be asked for
    fa = codec.encode_residual16(net, a, 12, shift=other, residual_segment=300)[0]
    assert codec.peek(fa)["shift"] == other and fa != auto[0]
    with pytest.raises(ValueError, match=rf"encode_residual16: shift=0 does not fit image 0 .*the smallest shift that fits is {smin}$"):
        codec.encode_residual16(net, a, 12, shift=0)
    fb = codec.encode_residual16(net, b, 10, max_error=2)[0]
    fc = codec.encode_residual16(net, c, 12, max_error=1)[0]
    out, dinfo = codec.decode_images(net, [fa, auto[0], fc])  # one size and depth; shift, tau and segment differ
    assert torch.equal(out[0], a[0]) and torch.equal(out[1], a[0]) and int(_err(out[2], c[0]).max()) <= 1
    assert [d["shift"] for d in dinfo[:2]] == [other, s0] and dinfo[2]["max_error"] == 1
    out, dinfo = codec.decode_images(net, [fa, fb])  # two depths and sizes: each in the top-left of one canvas
    assert tuple(out.shape) == (2, 100, 100, 3) and [d["depth"] for d in dinfo] == [12, 10]
    assert torch.equal(out[0, :70, :100], a[0]) and int(_err(out[1, :100, :75], b[0]).max()) <= 2


def test_refusals_by_name():
    net = StubNet()
    imgs = _images(2, 64, 64, 10)
    files = codec.encode_residual16(net, imgs, 10, max_error=1)
    plain = codec.encode_images(net, imgs, depth=10)
    u8 = (imgs.to(torch.int32) >> 2).to(torch.uint8)
    seg = codec.encode_images(net, u8, max_error=1, residual_segment=256)
    for kw, word in ((dict(slices=2), "slices="), (dict(out_size=(32, 32)), "out_size="), (dict(filter="bicubic"), "filter="),
                     (dict(depth=10, msb=True), "msb=True")):
        with pytest.raises(ValueError, match=rf"decode_images: {word} on a residual file \(MLR3\) is not supported"):
            codec.decode_images(net, files, **kw)
    for other in (plain, seg):
        with pytest.raises(ValueError, match=r"deep residual files \(MLR3\) and other files in one call"):
            codec.decode_images(net, [files[0], other[1]])
    with pytest.raises(ValueError, match=r"decode_images: depth=12, but file 0 \(MLR3\) holds samples of depth 10"):
        codec.decode_images(net, files, depth=12)
    with pytest.raises(ValueError, match="model is variable-rate"):
        codec.decode_images(StubNet(True), files)
    with pytest.raises(ValueError, match=r"ref must be uint16 \(2, 64, 64, 3\)"):
        codec.decode_images(net, files, ref=imgs[:, :32])
    for kw, word in ((dict(depth=8), "depth must be an integer in \\[9, 16\\]"), (dict(max_error=128), "max_error must be"),
                     (dict(shift=4), "shift must be an integer in \\[0, depth - 7 = 3\\]"),
                     (dict(residual_segment=100), "residual_segment must be"), (dict(residual_coder="gpu"), "residual_coder must be")):
        with pytest.raises(ValueError, match="encode_residual16: " + word):
            codec.encode_residual16(net, imgs, **{"depth": 10, **kw})
    with pytest.raises(ValueError, match="uint16 tensor or array expected"):
        codec.encode_residual16(net, u8, 10)
    # a corrupt file: the digest, a padding bit, a segment -- each refused by a check
    f = files[1]
    s = codec.parse_container_residual_deep(f)
    with pytest.raises(RuntimeError, match="the digest of the decoded base image"):
        codec.decode_images(net, [files[0], f[:16] + bytes([f[16] ^ 1]) + f[17:]])
    big = codec.encode_residual16(net, _images(1, 64, 100, 10), 10, shift=2)[0]
    sb = codec.parse_container_residual_deep(big)
    at = sb.lo_off + 8 * 2 + 7  # row 0, group 1 (36 columns), bit plane 0, bits 56..63
    with pytest.raises(ValueError, match="file 0: the low-bit plane has bits set beyond column 100"):
        codec.decode_images(net, [big[:at] + bytes([big[at] | 0x80]) + big[at + 1:]])
    lens = np.frombuffer(f, ">u4", s.n_seg, s.index_off)
    at = s.data_off + int(lens[:2].sum()) + int(lens[2]) // 2
    with pytest.raises(ValueError, match="decode_images: file 1: segment 2 of the residual string is corrupt"):
        codec.decode_images(net, [files[0], f[:at] + bytes([f[at] ^ 0x08]) + f[at + 1:]])


def test_the_8_bit_entry_points_keep_refusing_deep_samples():
    net = StubNet()
    imgs = _images(1, 64, 64, 10)
    with pytest.raises(ValueError, match=r"encode_images: max_error= \(residual coding\) together with depth= is not supported"):
        codec.encode_images(net, imgs, depth=10, max_error=0)
    assert "encode_residual16" in codec.encode_images.__doc__
