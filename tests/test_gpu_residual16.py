"""Residual coding of 9..16-bit samples on the GPU (needs a MI355X: `-m gpu`): the kernels of csrc/residual16.hip
against tests/residual16_oracle.py, bit for bit, and "MLR3" files end to end through the codec.

Everything is integer, so every comparison is equality.  Sizes (H x W): 1 x 1; 3 x 64 (exactly one 64-column group);
19 x 261 (two column tiles, the last 5 wide; three row groups, the last short); 67 x 70 (crosses a block's 64 rows,
a partial 64-column group); 9 x 320.  Depths 9, 10, 12, 16; tau 0, 1, 127; shifts 0, the smallest that fits and
depth - 7.  Two kinds of picture: "random" (full-range words, some above maxv where the depth leaves room: large q,
saturated symbols at shift 0) and "near" (a ramp and a noisy copy: small q).  Dense HWC, dense CHW and a strided view
must give the same outputs.  The test switch MLIC_POISON pre-fills every output, so an unwritten word fails the
comparison."""
import ctypes as C

import numpy as np
import pytest
import torch

import residual16_oracle as orc
from mlic_amd import _lib, codec, get_model, synthetic

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SIZES = [(1, 1), (3, 64), (19, 261), (67, 70), (9, 320)]
DEPTHS = [9, 10, 12, 16]
TAUS = [0, 1, 127]
_NETS = {}
_PICS = {}
_ORACLE = {}
_CODED = {}


@pytest.fixture(autouse=True)
def _no_range_fallbacks(request):
    yield
    hit = {k: n.range_fallbacks(reset=True) for k, n in _NETS.items()}
    hit = {k: v for k, v in hit.items() if any(v.values())}
    assert not hit, (request.node.name, hit)


def net_for(name):
    if name not in _NETS:
        n = get_model(name)
        n.load_state_dict(synthetic.synth_state_dict(name, rate=1))
        n = n.to(DEV).eval()
        n.update()
        _NETS[name] = n
    return _NETS[name]


# ------------------------------------------------------------------------------------------ 1. kernels
def pictures(H, W, d):
    """{kind: (base, x)} uint16 numpy [H,W,3], shared and changed by none."""
    key = (H, W, d)
    if key not in _PICS:
        rng = np.random.default_rng(100000 * d + 1000 * H + W)
        maxv = (1 << d) - 1
        top = min(65535, maxv + 40)  # words above maxv read as maxv
        rb = rng.integers(0, top + 1, (H, W, 3)).astype(np.uint16)
        rx = rng.integers(0, top + 1, (H, W, 3)).astype(np.uint16)
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        ramp = np.stack([(yy * (37 << (d - 8)) // 5 + xx * (11 << (d - 8)) // 3 + (c << (d - 3))) % (maxv + 1) for c in range(3)], -1)
        near = np.clip(ramp + rng.integers(-300, 301, ramp.shape), 0, maxv)
        _PICS[key] = {"random": (rb, rx), "near": (ramp.astype(np.uint16), near.astype(np.uint16))}
    return _PICS[key]


def samples(a, d):
    return np.minimum(a.astype(np.int64), (1 << d) - 1).transpose(2, 0, 1)


def oracle(H, W, d, kind, tau, s):
    key = (H, W, d, kind, tau, s)
    if key not in _ORACLE:
        base, x = pictures(H, W, d)[kind]
        _ORACLE[key] = orc.front(samples(base, d), samples(x, d), d, tau, s)
    return _ORACLE[key]


def forms(a):
    """One [B,H,W,3] uint16 numpy batch as (tensor, layout): dense HWC, dense CHW, a strided HWC view."""
    B, H, W, _ = a.shape
    hwc = torch.from_numpy(a.copy()).to(DEV)
    chw = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2))).to(DEV)
    big = np.full((B, H + 2, W + 3, 4), 0xBEEF, np.uint16)
    big[:, 1:H + 1, 2:W + 2, :3] = a
    view = torch.from_numpy(big).to(DEV)[:, 1:H + 1, 2:W + 2, :3]
    assert view.stride(2) == 4 and view.stride(1) == 4 * (W + 3)  # neither the HWC nor the CHW form
    return [(hwc, "hwc"), (chw, "chw"), (view, "hwc")]


def shifts_of(d, max_abs_q):
    return sorted({0, codec.residual_min_shift(d, max_abs_q), d - 7})


def check_front(out, want, b=0, with_x=True):
    assert np.array_equal(out["ctx"][b].cpu().numpy(), want["ctx"])
    assert np.array_equal(out["ctx_count"][b].cpu().numpy(), want["ctx_count"])
    assert int(out["digest"][b]) & orc.MASK == want["digest"]
    if with_x:
        assert np.array_equal(out["sym"][b].cpu().numpy(), want["sym"])
        assert np.array_equal(out["plane"][b].cpu().numpy().view(np.uint64), want["plane"])
        assert np.array_equal(out["hist"][b].cpu().numpy(), want["hist"])
        assert int(out["max_err"][b]) == want["max_err"] <= 127
        assert int(out["max_abs_q"][b]) == want["max_abs_q"] and int(out["sum_abs_q"][b]) == want["sum_abs_q"]


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("d", DEPTHS)
@pytest.mark.parametrize("H,W", SIZES)
def test_front_and_stats_match_the_oracle_in_every_layout(H, W, d, tau):
    for kind, (base, x) in pictures(H, W, d).items():
        mq = oracle(H, W, d, kind, tau, 0)["max_abs_q"]
        bf, xf = forms(base[None]), forms(x[None])
        for s in shifts_of(d, mq):
            want = oracle(H, W, d, kind, tau, s)
            assert want["max_err"] <= tau
            for (bt, bl), (xt, xl) in zip(bf, (xf[1], xf[2], xf[0])):  # every base form, every x form
                out = codec.residual_front16(bt, xt, d, tau, s, bl, xl)
                check_front(out, want)
        for (bt, bl), (xt, xl) in zip(bf, xf):
            st = codec.residual_stats16(bt, xt, d, tau, bl, xl)
            assert int(st["max_abs_q"][0]) == mq and int(st["sum_abs_q"][0]) == want["sum_abs_q"]
            check_front(codec.residual_front16(bt, None, d, tau, 0, bl), want, with_x=False)


@pytest.mark.parametrize("d", DEPTHS)
@pytest.mark.parametrize("H,W", SIZES)
def test_apply_matches_the_oracle_with_and_without_ref_and_into_a_strided_out(H, W, d):
    for tau in TAUS:
        for kind, (base, x) in pictures(H, W, d).items():
            mq = oracle(H, W, d, kind, tau, 0)["max_abs_q"]
            s = codec.residual_min_shift(d, mq)  # the smallest shift whose symbols the apply pass accepts
            for s in sorted({s, d - 7}):
                want = oracle(H, W, d, kind, tau, s)
                sym = torch.from_numpy(want["sym"][None]).to(DEV)
                plane = torch.from_numpy(want["plane"].view(np.int64)[None].copy()).to(DEV)
                xf = forms(x[None])
                rec = want["rec"].transpose(1, 2, 0)
                dd = want["rec"] - samples(x, d)
                for bt, bl in forms(base[None]):
                    out = codec.residual_apply16(bt, sym, plane, d, tau, s, bl)
                    got = out[0].cpu().numpy() if bl == "hwc" else out[0].cpu().numpy().transpose(1, 2, 0)
                    assert np.array_equal(got, rec)
                    ref = xf[1][0] if bl == "chw" else xf[2][0]  # CHW beside CHW, a strided view beside HWC
                    out, sq, me = codec.residual_apply16(bt, sym, plane, d, tau, s, bl, ref=ref)
                    got = out[0].cpu().numpy() if bl == "hwc" else out[0].cpu().numpy().transpose(1, 2, 0)
                    assert np.array_equal(got, rec)
                    assert int(sq[0]) == int((dd * dd).sum()) and int(me[0]) == int(np.abs(dd).max()) <= tau
                # into a window of a poisoned canvas: only the image's words change
                canvas = torch.full((1, H + 3, W + 5, 4), 0x7ABC, dtype=torch.int16, device=DEV)
                win = canvas.view(torch.uint16)[:, 2:H + 2, 1:W + 1, :3]
                codec.residual_apply16(forms(base[None])[0][0], sym, plane, d, tau, s, "hwc", out=win)
                c = canvas.cpu().numpy().view(np.uint16)
                assert np.array_equal(c[0, 2:H + 2, 1:W + 1, :3], rec)
                c[0, 2:H + 2, 1:W + 1, :3] = 0x7ABC
                assert (c == 0x7ABC).all()


def test_apply_refuses_a_symbol_outside_255_through_the_status_word():
    H, W, d = 19, 261, 12
    base, x = pictures(H, W, d)["near"]
    want = oracle(H, W, d, "near", 0, 5)
    for v in (256, -256, 32767):
        sym = want["sym"][None].repeat(3, 0).copy()
        sym[1, 2, 18, 260] = v
        b3 = torch.from_numpy(base[None].repeat(3, 0)).to(DEV)
        plane = torch.from_numpy(want["plane"].view(np.int64)[None].repeat(3, 0)).to(DEV)
        with pytest.raises(ValueError, match=r"residual_apply16: image 1 holds a symbol outside \[-255, 255\]"):
            codec.residual_apply16(b3, torch.from_numpy(sym).to(DEV), plane, d, 0, 5, "hwc")


@pytest.mark.parametrize("H,W", [(19, 261), (67, 70)])
def test_a_batch_gives_the_bits_of_one_image_at_a_time_and_repeats(H, W):
    d, tau, s = 12, 1, 5
    rng = np.random.default_rng(7)
    base = rng.integers(0, 4096, (3, H, W, 3)).astype(np.uint16)
    x = rng.integers(0, 4096, (3, H, W, 3)).astype(np.uint16)
    bt, xt = torch.from_numpy(base).to(DEV), torch.from_numpy(x).to(DEV)
    first = codec.residual_front16(bt, xt, d, tau, s, "hwc")
    again = codec.residual_front16(bt, xt, d, tau, s, "hwc")
    for k in first:
        assert torch.equal(first[k], again[k]), k
    for b in range(3):
        one = codec.residual_front16(bt[b:b + 1], xt[b:b + 1], d, tau, s, "hwc")
        for k in first:
            assert torch.equal(first[k][b:b + 1], one[k]), (k, b)
        check_front(first, orc.front(samples(base[b], d), samples(x[b], d), d, tau, s), b)
    out = codec.residual_apply16(bt, first["sym"], first["plane"], d, tau, s, "hwc", ref=xt)
    for b in range(3):
        o1 = codec.residual_apply16(bt[b:b + 1], first["sym"][b:b + 1], first["plane"][b:b + 1], d, tau, s, "hwc",
                                    ref=xt[b:b + 1])
        assert np.array_equal(out[0][b:b + 1].cpu().numpy(), o1[0].cpu().numpy())
        assert int(out[1][b]) == int(o1[1][0]) and int(out[2][b]) == int(o1[2][0])


def test_front_writes_nothing_outside_its_outputs():
    """The C entry on buffers with a guard behind every output: the guards keep their poison."""
    H, W, d, tau, s, B, G = 19, 261, 10, 1, 3, 2, 64
    rng = np.random.default_rng(11)
    base = torch.from_numpy(rng.integers(0, 1024, (B, H, W, 3)).astype(np.uint16)).to(DEV)
    x = torch.from_numpy(rng.integers(0, 1024, (B, H, W, 3)).astype(np.uint16)).to(DEV)
    n = 3 * H * W
    sizes = {"ctx": (torch.uint8, B * n), "count": (torch.int32, B * 24), "digest": (torch.int64, B),
             "sym": (torch.int16, B * n), "plane": (torch.int64, B * codec.residual_plane_words(H, W, s)),
             "hist": (torch.int32, B * 24 * 128), "merr": (torch.int32, B), "mq": (torch.int32, B), "sq": (torch.int64, B)}
    buf = {k: torch.full((cnt + G,), 0x5A, dtype=dt, device=DEV) for k, (dt, cnt) in sizes.items()}
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = (C.c_int64 * 4)(*codec._strides(base, "hwc"))
    _lib.call("mlic_image_residual_front_u16", codec._stream(), p(base), st, p(x), st, B, H, W, d, tau, s, p(buf["ctx"]),
              p(buf["count"]), p(buf["digest"]), p(buf["sym"]), p(buf["plane"]), p(buf["hist"]), p(buf["merr"]),
              p(buf["mq"]), p(buf["sq"]))
    torch.cuda.synchronize()
    want = codec.residual_front16(base, x, d, tau, s, "hwc")
    for k, (dt, cnt) in sizes.items():
        assert bool((buf[k][cnt:] == 0x5A).all()), k
    assert torch.equal(buf["sym"][:B * n].view(B, 3, H, W), want["sym"])
    assert torch.equal(buf["plane"][:sizes["plane"][1]].view(B, -1), want["plane"])
    assert torch.equal(buf["ctx"][:B * n].view(B, 3, H, W), want["ctx"])


# ------------------------------------------------------------------------------------------ 2. end to end
E2E_DEPTHS = (10, 16)
E2E_TAUS = (0, 2)
H2, W2 = 75, 100


def _images16(B, d, seed=80):
    x = torch.cat([synthetic.synth_image(H2, W2, seed + i) for i in range(B)])
    return (x * ((1 << d) - 1)).round().clamp(0, (1 << d) - 1).to(torch.int32).to(torch.uint16).permute(0, 2, 3, 1).contiguous()


def coded(d):
    """Per depth, shared and changed by none: two images, their plain files, and per tau the "MLR3" files from the
    device and from the host coder."""
    if d not in _CODED:
        net = net_for("MLICPP_S")
        imgs = _images16(2, d)
        plain = codec.encode_images(net, imgs, depth=d)
        res = {}
        for tau in E2E_TAUS:
            dev = codec.encode_residual16(net, imgs, d, max_error=tau, residual_segment=256, return_info=True)
            host = codec.encode_residual16(net, imgs, d, max_error=tau, residual_segment=256, residual_coder="host")
            res[tau] = (dev[0], dev[1], host)
        _CODED[d] = (net, imgs, plain, res)
    return _CODED[d]


@pytest.mark.parametrize("d", E2E_DEPTHS)
def test_files_round_trip_within_the_bound_and_device_and_host_coders_agree(d):
    net, imgs, plain, res = coded(d)
    for tau in E2E_TAUS:
        files, info, host = res[tau]
        assert files == host and all(f[:4] == b"MLR3" and codec.is_residual_deep_file(f) for f in files)
        assert [codec.strip_residual(f) for f in files] == plain
        for coder in ("device", "host"):
            out, dinfo = codec.decode_images(net, files, ref=imgs, residual_coder=coder)
            assert out.dtype == torch.uint16 and tuple(out.shape) == (2, H2, W2, 3)
            err = (out.cpu().to(torch.int32) - imgs.to(torch.int32)).abs()
            assert int(err.max()) <= tau and (tau or torch.equal(out.cpu(), imgs)), (tau, coder, int(err.max()))
            for b in range(2):
                assert dinfo[b]["max_abs_err"] == int(err[b].max()) and dinfo[b]["depth"] == d
                assert dinfo[b]["shift"] == info[b]["shift"] == codec.peek(files[b])["shift"]
                assert info[b]["bytes"] == len(files[b])


@pytest.mark.parametrize("d", E2E_DEPTHS)
def test_cpu_restatement_and_gpu_front_agree_on_the_real_base(d):
    net, imgs, plain, res = coded(d)
    base, _ = codec.decode_images(net, plain, depth=d)
    s = res[0][1][0]["shift"]
    gpu = codec.residual_front16(base, imgs.to(DEV), d, 0, s, "hwc")
    cpu = codec.residual_front16(base.cpu(), imgs, d, 0, s, "hwc")
    assert set(gpu) == set(cpu)
    for k in gpu:
        assert torch.equal(gpu[k].cpu(), cpu[k]), k
    a = codec.residual_apply16(base, gpu["sym"], gpu["plane"], d, 0, s, "hwc")
    assert torch.equal(a.cpu(), imgs)
    assert torch.equal(codec.residual_apply16(base.cpu(), cpu["sym"], cpu["plane"], d, 0, s, "hwc"), imgs)


def test_corrupt_files_are_refused_by_checks():
    d = 10
    net, imgs, plain, res = coded(d)
    files = res[2][0]
    f = files[1]
    # the digest
    bad = f[:16] + bytes([f[16] ^ 1]) + f[17:]
    with pytest.raises(RuntimeError, match="the digest of the decoded base image"):
        codec.decode_images(net, [files[0], bad])
    only, oinfo = codec.decode_images(net, [files[0], bad], enhance=False)
    want, _ = codec.decode_images(net, plain, depth=d)
    assert torch.equal(only.cpu(), want.cpu()) and oinfo[1]["enhanced"] is False
    # a padding bit of the low-bit plane (W = 100: the second group of a row has 36 columns)
    s = codec.parse_container_residual_deep(f)
    assert s.shift > 0
    at = s.lo_off + 8 * (1 * s.shift) + 7  # row 0, group 1, bit plane 0, byte 7: bits 56..63
    bad = f[:at] + bytes([f[at] | 0x80]) + f[at + 1:]
    with pytest.raises(ValueError, match="file 1: the low-bit plane has bits set beyond column 100"):
        codec.decode_images(net, [files[0], bad])
    # a segment
    lens = np.frombuffer(f, ">u4", s.n_seg, s.index_off)
    at = s.data_off + int(lens[:5].sum()) + int(lens[5]) // 2
    bad = f[:at] + bytes([f[at] ^ 0x08]) + f[at + 1:]
    for coder in ("device", "host"):
        with pytest.raises(ValueError, match="decode_images: file 1: segment 5 of the residual string is corrupt"):
            codec.decode_images(net, [files[0], bad], residual_coder=coder)
    t = codec._file_tables(f, s)
    ctx = codec.residual_front16(want[1:2], None, d, 2, 0, "hwc")["ctx"]
    with pytest.raises(codec.ResidualSegmentError) as e:
        codec.residual_decode_segments([bad[s.data_off:s.data_off + s.data_len]], [lens], ctx, t, 256)
    assert e.value.segment == 5 and e.value.image == 0
