"""Residual coding of Y'CbCr frames on the GPU (needs a MI355X: `-m gpu`): the kernels of csrc/residual_yuv.hip against
tests/residual_yuv_oracle.py, bit for bit, the segment coders for a given N, and "MLR4" files end to end.

Everything is integer, so every comparison is equality.  Luma sizes (H x W), each for a boundary: 1 x 1 (every plane a
single sample); 2 x 2; 3 x 64 (exactly one luma group, chroma 32); 19 x 261 (odd: ceil chroma 10 x 131, second column
tile 5 wide); 67 x 130 (crosses a block's rows; chroma 65, one group plus one); 9 x 514 (chroma 257: two tiles plus
one).  Subsampling 4:2:0, 4:2:2, 4:4:4; depth 8 (bytes), 10, 12, 16 and MSB alignment at depth 10; tau 0, 1, 127; above
depth 8 the shifts 0, the smallest that fits and depth - 7.  Two kinds of picture: "random" (full-range words, some
above maxv, luma outside 16..235 with full_range=False) and "near" (a ramp and a noisy copy).  Dense planar,
semi-planar (one interleaved CbCr buffer, NV12 and NV21 order) and pitched planes (rows padded by a poison value) must
give the same outputs.  The test switch MLIC_POISON pre-fills every output, so an unwritten word fails."""
import numpy as np
import pytest
import torch

import residual_yuv_oracle as orc
from mlic_amd import codec, get_model, synthetic
from mlic_amd.codec import YuvFormat

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SIZES = [(1, 1), (2, 2), (3, 64), (19, 261), (67, 130), (9, 514)]
SUBS = [(2, 2), (2, 1), (1, 1)]
DEPTHS = [(8, False), (10, False), (10, True), (12, False), (16, False)]  # (depth, msb)
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


def fmt_of(sub, d, msb):
    return YuvFormat(sub, "bt709", False, "left", d, msb)


# ------------------------------------------------------------------------------------------ 1. kernels
def pictures(H, W, sub, d, msb, seed=0):
    """{kind: (base, x)}: two lists of three word planes (numpy, the plane's type), shared and changed by none."""
    key = (H, W, sub, d, msb, seed)
    if key not in _PICS:
        rng = np.random.default_rng(1000003 * seed + 100000 * d + 1000 * H + W + 7 * sub[0] + sub[1] + 13 * msb)
        maxv = (1 << d) - 1
        hc, wc = orc.chroma_size(H, W, sub)
        shapes = [(H, W), (hc, wc), (hc, wc)]
        dt = np.uint8 if d == 8 else np.uint16
        top = 255 if d == 8 else 65535 if msb else min(65535, maxv + 40)  # LSB words above maxv read as maxv
        rnd = [[rng.integers(0, top + 1, s).astype(dt) for s in shapes] for _ in range(2)]
        near = [[], []]
        for p, (h, w) in enumerate(shapes):
            yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
            ramp = (yy * (37 << (d - 8)) // 5 + xx * (11 << (d - 8)) // 3 + (p << (d - 3))) % (maxv + 1)
            noisy = np.clip(ramp + rng.integers(-(3 << (d - 8)), (3 << (d - 8)) + 1, ramp.shape), 0, maxv)
            near[0].append(orc.words(ramp, d, msb))
            near[1].append(orc.words(noisy, d, msb))
        _PICS[key] = {"random": (rnd[0], rnd[1]), "near": (near[0], near[1])}
    return _PICS[key]


def smp(planes, d, msb):
    return [orc.samples(v, d, msb) for v in planes]


def oracle(H, W, sub, d, msb, kind, tau, s, seed=0):
    key = (H, W, sub, d, msb, kind, tau, s, seed)
    if key not in _ORACLE:
        base, x = pictures(H, W, sub, d, msb, seed)[kind]
        _ORACLE[key] = orc.front(smp(base, d, msb), smp(x, d, msb), d, tau, s)
    return _ORACLE[key]


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(DEV)


def _poison(d):
    return 0xA5 if d == 8 else 0xBEEF


def forms(planes, d):
    """Three word planes [B,h,w] (numpy) as four device forms: dense planar, NV12 (Cb Cr interleaved, column stride 2),
    NV21 (Cr Cb) and pitched views with poisoned padding.  -> [(name, (y, cb, cr))]."""
    y, cb, cr = planes
    B, hc, wc = cb.shape
    out = [("planar", tuple(_dev(v) for v in planes))]
    for name, order in (("nv12", (cb, cr)), ("nv21", (cr, cb))):
        uv = np.stack(order, -1)  # [B,hc,wc,2]
        t = _dev(uv)
        a, b = t[..., 0], t[..., 1]
        assert a.stride(2) == 2 and b.data_ptr() - a.data_ptr() == t.element_size()
        out.append((name, (_dev(y), a, b) if name == "nv12" else (_dev(y), b, a)))
    pitched = []
    for v in planes:
        _, h, w = v.shape
        big = np.full((B, h + 1, w + 5), _poison(d), v.dtype)
        big[:, :h, 3:w + 3] = v
        pitched.append(_dev(big)[:, :h, 3:w + 3])
    out.append(("pitched", tuple(pitched)))
    return out


def shifts_of(d, max_abs_q):
    return [0] if d == 8 else sorted({0, codec.residual_min_shift(d, max_abs_q), d - 7})


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
    else:
        assert set(out) == {"ctx", "ctx_count", "digest"}


@pytest.mark.parametrize("d,msb", DEPTHS)
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("H,W", SIZES)
def test_front_and_stats_match_the_oracle_in_every_plane_form(H, W, sub, d, msb):
    fmt = fmt_of(sub, d, msb)
    assert orc.n_samples(H, W, sub) == codec.residual_yuv_samples(H, W, sub)
    for kind, (base, x) in pictures(H, W, sub, d, msb).items():
        bf = forms([v[None] for v in base], d)
        xf = forms([v[None] for v in x], d)
        xf = xf[1:] + xf[:1]  # every base form beside another x form
        for tau in TAUS:
            first = oracle(H, W, sub, d, msb, kind, tau, 0)
            mq = first["max_abs_q"]
            for s in shifts_of(d, mq):
                want = oracle(H, W, sub, d, msb, kind, tau, s)
                assert want["max_err"] <= tau
                assert want["plane"].size == codec.residual_yuv_plane_words(H, W, sub, s) == orc.plane_words(H, W, sub, s)
                for (bn, bt), (xn, xt) in zip(bf, xf):
                    check_front(codec.residual_front_yuv(bt, xt, fmt, tau, s), want)
            for (bn, bt), (xn, xt) in zip(bf, xf):
                st = codec.residual_stats_yuv(bt, xt, fmt, tau)
                assert int(st["max_abs_q"][0]) == mq and int(st["sum_abs_q"][0]) == first["sum_abs_q"], (bn, xn)
        for bn, bt in bf:
            check_front(codec.residual_front_yuv(bt, None, fmt, 0, 0), first, with_x=False)


def _plane_np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("d,msb", DEPTHS)
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("H,W", SIZES)
def test_apply_matches_the_oracle_with_ref_and_into_pitched_and_semi_planar_out(H, W, sub, d, msb):
    fmt = fmt_of(sub, d, msb)
    for tau in TAUS:
        for kind, (base, x) in pictures(H, W, sub, d, msb).items():
            mq = oracle(H, W, sub, d, msb, kind, tau, 0)["max_abs_q"]
            for s in ([0] if d == 8 else sorted({codec.residual_min_shift(d, mq), d - 7})):
                want = oracle(H, W, sub, d, msb, kind, tau, s)
                sym = _dev(want["sym"][None])
                plane = _dev(want["plane"].view(np.int64)[None].copy())
                rec_w = [orc.words(v, d, msb) for v in want["rec"]]
                dd = [r - v for r, v in zip(want["rec"], smp(x, d, msb))]
                ap = {"sq_err": [int((v * v).sum()) for v in dd], "max_err": max(int(np.abs(v).max()) for v in dd)}
                assert ap["max_err"] <= tau
                xf = forms([v[None] for v in x], d)
                for k, (bn, bt) in enumerate(forms([v[None] for v in base], d)):
                    out = codec.residual_apply_yuv(bt, sym, plane, fmt, tau, s)
                    assert all(np.array_equal(_plane_np(o[0]), r) for o, r in zip(out, rec_w)), (bn, kind, tau, s)
                    r = codec.residual_apply_yuv(bt, sym, plane, fmt, tau, s, ref=xf[(k + 1) % 4][1])
                    assert all(np.array_equal(_plane_np(o[0]), w) for o, w in zip(r[:3], rec_w))
                    assert r[3][0].cpu().tolist() == ap["sq_err"] and int(r[4][0]) == ap["max_err"]
                # out= into pitched and semi-planar destinations: the padding keeps its poison
                bt = forms([v[None] for v in base], d)[0][1]
                for name, dst in forms([np.full_like(v[None], _poison(d) & 0x7F7F) for v in base], d)[1:]:
                    keep = [t._base if t._base is not None else t for t in dst]
                    before = [t.cpu().numpy().copy() for t in keep]
                    codec.residual_apply_yuv(bt, sym, plane, fmt, tau, s, out=dst)
                    assert all(np.array_equal(_plane_np(o[0]), w) for o, w in zip(dst, rec_w)), name
                    if name == "pitched":
                        for t, b0, w in zip(keep, before, rec_w):
                            now = t.cpu().numpy()
                            h, ww = w.shape
                            now[0, :h, 3:ww + 3] = b0[0, :h, 3:ww + 3]
                            assert np.array_equal(now, b0), name


def test_apply_flags_a_symbol_outside_255_and_writes_base_there():
    H, W, sub, d, msb = 19, 261, (2, 2), 12, False
    fmt = fmt_of(sub, d, msb)
    base, x = pictures(H, W, sub, d, msb)["near"]
    want = oracle(H, W, sub, d, msb, "near", 0, 5)
    N = want["sym"].size
    b3 = tuple(_dev(v[None].repeat(3, 0)) for v in base)
    plane = _dev(want["plane"].view(np.int64)[None].repeat(3, 0))
    for v in (256, -256, 32767):
        sym = want["sym"][None].repeat(3, 0).copy()
        sym[1, N - 1] = v
        with pytest.raises(ValueError, match=r"residual_apply_yuv: frame 1 holds a symbol outside \[-255, 255\]"):
            codec.residual_apply_yuv(b3, _dev(sym), plane, fmt, 0, 5)
        # the status word and the planes, through out=: the flagged sample is base, the others rec
        out = tuple(torch.zeros_like(t.view(torch.int16)).view(torch.uint16) for t in b3)
        with pytest.raises(ValueError):
            codec.residual_apply_yuv(b3, _dev(sym), plane, fmt, 0, 5, out=out)
        torch.cuda.synchronize()
        ap = orc.apply(smp(base, d, msb), sym[1], want["plane"], d, 0, 5)
        assert ap["bad"] and int(ap["rec"][2][-1, -1]) == int(base[2][-1, -1])
        assert all(np.array_equal(_plane_np(o[1]), orc.words(r, d, msb)) for o, r in zip(out, ap["rec"]))


@pytest.mark.parametrize("H,W,sub", [(19, 261, (2, 2)), (67, 130, (2, 1))])
def test_a_batch_gives_the_bits_of_one_frame_at_a_time(H, W, sub):
    d, msb, tau, s = 12, False, 1, 5
    fmt = fmt_of(sub, d, msb)
    pics = [pictures(H, W, sub, d, msb, seed)["random" if seed != 1 else "near"] for seed in range(3)]
    base = [np.stack([p[0][k] for p in pics]) for k in range(3)]
    x = [np.stack([p[1][k] for p in pics]) for k in range(3)]
    bt, xt = tuple(_dev(v) for v in base), tuple(_dev(v) for v in x)
    first = codec.residual_front_yuv(bt, xt, fmt, tau, s)
    for b in range(3):
        one = codec.residual_front_yuv(tuple(t[b:b + 1] for t in bt), tuple(t[b:b + 1] for t in xt), fmt, tau, s)
        for k in first:
            assert torch.equal(first[k][b:b + 1], one[k]), (k, b)
        check_front(first, orc.front(smp([v[b] for v in base], d, msb), smp([v[b] for v in x], d, msb), d, tau, s), b)
    s2 = d - 7  # the random frames' symbols fit
    f2 = codec.residual_front_yuv(bt, xt, fmt, tau, s2)
    out = codec.residual_apply_yuv(bt, f2["sym"], f2["plane"], fmt, tau, s2, ref=xt)
    for b in range(3):
        o1 = codec.residual_apply_yuv(tuple(t[b:b + 1] for t in bt), f2["sym"][b:b + 1], f2["plane"][b:b + 1], fmt, tau,
                                      s2, ref=tuple(t[b:b + 1] for t in xt))
        assert all(np.array_equal(_plane_np(out[k][b]), _plane_np(o1[k][0])) for k in range(3))
        assert out[3][b].tolist() == o1[3][0].tolist() and int(out[4][b]) == int(o1[4][0]) <= tau


# --------------------------------------------------------------------------- identities with the existing kernels
def _rgb_planes(H, W, d, seed):
    rng = np.random.default_rng(seed)
    dt = np.uint8 if d == 8 else np.uint16
    return [rng.integers(0, 1 << d, (3, H, W)).astype(dt) for _ in range(2)]


def test_444_planes_give_the_rgb_kernels_outputs_at_depth_10_and_8():
    H, W = 19, 261
    base, x = _rgb_planes(H, W, 10, 5)
    fmt = fmt_of((1, 1), 10, False)
    s = 3
    got = codec.residual_front_yuv(tuple(_dev(base[c][None]) for c in range(3)),
                                   tuple(_dev(x[c][None]) for c in range(3)), fmt, 1, s)
    want = codec.residual_front16(_dev(base[None]), _dev(x[None]), 10, 1, s, "chw")
    for k in ("ctx", "sym"):
        assert torch.equal(got[k], want[k].reshape(1, -1)), k
    for k in ("ctx_count", "digest", "plane", "hist", "max_err", "max_abs_q", "sum_abs_q"):
        assert torch.equal(got[k], want[k]), k
    base, x = _rgb_planes(H, W, 8, 6)
    fmt = fmt_of((1, 1), 8, False)
    got = codec.residual_front_yuv(tuple(_dev(base[c][None]) for c in range(3)),
                                   tuple(_dev(x[c][None]) for c in range(3)), fmt, 2, 0)
    want = codec.residual_front(_dev(base[None]), _dev(x[None]), 2, "chw")
    for k in ("ctx", "sym"):
        assert torch.equal(got[k], want[k].reshape(1, -1)), k
    for k in ("ctx_count", "digest", "hist", "max_err"):
        assert torch.equal(got[k], want[k]), k


# ------------------------------------------------------------------------------------------ 2. segments
@pytest.mark.parametrize("L", [256, 4096])
def test_device_segment_coders_for_a_given_n_match_the_host_ones(L):
    H, W, sub, d, msb = 19, 261, (2, 2), 10, False
    want = oracle(H, W, sub, d, msb, "near", 0, 3)
    N = orc.n_samples(H, W, sub)
    assert want["sym"].size == N and N % 3 != 0  # not an RGB image's sample count
    sym, ctx = _dev(want["sym"][None]), _dev(want["ctx"][None])
    tabs = [codec.residual_tables(want["hist"])]
    dev = codec.residual_encode_segments(sym, ctx, tabs, L, "device")
    host = codec.residual_encode_segments(sym, ctx, tabs, L, "host")
    assert dev[0][0] == host[0][0] and np.array_equal(dev[0][1], host[0][1])
    assert len(dev[0][1]) == -(-N // L)
    for coder in ("device", "host"):
        back = codec.residual_decode_segments([dev[0][0]], [dev[0][1]], ctx, tabs, L, coder)
        assert tuple(back.shape) == (1, N) and np.array_equal(back[0].cpu().numpy(), want["sym"])
    k = len(dev[0][1]) - 1
    at = int(dev[0][1][:k].sum()) + int(dev[0][1][k]) // 2
    bad = dev[0][0][:at] + bytes([dev[0][0][at] ^ 0x08]) + dev[0][0][at + 1:]
    for coder in ("device", "host"):
        with pytest.raises(codec.ResidualSegmentError) as e:
            codec.residual_decode_segments([bad], [dev[0][1]], ctx, tabs, L, coder)
        assert e.value.segment == k and e.value.image == 0 and f"segment {k}" in str(e.value)


# ------------------------------------------------------------------------------------------ 3. end to end
H2, W2 = 70, 66
E2E = {"i420": ("i420", YuvFormat((2, 2), "bt709", False, "left", 8)),
       "nv12": ("nv12", YuvFormat((2, 2), "bt601", True, "centre", 8)),
       "i422p10": ("i422", YuvFormat((2, 1), "bt709", False, "left", 10)),
       "p010": ("nv12", YuvFormat((2, 2), "bt2020", False, "left", 10, True))}
E2E_TAUS = (0, 2)


def _frames(name, B=2):
    """B raw frame buffers [B, samples] of synthetic pictures in the format's layout, through the project's egress."""
    layout, fmt = E2E[name]
    x = torch.cat([synthetic.synth_image(H2, W2, 90 + i) for i in range(B)])
    y, cb, cr = codec.egress_yuv(x.float(), H2, W2, fmt)  # the CPU restatement
    n = codec.yuv_frame_samples(H2, W2, layout)
    buf = np.zeros((B, n), np.uint8 if fmt.depth == 8 else np.uint16)
    py, pcb, pcr = codec.split_yuv(buf, H2, W2, layout, fmt.depth)
    py[...], pcb[...], pcr[...] = y.numpy(), cb.numpy(), cr.numpy()
    if fmt.depth == 8 and not fmt.full_range:
        py[:, 0, :8] = [0, 1, 15, 236, 254, 255, 3, 250]  # samples outside the legal range come back exactly
    return buf


def coded(name):
    if name not in _CODED:
        layout, fmt = E2E[name]
        net = net_for("MLICPP_S")
        buf = _frames(name)
        planes = codec.split_yuv(buf, H2, W2, layout, fmt.depth)
        plain = codec.encode_yuv(net, *planes, fmt)
        res = {}
        for tau in E2E_TAUS:
            dev = codec.encode_residual_yuv(net, *planes, fmt, max_error=tau, residual_segment=256, return_info=True)
            host = codec.encode_residual_yuv(net, *planes, fmt, max_error=tau, residual_segment=256,
                                             residual_coder="host")
            res[tau] = (dev[0], dev[1], host)
        _CODED[name] = (net, fmt, planes, plain, res)
    return _CODED[name]


def _np16(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("name", list(E2E))
def test_files_round_trip_within_the_bound_and_coders_and_batches_agree(name):
    net, fmt, planes, plain, res = coded(name)
    for tau in E2E_TAUS:
        files, info, host = res[tau]
        assert files == host and all(f[:4] == b"MLR4" and codec.is_residual_yuv_file(f) for f in files)
        assert [codec.strip_residual(f) for f in files] == plain
        out, dinfo = codec.decode_yuv(net, files, fmt, ref=planes)
        for o, p in zip(out, planes):
            assert o.dtype == fmt.dtype and tuple(o.shape) == tuple(p.shape)
            got, src = _np16(o).astype(np.int64), np.asarray(p).astype(np.int64)
            if fmt.msb:
                assert not (got & ((1 << (16 - fmt.depth)) - 1)).any()  # the low bits of MSB-aligned words are zero
                got, src = got >> (16 - fmt.depth), src >> (16 - fmt.depth)
            err = np.abs(got - src)
            assert err.max() <= tau and (tau or np.array_equal(got, src)), (name, tau, int(err.max()))
        for b in range(2):
            assert dinfo[b]["max_abs_err"] <= tau and dinfo[b]["depth"] == fmt.depth and dinfo[b]["sub"] == fmt.sub
            assert (dinfo[b]["sq_err"] == [0, 0, 0]) if tau == 0 else True
            assert info[b]["bytes"] == len(files[b]) and info[b]["sub"] == fmt.sub and info[b]["depth"] == fmt.depth
            pk = codec.peek(files[b])
            assert pk["residual"] and (pk["H"], pk["W"]) == (H2, W2) and pk["max_error"] == tau
            assert pk["depth"] == fmt.depth and pk["shift"] == info[b]["shift"] == dinfo[b]["shift"]
            assert pk["sub"] == fmt.sub and pk["matrix"] == fmt.matrix and pk["full_range"] == fmt.full_range
            assert pk["site_x"] == fmt.site_x and pk["segments"] == info[b]["segments"]
            assert pk["low_bytes"] == info[b]["low_bytes"] and pk["base_bytes"] == len(plain[b])
            one = codec.encode_residual_yuv(net, *(p[b:b + 1] for p in planes), fmt, max_error=tau, residual_segment=256)
            assert one[0] == files[b]


@pytest.mark.parametrize("name", ["i420", "p010"])
def test_enhance_false_is_the_plain_decode_and_corrupt_or_mismatched_files_are_refused(name):
    net, fmt, planes, plain, res = coded(name)
    files = res[2][0]
    want, _ = codec.decode_yuv(net, plain, fmt)
    only, oinfo = codec.decode_yuv(net, files, fmt, enhance=False)
    strip, _ = codec.decode_yuv(net, [codec.strip_residual(f) for f in files], fmt)
    for a, b, c in zip(only, want, strip):
        assert np.array_equal(_np16(a), _np16(b)) and np.array_equal(_np16(a), _np16(c))
    assert oinfo[0]["enhanced"] is False
    f = files[1]
    bad = f[:16] + bytes([f[16] ^ 1]) + f[17:]
    with pytest.raises(RuntimeError, match="the digest of the decoded base image"):
        codec.decode_yuv(net, [files[0], bad], fmt)
    s = codec.parse_container_residual_yuv(f)
    other = {"depth": YuvFormat(fmt.sub, "bt709", fmt.full_range, fmt.site_x, 12 if fmt.depth == 10 else 10),
             "sub": YuvFormat((2, 1), fmt.matrix, fmt.full_range, fmt.site_x, fmt.depth, fmt.msb),
             "matrix": YuvFormat(fmt.sub, "bt601", fmt.full_range, fmt.site_x, fmt.depth, fmt.msb),
             "full_range": YuvFormat(fmt.sub, fmt.matrix, not fmt.full_range, fmt.site_x, fmt.depth, fmt.msb),
             "site_x": YuvFormat(fmt.sub, fmt.matrix, fmt.full_range, "centre", fmt.depth, fmt.msb)}
    for field, wrong in other.items():
        with pytest.raises(ValueError, match=rf"decode_yuv: file 0 \(MLR4\) was written with {field}="):
            codec.decode_yuv(net, files, wrong)
    with pytest.raises(ValueError, match="residual \\(MLR4\\) and plain files cannot be mixed"):
        codec.decode_yuv(net, [files[0], plain[1]], fmt)
    with pytest.raises(ValueError, match="decode_yuv decodes it"):
        codec.decode_images(net, files)
    # a segment
    lens = np.frombuffer(f, ">u4", s.n_seg, s.index_off)
    at = s.data_off + int(lens[:5].sum()) + int(lens[5]) // 2
    bad = f[:at] + bytes([f[at] ^ 0x08]) + f[at + 1:]
    for coder in ("device", "host"):
        with pytest.raises(ValueError, match="decode_yuv: file 1: segment 5 of the residual string is corrupt"):
            codec.decode_yuv(net, [files[0], bad], fmt, residual_coder=coder)


def test_cpu_restatement_and_gpu_kernels_agree_on_the_real_base():
    net, fmt, planes, plain, res = coded("p010")
    base, _ = codec.decode_yuv(net, plain, fmt)
    x = tuple(torch.from_numpy(np.ascontiguousarray(p)) for p in planes)
    s = res[0][1][0]["shift"]
    gpu = codec.residual_front_yuv(base, tuple(t.to(DEV) for t in x), fmt, 0, s)
    cpu = codec.residual_front_yuv(tuple(t.cpu() for t in base), x, fmt, 0, s)
    assert set(gpu) == set(cpu)
    for k in gpu:
        assert torch.equal(gpu[k].cpu(), cpu[k]), k
    a = codec.residual_apply_yuv(base, gpu["sym"], gpu["plane"], fmt, 0, s)
    c = codec.residual_apply_yuv(tuple(t.cpu() for t in base), cpu["sym"], cpu["plane"], fmt, 0, s)
    for u, v, w in zip(a, c, x):
        assert np.array_equal(_np16(u), _np16(v)) and np.array_equal(_np16(u) >> 6, _np16(w) >> 6)
