"""The entropy front's kernels alone, through their kernel-level C entries, against tests/quant_oracle.py:
quant_phase (the encoder's quantisation of one checkerboard phase), phase_indexes and phase_dequant (the
decoder's side of the same contract), recip_plane, ckbd_mask, eb_forward and eb_dequant.

Every symbol, index, narrow symbol / index, overflow flag, y_hat, z_hat, reciprocal and mask is compared bit
for bit.  The two likelihoods are the only toleranced quantities: the GaussianConditional under the project's
bound of test_gc_likelihood_elementwise, the bottleneck's under a bound calibrated in the test from the error
of a plain fp32 torch restatement against float64.

Every output buffer is filled with a poison pattern before the call (0x7FFFFFFF words: a NaN as fp32; 0x7FFF
and 0xFF for the narrow streams), the padding between batch strides and a tail behind every buffer included,
and the whole buffer is compared afterwards: what the contract says is written holds the oracle's bits, all
else still holds the poison.  Inputs carry NaN in their padding.  Each test prints what it measured before it
asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import quant_oracle as qo

pytestmark = pytest.mark.gpu

F = np.float32
DEV = "cuda"
P32, P16, P8 = 0x7FFFFFFF, 0x7FFF, 0xFF
TAIL = 64                                            # poisoned elements behind every output buffer
SHAPES = [(1, 1, 1, 2), (2, 3, 5, 6), (2, 5, 7, 38), (1, 32, 8, 16)]
FORMS = ("none", "image", "image_dyadic", "plane_const", "plane")
SID = lambda s: "x".join(str(v) for v in s)  # noqa: E731


def table():
    from mlic_amd import entropy
    return entropy.get_scale_table().numpy()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t, off=0):
    return None if t is None else t.data_ptr() + off * t.element_size()


def poisoned(count, kind):
    """A device buffer of `count` + TAIL elements of poison: kind 32 (fp32 / int32 words), 16 or 8."""
    dt, v = {32: (torch.int32, P32), 16: (torch.int16, P16), 8: (torch.uint8, P8)}[kind]
    return torch.full((count + TAIL,), v, dtype=dt, device=DEV)


def host(t):
    """The device buffer's bit patterns as an unsigned numpy array."""
    a = t.cpu().numpy()
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.itemsize])


def strided(a, bs):
    """[B][k] host array -> device [B][bs] with NaN in the padding."""
    B, k = a.shape
    h = np.full((B, bs), np.nan, F)
    h[:, :k] = a
    return up(h)


def gains(form, shape, seed=7):
    """-> (the oracle's gain argument, per-image [B] or None, plane [B][H][W] or None)."""
    B, C_, H, W = shape
    if form == "none":
        return None, None, None
    per = np.asarray({"image": (0.37, 1.9), "plane_const": (0.37, 1.9), "image_dyadic": (0.5, 2.0)}.get(form, (1, 1))[:B], F)
    if form in ("image", "image_dyadic"):
        return per, per, None
    if form == "plane_const":
        pl = np.broadcast_to(per.reshape(B, 1, 1), (B, H, W)).copy()
        return pl, None, pl
    rng = np.random.default_rng(seed)
    pl = rng.choice(np.asarray(qo.ROI_GAINS + (0.5, 2.0), F), (B, H, W))
    return pl, None, pl


class Front:
    """One geometry on the device: the strides (contiguous, or every batch stride two channels longer and the
    likelihood a slice of a three times wider tensor), the inputs, poisoned outputs, and the three entries."""

    def __init__(self, shape, padded, form, y, params, params_a, nlim=32767):
        from mlic_amd import _lib
        self.lib = _lib
        B, Cn, H, W = self.shape = shape
        self.n = n = Cn * H * W
        pad = 2 * H * W if padded else 0
        self.y_bs, self.p_bs, self.yh_bs = n + pad, 2 * n + pad, n + pad
        self.lik_bs, self.lik_off = (3 * n, n) if padded else (n, 0)
        self.form, self.nlim = form, nlim
        self.gain, per, plane = gains(form, shape)
        self.table = up(table())
        self.y = strided(y.reshape(B, n), self.y_bs) if y is not None else None
        self.params = strided(params.reshape(B, 2 * n), self.p_bs)
        self.params_a = strided(params_a.reshape(B, 2 * n), self.p_bs) if params_a is not None else None
        self.sc = up(per) if per is not None else None
        self.rs = up((F(1.0) / per).astype(F)) if per is not None else None
        self.scp = up(plane) if plane is not None else None
        self.rsp = up((F(1.0) / plane).astype(F)) if plane is not None else None
        self.nsq = B * n // 2

    def outputs(self):
        B = self.shape[0]
        return {"yh": poisoned(B * self.yh_bs, 32), "lik": poisoned(B * self.lik_bs, 32),
                "sym": poisoned(self.nsq, 32), "idx": poisoned(self.nsq, 32), "sym16": poisoned(self.nsq, 16),
                "idx8": poisoned(self.nsq, 8), "ovf": torch.tensor([0, P32, P32, P32], dtype=torch.int32, device=DEV)}

    def desc(self, phase, o, use):
        B, Cn, H, W = self.shape
        g = lambda k: ptr(o[k]) if k in use else None  # noqa: E731
        return self.lib.QuantDesc(
            y=ptr(self.y), y_bs=self.y_bs, params=ptr(self.params), params_bs=self.p_bs,
            params_a=ptr(self.params_a) if "lik" in use else None, params_a_bs=self.p_bs,
            yh=g("yh"), yh_bs=self.yh_bs, lik=ptr(o["lik"], self.lik_off) if "lik" in use else None,
            lik_bs=self.lik_bs, sym=g("sym"), idx=g("idx"), sym16=g("sym16"), idx8=g("idx8"),
            ovf=ptr(o["ovf"]) if "sym16" in use else None, nlim=self.nlim, ntable=int(self.table.numel()),
            table=ptr(self.table), phase=phase, vbr=int(self.form != "none"), sc=ptr(self.sc), rs=ptr(self.rs),
            scp=ptr(self.scp), rsp=ptr(self.rsp), B=B, C=Cn, H=H, W=W)

    def run(self, entry, phase, o, use):
        d = self.desc(phase, o, use)
        self.lib.call(entry, stream(), C.byref(d))

    # ---- the expected contents of whole buffers
    def expect_yh(self, yh, mine, phase):
        """Poison, with the oracle's y_hat at the phase's pixels and (phase 0) +0 at the others."""
        B, Cn, H, W = self.shape
        e = np.full((B, self.yh_bs), P32, np.uint32)
        img = np.full((B, Cn, H, W), P32, np.uint32)
        img[..., mine] = qo.bits(yh)[..., mine]
        if phase == 0:
            img[..., ~mine] = 0
        e[:, :self.n] = img.reshape(B, self.n)
        return np.concatenate([e.ravel(), np.full(TAIL, P32, np.uint32)])

    def squeezed(self, a, pat):
        a = np.ascontiguousarray(a).ravel()
        u = a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.itemsize])
        return np.concatenate([u, np.full(TAIL, pat, u.dtype)])

    def lik_region(self, got):
        """(the [B][C][H][W] likelihoods as fp32, everything else of the wide buffer as bits)."""
        B, Cn, H, W = self.shape
        body = got[:B * self.lik_bs].reshape(B, self.lik_bs)
        inside = body[:, self.lik_off:self.lik_off + self.n].copy().view(F).reshape(B, Cn, H, W)
        rest = body.copy()
        rest[:, self.lik_off:self.lik_off + self.n] = P32
        return inside, np.concatenate([rest.ravel(), got[B * self.lik_bs:]])


def check_gc_lik(got, lik64, where):
    """The project's GaussianConditional bound (test_gc_likelihood_elementwise): max(8 ulp of the value,
    4 * 2^-24) against the floored float64 likelihood, and the floor taken at the same elements."""
    exp = np.maximum(lik64, np.float64(qo.FLOOR))
    err = np.abs(got.astype(np.float64) - exp)
    bound = np.maximum(8 * 2.0 ** -23 * np.abs(exp), 4 * 2.0 ** -24)
    worst = float((err / bound).max())
    print(f"{where}: lik max abs err {err.max():.3e}, max err / bound {worst:.3f}, at the floor {int((got == qo.FLOOR).sum())}")
    assert (err <= bound).all(), (where, float(err.max()), worst)
    assert np.array_equal(got == qo.FLOOR, lik64 <= np.float64(qo.FLOOR)), where
    return float(err.max())


def quant_and_check(shape, padded, form, phase, nlim, overflow, nan=False, seed=31):
    """One quant_phase call with every output, checked whole against the oracle.  -> (Front, outputs, oracle)"""
    t = table()
    gain = gains(form, shape)[0]
    y, params, params_a, kinds = qo.quant_case(shape, seed + phase, t, gain=gain, nlim=nlim, overflow=overflow, nan=nan)
    fr = Front(shape, padded, form, y, params, params_a, nlim)
    use = {"yh", "sym", "idx", "sym16", "idx8"} | ({"lik"} if phase == 1 and not nan else set())
    o = fr.outputs()
    fr.run("mlic_quant_phase_run", phase, o, use)
    ref = qo.quant_phase(y, params, t, phase, gain=gain, params_a=params_a if "lik" in use else None, nlim=nlim)
    where = f"quant_phase {SID(shape)} padded={padded} {form} phase={phase} nlim={nlim} overflow={overflow}"
    h = {k: host(v) for k, v in o.items()}
    if nan:
        return fr, h, ref, where
    assert ref["sym_defined"].all()
    assert np.array_equal(h["yh"], fr.expect_yh(ref["yh"], ref["mine"], phase)), where + ": y_hat"
    assert np.array_equal(h["sym"], fr.squeezed(ref["sym"], P32)), where + ": sym"
    assert np.array_equal(h["idx"], fr.squeezed(ref["idx"], P32)), where + ": idx"
    assert np.array_equal(h["sym16"], fr.squeezed(ref["sym16"], P16)), where + ": sym16"
    assert np.array_equal(h["idx8"], fr.squeezed(ref["idx8"], P8)), where + ": idx8"
    assert ref["ovf"] == int(overflow and "sym" in kinds)     # the smallest shape holds no overflowing row
    assert h["ovf"].tolist() == [ref["ovf"], P32, P32, P32], where + ": overflow flag"
    if "lik" in use:
        inside, rest = fr.lik_region(h["lik"])
        assert (rest == P32).all(), where + ": written outside the likelihood slice"
        check_gc_lik(inside, ref["lik64"], where)
    else:
        assert (h["lik"] == P32).all(), where
    if shape != SHAPES[0]:
        assert {"tie", "sym", "scale"} <= kinds
    return fr, h, ref, where


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_quant_phase_against_oracle(shape, padded, form):
    """Both phases, at the int16 range and at a narrow range of 1, each with the rows that overflow the range
    (the flag must be 1 and the symbols saturate) and without them (the flag must stay 0).  Phase 1 also writes
    the likelihood: the two parameter sets are independent draws, so one taken from the wrong set shows at
    every pixel."""
    for phase in (0, 1):
        for nlim in (32767, 1):
            for overflow in (True, False):
                quant_and_check(shape, padded, form, phase, nlim, overflow)


@pytest.mark.parametrize("form", ["none", "plane"])
def test_quant_phase_nan_input(form):
    """One NaN y per pair of pixels of the planted row.  Only what the kernel defines is asserted there: the narrow
    symbol saturates high and the flag is set (nothing else overflows in this case).  The int32 symbol of a NaN
    is whatever the hardware's float-to-int conversion gives and is left out; y_hat there is a NaN."""
    shape = (2, 3, 5, 6)
    for phase in (0, 1):
        fr, h, ref, where = quant_and_check(shape, True, form, phase, 32767, overflow=False, nan=True)
        bad = ~ref["sym_defined"].ravel()
        assert bad.sum() == shape[0] and np.isnan(ref["q"].ravel()[bad]).all()
        n = bad.size
        assert (h["sym16"][:n][bad] == 32767).all(), where
        assert h["ovf"].tolist() == [1, P32, P32, P32], where
        assert np.array_equal(h["sym16"], fr.squeezed(ref["sym16"], P16)), where
        assert np.array_equal(h["sym"][:n][~bad], fr.squeezed(ref["sym"], P32)[:n][~bad]) and (h["sym"][n:] == P32).all()
        assert np.array_equal(h["idx"], fr.squeezed(ref["idx"], P32)), where
        assert np.array_equal(h["idx8"], fr.squeezed(ref["idx8"], P8)), where
        exp = fr.expect_yh(ref["yh"], ref["mine"], phase)
        got_nan = np.isnan(h["yh"].view(F)) & (h["yh"] != P32)
        assert got_nan.sum() == shape[0] and np.isnan(exp.view(F)[got_nan]).all(), where
        assert np.array_equal(h["yh"][~got_nan], exp[~got_nan]), where


@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_constant_plane_gives_the_per_image_bits(shape, padded):
    """A gain plane that holds one value per image must reproduce the per-image form in every output bit, the
    likelihood included (the two forms run the same expressions)."""
    t = table()
    for phase in (0, 1):
        per = gains("image", shape)[0]
        y, params, params_a, _ = qo.quant_case(shape, 41 + phase, t, gain=per)
        outs = []
        for form in ("image", "plane_const"):
            fr = Front(shape, padded, form, y, params, params_a)
            o = fr.outputs()
            fr.run("mlic_quant_phase_run", phase, o, {"yh", "lik", "sym", "idx", "sym16", "idx8"})
            outs.append({k: host(v) for k, v in o.items()})
        for k in outs[0]:
            assert np.array_equal(outs[0][k], outs[1][k]), (SID(shape), phase, k)


@pytest.mark.parametrize("form", ["none", "image", "image_dyadic", "plane"])
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_decoder_reproduces_encoder(shape, form):
    """The contract between the two sides: from the same entropy parameters phase_indexes gives quant_phase's
    indexes (idx8 and idx), and from quant_phase's symbols (the narrow stream, and separately the int32 one)
    phase_dequant gives quant_phase's y_hat bit for bit at the phase's pixels, +0 at the others in phase 0 and
    nothing at the others in phase 1.  The case holds the tie, table-edge and clamped-scale rows, and the edge
    symbols that still fit the narrow range; both stride layouts."""
    for padded in (False, True):
        for phase in (0, 1):
            fr, h, ref, where = quant_and_check(shape, padded, form, phase, 32767, overflow=False, seed=51)
            for use in ({"idx8"}, {"idx"}):
                o = fr.outputs()
                fr.run("mlic_phase_indexes_run", phase, o, use)
                g = {k: host(v) for k, v in o.items()}
                for k in o:
                    if k in use:
                        assert np.array_equal(g[k], h[k]), (where, "phase_indexes", k)
                    elif k != "ovf":
                        assert (g[k] == {4: P32, 2: P16, 1: P8}[g[k].itemsize]).all(), (where, "phase_indexes wrote", k)
            for src in ("sym16", "sym"):
                o = fr.outputs()
                o[src] = up(h[src].view({"sym16": np.int16, "sym": np.int32}[src]))
                fr.run("mlic_phase_dequant_run", phase, o, {"yh", src})
                got = host(o["yh"])
                assert np.array_equal(got, h["yh"]), (where, "phase_dequant from", src)
                mine, back = qo.phase_dequant(ref[src], fr.params.cpu().numpy()[:, :2 * fr.n].reshape(
                    shape[0], 2 * shape[1], shape[2], shape[3]), phase, gain=fr.gain)
                assert np.array_equal(got, fr.expect_yh(back, mine, phase)), (where, "phase_dequant oracle", src)


def test_recip_plane_bit_exact():
    """4099 gains (a block boundary plus three): a log sweep over [2^-20, 2^20], the VBR models' Gain values and
    1 +- one ulp; the kernel's quotient is numpy's correctly rounded fp32 1 / g bit for bit.  Every result here
    is a normal number: quotients in the subnormal range are out of scope."""
    from mlic_amd import _lib
    special = np.asarray(qo.ROI_GAINS + (0.51801, 0.06556, 0.13944, 0.002424), F)
    edge = np.asarray([np.nextafter(F(1), F(0)), np.nextafter(F(1), F(2))], F)
    g = np.concatenate([np.exp2(np.linspace(-20.0, 20.0, 4099 - special.size - 2)).astype(F), special, edge])
    assert g.size == 4099
    gd, r = up(g), poisoned(g.size, 32)
    _lib.call("mlic_recip_plane_run", stream(), ptr(gd), ptr(r), g.size)
    exp = (F(1.0) / g).astype(F)
    assert (np.abs(exp) >= np.finfo(F).tiny).all()
    got = host(r)
    print(f"recip_plane: {int((got[:g.size] != qo.bits(exp)).sum())} of {g.size} differ")
    assert np.array_equal(got, np.concatenate([qo.bits(exp), np.full(TAIL, P32, np.uint32)]))


@pytest.mark.parametrize("keep_anchor", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_ckbd_mask_bit_exact(shape, keep_anchor):
    """Both masks with padded strides (different for input and output): the kept pixels pass their bits through,
    -0 and NaN included, the others are +0, the padding is untouched."""
    from mlic_amd import _lib
    B, Cn, H, W = shape
    n = Cn * H * W
    x = np.random.default_rng(3).normal(0, 1, shape).astype(F)
    flat = x.reshape(B, n)
    flat[:, 0::7] = -0.0
    flat[:, 1::5] = np.nan
    flat[:, 0] = [-0.0, np.nan][keep_anchor]      # pixel (0, 0) is a non-anchor, (0, 1) an anchor
    flat[:, 1] = [np.nan, -0.0][keep_anchor]
    x_bs, y_bs = n + 2 * H * W, n + 3 * H * W
    xd, yd = strided(flat, x_bs), poisoned(B * y_bs, 32)
    _lib.call("mlic_ckbd_mask_run", stream(), ptr(xd), x_bs, ptr(yd), y_bs, B, Cn, H, W, keep_anchor)
    e = np.full((B, y_bs), P32, np.uint32)
    e[:, :n] = qo.bits(qo.ckbd_mask(x, keep_anchor)).reshape(B, n)
    kept = qo.anchors(H, W) == bool(keep_anchor)
    assert (qo.bits(x)[..., kept] == e[:, :n].reshape(B, Cn, H, W)[..., kept]).all()
    assert np.array_equal(host(yd), np.concatenate([e.ravel(), np.full(TAIL, P32, np.uint32)]))


# =============================================================================================
# entropy bottleneck
SLACK = 256   # floats behind the parameter block: a channel index that runs past C still reads inside it


def eb_device(p):
    """The 15 parameter tensors in one device block, in EB_NAMES order -> (block, {name: byte pointer})."""
    parts = [p[k].ravel() for k in qo.EB_NAMES]
    blk = up(np.concatenate(parts + [np.zeros(SLACK, F)]))
    offs = np.concatenate([[0], np.cumsum([a.size for a in parts])])
    return blk, {k: ptr(blk, int(offs[i])) for i, k in enumerate(qo.EB_NAMES)}


def eb_run(zd, pp, shape, want):
    from mlic_amd import _lib
    B, Cn, H, W = shape
    n = B * Cn * H * W
    o = {k: poisoned(n, 32) for k in ("z_hat", "lik", "sym")}
    _lib.call("mlic_eb_forward_run", stream(), ptr(zd), *[ptr(o[k]) if k in want else None for k in ("z_hat", "lik", "sym")],
              *[pp[k] for k in qo.EB_NAMES], B, Cn, H, W)
    return o, {k: host(v) for k, v in o.items()}


@pytest.mark.parametrize("shape,seed", [((2, 5, 3, 7), 3), ((1, 7, 9, 11), 4)], ids=["2x5x3x7", "1x7x9x11"])
def test_eb_forward_and_dequant(shape, seed):
    """z_hat, the symbols and eb_dequant(symbols) bit for bit (the last equal to z_hat); every subset of the
    optional outputs leaves the others' buffers untouched and the written ones unchanged; the likelihood against
    float64 under max(4 * E32, 4 * 2^-24), E32 being the largest error of the plain fp32 torch restatement on the
    same inputs (the factor covers expf / tanhf / log1pf differing by a few ulp between the GPU and the CPU), and
    never looser than the project's rtol 1e-4 + atol 1e-7 of this likelihood (test_oracle_golden).  An element
    below 2^-22 has no relative term left to speak of: the absolute one holds it (at most a quarter of a case,
    checked on the CPU in test_quant_oracle_cpu)."""
    from mlic_amd import _lib
    z, p = qo.eb_case(shape, seed)
    B, Cn, H, W = shape
    n = z.size
    zd = up(z)
    blk, pp = eb_device(p)
    zh, sym = qo.eb_quant(z, p["quantiles"])
    tail = np.full(TAIL, P32, np.uint32)
    o, full = eb_run(zd, pp, shape, {"z_hat", "lik", "sym"})
    assert np.array_equal(full["z_hat"], np.concatenate([qo.bits(zh).ravel(), tail]))
    assert np.array_equal(full["sym"], np.concatenate([sym.ravel().view(np.uint32), tail]))
    assert (full["lik"][n:] == P32).all()
    for want in ({"z_hat"}, {"lik"}, {"sym"}, {"z_hat", "sym"}, {"lik", "sym"}, {"z_hat", "lik"}):
        _, part = eb_run(zd, pp, shape, want)
        for k in part:
            assert np.array_equal(part[k], full[k]) if k in want else (part[k] == P32).all(), (want, k)
    back = poisoned(n, 32)
    _lib.call("mlic_eb_dequant_run", stream(), ptr(o["sym"]), pp["quantiles"], ptr(back), B, Cn, H, W)
    assert np.array_equal(host(back), full["z_hat"])
    assert np.array_equal(host(back)[:n], qo.bits(qo.eb_dequant(sym, p["quantiles"])).ravel())
    # the likelihood
    l64 = qo.eb_lik64(p, zh)
    exp = np.maximum(l64, np.float64(qo.FLOOR))
    t32 = np.maximum(qo.eb_lik_torch(p, zh, torch.float32), qo.FLOOR).astype(np.float64)
    e32 = float(np.abs(t32 - exp).max())
    got = full["lik"][:n].view(F).reshape(shape).astype(np.float64)
    err = np.abs(got - exp)
    bound = np.minimum(max(4 * e32, 4 * 2.0 ** -24), 1e-7 + 1e-4 * exp)
    small = l64 < 2.0 ** -22
    print(f"eb_forward {SID(shape)}: kernel max abs err {err.max():.3e}, E32 {e32:.3e}, max err / bound "
          f"{(err / bound).max():.3f}, below 2^-22: {small.mean():.3f} of the case (max err there {err[small].max():.3e})")
    assert small.mean() <= 0.25
    assert (err <= bound).all(), (float(err.max()), e32, float((err / bound).max()))


def test_eb_negative_zero_median():
    """A median of exactly -0 with z in [-0.5, -0]: rint gives -0, and z_hat must be the decoder's
    (float) 0 + -0 = +0, not -0 + -0 = -0 (the named case of the sign the two sides once disagreed in;
    quant_phase's twin is the m = -0 tie row of every quantisation case)."""
    from mlic_amd import _lib
    shape = (1, 5, 1, 4)
    z, p = qo.eb_case(shape, 5)
    p["quantiles"][0, 0, 1] = -0.0
    z[0, 0, 0] = [-0.5, -0.25, -0.0, 0.5]
    zh, sym = qo.eb_quant(z, p["quantiles"])
    assert (qo.bits(zh)[0, 0, 0] == 0).all() and (sym[0, 0, 0] == 0).all()
    blk, pp = eb_device(p)
    o, full = eb_run(up(z), pp, shape, {"z_hat", "sym"})
    assert np.array_equal(full["z_hat"][:z.size], qo.bits(zh).ravel())
    back = poisoned(z.size, 32)
    _lib.call("mlic_eb_dequant_run", stream(), ptr(o["sym"]), pp["quantiles"], ptr(back), *shape)
    assert np.array_equal(host(back), full["z_hat"])
