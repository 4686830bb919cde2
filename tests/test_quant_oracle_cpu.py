"""tests/quant_oracle.py (the numpy statement the entropy-front kernels are held to on the GPU) against other
formulations of the same operations on the CPU: tests/roi_oracle.py's torch slice loop, the reference's
checkerboard helpers, torch.round / searchsorted / clamp, and compressai's matmul form of the bottleneck."""
import types

import numpy as np
import pytest
import torch

import mlic_ref_cpu as ref
import quant_oracle as qo
import roi_oracle
from mlic_amd import entropy

F = np.float32
SHAPES = [(1, 1, 1, 2), (2, 3, 5, 6), (2, 5, 7, 38), (1, 32, 8, 16)]
TABLE = entropy.get_scale_table().numpy()


def gc_bound(ref64):
    """The project's bound of a GaussianConditional likelihood (test_gc_likelihood_elementwise)."""
    return np.maximum(8 * 2.0 ** -23 * np.abs(ref64), 4 * 2.0 ** -24)


class OneSlice(roi_oracle.RefMLICRoi):
    """RefMLICRoi's slice loop on one slice with the networks replaced by planted entropy parameters and a zero
    LRP: what is left is its checkerboard masking, its phase function and its likelihood merge."""

    def __init__(self, C, pa, pn):
        self.cfg = types.SimpleNamespace(slice_num=1, slice_ch=C, hyper_M=1)
        self.pa, self.pn = torch.from_numpy(pa), torch.from_numpy(pn)

    def entropy_parameters(self, x, kind, i):
        return self.pa if kind == "anchor" else self.pn

    def lrp(self, x, kind, i):
        return torch.zeros(self.pa.shape[0], self.cfg.slice_ch, *self.pa.shape[2:])

    def local_context(self, x, i):
        return x


def plane(shape, kind, seed):
    B, C, H, W = shape
    rng = np.random.default_rng(seed)
    if kind == "const":
        return np.broadcast_to(np.asarray([0.37, 1.9][:B], F).reshape(B, 1, 1), (B, H, W)).copy()
    if kind == "dyadic":
        return np.broadcast_to(np.asarray([0.5, 2.0][:B], F).reshape(B, 1, 1), (B, H, W)).copy()
    g = rng.choice(np.asarray(qo.ROI_GAINS + (0.5, 2.0), F), (B, H, W // 2))
    return np.repeat(g, 2, axis=2)      # roi_oracle's planes are equal over a squeezed pair of columns


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("kind", ["const", "dyadic", "pairs"])
def test_oracle_matches_roi_oracle_slice_loop(shape, kind):
    B, C, H, W = shape
    g = plane(shape, kind, 5)
    # the anchor phase's and the non-anchor phase's cases, each planted in its own parameters
    ya, pa, _, _ = qo.quant_case(shape, 11, TABLE, gain=g, overflow=False)
    yn, pn, _, kinds = qo.quant_case(shape, 12, TABLE, gain=g, overflow=False)
    anc = qo.anchors(H, W)
    y = np.where(anc, ya, yn)
    rec = {}
    yh, lik = OneSlice(C, pa, pn)._slice_loop_g(
        torch.zeros(B, 2, H, W), torch.from_numpy(g).unsqueeze(1), y=torch.from_numpy(y),
        record=lambda ph, s, i: rec.__setitem__(ph, (s.numpy(), i.numpy())))
    o0 = qo.quant_phase(y, pa, TABLE, 0, gain=g)
    o1 = qo.quant_phase(y, pn, TABLE, 1, gain=g, params_a=pa)
    for ph, o in ((0, o0), (1, o1)):
        assert np.array_equal(rec[ph][0], o["sym"]), (ph, "symbols")
        assert np.array_equal(rec[ph][1], o["idx"]), (ph, "indexes")
        assert o["ovf"] == 0 and np.array_equal(o["sym16"].astype(np.int32), o["sym"])
    merged = np.where(anc, o0["yh"], o1["yh"])
    assert np.array_equal(yh.numpy(), merged)           # values: the loop's + 0 LRP turns -0 into +0
    exp = np.maximum(o1["lik64"], np.float64(qo.FLOOR))
    got = lik.numpy().astype(np.float64)
    assert (np.abs(got - exp) <= gc_bound(exp)).all(), float(np.abs(got - exp).max())
    if shape != SHAPES[0]:
        assert {"tie", "sym", "scale"} <= kinds


@pytest.mark.parametrize("shape", SHAPES[1:], ids=str)
@pytest.mark.parametrize("gain", [None, (0.37, 1.9), (0.5, 2.0)], ids=str)
def test_oracle_matches_torch_formulations(shape, gain):
    B, C, H, W = shape
    gain = None if gain is None else np.asarray(gain[:B], F)
    for nlim in (32767, 1):
        y, p, pa, kinds = qo.quant_case(shape, 21, TABLE, gain=gain, nlim=nlim)
        assert {"tie", "sym", "scale"} <= kinds
        ty, ts, tm = torch.from_numpy(y), torch.from_numpy(p[:, :C]), torch.from_numpy(p[:, C:])
        tg = torch.ones(B, 1, 1, 1) if gain is None else torch.from_numpy(gain).view(B, 1, 1, 1)
        q = torch.round((ty - tm) * tg)
        yh = q * (1.0 / tg) + tm
        tt = torch.from_numpy(TABLE)
        idx = torch.searchsorted(tt[:-1].contiguous(), torch.clamp(ts * tg, min=0.11).contiguous(), right=False)
        for ph in (0, 1):
            o = qo.quant_phase(y, p, TABLE, ph, gain=gain, nlim=nlim)
            sq = ref.ckbd_squeeze(q, ph == 0)
            assert np.array_equal(o["sym"], sq.int().numpy())
            assert np.array_equal(o["idx"], ref.ckbd_squeeze(idx.float(), ph == 0).int().numpy())
            assert np.array_equal(o["sym16"], torch.clamp(sq, -nlim - 1, nlim).to(torch.int16).numpy())
            assert o["ovf"] == int(bool((sq != torch.clamp(sq, -nlim - 1, nlim)).any())) == 1
            keep = ref.ckbd_anchor(yh) if ph == 0 else ref.ckbd_nonanchor(yh)
            # values: torch.round keeps a -0, which the contract drops (m = -0 rows)
            assert np.array_equal(o["yh"][..., o["mine"]], keep.numpy()[..., o["mine"]])
            # the decoder's statement reproduces the encoder's y_hat from either symbol stream
            y2, p2, _, _ = qo.quant_case(shape, 21, TABLE, gain=gain, nlim=nlim, overflow=False)
            o2 = qo.quant_phase(y2, p2, TABLE, ph, gain=gain, nlim=nlim)
            assert o2["ovf"] == 0
            for sym in (o2["sym"], o2["sym16"]):
                mine, back = qo.phase_dequant(sym, p2, ph, gain=gain)
                assert np.array_equal(qo.bits(back), qo.bits(o2["yh"]))
                unsq = ref.ckbd_unsqueeze(torch.from_numpy(sym.astype(F)), ph == 0)
                assert np.array_equal((unsq * (1.0 / tg) + torch.from_numpy(p2[:, C:])).numpy()[..., mine],
                                      back[..., mine])


def test_oracle_rounds_ties_to_even_and_drops_negative_zero():
    t = TABLE
    y = np.asarray([0.5, -0.5, 1.5, 2.5, -2.5, 3.5], F).reshape(1, 1, 1, 6)
    p = np.concatenate([np.ones((1, 1, 1, 6), F), np.zeros((1, 1, 1, 6), F)], 1)
    p[0, 1, 0, 1] = -0.0
    q = np.concatenate([qo.quant_phase(y, p, t, ph)["q"] for ph in (0, 1)], -1)  # anchors w = 1, 3, 5 then 0, 2, 4
    assert q.ravel().tolist() == [0.0, 2.0, 4.0, 0.0, 2.0, -2.0] and not np.signbit(q).ravel()[0]
    yh = qo.quant_phase(y, p, t, 0)["yh"]
    assert qo.bits(yh)[0, 0, 0, 1] == 0          # rint(-0.5) = -0 is made +0, so +0 + -0 = +0 as in the decoder
    nan = qo.quant_phase(np.full((1, 1, 1, 2), np.nan, F), p[..., :2], t, 0, nlim=5)
    assert nan["sym16"].ravel().tolist() == [5] and nan["ovf"] == 1 and not nan["sym_defined"].any()


def test_ckbd_mask_matches_reference_helpers():
    x = np.random.default_rng(0).normal(0, 1, (2, 3, 5, 6)).astype(F)
    assert np.array_equal(qo.ckbd_mask(x, 1), ref.ckbd_anchor(torch.from_numpy(x)).numpy())
    assert np.array_equal(qo.ckbd_mask(x, 0), ref.ckbd_nonanchor(torch.from_numpy(x)).numpy())


@pytest.mark.parametrize("shape,seed", [((2, 5, 3, 7), 3), ((1, 7, 9, 11), 4)], ids=str)
def test_bottleneck_oracle_and_case(shape, seed):
    z, p = qo.eb_case(shape, seed)
    B, C, H, W = shape
    med = torch.from_numpy(p["quantiles"][:, :, 1:2]).view(1, C, 1, 1)
    zh, sym = qo.eb_quant(z, p["quantiles"])
    r = torch.round(torch.from_numpy(z) - med)
    assert np.array_equal(qo.bits(zh), qo.bits((r + 0.0 + med).numpy())) and np.array_equal(sym, r.int().numpy())
    assert np.array_equal(qo.bits(qo.eb_dequant(sym, p["quantiles"])), qo.bits(zh))
    # what the case is for: ties about a non-integer median, the floor on either side, both softplus branches
    d = z - med.numpy()
    assert all((d == v).any() for v in (0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 40.0, -40.0))
    assert (med.numpy() != np.rint(med.numpy())).all()
    mats = np.concatenate([p[f"m{i}"].ravel() for i in range(5)])
    assert all((mats == v).any() for v in (19.5, 20.0, 20.5, 30.0))
    fac = np.concatenate([p[f"f{i}"].ravel() for i in range(4)])
    assert (np.abs(fac) < 0.01).any() and (fac > 2.8).any() and (fac < -2.8).any()
    l64 = qo.eb_lik64(p, zh)
    assert (l64[d == 40.0] < 1e-9).all() and (l64[d == -40.0] < 1e-9).all()
    t64 = qo.eb_lik_torch(p, zh, torch.float64)
    assert np.abs(l64 - t64).max() <= 1e-13
    # the fp32 restatement: inside the project's own tolerance of this likelihood (test_oracle_golden), and few
    # enough elements so small that only the absolute term holds them
    t32 = qo.eb_lik_torch(p, zh, torch.float32).astype(np.float64)
    e32 = np.abs(t32 - l64)
    print(f"eb {shape}: E32 = {e32.max():.3e}, share below 2^-22 = {(l64 < 2.0 ** -22).mean():.3f}")
    assert (e32 <= 1e-7 + 1e-4 * np.abs(l64)).all(), float(e32.max())
    assert (l64 < 2.0 ** -22).mean() <= 0.25
    # RefMLIC's own statement (the project's CPU oracle) agrees with the fp32 restatement bit for bit or nearly
    m = ref.RefMLIC.__new__(ref.RefMLIC)
    names = {"quantiles": "quantiles", **{f"m{i}": f"_matrix{i}" for i in range(5)},
             **{f"b{i}": f"_bias{i}" for i in range(5)}, **{f"f{i}": f"_factor{i}" for i in range(4)}}
    m.sd = {f"entropy_bottleneck.{names[k]}": torch.from_numpy(v) for k, v in p.items()}
    got = m.eb_likelihood(torch.from_numpy(z)).numpy().astype(np.float64)
    assert np.allclose(got, np.maximum(l64, np.float64(qo.FLOOR)), rtol=1e-4, atol=1e-7)
