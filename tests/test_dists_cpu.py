"""DISTS without a GPU: the float32-features / float64-statistics torch path of metrics.DISTS against the float64
oracle (tests/dists_oracle.py, the package's literal form), the weight loader's two spellings and refusals, the
library's host-only entry points and the harness field.

Errors are absolute (the terms can be exactly 0, or about 1e-8).  CPU_MAX_VALUE and CPU_MAX_TERM are the largest
errors of the float32 path over the 20 non-identical cases as the parity test prints them (both at 37x53 "inv";
DESIGN.md §3 records them); the bound here is twice that, for another platform's BLAS summation order.  They are
also the yardstick of the GPU gate (tests/test_gpu_dists.py: 8 x)."""
import ctypes as C
import inspect

import pytest
import torch

import dists_oracle as oracle
from mlic_amd import _lib, bitstream, metrics

CPU_MAX_VALUE, CPU_MAX_TERM = 2.16e-8, 1.23e-8
VALUE_TOL, TERM_TOL = 2 * CPU_MAX_VALUE, 2 * CPU_MAX_TERM


@pytest.fixture(scope="module")
def metric():
    return metrics.DISTS(oracle.weights())


@pytest.mark.parametrize("kind", oracle.DISTORTIONS)
@pytest.mark.parametrize("shape", list(oracle.SHAPES))
def test_cpu_path_matches_the_oracle(metric, shape, kind):
    a, b, want, want_terms = oracle.case(shape, kind)
    got, terms = metric(a, b, return_terms=True)  # the "v" case is a strided view, taken as it is
    assert got.dtype == torch.float64 and got.shape == (1,) and terms.shape == (1, 12)
    assert torch.equal(metric(a, b), got)
    if kind == "same":
        # the literal form leaves rounding residue, the difference form none
        assert abs(want.item()) <= 1e-15 and got.item() == 0.0 and not terms.any()
        return
    err, terr = oracle.abs_err(got, want), oracle.abs_err(terms, want_terms)
    print(f"{shape} {kind}: oracle {want.item():.6e} float32 {got.item():.6e} abs err {err:.2e} term abs err {terr:.2e}")
    assert err <= VALUE_TOL and terr <= TERM_TOL
    if shape == "16x16":
        assert terms[0, 11].item() == 0.0  # set 5 is one pixel: no variance, no covariance


def test_difference_form_equals_the_literal_form():
    """Both forms in float64 on the oracle's own features: the algebra, without the precision."""
    sd = oracle.weights()
    w = sd["alpha"].double().sum() + sd["beta"].double().sum()
    al = (sd["alpha"].double() / w).flatten().split(oracle.SET_C)
    be = (sd["beta"].double() / w).flatten().split(oracle.SET_C)
    for shape in ("16x16", "37x53"):
        a = oracle.case(shape, "same")[0]
        fa = oracle.features(a, sd)
        for kind in ("n1", "blur", "inv", "off"):
            _, b, want, want_terms = oracle.case(shape, kind)
            terms = []
            for x, y, ak, bk in zip(fa, oracle.features(b, sd), al, be):
                x, y = x.flatten(2), y.flatten(2)
                d = x - y
                vd = (d - d.mean(2, keepdim=True)).square().mean(2)
                terms.append((ak * d.mean(2).square() / (x.mean(2).square() + y.mean(2).square() + oracle.C1)).sum(1))
                terms.append((bk * vd / (x.var(2, unbiased=False) + y.var(2, unbiased=False) + oracle.C2)).sum(1))
            t = torch.stack(terms, 1)
            assert oracle.abs_err(t.sum(1), want) <= 1e-14 and oracle.abs_err(t, want_terms) <= 1e-14


def test_values_are_ordered():
    for shape in oracle.SHAPES:
        v = {k: oracle.case(shape, k)[2].item() for k in ("n1", "n8", "inv")}
        assert v["inv"] > v["n8"] > v["n1"] > 0


def _torchvision_spelling(sd):
    feats = {k.split(".", 1)[1]: v for k, v in sd.items() if k.startswith("stage") and not k.endswith(".filter")}
    return feats, {"alpha": sd["alpha"], "beta": sd["beta"]}


def test_both_weight_spellings_give_the_same_bits(metric):
    sd = oracle.weights()
    assert "stage2.4.filter" in sd and "mean" in sd  # the package's buffers are in the state_dict, and ignored
    feats, head = _torchvision_spelling(sd)
    assert sorted(feats)[:3] == ["0.bias", "0.weight", "10.bias"] and len(feats) == 26
    other = metrics.DISTS((feats, head))  # no mean / std: the package's constants
    a, b, _, _ = oracle.case("37x53", "n8")
    v, t = metric(a, b, return_terms=True)
    v2, t2 = other(a, b, return_terms=True)
    assert torch.equal(v, v2) and torch.equal(t, t2)
    # a mean of its own is used
    moved = dict(sd, mean=sd["mean"] + 0.1)
    assert not torch.equal(metrics.DISTS(moved)(a, b), v)
    # the trunk is the LPIPS tests' trunk
    lp = metrics.lpips_synthetic_weights(oracle.SEED)
    assert torch.equal(lp["net.slice3.12.weight"], sd["stage3.12.weight"])
    assert float(sd["alpha"].min()) > 0 and abs(float(sd["beta"].mean()) - 0.1) < 2e-3


def test_loader_refusals_name_the_tensor():
    sd = oracle.weights()
    with pytest.raises(ValueError, match=r"missing tensor 12\.bias"):
        metrics.DISTS({k: v for k, v in sd.items() if k != "stage3.12.bias"})
    with pytest.raises(ValueError, match=r"missing tensor beta"):
        metrics.DISTS({k: v for k, v in sd.items() if k != "beta"})
    with pytest.raises(ValueError, match=r"missing tensor std"):
        metrics.DISTS({k: v for k, v in sd.items() if k != "std"})
    with pytest.raises(ValueError, match=r"extra conv tensor stage5\.30\.weight"):
        metrics.DISTS(dict(sd, **{"stage5.30.weight": torch.zeros(512, 512, 3, 3)}))
    with pytest.raises(ValueError, match=r"tensor stage2\.5\.weight has shape \(128, 64, 3, 1\)"):
        metrics.DISTS(dict(sd, **{"stage2.5.weight": torch.zeros(128, 64, 3, 1)}))
    with pytest.raises(ValueError, match=r"tensor alpha has shape \(1, 1474, 1, 1\)"):
        metrics.DISTS(dict(sd, alpha=torch.ones(1, 1474, 1, 1)))
    with pytest.raises(ValueError, match="unexpected tensor classifier"):
        metrics.DISTS(dict(sd, **{"classifier.weight": torch.zeros(3)}))
    with pytest.raises(ValueError, match="alpha and beta must be finite and nonzero"):
        metrics.DISTS(dict(sd, alpha=-sd["beta"]))
    with pytest.raises(ValueError, match="alpha and beta must be finite and nonzero"):
        metrics.DISTS(dict(sd, beta=sd["beta"] * float("inf")))
    feats, head = _torchvision_spelling(sd)
    with pytest.raises(ValueError, match="missing tensor alpha"):
        metrics.DISTS((feats, {"beta": head["beta"]}))
    with pytest.raises(ValueError, match="weights must be"):
        metrics.DISTS((feats, [head["alpha"], head["beta"]]))


def test_python_argument_errors(metric):
    with pytest.raises(ValueError, match="at least 16"):
        metric(torch.rand(1, 3, 15, 40), torch.rand(1, 3, 15, 40))
    with pytest.raises(ValueError):
        metric(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 17))
    with pytest.raises(ValueError):
        metric(torch.rand(1, 1, 16, 16), torch.rand(1, 1, 16, 16))
    with pytest.raises(ValueError, match="precision"):
        metric.set_precision(1)


def test_nan_pixels_count_as_zero(metric):
    a, b, _, _ = oracle.case("16x16", "n8")
    an = a.clone()
    an[0, 1, 3, 4] = float("nan")
    az = a.clone()
    az[0, 1, 3, 4] = 0.0
    assert torch.equal(metric(an, b), metric(az, b))
    assert torch.equal(oracle.dists(an, b)[0], oracle.dists(az, b)[0])


def test_exported_from_the_package():
    import mlic_amd
    assert mlic_amd.DISTS is metrics.DISTS and mlic_amd.dists_synthetic_weights is metrics.dists_synthetic_weights
    sd, again = metrics.dists_synthetic_weights(3), metrics.dists_synthetic_weights(3)
    assert len(sd) == 26 + 2 + 2 + 4 and all(torch.equal(sd[k], again[k]) for k in sd)
    assert not torch.equal(sd["alpha"], metrics.dists_synthetic_weights(4)["alpha"])
    assert metrics.DISTS_MIN_SIDE == 16


def _scratch_bytes(B, H, W):
    n = C.c_size_t(0)
    rc = _lib.lib().mlic_dists_scratch_bytes(B, H, W, C.byref(n))
    return rc, n.value


def test_scratch_bytes_host_only():
    rc, n1 = _scratch_bytes(1, 37, 53)
    assert rc == 0 and n1 > 0
    # two ping-pong buffers of 2 x 64 planes and the pooled planes on the CEIL grid (19 x 27), at least
    assert n1 >= 2 * (2 * 64 * 37 * 53 * 4) + 2 * 64 * 19 * 27 * 4
    prev = n1
    for B in (2, 3, 8, 32):
        rc, n = _scratch_bytes(B, 37, 53)
        assert rc == 0 and n > prev
        prev = n
    # the chunk cap: one 1920 x 1088 pair is most of 4 GiB, so the need stops growing with B
    rc, big1 = _scratch_bytes(1, 1088, 1920)
    rc2, big8 = _scratch_bytes(8, 1088, 1920)
    assert rc == 0 and rc2 == 0 and big1 == big8 and 2 ** 31 < big1 <= 2 ** 32
    rc, k4 = _scratch_bytes(4, 256, 256)
    rc2, k400 = _scratch_bytes(400, 256, 256)
    rc3, k4000 = _scratch_bytes(4000, 256, 256)
    assert rc == 0 and rc2 == 0 and rc3 == 0 and k4 < k400 == k4000 <= 2 ** 32
    for bad, word in (((1, 15, 40), b"16"), ((1, 40, 15), b"16"), ((0, 40, 40), b"B must be positive"),
                      ((1, 4096, 4096), b"2^23")):
        rc, _ = _scratch_bytes(*bad)
        assert rc != 0, bad
        assert word in _lib.lib().mlic_last_error()


def test_kernel_entry_refuses_a_null_handle_before_the_gpu():
    lib = _lib.lib()
    st = (C.c_int64 * 3)(3 * 16 * 16, 16 * 16, 16)
    fake = C.c_void_p(4096)
    rc, need = _scratch_bytes(1, 16, 16)
    assert rc == 0
    assert lib.mlic_image_dists_u8(None, None, fake, st, fake, st, 1, 16, 16, fake, need, fake, None) != 0
    assert b"null mlic_dists handle" in lib.mlic_last_error()
    assert lib.mlic_dists_set_precision(None, 2) != 0
    assert b"null mlic_dists handle" in lib.mlic_last_error()
    n = C.c_int64(0)
    assert lib.mlic_dists_range_fallbacks(None, C.byref(n), 0) != 0
    assert lib.mlic_dists_profile(None, 0, None) != 0
    assert lib.mlic_dists_destroy(None) == 0
    h = C.c_void_p()
    assert lib.mlic_dists_create(1, None, None, None, None, None, C.byref(h)) != 0
    assert b"dists_create: null tensor table" in lib.mlic_last_error()


class _StubNet:
    """compress / decompress of the harness without a codec: x_hat = the padded input, darkened."""

    def compress(self, x):
        self.x = x
        return {"strings": [[b"yy"], [b"z"]], "shape": (x.size(2) // 64, x.size(3) // 64)}

    def decompress(self, strings, shape):
        return {"x_hat": self.x * 0.9}


def test_code_image_dists_field(metric):
    assert inspect.signature(bitstream.code_image).parameters["dists"].default is None
    img = oracle.case("37x53", "same")[0]
    plain = bitstream.code_image(_StubNet(), img)
    r = bitstream.code_image(_StubNet(), img, dists=metric)
    assert "dists" not in plain and set(r) - set(plain) == {"dists"}
    for k in ("H", "W", "bytes", "bpp", "psnr"):
        assert plain[k] == r[k]
    assert torch.equal(plain["x_hat"], r["x_hat"])
    assert isinstance(r["dists"], float) and r["dists"] > 0
    assert r["dists"] == metric(img, r["x_hat"]).item()
    small = img[:, :, :15, :40]
    assert bitstream.code_image(_StubNet(), small, dists=metric)["dists"] is None
    both = bitstream.code_image(_StubNet(), img, dists=metric, lpips=lambda a, b: torch.zeros(1))
    assert both["dists"] == r["dists"] and both["lpips"] == 0.0
