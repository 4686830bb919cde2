"""LPIPS-VGG without a GPU: the float32 torch path of metrics.LPIPS against the float64 oracle
(tests/lpips_oracle.py), the weight loader's two spellings and refusals, the library's host-only entry points and
the harness field.

Gate of the float32 path (CPU_TOL, relative, on the value and on every term).  A feature value carries about
1e-6 relative rounding error after thirteen fp32 convs (sqrt(K) * 2^-24 with K <= 4608 per layer).  The head
subtracts two unit vectors ua - ub; the part of that error that does not cancel enters the difference d with
about 1e-6 |u|, and for the weakest distortion of the cases (noise sigma 1/255) |d| is about 1e-2 |u|, so d is
good to 1e-4 and d^2 to 2e-4; the means over channels and pixels only average it down.  The measured maxima are
printed by the parity test (DESIGN.md §3 records them)."""
import ctypes as C
import inspect

import pytest
import torch

import lpips_oracle as oracle
from mlic_amd import _lib, bitstream, metrics

CPU_TOL = 2e-4


@pytest.fixture(scope="module")
def metric():
    return metrics.LPIPS(oracle.weights())


@pytest.mark.parametrize("kind", oracle.DISTORTIONS)
@pytest.mark.parametrize("shape", list(oracle.SHAPES))
def test_cpu_path_matches_the_oracle(metric, shape, kind):
    a, b, want, want_terms = oracle.case(shape, kind)
    got, terms = metric(a, b, return_terms=True)  # the "v" case is a strided view, taken as it is
    assert got.dtype == torch.float64 and got.shape == (1,) and terms.shape == (1, 5)
    assert torch.equal(metric(a, b), got)
    if kind == "same":
        assert want.item() == 0.0 and got.item() == 0.0 and not terms.any()
        return
    err, terr = oracle.rel_err(got, want), oracle.rel_err(terms, want_terms)
    print(f"{shape} {kind}: oracle {want.item():.6e} float32 {got.item():.6e} rel err {err:.2e} term rel err {terr:.2e}")
    assert err <= CPU_TOL and terr <= CPU_TOL


def test_values_are_ordered():
    for shape in oracle.SHAPES:
        v = {k: oracle.case(shape, k)[2].item() for k in ("n1", "n8", "inv")}
        assert v["inv"] > v["n8"] > v["n1"] > 0


def _torchvision_spelling(sd):
    feats = {k.split(".", 2)[2]: v for k, v in sd.items() if k.startswith("net.")}
    return feats, [sd[f"lin{k}.model.1.weight"] for k in range(5)]


def test_both_weight_spellings_give_the_same_bits(metric):
    sd = oracle.weights()
    feats, lins = _torchvision_spelling(sd)
    assert sorted(feats)[:3] == ["0.bias", "0.weight", "10.bias"]
    other = metrics.LPIPS((feats, lins))
    dup = dict(sd)
    dup["lins.0.model.1.weight"] = torch.zeros(1, 64, 1, 1)  # the package's duplicate: ignored
    third = metrics.LPIPS(dup)
    a, b, _, _ = oracle.case("37x53", "n8")
    v, t = metric(a, b, return_terms=True)
    for m in (other, third):
        v2, t2 = m(a, b, return_terms=True)
        assert torch.equal(v, v2) and torch.equal(t, t2)
    # the default shift and scale are the package's constants
    bare = {k: v for k, v in sd.items() if not k.startswith("scaling_layer.")}
    assert torch.equal(metrics.LPIPS(bare)(a, b), v)


def test_loader_refusals_name_the_tensor():
    sd = oracle.weights()
    missing = {k: v for k, v in sd.items() if k != "net.slice3.12.bias"}
    with pytest.raises(ValueError, match=r"missing tensor 12\.bias"):
        metrics.LPIPS(missing)
    nolin = {k: v for k, v in sd.items() if k != "lin3.model.1.weight"}
    with pytest.raises(ValueError, match=r"missing tensor lin3\.model\.1\.weight"):
        metrics.LPIPS(nolin)
    extra = dict(sd)
    extra["net.slice5.30.weight"] = torch.zeros(512, 512, 3, 3)
    with pytest.raises(ValueError, match=r"extra conv tensor net\.slice5\.30\.weight"):
        metrics.LPIPS(extra)
    shaped = dict(sd)
    shaped["net.slice2.5.weight"] = torch.zeros(128, 64, 3, 1)
    with pytest.raises(ValueError, match=r"tensor net\.slice2\.5\.weight has shape \(128, 64, 3, 1\)"):
        metrics.LPIPS(shaped)
    feats, lins = _torchvision_spelling(sd)
    with pytest.raises(ValueError, match=r"tensor lin1\.model\.1\.weight has shape"):
        metrics.LPIPS((feats, lins[:1] + [lins[0]] + lins[2:]))
    with pytest.raises(ValueError, match="five lin tensors"):
        metrics.LPIPS((feats, lins[:4]))
    with pytest.raises(ValueError, match="unexpected tensor classifier"):
        metrics.LPIPS(dict(sd, **{"classifier.weight": torch.zeros(3)}))


def test_python_argument_errors(metric):
    with pytest.raises(ValueError, match="at least 16"):
        metric(torch.rand(1, 3, 15, 40), torch.rand(1, 3, 15, 40))
    with pytest.raises(ValueError):
        metric(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 17))
    with pytest.raises(ValueError):
        metric(torch.rand(1, 1, 16, 16), torch.rand(1, 1, 16, 16))


def test_nan_pixels_count_as_zero(metric):
    a, b, _, _ = oracle.case("16x16", "n8")
    an = a.clone()
    an[0, 1, 3, 4] = float("nan")
    az = a.clone()
    az[0, 1, 3, 4] = 0.0
    assert torch.equal(metric(an, b), metric(az, b))
    assert torch.equal(oracle.lpips(an, b)[0], oracle.lpips(az, b)[0])


def test_exported_from_the_package():
    import mlic_amd
    assert mlic_amd.LPIPS is metrics.LPIPS and mlic_amd.lpips_synthetic_weights is metrics.lpips_synthetic_weights
    sd, again = metrics.lpips_synthetic_weights(3), metrics.lpips_synthetic_weights(3)
    assert len(sd) == 26 + 5 + 2 and all(torch.equal(sd[k], again[k]) for k in sd)
    assert not torch.equal(sd["net.slice1.0.weight"], metrics.lpips_synthetic_weights(4)["net.slice1.0.weight"])


def _scratch_bytes(B, H, W):
    n = C.c_size_t(0)
    rc = _lib.lib().mlic_lpips_scratch_bytes(B, H, W, C.byref(n))
    return rc, n.value


def test_scratch_bytes_host_only():
    rc, n1 = _scratch_bytes(1, 72, 136)
    assert rc == 0 and n1 > 0
    # two ping-pong buffers of 2 x 64 planes and the pooled planes, at least
    assert n1 >= 2 * (2 * 64 * 72 * 136 * 4) + 2 * 64 * 36 * 68 * 4
    prev = n1
    for B in (2, 3, 8, 32):
        rc, n = _scratch_bytes(B, 72, 136)
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
    for bad, word in (((1, 15, 40), b"16"), ((1, 40, 15), b"16"), ((0, 40, 40), b"B must be positive")):
        rc, _ = _scratch_bytes(*bad)
        assert rc != 0, bad
        assert word in _lib.lib().mlic_last_error()


def test_kernel_entry_refuses_a_null_handle_before_the_gpu():
    """A null handle fails with a message and without a GPU call (this machine has no device: a HIP call
    would fail differently or crash on the fake pointers); so do the handle's other entry points."""
    lib = _lib.lib()
    st = (C.c_int64 * 3)(3 * 16 * 16, 16 * 16, 16)
    fake = C.c_void_p(4096)
    rc, need = _scratch_bytes(1, 16, 16)
    assert rc == 0
    assert lib.mlic_image_lpips_u8(None, None, fake, st, fake, st, 1, 16, 16, fake, need, fake, None) != 0
    assert b"null mlic_lpips handle" in lib.mlic_last_error()
    assert lib.mlic_lpips_set_precision(None, 2) != 0
    assert b"null mlic_lpips handle" in lib.mlic_last_error()
    n = C.c_int64(0)
    assert lib.mlic_lpips_range_fallbacks(None, C.byref(n), 0) != 0
    assert lib.mlic_lpips_destroy(None) == 0


class _StubNet:
    """compress / decompress of the harness without a codec: x_hat = the padded input, darkened."""

    def compress(self, x):
        self.x = x
        return {"strings": [[b"yy"], [b"z"]], "shape": (x.size(2) // 64, x.size(3) // 64)}

    def decompress(self, strings, shape):
        return {"x_hat": self.x * 0.9}


def test_code_image_lpips_field(metric):
    assert inspect.signature(bitstream.code_image).parameters["lpips"].default is None
    img = oracle.case("37x53", "same")[0]
    plain = bitstream.code_image(_StubNet(), img)
    r = bitstream.code_image(_StubNet(), img, lpips=metric)
    assert "lpips" not in plain and set(r) - set(plain) == {"lpips"}
    for k in ("H", "W", "bytes", "bpp", "psnr"):
        assert plain[k] == r[k]
    assert torch.equal(plain["x_hat"], r["x_hat"])
    assert isinstance(r["lpips"], float) and r["lpips"] > 0
    assert r["lpips"] == metric(img, r["x_hat"]).item()
    small = img[:, :, :15, :40]
    assert bitstream.code_image(_StubNet(), small, lpips=metric)["lpips"] is None
