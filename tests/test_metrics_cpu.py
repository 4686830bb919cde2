"""MS-SSIM without a GPU: the float32 torch path of metrics.ms_ssim_u8 against the float64 oracle
(tests/msssim_oracle.py), the error cases, and the host-only scratch-size entry point of the C ABI.

Gates: 1e-5 on the value (half a unit of the fifth decimal; the reference prints four, six in validation
logs) and 5e-5 on every per-level per-channel term; float32 arithmetic of the reference's own form deviates
from the oracle by at most 2.6e-6 / 1.9e-5 on these inputs."""
import ctypes as C

import pytest
import torch

import msssim_oracle as oracle
from mlic_amd import _lib, metrics

VALUE_TOL, TERM_TOL = 1e-5, 5e-5


@pytest.mark.parametrize("kind", oracle.DISTORTIONS)
@pytest.mark.parametrize("shape", list(oracle.SHAPES))
def test_cpu_path_matches_oracle(shape, kind):
    a, b, want, want_terms = oracle.case(shape, kind)
    got, terms = metrics.ms_ssim_u8(a, b, return_terms=True)  # the 180x250 case is a strided view, taken as it is
    assert got.dtype == torch.float64 and got.shape == (1,) and got.device.type == "cpu"
    assert terms.dtype == torch.float64 and terms.shape == want_terms.shape
    err = (got - want).abs().max().item()
    terr = (terms - want_terms).abs().max().item()
    print(f"{shape} {kind}: oracle {want.item():.7f} cpu {got.item():.7f} err {err:.2e} term err {terr:.2e}")
    assert torch.isfinite(got).all() and torch.isfinite(terms).all()
    assert err <= VALUE_TOL
    assert terr <= TERM_TOL
    assert torch.equal(metrics.ms_ssim_u8(a, b), got)
    if kind == "same":
        assert got.item() >= 1 - 1e-6
    if kind == "inv":
        assert got.item() == 0.0


def test_batch_is_per_image():
    a = torch.cat([oracle.case("176x208", "n8")[0], oracle.case("176x208", "blur")[0]])
    b = torch.cat([oracle.case("176x208", "n8")[1], oracle.case("176x208", "blur")[1]])
    want = torch.cat([oracle.case("176x208", "n8")[2], oracle.case("176x208", "blur")[2]])
    got = metrics.ms_ssim_u8(a, b)
    assert got.shape == (2,)
    assert (got - want).abs().max().item() <= VALUE_TOL
    ov, _ = oracle.ms_ssim(a, b)
    assert torch.equal(ov, want)  # the oracle separates images too


def test_errors():
    a = torch.rand(1, 3, 160, 200)
    with pytest.raises(ValueError):
        metrics.ms_ssim_u8(a, a)
    with pytest.raises(ValueError):
        metrics.ms_ssim_u8(torch.rand(1, 3, 200, 160), torch.rand(1, 3, 200, 160))
    with pytest.raises(ValueError):
        metrics.ms_ssim_u8(torch.rand(1, 3, 176, 208), torch.rand(1, 3, 176, 209))
    with pytest.raises(ValueError):
        metrics.ms_ssim_u8(torch.rand(1, 3, 176, 208), torch.rand(1, 1, 176, 208))


def test_ms_ssim_db():
    assert abs(metrics.ms_ssim_db(0.99) - 20.0) <= 1e-12
    assert abs(metrics.ms_ssim_db(torch.tensor(0.99, dtype=torch.float64)).item() - 20.0) <= 1e-12


def test_exported_from_the_package():
    import mlic_amd
    assert mlic_amd.ms_ssim_u8 is metrics.ms_ssim_u8 and mlic_amd.ms_ssim_db is metrics.ms_ssim_db


def test_code_image_ms_ssim_switch_defaults_off():
    """code_image's signature carries the switch and it defaults to off."""
    import inspect
    from mlic_amd import bitstream
    p = inspect.signature(bitstream.code_image).parameters
    assert p["ms_ssim"].default is False


def _scratch_bytes(B, Cn, H, W):
    n = C.c_size_t(0)
    rc = _lib.lib().mlic_ms_ssim_scratch_bytes(B, Cn, H, W, C.byref(n))
    return rc, n.value


def test_scratch_bytes_host_only():
    rc, n1 = _scratch_bytes(1, 3, 161, 161)
    assert rc == 0 and n1 > 0
    prev = n1
    for B in (2, 3, 8, 32):
        rc, n = _scratch_bytes(B, 3, 161, 161)
        assert rc == 0 and n >= prev
        prev = n
    # it holds at least the eight pooled planes and one pair of partial sums per level and plane
    assert n1 >= 2 * 3 * 4 * (81 * 81 + 41 * 41 + 21 * 21 + 11 * 11) + 5 * 3 * 16
    for bad in ((1, 3, 160, 400), (1, 3, 400, 160), (0, 3, 200, 200), (1, 0, 200, 200)):
        rc, _ = _scratch_bytes(*bad)
        assert rc != 0, bad
        assert len(_lib.lib().mlic_last_error()) > 0


def test_kernel_entry_checks_arguments_before_the_gpu():
    """Bad sizes, null pointers and a short scratch fail with a message and without a GPU call (this
    machine has no device: a HIP call would fail differently or crash on the fake pointers)."""
    lib = _lib.lib()
    st = (C.c_int64 * 3)(3 * 161 * 161, 161 * 161, 161)
    fake = C.c_void_p(4096)
    rc, need = _scratch_bytes(1, 3, 161, 161)
    assert rc == 0
    assert lib.mlic_image_ms_ssim_u8(None, fake, st, fake, st, 1, 3, 160, 161, fake, need, fake, None) != 0
    assert b"160" in lib.mlic_last_error()
    assert lib.mlic_image_ms_ssim_u8(None, None, st, fake, st, 1, 3, 161, 161, fake, need, fake, None) != 0
    assert b"null" in lib.mlic_last_error()
    assert lib.mlic_image_ms_ssim_u8(None, fake, st, fake, st, 1, 3, 161, 161, fake, need, None, None) != 0
    assert b"null" in lib.mlic_last_error()
    assert lib.mlic_image_ms_ssim_u8(None, fake, st, fake, st, 1, 3, 161, 161, None, need, fake, None) != 0
    assert b"scratch" in lib.mlic_last_error()
    assert lib.mlic_image_ms_ssim_u8(None, fake, st, fake, st, 1, 3, 161, 161, fake, need - 1, fake, None) != 0
    assert b"scratch" in lib.mlic_last_error()
