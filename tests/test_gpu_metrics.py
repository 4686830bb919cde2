"""MS-SSIM on the GPU: mlic_image_ms_ssim_u8 (csrc/metrics.hip) and metrics.ms_ssim_u8 on CUDA tensors
against the float64 oracle (tests/msssim_oracle.py), with the gates of tests/test_metrics_cpu.py: 1e-5 on
the value, 5e-5 on every per-level per-channel term.  Every direct call runs on NaN-filled scratch, out
and terms, with a sentinel-filled guard behind the scratch inside the same allocation."""
import ctypes as C
import math

import pytest
import torch

import msssim_oracle as oracle
from mlic_amd import _lib, bitstream, get_model, metrics, synthetic

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
VALUE_TOL, TERM_TOL = 1e-5, 5e-5
GUARD, SENTINEL = 4096, 0xA5


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_kernel(a, b, with_terms=True):
    """mlic_image_ms_ssim_u8 on two CUDA [B,C,H,W] float32 tensors (views with unit column stride as they
    are): (out [B], terms [B,5,C]) on the CPU.  Poisoned buffers, guarded scratch."""
    assert a.is_cuda and a.dtype == torch.float32 and a.stride(3) == 1 and b.stride(3) == 1
    B, Cn, H, W = a.shape
    need = C.c_size_t()
    _lib.call("mlic_ms_ssim_scratch_bytes", B, Cn, H, W, C.byref(need))
    need = need.value
    buf = torch.empty(need + GUARD, dtype=torch.uint8, device=DEV)
    buf[:need].fill_(0xFF)  # all-ones words: NaN as float and as double
    buf[need:].fill_(SENTINEL)
    out = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
    terms = torch.full((B, 5, Cn), float("nan"), dtype=torch.float64, device=DEV)
    sa, sb = (C.c_int64 * 3)(*a.stride()[:3]), (C.c_int64 * 3)(*b.stride()[:3])
    _lib.call("mlic_image_ms_ssim_u8", _stream(), _p(a), sa, _p(b), sb, B, Cn, H, W, _p(buf), need, _p(out),
              _p(terms) if with_terms else None)
    torch.cuda.synchronize()
    assert bool((buf[need:] == SENTINEL).all()), "the kernel wrote behind its scratch"
    if not with_terms:
        assert bool(torch.isnan(terms).all())
    return out.cpu(), terms.cpu()


@pytest.mark.parametrize("kind", oracle.DISTORTIONS)
@pytest.mark.parametrize("shape", list(oracle.SHAPES))
def test_parity_with_oracle(shape, kind):
    a, b, want, want_terms = oracle.case(shape, kind)
    ad, bd = oracle.on_device(shape, kind, DEV)  # the strided case keeps its storage and strides
    assert ad.stride() == a.stride() and bd.stride() == b.stride()
    got, terms = run_kernel(ad, bd)
    pv, pt = metrics.ms_ssim_u8(ad, bd, return_terms=True)
    assert pv.is_cuda and pv.dtype == torch.float64 and pv.shape == (1,)
    pv, pt = pv.cpu(), pt.cpu()
    err, terr = (got - want).abs().max().item(), (terms - want_terms).abs().max().item()
    perr, pterr = (pv - want).abs().max().item(), (pt - want_terms).abs().max().item()
    print(f"{shape} {kind}: oracle {want.item():.7f} kernel {got.item():.7f} err {err:.2e} term err {terr:.2e}; "
          f"python err {perr:.2e} term err {pterr:.2e}")
    assert torch.isfinite(got).all() and torch.isfinite(terms).all()
    assert torch.isfinite(pv).all() and torch.isfinite(pt).all()
    assert err <= VALUE_TOL and perr <= VALUE_TOL
    assert terr <= TERM_TOL and pterr <= TERM_TOL
    assert torch.equal(pv, got) and torch.equal(pt, terms)  # one kernel, one result
    assert torch.equal(metrics.ms_ssim_u8(ad, bd).cpu(), got)
    if kind == "same":
        assert got.item() >= 1 - 1e-6
    if kind == "inv":
        assert got.item() == 0.0


def test_same_call_twice_same_bits_and_terms_optional():
    a, b, _, _ = oracle.case("333x517", "n8")
    ad, bd = a.to(DEV), b.to(DEV)
    v1, t1 = run_kernel(ad, bd)
    v2, t2 = run_kernel(ad, bd)
    assert torch.equal(v1, v2) and torch.equal(t1, t2)
    v3, _ = run_kernel(ad, bd, with_terms=False)
    assert torch.equal(v1, v3)


def test_batch_of_two_equals_two_single_calls():
    a = oracle.case("176x208", "n8")[0]
    b0, b1 = oracle.case("176x208", "n8")[1], oracle.case("176x208", "blur")[1]
    want = torch.cat([oracle.case("176x208", "n8")[2], oracle.case("176x208", "blur")[2]])
    a2, b2 = torch.cat([a, a]).to(DEV), torch.cat([b0, b1]).to(DEV)
    v, t = run_kernel(a2, b2)
    assert (v - want).abs().max().item() <= VALUE_TOL
    assert v[0].item() != v[1].item()
    for i in range(2):
        vi, ti = run_kernel(a2[i:i + 1], b2[i:i + 1])
        assert torch.equal(vi[0], v[i]) and torch.equal(ti[0], t[i])


def test_strided_view_equals_contiguous_copy():
    ad, bd = oracle.on_device("180x250v", "n8", DEV)
    assert not ad.is_contiguous()
    v, t = run_kernel(ad, bd)
    vc, tc = run_kernel(ad.contiguous(), bd.contiguous())
    assert torch.equal(v, vc) and torch.equal(t, tc)
    # a view of one operand only, and a view whose column stride is not 1 (copied by the Python layer)
    vm, _ = run_kernel(ad, bd.contiguous())
    assert torch.equal(vm, v)
    at = ad.contiguous().transpose(2, 3).contiguous().transpose(2, 3)
    assert at.stride(3) != 1
    assert torch.equal(metrics.ms_ssim_u8(at, bd).cpu(), v)


def test_sq_err_shares_the_u8_convention():
    """mlic_image_sq_err_u8 on the same tensors: the exact integer sum of the uint8 images' squared
    differences, and bitstream.psnr_u8's PSNR (the unclamped noisy image exercises the clamp)."""
    for kind in ("n8", "n32", "off"):
        a, b, _, _ = oracle.case("176x208", kind)
        ad, bd = a.to(DEV).contiguous(), b.to(DEV).contiguous()
        out = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
        _lib.call("mlic_image_sq_err_u8", _stream(), _p(ad), _p(bd), 1, ad[0].numel(), _p(out))
        torch.cuda.synchronize()
        want = ((bitstream.to_u8(a).long() - bitstream.to_u8(b).long()) ** 2).sum().item()
        assert out.item() == float(want)
        assert torch.equal(oracle.to_u8_f64(a), bitstream.to_u8(a).double())
        psnr = 20 * math.log10(255.0) - 10 * math.log10(out.item() / ad.numel())
        assert abs(psnr - bitstream.psnr_u8(ad, bd)) <= 1e-3
        assert abs(psnr - bitstream.psnr_u8(a, b)) <= 1e-3


def test_python_errors_on_the_device():
    a = torch.rand(1, 3, 160, 200, device=DEV)
    with pytest.raises(ValueError):
        metrics.ms_ssim_u8(a, a)
    with pytest.raises(ValueError):
        metrics.ms_ssim_u8(torch.rand(1, 3, 176, 208, device=DEV), torch.rand(1, 3, 176, 209, device=DEV))


def test_harness_reports_ms_ssim():
    net = get_model("MLICPP_S")
    net.load_state_dict(synthetic.synth_state_dict("MLICPP_S", 0))
    net = net.to(DEV).eval()
    net.update()
    img = synthetic.synth_image(192, 256, 3).to(DEV)[:, :, :180, :250]
    r = bitstream.code_image(net, img, ms_ssim=True)
    assert r["x_hat"].shape == img.shape and not r["x_hat"].is_contiguous()
    assert isinstance(r["ms_ssim"], float) and math.isfinite(r["ms_ssim"])
    assert r["ms_ssim"] == metrics.ms_ssim_u8(img, r["x_hat"]).item()
    want, _ = oracle.ms_ssim(img.cpu(), r["x_hat"].cpu())
    print(f"harness ms_ssim {r['ms_ssim']:.7f} oracle {want.item():.7f} psnr {r['psnr']:.3f}")
    assert abs(r["ms_ssim"] - want.item()) <= VALUE_TOL
    plain = bitstream.code_image(net, img)
    assert "ms_ssim" not in plain
    assert set(r) - set(plain) == {"ms_ssim"}
    assert torch.equal(plain["x_hat"], r["x_hat"]) and plain["bytes"] == r["bytes"] and plain["psnr"] == r["psnr"]
    small = synthetic.synth_image(128, 192, 3).to(DEV)
    assert bitstream.code_image(net, small, ms_ssim=True)["ms_ssim"] is None
    assert not any(net.range_fallbacks(reset=True).values())
