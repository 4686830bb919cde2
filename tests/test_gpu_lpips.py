"""LPIPS-VGG on the GPU: mlic_image_lpips_u8 (csrc/lpips.hip) and metrics.LPIPS on CUDA tensors against the
float64 oracle (tests/lpips_oracle.py).  Every direct call runs on NaN-filled scratch, out and terms, with a
sentinel-filled guard behind the scratch inside the same allocation.

Gate (relative, on the value and on every term): 8 x the largest error of the float32 torch-CPU restatement
(metrics.LPIPS on CPU tensors) against the oracle on these same cases -- split-fp16 operands carry about 2^-22
against fp32's 2^-24 (4 x), and a different summation order doubles it (2 x).  CPU_MAX_* are those maxima as
tests/test_lpips_cpu.py prints them (the value's at 72x136v "off", the terms' at 37x53 "n1"); the GPU's
own maxima are recorded in DESIGN.md §3."""
import ctypes as C
import math

import pytest
import torch

import lpips_oracle as oracle
from mlic_amd import _lib, bitstream, get_model, metrics, synthetic

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CPU_MAX_VALUE, CPU_MAX_TERM = 2.91e-7, 6.12e-6
VALUE_TOL, TERM_TOL = 8 * CPU_MAX_VALUE, 8 * CPU_MAX_TERM
GUARD, SENTINEL = 4096, 0xA5
EPI_RELU_IN = 512


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def make_handle(sd):
    """mlic_lpips_create on the `lpips` package's own names (the Python class passes the bare features names)."""
    names = list(sd)
    return metrics.lpips_create_handle(names, [sd[k].float().to(DEV) for k in names], DEV)


@pytest.fixture(scope="module")
def handle():
    h = make_handle(oracle.weights())
    yield h
    _lib.call("mlic_lpips_destroy", h)


@pytest.fixture(scope="module")
def metric():
    m = metrics.LPIPS(oracle.weights())
    yield m
    m.close()


def fallbacks(h, reset=False):
    n = C.c_int64(-1)
    _lib.call("mlic_lpips_range_fallbacks", h, C.byref(n), 1 if reset else 0)
    return n.value


def run_kernel(h, a, b, with_terms=True):
    """mlic_image_lpips_u8 on two CUDA [B,3,H,W] float32 tensors (views with unit column stride as they are):
    (out [B], terms [B,5]) on the CPU.  Poisoned buffers, guarded scratch."""
    assert a.is_cuda and a.dtype == torch.float32 and a.stride(3) == 1 and b.stride(3) == 1
    B, _, H, W = a.shape
    need = C.c_size_t()
    _lib.call("mlic_lpips_scratch_bytes", B, H, W, C.byref(need))
    need = need.value
    buf = torch.empty(need + GUARD, dtype=torch.uint8, device=DEV)
    buf[:need].fill_(0xFF)  # all-ones words: NaN as float, as double and as fp16
    buf[need:].fill_(SENTINEL)
    out = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
    terms = torch.full((B, 5), float("nan"), dtype=torch.float64, device=DEV)
    sa, sb = (C.c_int64 * 3)(*a.stride()[:3]), (C.c_int64 * 3)(*b.stride()[:3])
    _lib.call("mlic_image_lpips_u8", h, _stream(), _p(a), sa, _p(b), sb, B, H, W, _p(buf), need, _p(out),
              _p(terms) if with_terms else None)
    torch.cuda.synchronize()
    assert bool((buf[need:] == SENTINEL).all()), "the kernels wrote behind their scratch"
    if not with_terms:
        assert bool(torch.isnan(terms).all())
    return out.cpu(), terms.cpu()


def check_gate(tag, got, terms, want, want_terms):
    assert torch.isfinite(got).all() and torch.isfinite(terms).all()
    err, terr = oracle.rel_err(got, want), oracle.rel_err(terms, want_terms)
    print(f"{tag}: oracle {want.flatten()[0].item():.6e} gpu {got.flatten()[0].item():.6e} rel err {err:.2e} "
          f"term rel err {terr:.2e}")
    assert err <= VALUE_TOL, (tag, err)
    assert terr <= TERM_TOL, (tag, terr)


@pytest.mark.parametrize("kind", oracle.DISTORTIONS)
@pytest.mark.parametrize("shape", list(oracle.SHAPES))
def test_parity_with_oracle(handle, metric, shape, kind):
    a, b, want, want_terms = oracle.case(shape, kind)
    ad, bd = oracle.on_device(shape, kind, DEV)  # the strided case keeps its storage and strides
    assert ad.stride() == a.stride() and bd.stride() == b.stride()
    got, terms = run_kernel(handle, ad, bd)
    pv, pt = metric(ad, bd, return_terms=True)
    assert pv.is_cuda and pv.dtype == torch.float64 and pv.shape == (1,) and pt.shape == (1, 5)
    assert torch.equal(pv.cpu(), got) and torch.equal(pt.cpu(), terms)  # one library, one result
    assert torch.equal(metric(ad, bd).cpu(), got)
    if kind == "same":
        assert got.item() == 0.0 and not terms.any()  # subtract, then square: exactly 0
    else:
        check_gate(f"{shape} {kind}", got, terms, want, want_terms)


def test_values_are_ordered(handle):
    for shape in oracle.SHAPES:
        v = {k: run_kernel(handle, *oracle.on_device(shape, k, DEV))[0].item() for k in ("n1", "n8", "inv")}
        assert v["inv"] > v["n8"] > v["n1"] > 0, (shape, v)


def test_same_call_twice_same_bits_and_terms_optional(handle):
    ad, bd = oracle.on_device("72x136", "n8", DEV)
    v1, t1 = run_kernel(handle, ad, bd)
    v2, t2 = run_kernel(handle, ad, bd)
    assert torch.equal(v1, v2) and torch.equal(t1, t2)
    v3, _ = run_kernel(handle, ad, bd, with_terms=False)
    assert torch.equal(v1, v3)
    assert abs(t1.sum().item() - v1.item()) <= 1e-15


def test_batch_of_three_equals_three_single_calls(handle):
    kinds = ("n1", "blur", "inv")
    a = oracle.case("37x53", "n1")[0]
    a3 = torch.cat([a, a, a]).to(DEV)
    b3 = torch.cat([oracle.case("37x53", k)[1] for k in kinds]).to(DEV)
    want = torch.cat([oracle.case("37x53", k)[2] for k in kinds])
    want_terms = torch.cat([oracle.case("37x53", k)[3] for k in kinds])
    v, t = run_kernel(handle, a3, b3)
    check_gate("37x53 batch", v, t, want, want_terms)
    assert len(set(v.tolist())) == 3
    for i in range(3):
        vi, ti = run_kernel(handle, a3[i:i + 1], b3[i:i + 1])
        assert torch.equal(vi[0], v[i]) and torch.equal(ti[0], t[i])


def test_chunked_batch_equals_single_calls(handle):
    """More pairs than one chunk holds (the scratch need stops growing at the chunk size): the images of the
    first chunk, of the boundary and of the ragged last chunk equal their single calls."""
    H = W = 256

    def need(B):
        n = C.c_size_t()
        _lib.call("mlic_lpips_scratch_bytes", B, H, W, C.byref(n))
        return n.value

    nb = 1
    while need(nb + 1) > need(nb):
        nb += 1
    assert 8 <= nb <= 64 and need(nb) <= 2 ** 32 and need(1000) == need(nb)
    B = nb + 2
    base = synthetic.synth_image(H, W, 9).to(DEV)
    gen = torch.Generator(device="cpu").manual_seed(3)
    noise = torch.randn(B, 3, H, W, generator=gen).to(DEV)
    sigma = (torch.arange(B, device=DEV).float() % 7 + 1).view(B, 1, 1, 1) / 255.0
    a = base.expand(B, 3, H, W).contiguous()
    b = a + noise * sigma
    v, t = run_kernel(handle, a, b)
    assert torch.isfinite(v).all() and (v > 0).all()
    for i in (0, nb - 1, nb, B - 1):
        vi, ti = run_kernel(handle, a[i:i + 1], b[i:i + 1])
        assert torch.equal(vi[0], v[i]) and torch.equal(ti[0], t[i]), i


def test_strided_view_equals_contiguous_copy(handle, metric):
    ad, bd = oracle.on_device("72x136v", "n8", DEV)
    assert not ad.is_contiguous() and not bd.is_contiguous()
    v, t = run_kernel(handle, ad, bd)
    vc, tc = run_kernel(handle, ad.contiguous(), bd.contiguous())
    assert torch.equal(v, vc) and torch.equal(t, tc)
    # a view of one operand only, and a view whose column stride is not 1 (copied by the Python layer)
    vm, tm = run_kernel(handle, ad, bd.contiguous())
    assert torch.equal(vm, v) and torch.equal(tm, t)
    at = ad.contiguous().transpose(2, 3).contiguous().transpose(2, 3)
    assert at.stride(3) != 1
    assert torch.equal(metric(at, bd).cpu(), v)


def test_precision_0_passes_the_same_gate_and_nothing_fell_back(handle, metric):
    """Runs after the tests above (file order): no call so far needed the fp32 re-run."""
    assert fallbacks(handle) == 0 and metric.range_fallbacks() == 0
    h = make_handle(oracle.weights())
    try:
        _lib.call("mlic_lpips_set_precision", h, 0)
        for shape in oracle.SHAPES:
            for kind in oracle.DISTORTIONS:
                _, _, want, want_terms = oracle.case(shape, kind)
                got, terms = run_kernel(h, *oracle.on_device(shape, kind, DEV))
                if kind == "same":
                    assert got.item() == 0.0 and not terms.any()
                else:
                    check_gate(f"precision 0 {shape} {kind}", got, terms, want, want_terms)
        assert fallbacks(h) == 0
        assert _lib.lib().mlic_lpips_set_precision(h, 1) != 0
        assert b"precision" in _lib.lib().mlic_last_error()
    finally:
        _lib.call("mlic_lpips_destroy", h)


def test_range_fallback_is_counted_and_stays_within_the_gate(handle):
    """conv1_1 scaled by 3e4: its activations pass fp16's 65520, the guard fires at conv1_2's operand pack and
    the call runs again with the fp32 convs.  The handled numeric guard, not a fault.  Policy: the whole call
    is re-run, so a batch is one fallback."""
    sd = oracle.weights(3e4)
    a, b, _, _ = oracle.case("37x53", "n8")
    want, want_terms = oracle.lpips(a, b, sd)
    ad, bd = oracle.on_device("37x53", "n8", DEV)
    before, _ = run_kernel(handle, ad, bd)
    h = make_handle(sd)
    try:
        got, terms = run_kernel(h, ad, bd)
        check_gate("range fallback 37x53 n8", got, terms, want, want_terms)
        assert fallbacks(h) == 1
        assert fallbacks(h, reset=True) == 1 and fallbacks(h) == 0
        a2, b2 = torch.cat([ad, ad]), torch.cat([bd, oracle.on_device("37x53", "blur", DEV)[1]])
        v2, _ = run_kernel(h, a2, b2)
        assert fallbacks(h) == 1  # one call, one re-run
        assert torch.equal(v2[0], got[0])  # the fp32 re-run is per image too
    finally:
        _lib.call("mlic_lpips_destroy", h)
    after, _ = run_kernel(handle, ad, bd)
    assert torch.equal(before, after) and fallbacks(handle) == 0


def test_entry_checks_its_arguments(handle):
    lib = _lib.lib()
    ad, bd = oracle.on_device("16x16", "n8", DEV)
    st = (C.c_int64 * 3)(*ad.stride()[:3])
    need = C.c_size_t()
    _lib.call("mlic_lpips_scratch_bytes", 1, 16, 16, C.byref(need))
    buf = torch.zeros(need.value, dtype=torch.uint8, device=DEV)
    out = torch.zeros(1, dtype=torch.float64, device=DEV)

    def call(B=1, H=16, W=16, scratch=buf, nbytes=need.value, o=out):
        return lib.mlic_image_lpips_u8(handle, _stream(), _p(ad), st, _p(bd), st, B, H, W,
                                       None if scratch is None else _p(scratch), nbytes, None if o is None else _p(o),
                                       None)

    for kw, word in ((dict(B=0), b"B must be positive"), (dict(H=15), b"at least 16"), (dict(W=15), b"at least 16"),
                     (dict(nbytes=need.value - 1), b"scratch too small"), (dict(scratch=None), b"scratch too small"),
                     (dict(o=None), b"null out")):
        assert call(**kw) != 0, kw
        assert word in lib.mlic_last_error(), (kw, lib.mlic_last_error())
    assert call() == 0


def test_pack_flag_relu_in_equals_relu_then_conv():
    """mlic_conv_run on impl 7 (conv_x4) with EPI_RELU_IN equals the same conv on relu(x), bit for bit."""
    gen = torch.Generator().manual_seed(11)
    B, Cin, Cout, H, W = 2, 64, 128, 18, 26
    x = torch.randn(B, Cin, H, W, generator=gen).to(DEV)
    w = (torch.randn(Cout, Cin, 3, 3, generator=gen) * 0.05).to(DEV)
    bias = torch.randn(Cout, generator=gen).to(DEV)
    outs = []
    for inp, epi in ((x, EPI_RELU_IN), (torch.relu(x), 0)):
        y = torch.full((B, Cout, H, W), float("nan"), device=DEV)
        _lib.call("mlic_conv_run", _stream(), 7, _p(inp), _p(w), _p(bias), _p(y), B, Cin, Cout, H, W, 3, 1, epi,
                  None, None)
        outs.append(y)
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])
    ref = torch.nn.functional.conv2d(torch.relu(x).double(), w.double(), bias.double(), padding=1)
    assert (outs[0].double() - ref).abs().max().item() <= 1e-5
    # the other families do not know the flag: refused, not ignored
    y = torch.empty(B, Cout, H, W, device=DEV)
    assert _lib.lib().mlic_conv_run(_stream(), 2, _p(x), _p(w), _p(bias), _p(y), B, Cin, Cout, H, W, 3, 1,
                                    EPI_RELU_IN, None, None) != 0
    assert b"EPI_RELU_IN" in _lib.lib().mlic_last_error()


def test_harness_reports_lpips(metric):
    net = get_model("MLICPP_S")
    net.load_state_dict(synthetic.synth_state_dict("MLICPP_S", 0))
    net = net.to(DEV).eval()
    net.update()
    img = synthetic.synth_image(128, 192, 3).to(DEV)
    r = bitstream.code_image(net, img, lpips=metric)
    assert isinstance(r["lpips"], float) and math.isfinite(r["lpips"]) and r["lpips"] > 0
    assert r["lpips"] == metric(img, r["x_hat"]).item()
    print(f"harness lpips {r['lpips']:.6e} psnr {r['psnr']:.3f}")
    plain = bitstream.code_image(net, img)
    assert "lpips" not in plain and set(r) - set(plain) == {"lpips"}
    assert torch.equal(plain["x_hat"], r["x_hat"]) and plain["bytes"] == r["bytes"] and plain["psnr"] == r["psnr"]
    assert metric.range_fallbacks() == 0
