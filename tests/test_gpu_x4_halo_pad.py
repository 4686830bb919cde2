"""conv_x4's halo form on the padded halo image (row pitch 144 bytes, no XOR: a tap's shift is a constant
byte offset) against the per-tap form: the same operands in the same MFMA order, so with the K loop unsplit
the outputs are bit-identical, and both agree with a float64 reference to the split-fp16 tolerance.

Kernel cases go through mlic_conv_run as tests/test_gpu_conv.py does (its run / check restated here); the
whole-model case compares forward, compress and decompress of MLICPP_L with "x4_halo" 0 against 1."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from mlic_amd import _lib, get_model, synthetic

pytestmark = pytest.mark.gpu

GELU, SHUFFLE = 1, 128
X4 = 7
DEV = torch.device("cuda:0")


def run(B, Cin, Cout, H, W, K, epi, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, Cin, H, W, generator=g) - 0.5).to(DEV)
    w = ((torch.rand(Cout, Cin, K, K, generator=g) - 0.5) / (Cin * K * K) ** 0.5).to(DEV)
    b = (torch.rand(Cout, generator=g) - 0.5).to(DEV)
    oshape = (B, Cout // 4, 2 * H, 2 * W) if epi & SHUFFLE else (B, Cout, H, W)
    y = torch.full(oshape, float("nan"), device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    _lib.call("mlic_conv_run", C.c_void_p(st), X4, ptr(x), ptr(w), ptr(b), ptr(y), B, Cin, Cout, H, W, K, 1, epi,
              None, None)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=K // 2)
    if epi & GELU:
        ref = F.gelu(ref)
    if epi & SHUFFLE:
        ref = F.pixel_shuffle(ref, 2)
    return y, ref.float()


def check(y, ref, rtol=2e-5):
    assert torch.isfinite(y).all(), "unwritten or non-finite outputs"
    err = (y - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err <= rtol * scale + 1e-6, f"max err {err:.3e} (scale {scale:.3e})"


def _arms(shape, splits):
    res = {}
    try:
        for split in splits:
            _lib.call("mlic_set_kernel_option", b"x4_splitk", split)
            for halo in (1, 0):
                _lib.call("mlic_set_kernel_option", b"x4_halo", halo)
                res[(split, halo)] = run(*shape)
    finally:
        _lib.call("mlic_set_kernel_option", b"x4_halo", -1)
        _lib.call("mlic_set_kernel_option", b"x4_splitk", -1)
    return res


@pytest.mark.parametrize("shape", [
    (1, 32, 64, 8, 32, 3, 0),                   # one chunk, exactly one tile, 64-row tile
    (1, 64, 128, 9, 33, 3, 0),                  # one row and one column over a tile (clamped halo lines on both
                                                # edges); two chunks: both halo slots; 128-row tile
    (2, 96, 192, 16, 40, 3, GELU),              # odd chunk count (slot parity across the loop end), B = 2, 192 rows
    (1, 64, 224, 10, 34, 3, 0),                 # 224-row tile
    (1, 192, 768, 17, 65, 3, SHUFFLE | GELU),   # the 256-row instantiation at the LDS limit; 6 chunks; three
                                                # column tiles; ragged edges; the shuffle epilogue
    (1, 40, 64, 8, 31, 3, 0),                   # Cin not a multiple of 32; W < 32
    (1, 64, 96, 12, 36, 5, 0),                  # 5 x 5, 96-row tile
    (1, 288, 96, 13, 37, 5, 0),                 # 5 x 5, 96-row tile, 9 chunks
])
def test_x4_halo_pad_vs_per_tap(shape):
    res = _arms(shape, (0,))
    for y, ref in res.values():
        check(y, ref)
    assert torch.equal(res[(0, 1)][0], res[(0, 0)][0])


def test_x4_halo_pad_split_k():
    """Split-K forced on for the few-tile 5 x 5 shape: the halo form's K ranges lie on chunk boundaries, so the
    sums are ordered differently from the per-tap form's; each arm is checked against float64."""
    res = _arms((1, 288, 96, 13, 37, 5, 0), (0, 1))
    for y, ref in res.values():
        check(y, ref)
    assert torch.equal(res[(0, 1)][0], res[(0, 0)][0])


def _whole_model(net, x):
    f = net(x)
    c = net.compress(x)
    d = net.decompress(c["strings"], c["shape"])
    return f["x_hat"].cpu(), f["likelihoods"]["y_likelihoods"].cpu(), c["strings"], d["x_hat"].cpu()


def test_whole_model_same_bits():
    """MLICPP_L at 128 x 192, two images: forward() (x_hat, likelihoods), compress() bytes and decompress() x_hat
    with every 3 x 3 and 5 x 5 stride-1 x4 conv staged per tap ("x4_halo" 0) and on the halo image (1)."""
    net = get_model("MLICPP_L")
    net.load_state_dict(synthetic.synth_state_dict("MLICPP_L", 0))
    net = net.to(DEV).eval()
    net.update()
    x = torch.cat([synthetic.synth_image(128, 192, 80 + i) for i in range(2)]).to(DEV)
    outs = []
    try:
        for v in (0, 1):
            _lib.call("mlic_set_kernel_option", b"x4_halo", v)
            outs.append(_whole_model(net, x))
            torch.cuda.synchronize()
    finally:
        _lib.call("mlic_set_kernel_option", b"x4_halo", -1)
    (fx0, lk0, s0, dx0), (fx1, lk1, s1, dx1) = outs
    assert torch.isfinite(fx0).all()
    assert s0 == s1
    assert torch.equal(fx0, fx1) and torch.equal(lk0, lk1) and torch.equal(dx0, dx1)
    assert torch.equal(dx1, fx1)
