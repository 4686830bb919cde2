"""Work whose result nobody reads, skipped behind kernel options: each test runs the option off (the
whole-grid launches) against the option on and compares bit for bit, with the workspace NaN-poisoned
(conftest), so a read of a pixel the half form no longer writes would show.

"lrp_half": the LRP head (last depthwise + 128 -> 32 point conv with 0.5 tanh, checkerboard mask and the
residual into y_hat) on its phase's half only.  "intra_half": the intra context's queries.0 / keys.0 read
x1 through the resident 1x1's input parity mask (no masked copies), and its tail mlp.2 / mlp.4 runs on the
non-anchor half when the only consumer does.  "gdn_skip": g_a's first 1x1 stride-2 skip conv (3 -> N) computed
inside the GDN launch that adds it, where that launch is dwpw3's pointwise form.

The half forms engage only where the whole-grid layer runs as dw3x3 + pw_resident_kernel, i.e. from 1024
latent pixels per image (conv_select); below that both arms issue the same launches and the comparison
pins exactly that.  The grids 8 x 12, 12 x 20 and 8 x 68 are below it, 32 x 32 (strip depthwise as the
whole-grid comparator) and 16 x 68 (the LDS-tile depthwise as comparator, W > 64) are above it."""
import pytest
import torch

from mlic_amd import _lib, get_model, spec, synthetic

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
_NETS = {}

GRIDS = [(8, 12), (12, 20), (8, 68), (32, 32), (16, 68)]
ENGAGED = {(32, 32), (16, 68)}  # >= 1024 pixels per image: the resident 1x1 serves the latent convs


def net_for(name):
    if name not in _NETS:
        n = get_model(name)
        n.load_state_dict(synthetic.synth_state_dict(name, 0))
        _NETS[name] = n.to(DEV).eval()
    return _NETS[name]


def _randn(shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def _nonanchor(H, W):
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return ((y + x) % 2 == 0)


def _both(option, values, run):
    outs = []
    try:
        for v in values:
            _lib.call("mlic_set_kernel_option", option, v)
            outs.append(run())
            torch.cuda.synchronize()
    finally:
        _lib.call("mlic_set_kernel_option", option, -1)
    return outs


@pytest.mark.parametrize("hw", GRIDS)
@pytest.mark.parametrize("which,idx", [("lrpa", 0), ("lrpa", 9), ("lrpn", 0), ("lrpn", 9)])
def test_lrp_head_half_same_bits(which, idx, hw):
    """Every pixel of res + mask(0.5 tanh(lrp(x))) equals the whole-grid form's; the residual holds no -0.0
    (the one value the whole-grid form's `res + 0.0f` at dropped pixels would change)."""
    net = net_for("MLICPP_L")
    H, W = hw
    cin = spec.state_dict_shapes("MLICPP_L")[f"lrp_anchor.{idx}.lrp_transform.0.depth_conv.weight"][0]
    x = _randn((2, cin, H, W), 100 + idx)
    res = _randn((2, 32, H, W), 200 + idx, 3.0)
    assert not ((res == 0) & torch.signbit(res)).any()
    off, on = _both(b"lrp_half", (0, 1), lambda: net.run_module(which, idx, x, res, out_shape=(2, 32, H, W)).cpu())
    assert torch.isfinite(off).all()
    assert torch.equal(off, on)
    # the other half is the residual, untouched
    other = _nonanchor(H, W) if which == "lrpa" else ~_nonanchor(H, W)
    assert torch.equal(on[:, :, other], res.cpu()[:, :, other])
    assert not torch.equal(on, res.cpu())


@pytest.mark.parametrize("hw", GRIDS)
def test_intra_context_unread_work_same_bits(hw):
    """intra at slice 1: option 0 (two masked copies, whole-grid tail) against 1 (input parity mask, whole-grid
    tail: every pixel equal) and 2 (the slice loop's half tail forced for the module entry: the non-anchor
    pixels equal; where the half form engages the anchor pixels are not written and keep the poison)."""
    net = net_for("MLICPP_L")
    H, W = hw
    x1 = _randn((2, 32, H, W), 11, 2.0)
    x2 = _randn((2, 32, H, W), 12, 2.0)
    off, on, half = _both(b"intra_half", (0, 1, 2),
                          lambda: net.run_module("intra", 1, x1, x2, out_shape=(2, 64, H, W)).cpu())
    assert torch.isfinite(off).all()
    assert torch.equal(off, on)
    na = _nonanchor(H, W)
    assert torch.equal(off[:, :, na], half[:, :, na])
    if hw in ENGAGED and _lib.poison():
        assert torch.isnan(half[:, :, ~na]).all()
    else:
        assert torch.equal(off, half)


def _whole_model(net, x):
    f = net(x)
    c = net.compress(x)
    d = net.decompress(c["strings"], c["shape"])
    return f["x_hat"].cpu(), f["likelihoods"]["y_likelihoods"].cpu(), c["strings"], d["x_hat"].cpu()


@pytest.mark.parametrize("shape", [(2, 3, 64, 128), (1, 3, 70, 134)])
@pytest.mark.parametrize("name,N", [("MLICPP_L", 192), ("MLICPP_S", 96)])
def test_rbws0_skip_in_gdn_same_bits(name, N, shape):
    """g_a's first ResidualBlockWithStride with the 3 -> N skip conv as its own launch ("gdn_skip" 0) and computed
    in the GDN epilogue (1), the GDN on dwpw3's pointwise form at every grid ("pw3" 2).  70 x 134: odd output
    sizes (35 x 67), a strip edge that is no multiple of 64."""
    net = net_for(name)
    B, _, H, W = shape
    x = _randn(shape, 7).abs().clamp(max=1.0)
    out_shape = (B, N, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
    try:
        _lib.call("mlic_set_kernel_option", b"pw3", 2)
        off, on = _both(b"gdn_skip", (0, 1), lambda: net.run_module("rbws", 0, x, None, out_shape=out_shape).cpu())
    finally:
        _lib.call("mlic_set_kernel_option", b"pw3", -1)
    assert torch.isfinite(off).all()
    assert torch.equal(off, on)


@pytest.mark.parametrize("hw", [(128, 192), (192, 320)])
@pytest.mark.parametrize("option", [b"lrp_half", b"intra_half", b"gdn_skip"])
def test_whole_model_same_bits(option, hw):
    """forward() (x_hat, likelihoods), compress() bytes and decompress() x_hat with the option off and on, as
    test_ep_half_grid_same_bits does for "ep_half".  For "gdn_skip" both arms run with "pw3" = 2, so that the
    GDN of g_a's first block is the launch that can take the skip conv at these sizes."""
    net = net_for("MLICPP_L")
    net.update()
    x = torch.cat([synthetic.synth_image(hw[0], hw[1], 80 + i) for i in range(2)]).to(DEV)
    try:
        if option == b"gdn_skip":
            _lib.call("mlic_set_kernel_option", b"pw3", 2)
        (fx0, lk0, s0, dx0), (fx1, lk1, s1, dx1) = _both(option, (0, 1), lambda: _whole_model(net, x))
    finally:
        _lib.call("mlic_set_kernel_option", b"pw3", -1)
    assert s0 == s1
    assert torch.equal(fx0, fx1) and torch.equal(lk0, lk1) and torch.equal(dx0, dx1)
    assert torch.equal(dx1, fx1)


# a 512 x 512 image has a 32 x 32 latent: the smallest square input whose latent convs run on the resident 1x1,
# so the half forms engage inside the slice loop
@pytest.mark.parametrize("hw", [(128, 192), (512, 512)])
def test_whole_model_without_ep_half(hw):
    """"ep_half" = 0 with the new options on: the intra context's consumer then reads the whole grid, so the
    half tail must not engage (its anchor pixels would be poison) and the bits still match the all-off run."""
    net = net_for("MLICPP_L")
    net.update()
    x = torch.cat([synthetic.synth_image(hw[0], hw[1], 90 + i) for i in range(2)]).to(DEV)
    outs = []
    try:
        for ep, new in ((0, 0), (0, 1), (1, 1)):
            _lib.call("mlic_set_kernel_option", b"ep_half", ep)
            _lib.call("mlic_set_kernel_option", b"lrp_half", new)
            _lib.call("mlic_set_kernel_option", b"intra_half", new)
            _lib.call("mlic_set_kernel_option", b"gdn_skip", new)
            outs.append(_whole_model(net, x))
    finally:
        for o in (b"ep_half", b"lrp_half", b"intra_half", b"gdn_skip"):
            _lib.call("mlic_set_kernel_option", o, -1)
    for fx, lk, s, dx in outs[1:]:
        assert s == outs[0][2]
        assert torch.equal(fx, outs[0][0]) and torch.equal(lk, outs[0][1]) and torch.equal(dx, outs[0][3])
    assert torch.isfinite(outs[0][0]).all()
