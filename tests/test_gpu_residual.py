"""Residual coding on the GPU (needs a MI355X: `-m gpu`): the two kernels of csrc/residual.hip against their NumPy
restatement, and near-lossless / lossless files end to end through the codec.

Everything here is integer arithmetic, so every comparison is torch.equal / byte equality: the kernels' ctx,
ctx_count, sym, hist, digest, max_err, out, sq_err and max_abs_err are the restatement's (codec._residual_front_cpu,
codec._residual_apply_cpu) bit for bit, for every layout, size, batch, tau and input class below; the end-to-end
claims are a bound (|decode - input| <= tau, equality at tau 0) and identities (the output is the restatement
applied to the plain decode; strip_residual is the plain file).  The sizes put an image edge on every side of the
halo staging, widths on both sides of a 64-lane row, more rows than one row group, and (37 x 300) a second
256-pixel column tile; the crops start rows at every byte alignment.  Weights are the realistic-rate synthetic sets
of the parity tests; the suite's NaN poison is on and the range-fallback counters must stay 0."""
import pytest
import torch

from mlic_amd import _lib, codec, get_model, synthetic

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
RATE = {"MLICPP_S": 1, "MLICPP_L_VBR": 2}  # the parity tests' realistic-rate sets
_NETS = {}
_CODED = {}
TAUS = (0, 1, 2, 7, 127)
SIZES = [(1, 1), (1, 67), (3, 130), (37, 53), (64, 64), (65, 129), (37, 300)]
LAYOUTS = ["hwc", "chw", "rgba", "hwc_crop", "chw_crop"]


@pytest.fixture(autouse=True)
def _no_range_fallbacks(request):
    yield
    hit = {k: n.range_fallbacks(reset=True) for k, n in _NETS.items()}
    hit = {k: v for k, v in hit.items() if any(v.values())}
    assert not hit, (request.node.name, hit)


def net_for(name):
    if name not in _NETS:
        n = get_model(name)
        n.load_state_dict(synthetic.synth_state_dict(name, rate=RATE[name]))
        n = n.to(DEV).eval()
        n.update()
        _NETS[name] = n
    return _NETS[name]


# ------------------------------------------------------------------------------------------ 1. kernels
def _inputs(B, H, W, seed):
    """(name, base, x) uint8 [B,H,W,3] on the CPU: the input classes of the kernel tests."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda: torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)  # noqa: E731
    near = lambda b: (b.to(torch.int16) + torch.randint(-9, 10, b.shape, generator=g)).clamp(0, 255).to(torch.uint8)  # noqa: E731
    out = [("random", rnd(), rnd())]
    const = torch.full((B, H, W, 3), 77, dtype=torch.uint8)
    out.append(("constant", const, near(const)))
    lo, hi = torch.zeros_like(const), torch.full_like(const, 255)
    out += [("0-255", lo, hi), ("255-0", hi, lo)]
    for name, sl in (("v-left", (slice(None), slice(None), slice(1, None))), ("v-right", (slice(None), slice(None), slice(W - 1, None))),
                     ("h-top", (slice(None), slice(1, None))), ("h-bottom", (slice(None), slice(H - 1, None)))):
        b = torch.full((B, H, W, 3), 20, dtype=torch.uint8)
        b[sl] = 200
        out.append((name, b, near(b)))
    return out


_HOLDER = {"hwc": lambda B, H, W: (B, H, W, 3), "chw": lambda B, H, W: (B, 3, H, W),
           "rgba": lambda B, H, W: (B, H + 5, W + 7, 4), "hwc_crop": lambda B, H, W: (B, H + 3, W + 5, 3),
           "chw_crop": lambda B, H, W: (B, 3, H + 3, W + 5)}


def _view(big, kind, H, W):
    """The image inside its holder -> (view, layout).  The crops sit at odd offsets of a larger tensor, so rows
    start at every alignment; rgba leaves a fourth byte between pixels."""
    if kind == "rgba":
        return big[:, 2:2 + H, 3:3 + W, :3], "hwc"
    if kind == "hwc_crop":
        return big[:, 1:1 + H, 2:2 + W], "hwc"
    if kind == "chw_crop":
        return big[:, :, 2:2 + H, 3:3 + W], "chw"
    return big, kind


def _place(t, kind, poison=None):
    """The [B,H,W,3] CPU image t on the device in one of the layouts (or, with poison, a holder filled with that
    byte) -> (view, layout, holder)."""
    B, H, W, _ = t.shape
    shape = _HOLDER[kind](B, H, W)
    big = torch.full(shape, poison, dtype=torch.uint8, device=DEV) if poison is not None else \
        torch.randint(0, 256, shape, dtype=torch.uint8, device=DEV)
    v, lay = _view(big, kind, H, W)
    if poison is None:
        v.copy_(t.to(DEV) if lay == "hwc" else t.permute(0, 3, 1, 2).to(DEV))
    return v, lay, big


def _same(got, want, what):
    for k in want:
        assert torch.equal(got[k].cpu(), want[k]), (what, k)
    assert set(got) == set(want), what


@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("size", SIZES)
def test_kernels_are_the_restatement(size, kind):
    H, W = size
    for B in (1, 3):
        for name, base, x in _inputs(B, H, W, 100 * H + W + B):
            bv, lay, _ = _place(base, kind)
            xv, _, _ = _place(x, kind)
            for tau in TAUS:
                what = (size, kind, B, name, tau)
                want = codec._residual_front_cpu(base, x, tau)
                got = codec.residual_front(bv, xv, tau, lay)
                _same(got, want, what)
                assert int(got["max_err"].max()) <= tau
                if name in ("0-255", "255-0") and tau == 0:  # |q| = 255: everything in the escape bins
                    assert int(got["hist"][:, :, 127].sum()) == 3 * B * H * W
                if name == "constant":
                    assert int(got["ctx_count"][:, [0, 8, 16]].sum()) == 3 * B * H * W  # all class 0
                # apply: out through the same layout into a poisoned holder, scored against x
                ov, _, holder = _place(base, kind, poison=0xAB)
                out, sq, me = codec.residual_apply(bv, got["sym"], tau, lay, ref=xv, out=ov)
                w_out, w_sq, w_me = codec._residual_apply_cpu(base, want["sym"], tau, ref=x)
                o = out.cpu() if lay == "hwc" else out.permute(0, 2, 3, 1).cpu()
                assert torch.equal(o, w_out) and torch.equal(sq.cpu(), w_sq) and torch.equal(me.cpu(), w_me), what
                assert torch.equal(me.cpu(), want["max_err"]), what
                # nothing outside the image's bytes was written
                rest = holder.clone()
                _view(rest, kind, H, W)[0].fill_(0xAB)
                assert bool((rest == 0xAB).all()), what
                plain = codec.residual_apply(bv, got["sym"], tau, lay)
                assert torch.equal(plain, out), what
            # without x: the shared outputs, and only those
            f0 = codec.residual_front(bv, None, TAUS[1], lay)
            _same(f0, codec._residual_front_cpu(base, None, TAUS[1]), (size, kind, B, name, "no x"))


def test_front_is_repeatable_and_batch_independent():
    B, H, W = 3, 65, 129
    _, base, x = _inputs(B, H, W, 9)[0]
    bv, xv = base.to(DEV), x.to(DEV)
    a = codec.residual_front(bv, xv, 2, "hwc")
    for _ in range(3):
        b = codec.residual_front(bv, xv, 2, "hwc")
        assert all(torch.equal(a[k], b[k]) for k in a)
    for i in range(B):
        one = codec.residual_front(bv[i:i + 1], xv[i:i + 1], 2, "hwc")
        assert all(torch.equal(a[k][i:i + 1], one[k]) for k in a), i
        out = codec.residual_apply(bv[i:i + 1], one["sym"], 2, "hwc")
        assert torch.equal(out, codec.residual_apply(bv, a["sym"], 2, "hwc")[i:i + 1])


def test_wrappers_refuse_bad_arguments():
    base = torch.zeros(1, 4, 5, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="max_error must be an integer in"):
        codec.residual_front(base, None, 128)
    with pytest.raises(ValueError, match="does not match base"):
        codec.residual_front(base, torch.zeros(1, 4, 6, 3, dtype=torch.uint8, device=DEV), 1)
    with pytest.raises(ValueError, match="different devices"):
        codec.residual_front(base, torch.zeros(1, 4, 5, 3, dtype=torch.uint8), 1)
    with pytest.raises(ValueError, match="sym must be an int16 tensor"):
        codec.residual_apply(base, torch.zeros(1, 3, 4, 5, dtype=torch.int32, device=DEV), 1)
    with pytest.raises(ValueError, match="out has a zero column or channel stride"):
        codec.residual_apply(base, torch.zeros(1, 3, 4, 5, dtype=torch.int16, device=DEV), 1,
                             out=torch.zeros(1, 4, 5, 1, dtype=torch.uint8, device=DEV).expand(1, 4, 5, 3))


# --------------------------------------------------------------------------------------- 2. end to end
E2E = [("MLICPP_S", None, 128, 192), ("MLICPP_S", None, 100, 75), ("MLICPP_L_VBR", 3, 128, 192),
       ("MLICPP_L_VBR", 3, 100, 75)]


def _images(B, H, W, seed=60):
    x = torch.cat([synthetic.synth_image(H, W, seed + i) for i in range(B)])
    return (x * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(DEV)


def coded(name, level, H, W):
    """Per (model, level, size), shared by the tests and changed by none: three images, their plain files and
    plain decode, and the residual files of the batch for tau in 0, 1, 3."""
    key = (name, level, H, W)
    if key not in _CODED:
        net = net_for(name)
        imgs = _images(3, H, W)
        plain = codec.encode_images(net, imgs, level=level)
        base, _ = codec.decode_images(net, plain)
        res = {tau: codec.encode_images(net, imgs, level=level, max_error=tau, return_info=True) for tau in (0, 1, 3)}
        _CODED[key] = (net, imgs, plain, base, res)
    return _CODED[key]


@pytest.mark.parametrize("name,level,H,W", E2E)
def test_lossless_and_near_lossless_decode(name, level, H, W):
    net, imgs, plain, base, res = coded(name, level, H, W)
    for tau in (0, 1, 3):
        files, info = res[tau]
        out, dinfo = codec.decode_images(net, files, ref=imgs)
        err = (out.to(torch.int16) - imgs.to(torch.int16)).abs()
        assert int(err.max()) <= tau, (tau, int(err.max()))
        if tau == 0:
            assert torch.equal(out, imgs)
        # the output is the restatement applied to the plain decode
        f = codec._residual_front_cpu(base.cpu(), imgs.cpu(), tau)
        assert torch.equal(out.cpu(), codec._residual_apply_cpu(base.cpu(), f["sym"], tau))
        for b in range(3):
            assert dinfo[b]["max_abs_err"] == int(err[b].max()) <= tau and dinfo[b]["max_error"] == tau
            assert dinfo[b]["sq_err"] == int((err[b].to(torch.int64) ** 2).sum())
            assert dinfo[b]["residual_bytes"] == info[b]["residual_bytes"] and dinfo[b]["level"] == level
            d = codec.peek(files[b], n_levels=getattr(net, "levels", None))
            assert info[b]["bytes"] == len(files[b]) == info[b]["base_bytes"] + info[b]["residual_bytes"] + d["header_bytes"]
            assert d["max_error"] == tau and d["base_bytes"] == len(plain[b])
    # the symbols at tau > 0 are a function of those at tau 0, in the same contexts: they cost fewer bits
    assert all(res[0][1][b]["residual_bytes"] > res[tau][1][b]["residual_bytes"] for b in range(3) for tau in (1, 3))


@pytest.mark.parametrize("name,level,H,W", E2E)
def test_base_layer_is_the_plain_file(name, level, H, W):
    net, imgs, plain, base, res = coded(name, level, H, W)
    files = res[1][0]
    assert [codec.strip_residual(f) for f in files] == plain
    only, info = codec.decode_images(net, files, enhance=False)
    assert torch.equal(only, base) and torch.equal(only, codec.decode_images(net, [codec.strip_residual(f) for f in files])[0])
    assert info[0]["enhanced"] is False and info[0]["max_error"] == 1


@pytest.mark.parametrize("name,level,H,W", E2E[1::2])
def test_a_batch_gives_the_files_of_single_calls(name, level, H, W):
    net, imgs, plain, base, res = coded(name, level, H, W)
    for tau in (0, 3):
        assert [codec.encode_images(net, imgs[b], level=level, max_error=tau)[0] for b in range(3)] == res[tau][0]
    one, _ = codec.decode_images(net, [res[0][0][1]])
    assert torch.equal(one[0], imgs[1])


def test_altered_digest_raises_the_digest_error():
    net, imgs, plain, base, res = coded("MLICPP_S", None, 100, 75)
    f = res[1][0][0]
    for at in (16, 23):  # the digest field's first and last byte
        bad = f[:at] + bytes([f[at] ^ 0x10]) + f[at + 1:]
        with pytest.raises(RuntimeError, match="digest.*set_synthesis_precision.*precision mode"):
            codec.decode_images(net, [res[1][0][1], bad])
        out, _ = codec.decode_images(net, [bad], enhance=False)
        assert torch.equal(out, base[:1])


def test_refusals_on_residual_files():
    net, imgs, plain, base, res = coded("MLICPP_S", None, 100, 75)
    files = res[1][0]
    for kw, name in (({"slices": 2}, "slices="), ({"out_size": (50, 40)}, "out_size="), ({"filter": "bicubic"}, "filter="),
                     ({"depth": 10}, "depth=")):
        with pytest.raises(ValueError, match=f"decode_images: {name} on a residual file"):
            codec.decode_images(net, files, **kw)
    with pytest.raises(ValueError, match="residual files .MLR1. and other files in one call"):
        codec.decode_images(net, [files[0], plain[1]])
    with pytest.raises(ValueError, match="decode_tiled: a residual file .MLR1."):
        codec.decode_tiled(net, files[0])
    with pytest.raises(ValueError, match="max_error= .residual coding. together with layered="):
        codec.encode_images(net, imgs, max_error=1, layered=True)
    with pytest.raises(ValueError, match="max_error= .residual coding. together with max_bpp="):
        codec.encode_images(net, imgs, max_error=1, max_bpp=0.5)
    with pytest.raises(_lib.MlicError):
        codec.parse_container(files[0], False)
