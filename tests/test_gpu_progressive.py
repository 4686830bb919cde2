"""Progressive coding on the GPU (needs a MI355X: `-m gpu`): the phase_fill kernel, prefix decodes of plain and
layered strings, the layered file through the codec, and the refusals.

The bit-exact claims (phase_fill is phase_dequant on all-zero symbols; slices=S is the plain decode; every way of
asking for the first K slices gives the same x_hat; lanes, batching and repeats change nothing; each layer is the
rANS string of its slice's symbols) are asserted with torch.equal / byte equality.  Against the float oracle
(oracle.mlic_ref_cpu.RefMLIC.decode_streams fed the GPU's own z and y symbols for the decoded phases and zeros for
the rest; for zero fill the oracle's full-decode y_hat with the tail channels cleared, through its g_s) the gates are
the project's: assert_xhat_close's mean <= 5e-4 and max <= 0.25 (tests/test_gpu_roi.py), |dPSNR| <= 0.01 dB.  No
quantisation happens in the filled tail and the decoded part's symbols are given, so no rounding can flip.  The
measured differences go to PROG_PARITY ($MLIC_PARITY_OUT).  Weights are the realistic-rate synthetic sets of the
parity tests; the suite's NaN poison is on and the range-fallback counters must stay 0."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mlic_ref_cpu as ref
from mlic_amd import _lib, bitstream, codec, entropy, get_model, synthetic

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
RATE = {"MLICPP_L": 2, "MLICPP_M_SMALL_DEC": 1, "MLICPP_L_VBR": 2}  # the parity tests' realistic-rate sets
_NETS = {}
_CODED = {}
PROG_PARITY = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_parity():
    yield
    out = os.environ.get("MLIC_PARITY_OUT")
    if out and PROG_PARITY:
        import json
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        old = {}
        if os.path.exists(out):
            with open(out) as f:
                old = json.load(f)
        old.update(PROG_PARITY)
        with open(out, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)


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


def images(B, H, W, seed=40):
    return torch.cat([synthetic.synth_image(H, W, seed + i) for i in range(B)])


def coded(name, B, H, W, level=None):
    """One layered compress per (model, batch, size, level), shared by the tests: (x, compress output, kwargs,
    the plain decode's x_hat).  Nothing here is changed by a test."""
    key = (name, B, H, W, level)
    if key not in _CODED:
        net = net_for(name)
        x = images(B, H, W).to(DEV)
        kw = {} if level is None else {"s": level}
        c = net.compress(x, layered=True, **kw)
        full = net.decompress(c["strings"], c["shape"], **kw)["x_hat"]
        assert bool(torch.isfinite(full).all())
        _CODED[key] = (x, c, kw, full)
    return _CODED[key]


# ----------------------------------------------------------------------------------------- 1. kernel
def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bits(t):
    return t.view(torch.int32)


POISON = 0x7FC00ABC  # a NaN with a payload: what the kernels leave alone stays this


@pytest.mark.parametrize("shape", [(1, 1, 1, 2), (2, 3, 5, 6), (1, 32, 8, 12), (1, 5, 7, 10)])
@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("form", ["none", "image", "plane"])
def test_phase_fill_is_dequant_of_zero_symbols(shape, phase, form):
    B, Cn, H, W = shape
    n, hw = Cn * H * W, H * W
    yh_bs, p_bs = n + 2 * hw + 1, 2 * n + 3 * hw  # batch strides wider than the tensors
    g = torch.Generator().manual_seed(1000 * phase + n)
    params = torch.randn(B, p_bs, generator=g) * 3
    special = torch.tensor([0.0, -0.0, 1e-41, -1e-41, float("inf"), float("-inf"), float("nan"), 1.5, -2.25])
    means = params[:, n:2 * n]
    means[:, :min(n, special.numel())] = special[:min(n, special.numel())]
    means[:, -min(n, special.numel()):] = special[:min(n, special.numel())].flip(0)
    if n >= 2:  # both parities of the first row meet a -0 and a NaN
        means[:, 0], means[:, 1] = -0.0, -0.0
    if n >= 6:
        means[:, 2], means[:, 3] = float("nan"), float("nan")
    params = params.to(DEV)
    table = torch.linspace(0.11, 64.0, 64, device=DEV)
    sc = rs = scp = rsp = None
    if form == "image":
        sc = torch.tensor([0.37, 1.9][:B], device=DEV)
        rs = 1.0 / sc
    elif form == "plane":
        scp = torch.tensor([0.5, 0.37, 1.9, 2.0], device=DEV)[torch.randint(0, 4, (B, H, W), generator=g).to(DEV)]
        rsp = 1.0 / scp
    sym16 = torch.zeros(B * n // 2 + 1, dtype=torch.int16, device=DEV)
    sym32 = torch.zeros(B * n // 2 + 1, dtype=torch.int32, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(entry, **kw):
        yh = torch.full((B * yh_bs + 7,), POISON, dtype=torch.int32, device=DEV)
        d = _lib.QuantDesc(params=_ptr(params), params_bs=p_bs, yh=_ptr(yh), yh_bs=yh_bs, nlim=32767, ntable=64,
                           table=_ptr(table), phase=phase, vbr=int(form != "none"), B=B, C=Cn, H=H, W=W, **kw)
        _lib.call(entry, st, C.byref(d))
        torch.cuda.synchronize()
        return yh

    gains = dict(sc=_ptr(sc), rs=_ptr(rs), scp=_ptr(scp), rsp=_ptr(rsp))
    a = run("mlic_phase_dequant_run", sym16=_ptr(sym16), **gains)
    b = run("mlic_phase_dequant_run", sym=_ptr(sym32), **gains)
    # the fill call gets neither symbols nor gains: it must not read them
    f = run("mlic_phase_fill_run")
    assert torch.equal(a, b) and torch.equal(f, a), (int((f != a).sum()), int((a != b).sum()))
    # and the definition itself, element by element
    body = f[:B * yh_bs].view(B, yh_bs)
    assert bool((body[:, n:] == POISON).all()) and bool((f[B * yh_bs:] == POISON).all())
    got = body[:, :n].reshape(B, Cn, H, W)
    hh, ww = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    anchor = (((hh + ww) % 2) == 1).to(DEV)  # ckbd_anchor keeps (even row, odd column) and (odd row, even column)
    mine = anchor if phase == 0 else ~anchor
    m = params[:, n:2 * n].reshape(B, Cn, H, W)
    host = (np.float32(0.0) + m.cpu().numpy()).astype(np.float32)  # the host's fp32 sum: denormals are kept
    want = torch.from_numpy(host.view(np.int32)).to(DEV)
    assert torch.equal(got[..., mine], want[..., mine])
    other = got[..., ~mine]
    assert bool((other == (0 if phase == 0 else POISON)).all())
    neg0 = _bits(m.contiguous()) == -(1 << 31)
    assert bool((got[neg0 & mine.expand_as(neg0)] == 0).all())  # m = -0 gives +0


def test_anchor_parity_matches_the_oracle():
    """The mask the kernel test uses is the reference's ckbd_anchor."""
    y = torch.ones(1, 1, 4, 6)
    hh, ww = torch.meshgrid(torch.arange(4), torch.arange(6), indexing="ij")
    assert torch.equal(ref.ckbd_anchor(y)[0, 0] != 0, ((hh + ww) % 2) == 1)


# --------------------------------------------------------------------------------------- 2. identity
CASES = [("MLICPP_L", 1, 128, 192, None), ("MLICPP_L", 2, 128, 192, None), ("MLICPP_M_SMALL_DEC", 1, 128, 128, None),
         ("MLICPP_L_VBR", 1, 128, 192, 1), ("MLICPP_L_VBR", 1, 128, 192, 4)]


@pytest.mark.parametrize("name,B,H,W,level", CASES)
def test_all_slices_is_the_plain_decode_and_layers_hold_the_symbols(name, B, H, W, level):
    net = net_for(name)
    S = net.slice_num
    x, c, kw, full = coded(name, B, H, W, level)
    assert net.compress(x, **kw)["strings"] == c["strings"]  # layered=True changes no byte of the strings
    zs = c["strings"][1]
    assert torch.equal(net.decompress(c["strings"], c["shape"], slices=S, **kw)["x_hat"], full)
    assert torch.equal(net.decompress_layers(c["layers"], zs, c["shape"], **kw)["x_hat"], full)
    assert torch.equal(net.decompress_layers(c["layers"], zs, c["shape"], slices=S, fill="zero", **kw)["x_hat"], full)
    assert torch.equal(full, net(x, **kw)["x_hat"])
    net.compress(x, layered=True, **kw)  # encoded_streams reads the last compress
    gc = net.gaussian_conditional._buffers
    tabs = [gc[k].cpu() for k in ("_quantized_cdf", "_cdf_length", "_offset")]
    for b in range(B):
        ys, yi, _ = net.encoded_streams(b)
        per = ys.size // S
        assert len(c["layers"][b]) == S and ys.size == S * per
        got = []
        for k, layer in enumerate(c["layers"][b]):
            sl = slice(k * per, (k + 1) * per)
            dec = entropy.rans_decode(layer, yi[sl], *tabs)
            assert np.array_equal(dec, ys[sl]), (b, k)
            assert layer == entropy.rans_encode(ys[sl], yi[sl], *tabs), (b, k)
            got.append(dec)
        assert np.array_equal(np.concatenate(got), entropy.rans_decode(c["strings"][0][b], yi, *tabs))


# ----------------------------------------------------------------------------- 3. prefix consistency
def _file(c, b, H, W, level):
    return codec.write_container_layered(H, W, c["shape"], c["strings"][1][b], c["layers"][b], level)


@pytest.mark.parametrize("name,B,H,W,level", [("MLICPP_L", 2, 128, 192, None), ("MLICPP_L_VBR", 1, 128, 192, 4)])
@pytest.mark.parametrize("fill", ["mean", "zero"])
def test_prefix_decodes_agree(monkeypatch, name, B, H, W, level, fill):
    net = net_for(name)
    S, Cs = net.slice_num, net.slice_ch
    x, c, kw, full = coded(name, B, H, W, level)
    zs = c["strings"][1]
    files = [_file(c, b, H, W, level) for b in range(B)]
    seen = []
    real = codec.egress_u8
    monkeypatch.setattr(codec, "egress_u8", lambda xh, *a, **k: (seen.append(xh.clone()), real(xh, *a, **k))[1])
    for K in (0, 1, 3, S - 1):
        a = net.decompress(c["strings"], c["shape"], slices=K, fill=fill, **kw)["x_hat"]
        assert bool(torch.isfinite(a).all())
        assert torch.equal(net.decompress_layers(c["layers"], zs, c["shape"], slices=K, fill=fill, **kw)["x_hat"], a)
        assert torch.equal(net.decompress_layers([l[:K] for l in c["layers"]], zs, c["shape"], fill=fill, **kw)["x_hat"], a)
        seen.clear()
        img, info = codec.decode_images(net, [codec.truncate_layered(f, K) for f in files], fill=fill)
        assert len(seen) == 1 and torch.equal(seen[0], a) and [d["slices"] for d in info] == [K] * B
        assert torch.equal(img, real(a, H, W, "hwc"))
        assert torch.equal(net.decompress(c["strings"], c["shape"], slices=K, fill=fill, **kw)["x_hat"], a)  # a repeat
        try:
            for lanes in (1, 4):
                net.set_lanes(lanes)
                assert torch.equal(net.decompress(c["strings"], c["shape"], slices=K, fill=fill, **kw)["x_hat"], a), lanes
                assert torch.equal(net.decompress_layers(c["layers"], zs, c["shape"], slices=K, fill=fill,
                                                         **kw)["x_hat"], a), lanes
        finally:
            net.set_lanes(2)
        if B > 1:  # a batch equals per-image calls
            for b in range(B):
                one = net.decompress_layers([c["layers"][b][:K]], [zs[b]], c["shape"], fill=fill, **kw)["x_hat"]
                assert torch.equal(one, a[b:b + 1]), (K, b)


# --------------------------------------------------------------------------------------- 4. oracle
def assert_xhat_close(a, b):
    d = (a.float() - b.float()).abs()
    assert float(d.mean()) <= 5e-4, float(d.mean())
    assert float(d.max()) <= 0.25, float(d.max())


_ORACLE = {}


def _oracle(name, H, W):
    """(RefMLIC, z symbols [1,N,hz,wz], the 2 S phase symbol tensors, the oracle's full-decode y_hat), once."""
    if name not in _ORACLE:
        net = net_for(name)
        x, c, kw, full = coded(name, 1, H, W)
        net.compress(x, layered=True)
        ys, yi, zsym = net.encoded_streams(0)
        S, Cs = net.slice_num, net.slice_ch
        per = ys.size // (2 * S)
        phases = [torch.from_numpy(ys[p * per:(p + 1) * per].copy()).reshape(1, Cs, H // 16, W // 32) for p in range(2 * S)]
        z = torch.from_numpy(zsym.copy()).reshape(1, -1, H // 64, W // 64)
        m = ref.RefMLIC(name, synthetic.synth_state_dict(name, rate=RATE[name]))
        _ORACLE[name] = (m, z, phases, m.decode_streams(z, phases)["y_hat"])
    return _ORACLE[name]


@pytest.mark.parametrize("K", [0, 2, 9])
@pytest.mark.parametrize("fill", ["mean", "zero"])
def test_prefix_matches_the_float_oracle(K, fill):
    name, H, W = "MLICPP_L", 128, 192
    net = net_for(name)
    S, Cs = net.slice_num, net.slice_ch
    assert K in (0, 2, S - 1)
    x, c, kw, full = coded(name, 1, H, W)
    m, z, phases, y_full = _oracle(name, H, W)
    if fill == "mean":
        fed = [p if i < 2 * K else torch.zeros_like(p) for i, p in enumerate(phases)]
        o = m.decode_streams(z, fed)["x_hat"]
    else:
        y = y_full.clone()
        y[:, K * Cs:] = 0
        o = m.g_s(y)
    got = net.decompress_layers([c["layers"][0][:K]], c["strings"][1], c["shape"], fill=fill)["x_hat"].cpu()
    d = (got - o).abs()
    pg, po = ref.psnr_uint8(x.cpu(), got), ref.psnr_uint8(x.cpu(), o)
    r = {"mean_abs": float(d.mean()), "max_abs": float(d.max()), "psnr_gpu": pg, "psnr_oracle": po}
    PROG_PARITY[f"progressive_oracle_{name}_{H}x{W}_K{K}_{fill}"] = r
    print(r)
    assert_xhat_close(got, o)
    assert abs(pg - po) <= 0.01, r


# --------------------------------------------------------------------------------------- 5. effect
def test_effect_sizes_and_exact_error():
    name, H, W = "MLICPP_L", 128, 192
    net = net_for(name)
    S = net.slice_num
    x, c, kw, full = coded(name, 1, H, W)
    img = (x.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    lay, linfo = codec.encode_images(net, img, layered=True, return_info=True)
    plain = codec.encode_images(net, img)
    _, pinfo = codec.decode_images(net, plain, ref=img)
    _, a = codec.decode_images(net, lay, ref=img)
    _, b = codec.decode_images(net, lay, ref=img, slices=S)
    _, p = codec.decode_images(net, plain, ref=img, slices=S)
    assert a[0]["sq_err"] == b[0]["sq_err"] == p[0]["sq_err"] == pinfo[0]["sq_err"]
    d = codec.peek(lay[0])
    assert d["layer_bytes"] == linfo[0]["layer_bytes"] and d["layers_present"] == S
    assert d["header_bytes"] + d["z_len"] + sum(4 + n for n in d["layer_bytes"]) == len(lay[0]) == d["bytes"]
    sizes = [len(codec.truncate_layered(lay[0], K)) for K in range(S + 1)]
    for K in range(S):
        assert sizes[K + 1] - sizes[K] == 4 + d["layer_bytes"][K]
        assert d["layer_bytes"][K] == 0 or sizes[K + 1] > sizes[K]
    assert sizes[-1] == len(lay[0])
    over = len(lay[0]) - len(plain[0])
    print({"plain_bytes": len(plain[0]), "layered_bytes": len(lay[0]), "overhead": over, "layer_bytes": d["layer_bytes"],
           "psnr_by_K": [codec.decode_images(net, lay, ref=img, slices=K)[1][0]["psnr"] for K in (0, 1, 2, 5, S)]})


# ------------------------------------------------------------------------------------ 6. end to end
def test_codec_end_to_end_unpadded_size():
    name, B, H, W = "MLICPP_L", 2, 120, 200
    net = net_for(name)
    S = net.slice_num
    imgs = (images(B, H, W, 60).clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    files, info = codec.encode_images(net, imgs, layered=True, return_info=True)
    x = codec.ingest_u8(imgs.to(DEV), "hwc")
    c = net.compress(x, layered=True)
    for b, f in enumerate(files):
        assert f == codec.write_container_layered(H, W, (2, 4), c["strings"][1][b], c["layers"][b])
        assert f == codec._write_container_layered_c(H, W, (2, 4), c["strings"][1][b], c["layers"][b])
        assert info[b]["bytes"] == len(f) and info[b]["layer_bytes"] == [len(l) for l in c["layers"][b]]
    dec, dinfo = codec.decode_images(net, files, ref=imgs)
    assert torch.equal(dec, codec.egress_u8(net(x)["x_hat"], H, W, "hwc")) and dec.shape == (B, H, W, 3)
    # mixed truncations in one call: each file gets its own K, in input order
    cut = [codec.truncate_layered(files[0], 2), codec.truncate_layered(files[1], 5)]
    mixed, minfo = codec.decode_images(net, cut, ref=imgs)
    assert [d["slices"] for d in minfo] == [2, 5]
    for b, K in enumerate((2, 5)):
        direct = net.decompress_layers([c["layers"][b][:K]], [c["strings"][1][b]], c["shape"])["x_hat"]
        u8, sq = codec.egress_u8(direct, H, W, "hwc", ref=imgs[b:b + 1])
        assert torch.equal(mixed[b:b + 1], u8) and minfo[b]["sq_err"] == int(sq[0])
        assert minfo[b]["psnr"] == codec.psnr_from_sq_err(int(sq[0]), 3 * H * W)
    steps = codec.decode_progressive(net, files[0], ref=imgs[0])
    assert [s["slices"] for s in steps] == [1, 2, 4, S]
    for s in steps:
        K = s["slices"]
        direct = net.decompress_layers([c["layers"][0][:K]], [c["strings"][1][0]], c["shape"])["x_hat"]
        u8, sq = codec.egress_u8(direct, H, W, "hwc", ref=imgs[:1])
        assert s["image"].shape == (H, W, 3) and torch.equal(s["image"], u8[0])
        assert s["sq_err"] == int(sq[0]) and s["psnr"] == codec.psnr_from_sq_err(int(sq[0]), 3 * H * W)
        assert s["bytes"] == len(codec.truncate_layered(files[0], K))
    assert steps[-1]["sq_err"] == dinfo[0]["sq_err"]
    zero = codec.decode_progressive(net, files[0], steps=(0, 3), fill="zero", ref=imgs[0])
    assert [s["slices"] for s in zero] == [0, 3] and all(np.isfinite(s["psnr"]) for s in zero)
    # the harness record
    img0 = x[:1, :, :H, :W]
    r = bitstream.code_image(net, img0, progressive=True)
    assert r["bytes"] == len(files[0]) and r["layer_bytes"] == info[0]["layer_bytes"]
    assert len(r["prefix_psnr"]) == S + 1 and r["prefix_psnr"][-1] == r["psnr"]
    two = net.decompress_layers([c["layers"][0][:2]], [c["strings"][1][0]], c["shape"])["x_hat"][:, :, :H, :W]
    assert r["prefix_psnr"][2] == bitstream.psnr_u8(img0, two)
    assert torch.equal(r["x_hat"], net(x[:1])["x_hat"][:, :, :H, :W])


# ----------------------------------------------------------------------------------- 7. refusals
def test_refusals_reach_no_gpu_call():
    """Each refusal by its message; the models below never get a handle, so no kernel ran for them."""
    fixed = get_model("MLICPP_M_SMALL_DEC").to(DEV).eval()
    vbr = get_model("MLICPP_M_SMALL_DEC_VBR").to(DEV).eval()
    S = fixed.slice_num
    x = torch.zeros(2, 3, 128, 128, device=DEV)
    two = [[b"", b""], [b"", b""]]
    for net in (fixed, vbr):
        for bad in (-1, S + 1, 1.0, True, "2"):
            with pytest.raises(ValueError, match="slices must be"):
                net.decompress(two, (2, 2), slices=bad)
            with pytest.raises(ValueError, match="slices must be"):
                net.decompress_layers([[b""], [b""]], [b"", b""], (2, 2), slices=bad)
        with pytest.raises(ValueError, match="fill must be 'mean' or 'zero'"):
            net.decompress(two, (2, 2), slices=1, fill="median")
        with pytest.raises(ValueError, match="fill= goes with slices="):
            net.decompress(two, (2, 2), fill="zero")
        with pytest.raises(ValueError, match="batch-stream layout"):
            net.decompress([[b"one stream"], [b"", b""]], (2, 2), slices=1)
        with pytest.raises(ValueError, match="slices=2 but only 1 layers given"):
            net.decompress_layers([[b""], [b""]], [b"", b""], (2, 2), slices=2)
        with pytest.raises(ValueError, match="same number of layers"):
            net.decompress_layers([[b""], [b"", b""]], [b"", b""], (2, 2))
        with pytest.raises(ValueError, match=f"{S + 1} layers given, the model has {S} slices"):
            net.decompress_layers([[b""] * (S + 1)], [b""], (2, 2))
        with pytest.raises(ValueError, match="one list of layers and one z string per image"):
            net.decompress_layers([[b""]], [b"", b""], (2, 2))
        with pytest.raises(ValueError, match="layered=True is not supported with batch_stream"):
            net.compress(x, layered=True, batch_stream=True)
    g = torch.ones(2, 1, 8, 8, device=DEV)
    with pytest.raises(ValueError, match="layered=True is not supported with gain_map"):
        vbr.compress(x, layered=True, gain_map=g)
    with pytest.raises(ValueError, match="slices= is not supported with gain_map"):
        vbr.decompress(two, (2, 2), slices=1, gain_map=g)
    assert fixed._handle is None and vbr._handle is None
    # the C ABI's own refusals, before any GPU call
    lib = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    h = fixed._ensure_handle(DEV)
    buf = C.create_string_buffer(b"\x00" * 16, 16)
    one = (C.c_void_p * 4)(*[C.cast(buf, C.c_void_p)] * 4)
    ln = (C.c_size_t * 4)(16, 16, 16, 16)
    out = torch.zeros(2, 3, 128, 128, device=DEV)

    def prefix(y=one, spi=1, slices=1, fill=0, z=one):
        rc = lib.mlic_decompress_prefix(h, st, y, ln, spi, z, ln, 2, 2, 2, slices, fill, None, out.data_ptr())
        assert rc != 0
        return lib.mlic_last_error().decode()

    assert f"slices must be in [0, {S}], got -1" in prefix(slices=-1)
    assert f"slices must be in [0, {S}], got {S + 1}" in prefix(slices=S + 1)
    assert "fill must be 0 (mean) or 1 (zero)" in prefix(fill=2)
    assert "strings_per_image must be at least 1" in prefix(spi=0)
    assert "2 layer strings per image, 3 slices asked for" in prefix(spi=2, slices=3)
    holes = (C.c_void_p * 4)(C.cast(buf, C.c_void_p), None, C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p))
    assert "a null y string among those that are read" in prefix(y=holes, spi=2, slices=2)
    assert "a null z string" in prefix(z=holes)
    assert "bad arguments" in prefix(y=None)
    n = C.c_int()
    rc = lib.mlic_layer_streams(h, 0, None, None, 0, C.byref(n))
    assert rc != 0 and "layer_streams: image index" in lib.mlic_last_error().decode()  # nothing was compressed
    assert bool((out == 0).all())
    # after a gain-plane compress the layers are refused, and a scalar compress brings them back
    net = get_model("MLICPP_M_SMALL_DEC_VBR")
    net.load_state_dict(synthetic.synth_state_dict("MLICPP_M_SMALL_DEC_VBR", rate=1))
    net = net.to(DEV).eval()
    net.update()
    _NETS["MLICPP_M_SMALL_DEC_VBR"] = net
    xs = images(1, 128, 128, 85).to(DEV)
    net.compress(xs, gain_map=torch.ones(1, 1, 8, 8, device=DEV))
    with pytest.raises(_lib.MlicError, match="coded with a gain plane"):
        net.layer_streams(0)
    assert len(net.compress(xs, s=1, layered=True)["layers"][0]) == net.slice_num
