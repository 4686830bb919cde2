"""Segmented residual strings on the GPU (needs a MI355X: `-m gpu`): the kernels of csrc/residual_coder.hip against
the host coder, byte for byte and length for length, and "MLR2" files end to end through the codec.

A segment's bytes are defined as the host rANS coder's of its slice, so every comparison here is equality: the
device bytes and lengths are the host entry's (which tests/test_residual_seg_cpu.py pins to entropy.rans_encode), the
decode is the symbols, and residual_apply of the decoder's int16 output is the image (exact at tau 0, within tau
otherwise).  Sizes: 1 x 1 (one short segment), 16 x 24 and 17 x 23 (a short last segment, odd rows) and 64 x 96,
which at L = 256 is 72 segments: a full wave plus a partial one, segments crossing the channel planes.  L = 257 puts
every segment at an odd offset; L = 4096 exceeds the small images.  Output buffers are pre-filled with a sentinel
and carry a guard behind their capacity."""
import numpy as np
import pytest
import torch

from mlic_amd import codec, get_model, synthetic

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENTINEL = 0xA5
GUARD = 4096
SIZES = [(1, 1), (16, 24), (17, 23), (64, 96)]
SEGMENTS = [256, 257, 4096]
_NETS = {}
_KERNEL = {}
_CODED = {}


@pytest.fixture(autouse=True)
def _no_range_fallbacks(request):
    yield
    hit = {k: n.range_fallbacks(reset=True) for k, n in _NETS.items()}
    hit = {k: v for k, v in hit.items() if any(v.values())}
    assert not hit, (request.node.name, hit)


def net_for(name):
    if name not in _NETS:
        n = get_model(name)
        n.load_state_dict(synthetic.synth_state_dict(name, rate=1))
        n = n.to(DEV).eval()
        n.update()
        _NETS[name] = n
    return _NETS[name]


# ------------------------------------------------------------------------------------------ 1. kernels
def _pairs(H, W):
    """(kind, tau, base, x) uint8 [3,H,W,3]: three images with three different table sets per kind."""
    g = torch.Generator().manual_seed(1000 * H + W)
    rnd = lambda: torch.randint(0, 256, (3, H, W, 3), dtype=torch.uint8, generator=g)  # noqa: E731
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    ramp = torch.stack([((yy * (b + 1) + xx * 2) // 3 + 40 * b).clamp(0, 255) for b in range(3)])
    smooth = ramp.unsqueeze(-1).expand(3, H, W, 3).to(torch.uint8).contiguous()
    near = (smooth.to(torch.int16) + torch.randint(-6, 7, smooth.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    const = torch.stack([torch.full((H, W, 3), v, dtype=torch.uint8) for v in (0, 77, 255)])
    return [("random", 0, rnd(), rnd()), ("smooth", 2, smooth, near), ("constant", 0, const, const.clone())]


def kernel_case(H, W):
    """Per size, shared and changed by none: per kind the device tensors of residual_front and the tables."""
    if (H, W) not in _KERNEL:
        out = []
        for kind, tau, base, x in _pairs(H, W):
            f = codec.residual_front(base.to(DEV), x.to(DEV), tau, "hwc")
            tabs = [codec.residual_tables(f["hist"][b]) for b in range(3)]
            out.append((kind, tau, base.to(DEV), x.to(DEV), f, tabs))
        _KERNEL[(H, W)] = out
    return _KERNEL[(H, W)]


def _guarded(nbytes, dtype=torch.uint8):
    return torch.full((nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV).view(dtype)


@pytest.mark.parametrize("L", SEGMENTS)
@pytest.mark.parametrize("size", SIZES)
def test_kernels_give_the_host_coders_bytes(size, L):
    H, W = size
    N = 3 * H * W
    cap = codec.residual_segment_cap(H, W, L)
    for kind, tau, base, x, f, tabs in kernel_case(H, W):
        want = codec.residual_encode_segments(f["sym"], f["ctx"], tabs, L, "host")
        buf = _guarded(3 * cap)
        got = codec.residual_encode_segments(f["sym"], f["ctx"], tabs, L, "device", out=buf)
        for b in range(3):
            assert got[b][0] == want[b][0], (kind, b, len(got[b][0]), len(want[b][0]))
            assert np.array_equal(got[b][1], want[b][1]) and int(got[b][1].sum()) == len(got[b][0]), (kind, b)
        flat = buf.cpu().numpy()
        for b in range(3):  # past each image's length and behind the capacity nothing is written
            assert flat[b * cap:b * cap + len(got[b][0])].tobytes() == got[b][0]
            assert (flat[b * cap + len(got[b][0]):(b + 1) * cap] == SENTINEL).all(), (kind, b)
        assert (flat[3 * cap:] == SENTINEL).all(), kind
        if kind == "random" and N >= 1000:
            assert tabs[0]["m"][tabs[0]["m"] != 255].max() == 63 and int(f["hist"][0, :, 127].sum()) > 0  # escapes
        if kind == "constant":
            assert all(set(t["m"].tolist()) <= {0, 255} for t in tabs)
        if kind == "smooth" and N >= 64:
            assert any((t["m"] == 255).any() for t in tabs)  # absent contexts
        # the decode, straight into the buffer residual_apply reads
        sbuf = _guarded(2 * 3 * N, torch.int16)
        q = codec.residual_decode_segments([g[0] for g in got], [g[1] for g in got], f["ctx"], tabs, L, "device", out=sbuf)
        assert torch.equal(q, f["sym"]), kind
        assert (sbuf.view(torch.uint8)[2 * 3 * N:] == SENTINEL).all(), kind
        rec = codec.residual_apply(base, q, tau, "hwc")
        err = (rec.to(torch.int16) - x.to(torch.int16)).abs()
        assert int(err.max()) <= tau and (tau or torch.equal(rec, x)), (kind, int(err.max()))


def test_bytes_do_not_depend_on_repeats_or_the_batch():
    for kind, tau, base, x, f, tabs in kernel_case(64, 96):
        first = codec.residual_encode_segments(f["sym"], f["ctx"], tabs, 256)
        again = codec.residual_encode_segments(f["sym"], f["ctx"], tabs, 256)
        single = [codec.residual_encode_segments(f["sym"][b:b + 1], f["ctx"][b:b + 1], tabs[b:b + 1], 256)[0] for b in range(3)]
        for b in range(3):
            assert first[b][0] == again[b][0] == single[b][0], (kind, b)
            assert np.array_equal(first[b][1], again[b][1]) and np.array_equal(first[b][1], single[b][1])


def test_altered_bytes_name_their_segment():
    kind, tau, base, x, f, tabs = kernel_case(64, 96)[0]
    coded = codec.residual_encode_segments(f["sym"], f["ctx"], tabs, 256)
    data, segb = [c[0] for c in coded], [c[1] for c in coded]
    off = np.concatenate([[0], np.cumsum(segb[1])]).astype(int)
    for seg in (0, 37, 71):  # the first wave's first lane, a middle lane, the partial wave's last lane
        flipped = bytearray(data[1])
        flipped[off[seg] + int(segb[1][seg]) // 2] ^= 0x20
        zeroed = bytearray(data[1])
        zeroed[off[seg]:off[seg + 1]] = bytes(int(segb[1][seg]))
        for bad in (flipped, zeroed):  # every length stays valid, so every read stays inside host-checked bounds
            for coder in ("device", "host"):
                with pytest.raises(codec.ResidualSegmentError) as e:
                    codec.residual_decode_segments([data[0], bytes(bad), data[2]], segb, f["ctx"], tabs, 256, coder)
                assert (e.value.image, e.value.segment) == (1, seg), (coder, str(e.value))
    q = codec.residual_decode_segments(data, segb, f["ctx"], tabs, 256)  # and the run goes on clean
    assert torch.equal(q, f["sym"])


def test_a_small_capacity_is_refused_and_nothing_is_written_past_it():
    kind, tau, base, x, f, tabs = kernel_case(64, 96)[0]
    coded = codec.residual_encode_segments(f["sym"], f["ctx"], tabs, 256)
    need = max(len(c[0]) for c in coded)
    for cap in (8 * 72, (need - 4) // 4 * 4):
        buf = _guarded(3 * cap)
        with pytest.raises(codec.ResidualSegmentError, match="do not fit the capacity"):
            codec.residual_encode_segments(f["sym"], f["ctx"], tabs, 256, "device", cap=cap, out=buf)
        assert (buf.cpu().numpy()[3 * cap:] == SENTINEL).all()
    with pytest.raises(codec.ResidualSegmentError, match="do not fit the capacity"):
        codec.residual_encode_segments(f["sym"], f["ctx"], tabs, 256, "host", cap=8 * 72)


# ------------------------------------------------------------------------------------------ 2. end to end
E2E = [("MLICPP_S", None, 64, 64), ("MLICPP_S", None, 128, 192), ("MLICPP_S_VBR", 2, 64, 64),
       ("MLICPP_S_VBR", 2, 128, 192)]
TAUS = (0, 2)


def _images(B, H, W, seed=60):
    x = torch.cat([synthetic.synth_image(H, W, seed + i) for i in range(B)])
    return (x * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(DEV)


def coded(name, level, H, W):
    """Per (model, level, size), shared and changed by none: three images, their plain files and decode, and per tau
    the "MLR2" files of the batch from the device and from the host coder, and the "MLR1" files."""
    key = (name, level, H, W)
    if key not in _CODED:
        net = net_for(name)
        imgs = _images(3, H, W)
        plain = codec.encode_images(net, imgs, level=level)
        base, _ = codec.decode_images(net, plain)
        res = {}
        for tau in TAUS:
            dev = codec.encode_images(net, imgs, level=level, max_error=tau, residual_segment=256, return_info=True)
            host = codec.encode_images(net, imgs, level=level, max_error=tau, residual_segment=256, residual_coder="host")
            res[tau] = (dev[0], dev[1], host, codec.encode_images(net, imgs, level=level, max_error=tau))
        _CODED[key] = (net, imgs, plain, base, res)
    return _CODED[key]


@pytest.mark.parametrize("name,level,H,W", E2E)
def test_device_files_are_the_host_files_and_hold_the_bound(name, level, H, W):
    net, imgs, plain, base, res = coded(name, level, H, W)
    for tau in TAUS:
        files, info, host, serial = res[tau]
        assert files == host
        assert all(f[:4] == b"MLR2" and codec.is_residual_file(f) and codec.is_residual_seg_file(f) for f in files)
        for coder in ("device", "host"):
            out, dinfo = codec.decode_images(net, files, ref=imgs, residual_coder=coder)
            err = (out.to(torch.int16) - imgs.to(torch.int16)).abs()
            assert int(err.max()) <= tau and (tau or torch.equal(out, imgs)), (tau, coder, int(err.max()))
        n_seg = -(-3 * H * W // 256)
        for b in range(3):
            d = codec.peek(files[b], n_levels=getattr(net, "levels", None))
            assert d["residual_segment"] == 256 and d["segments"] == n_seg == info[b]["segments"] == dinfo[b]["segments"]
            assert d["max_error"] == tau == dinfo[b]["max_error"] and dinfo[b]["max_abs_err"] == int(err[b].max())
            assert info[b]["bytes"] == len(files[b]) == d["base_bytes"] + d["residual_bytes"] + d["header_bytes"]
            assert info[b]["residual_bytes"] == d["residual_bytes"] and d["base_bytes"] == len(plain[b])
        # an MLR1 and an MLR2 file of one image in one call: the same pixels
        both, binfo = codec.decode_images(net, [serial[1], files[1]])
        assert torch.equal(both[0], both[1]) and "segments" in binfo[1] and "segments" not in binfo[0]


@pytest.mark.parametrize("name,level,H,W", E2E)
def test_base_layer_and_batches(name, level, H, W):
    net, imgs, plain, base, res = coded(name, level, H, W)
    files = res[2][0]
    assert [codec.strip_residual(f) for f in files] == plain
    only, info = codec.decode_images(net, files, enhance=False)
    assert torch.equal(only, base) and info[0]["enhanced"] is False and info[0]["max_error"] == 2
    for tau in TAUS:
        single = [codec.encode_images(net, imgs[b], level=level, max_error=tau, residual_segment=256)[0] for b in range(3)]
        assert single == res[tau][0]


def test_a_corrupt_segment_in_a_file_names_the_file_and_the_segment():
    net, imgs, plain, base, res = coded("MLICPP_S", None, 64, 64)
    files = res[0][0]
    s = codec.parse_container_residual_seg(files[1])
    lens = np.frombuffer(files[1], ">u4", s.n_seg, s.index_off)
    at = s.data_off + int(lens[:5].sum()) + int(lens[5]) // 2  # inside segment 5
    bad = files[1][:at] + bytes([files[1][at] ^ 0x08]) + files[1][at + 1:]
    for coder in ("device", "host"):
        with pytest.raises(ValueError, match="decode_images: file 1: segment 5 of the residual string is corrupt"):
            codec.decode_images(net, [files[0], bad, files[2]], residual_coder=coder)
