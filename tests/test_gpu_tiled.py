"""Tiled coding on the GPU: the blend egress kernel (csrc/image_io.hip) against the CPU restatement
(codec.blend_tiles on CPU tensors, itself pinned to a float64 loop oracle in test_tiled_cpu.py), bit for bit, and
encode_tiled / decode_tiled with the synthetic-weight models: every embedded tile file is encode_images of that crop,
a full decode is the restatement's blend of net.decompress's per-tile x_hat, a region decode is the crop of the full
decode and touches only the tiles it needs, tile_batch is invisible, and the command line round-trips.

Every comparison is exact.  Every destination sits between sentinel bytes that are checked after the call."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from mlic_amd import _lib, bitstream, codec, get_model, synthetic

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 128
SENT = 0xA5
# (H, W, V): a 2 x 4 grid whose last column is 42 wide and whose rows are W * 3 = 990 bytes (odd-aligned starts),
# one tile, and exactly two tiles in x
IMAGES = [(200, 330, 32), (100, 90, 32), (128, 224, 32)]


def _random_tiles(H, W, V, seed, tile=T):
    """CPU fp32 tiles [3, pad64(h), pad64(w)]: values in about [-0.5, 1.5], some huge, +-inf, NaN, -0; NaN in the
    padding (never read)."""
    r = np.random.default_rng(seed)
    tiles = []
    for _, _, h, w in codec.tile_grid(H, W, tile, V)["rects"]:
        a = np.full((3, -(-h // 64) * 64, -(-w // 64) * 64), np.nan, np.float32)
        v = r.uniform(-0.5, 1.5, (3, h, w)).astype(np.float32)
        m = r.random((3, h, w))
        v[m < 0.01] = np.nan
        v[(m >= 0.01) & (m < 0.02)] = np.inf
        v[(m >= 0.02) & (m < 0.03)] = -np.inf
        v[(m >= 0.03) & (m < 0.04)] = 3.0e38
        v[(m >= 0.04) & (m < 0.05)] = -0.0
        a[:, :h, :w] = v
        tiles.append(torch.from_numpy(a))
    return tiles


def _dest(h, w, kind):
    """(whole buffer, the [h,w,3] / [3,h,w] destination view inside it, layout); the buffer is all sentinel."""
    if kind == "hwc":      # contiguous rows of w * 3 bytes starting at an odd address
        buf = torch.full((64 + h * w * 3 + 64 + 1,), SENT, dtype=torch.uint8, device=DEV)
        return buf, buf[65:65 + h * w * 3].view(h, w, 3), "hwc"
    if kind == "chw":
        buf = torch.full((64 + h * w * 3 + 64 + 1,), SENT, dtype=torch.uint8, device=DEV)
        return buf, buf[65:65 + h * w * 3].view(3, h, w), "chw"
    if kind == "window":   # canonical strides inside a wider canvas: the staged path with row gaps
        buf = torch.full((h + 2, w + 5, 3), SENT, dtype=torch.uint8, device=DEV)
        return buf, buf[1:h + 1, 2:w + 2], "hwc"
    if kind == "rgba":     # four bytes a pixel: the general path
        buf = torch.full((h + 2, w + 3, 4), SENT, dtype=torch.uint8, device=DEV)
        return buf, buf[1:h + 1, 1:w + 1, :3], "hwc"
    if kind == "transposed":  # column-major pixels: the general path
        buf = torch.full((w + 2, h + 2, 3), SENT, dtype=torch.uint8, device=DEV)
        return buf, buf[1:w + 1, 1:h + 1].permute(1, 0, 2), "hwc"
    raise AssertionError(kind)


def _check_blend(tiles_cpu, tiles_dev, H, W, V, region, kind, with_ref, tile=T):
    y0, x0, h, w = region or (0, 0, H, W)
    want = codec.blend_tiles(tiles_cpu, H, W, tile, V, region=region)  # CPU restatement, uint8 [h, w, 3]
    buf, dst, layout = _dest(h, w, kind)
    ref = None
    if with_ref:
        r = np.random.default_rng(h * 1000 + w).integers(0, 256, (h + 1, w + 2, 3), dtype=np.uint8)
        ref_hwc = torch.from_numpy(r).to(DEV)[1:, 2:]  # a strided reference
        ref = ref_hwc if layout == "hwc" else ref_hwc.permute(2, 0, 1)
    out = codec.blend_tiles(tiles_dev, H, W, tile, V, region=region, layout=layout, out=dst, ref=ref)
    torch.cuda.synchronize()
    got, sq = out if with_ref else (out, None)
    got_hwc = (got if layout == "hwc" else got.permute(1, 2, 0)).cpu()
    assert torch.equal(got_hwc, want), (region, kind, int((got_hwc != want).sum()))
    if with_ref:
        exp = int(((got_hwc.numpy().astype(np.int64) - ref_hwc.cpu().numpy().astype(np.int64)) ** 2).sum())
        assert int(sq.cpu()[0]) == exp and exp > 0
    dst.fill_(SENT)
    assert bool((buf == SENT).all()), "the blend wrote outside the region's bytes"
    return want


REGIONS = {
    (200, 330, 32): [None, (1, 3, 197, 325), (97, 99, 29, 27), (96, 96, 32, 32), (5, 7, 60, 77), (127, 287, 73, 43),
                     (199, 0, 1, 330), (0, 329, 200, 1), (3, 1, 131, 261)],
    (100, 90, 32): [None, (1, 1, 97, 87), (99, 89, 1, 1)],
    (128, 224, 32): [None, (0, 95, 128, 34), (11, 96, 5, 32), (64, 1, 63, 222)],
}


@pytest.mark.parametrize("image", IMAGES)
def test_blend_kernel_matches_the_cpu_restatement(image):
    H, W, V = image
    tiles = _random_tiles(H, W, V, seed=H + W)
    dev = [t.to(DEV) for t in tiles]
    for i, region in enumerate(REGIONS[image]):
        for kind in ("hwc", "chw", "rgba"):
            _check_blend(tiles, dev, H, W, V, region, kind, with_ref=(i + len(kind)) % 2 == 0)
    for kind in ("window", "transposed"):
        _check_blend(tiles, dev, H, W, V, REGIONS[image][1], kind, with_ref=True)
        _check_blend(tiles, dev, H, W, V, None, kind, with_ref=False)


@pytest.mark.parametrize("H, W, tile, V", [(200, 330, 128, 0), (130, 300, 128, 64), (100, 300, 128, 16), (260, 600, 256, 16),
                                           (129, 129, 128, 64)])
def test_blend_kernel_other_overlaps_and_tiles(H, W, tile, V):
    """V = 0 (no strips), V = 64 with T = 128 (every 256-pixel row piece crosses several tile columns and
    strips), and a larger tile."""
    tiles = _random_tiles(H, W, V, seed=H + W + V, tile=tile)
    dev = [t.to(DEV) for t in tiles]
    for region in (None, (1, 3, H - 2, W - 5)):
        for kind, with_ref in (("hwc", True), ("chw", False), ("rgba", True)):
            _check_blend(tiles, dev, H, W, V, region, kind, with_ref, tile=tile)


def test_blend_kernel_forms_agree_and_single_cover_is_egress():
    """The general form on a canonical destination gives the staged forms' bits; where one tile covers a pixel the
    result is egress_u8 of that tile."""
    H, W, V = 200, 330, 32
    tiles = _random_tiles(H, W, V, seed=1)
    dev = [t.to(DEV) for t in tiles]
    want = codec.blend_tiles(tiles, H, W, T, V)
    try:
        _lib.call("mlic_set_kernel_option", b"image_io_path", 0)
        forced = codec.blend_tiles(dev, H, W, T, V).cpu()
        forced_chw = codec.blend_tiles(dev, H, W, T, V, layout="chw").cpu()
    finally:
        _lib.call("mlic_set_kernel_option", b"image_io_path", -1)
    assert torch.equal(forced, want) and torch.equal(forced_chw.permute(1, 2, 0), want)
    got = codec.blend_tiles(dev, H, W, T, V).cpu()
    g = codec.tile_grid(H, W, T, V)
    cover = torch.zeros(H, W, dtype=torch.int64)
    for ty, tx, th, tw in g["rects"]:
        cover[ty:ty + th, tx:tx + tw] += 1
    for k, (ty, tx, th, tw) in enumerate(g["rects"]):
        e = codec.egress_u8(dev[k].unsqueeze(0), th, tw, "hwc")[0].cpu()
        one = cover[ty:ty + th, tx:tx + tw] == 1
        assert int(one.sum()) > 0 and torch.equal(got[ty:ty + th, tx:tx + tw][one], e[one]), k
    # a covering tile that is missing is refused by the host, before any launch
    with pytest.raises(ValueError, match="missing"):
        codec.blend_tiles([dev[0], None] + dev[2:], H, W, T, V)
    part = codec.blend_tiles([dev[0], None, None, None, dev[4], None, None, None], H, W, T, V, region=(0, 0, 200, 96))
    assert torch.equal(part.cpu(), want[:, :96])


# -------------------------------------------------------------------------------------------- codec
def _net(name):
    net = get_model(name)
    net.load_state_dict(synthetic.synth_state_dict(name, 0))
    net = net.to(DEV).eval()
    net.update()
    return net


@pytest.fixture(scope="module")
def net_s():
    return _net("MLICPP_S")


@pytest.fixture(scope="module")
def net_vbr():
    return _net("MLICPP_S_VBR")


def _u8_image(H, W, seed):
    x = synthetic.synth_image((H + 63) // 64 * 64, (W + 63) // 64 * 64, seed)[0, :, :H, :W]
    return torch.round(x * 255).to(torch.uint8).permute(1, 2, 0).contiguous()


@pytest.fixture(scope="module")
def coded(net_s):
    """The 200 x 330 image, its tiled file (V = 32) and the full decode, computed once and left unchanged."""
    img = _u8_image(200, 330, 3)
    data, einfo = codec.encode_tiled(net_s, img, tile=T, overlap=32, return_info=True)
    full, dinfo = codec.decode_tiled(net_s, data, ref=img)
    return img, data, einfo, full.cpu(), dinfo


def _tile_files(data):
    t = codec.parse_container_tiled(data)
    out = []
    for k in range(t.ny * t.nx):
        off, ln = codec.tiled_tile(data, t, k)
        out.append(data[off:off + ln])
    return out


@pytest.mark.parametrize("V", [0, 32])
@pytest.mark.parametrize("vbr", [False, True])
def test_embedded_tile_files_are_encode_images_of_the_crops(net_s, net_vbr, V, vbr):
    net, level = (net_vbr, 3) if vbr else (net_s, None)
    net.range_fallbacks(reset=True)
    H, W = 200, 330
    img = _u8_image(H, W, 3)
    data, info = codec.encode_tiled(net, img.to(DEV), tile=T, overlap=V, level=level, return_info=True)
    g = codec.tile_grid(H, W, T, V)
    files = _tile_files(data)
    assert len(files) == g["ny"] * g["nx"] == (8 if V else 6) and info["tile_bytes"] == [len(f) for f in files]
    for k, (ty, tx, th, tw) in enumerate(g["rects"]):
        alone = codec.encode_images(net, img[ty:ty + th, tx:tx + tw].contiguous(), level=level)[0]
        assert files[k] == alone, (k, len(files[k]), len(alone))
    assert len(set(files)) == len(files)
    d = codec.peek(data, n_levels=net.levels if vbr else None)
    assert d["tiled"] and d["vbr"] == vbr and d["level"] == level and d["grid"] == (g["ny"], g["nx"])
    assert not any(net.range_fallbacks(reset=True).values())


@pytest.mark.parametrize("image", IMAGES)
def test_full_decode_is_the_restatement_blend_of_the_tiles_x_hat(net_s, image):
    H, W, V = image
    net = net_s
    img = _u8_image(H, W, 4)
    data = codec.encode_tiled(net, img, tile=T, overlap=V)
    got, info = codec.decode_tiled(net, data, ref=img)
    g = codec.tile_grid(H, W, T, V)
    x_hats = []
    for f, (_, _, th, tw) in zip(_tile_files(data), g["rects"]):
        c = codec.parse_container(f)
        assert (c.H, c.W) == (th, tw)
        x_hats.append(net.decompress([[f[c.y_off:c.y_off + c.y_len]], [f[c.z_off:c.z_off + c.z_len]]],
                                     (c.hz, c.wz))["x_hat"][0].float().cpu())
    want = codec.blend_tiles(x_hats, H, W, T, V)
    assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), want)
    sq = int(((want.numpy().astype(np.int64) - img.numpy().astype(np.int64)) ** 2).sum())
    assert info["sq_err"] == sq and info["psnr"] == codec.psnr_from_sq_err(sq, 3 * H * W)
    assert info["tiles_decoded"] == list(range(len(x_hats))) and info["grid"] == (g["ny"], g["nx"])
    assert (info["H"], info["W"], info["tile"], info["overlap"], info["bytes"]) == (H, W, T, V, len(data))


def test_without_overlap_the_decode_is_each_tile_pasted_in_place(net_s):
    H, W = 200, 330
    img = _u8_image(H, W, 5)
    data = codec.encode_tiled(net_s, img, tile=T, overlap=0)
    got, _ = codec.decode_tiled(net_s, data)
    want = torch.zeros(H, W, 3, dtype=torch.uint8)
    for f, (ty, tx, th, tw) in zip(_tile_files(data), codec.tile_grid(H, W, T, 0)["rects"]):
        want[ty:ty + th, tx:tx + tw] = codec.decode_images(net_s, [f])[0][0].cpu()
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("region, tiles", [
    ((20, 30, 51, 47), [0]),                 # inside tile 0's interior
    ((131, 135, 40, 50), [5]),               # inside tile 5's interior
    ((90, 91, 45, 43), [0, 1, 4, 5]),        # across the corner four tiles share
    ((101, 197, 22, 100), [1, 2, 3, 5, 6, 7]),
    ((0, 0, 200, 330), list(range(8))),
    (None, list(range(8))),
])
def test_region_decode_is_the_crop_of_the_full_decode(net_s, coded, region, tiles):
    img, data, _, full, _ = coded
    y0, x0, h, w = region or (0, 0, 200, 330)
    ref = img[y0:y0 + h, x0:x0 + w]
    got, info = codec.decode_tiled(net_s, data, region=region, ref=ref)
    assert tuple(got.shape) == (h, w, 3) and torch.equal(got.cpu(), full[y0:y0 + h, x0:x0 + w])
    assert info["tiles_decoded"] == tiles and info["region"] == (y0, x0, h, w)
    assert info["sq_err"] == int(((got.cpu().numpy().astype(np.int64) - ref.numpy().astype(np.int64)) ** 2).sum())


def test_tile_batch_gives_the_same_file_and_pixels(net_s, coded):
    img, data, einfo, full, dinfo = coded
    for tb in (1, 8):
        assert codec.encode_tiled(net_s, img, tile=T, overlap=32, tile_batch=tb) == data
        got, info = codec.decode_tiled(net_s, data, tile_batch=tb, ref=img)
        assert torch.equal(got.cpu(), full) and info["sq_err"] == dinfo["sq_err"]
    assert einfo["grid"] == (2, 4) and einfo["bytes"] == len(data)


def test_vbr_tiled_round_trip(net_vbr):
    H, W, V, level = 128, 224, 32, 2
    img = _u8_image(H, W, 6)
    data = codec.encode_tiled(net_vbr, img, tile=T, overlap=V, level=level)
    got, info = codec.decode_tiled(net_vbr, data, ref=img)
    assert info["level"] == level and info["tiles_decoded"] == [0, 1] and info["psnr"] > 10
    part, pinfo = codec.decode_tiled(net_vbr, data, region=(3, 130, 100, 90))
    assert pinfo["tiles_decoded"] == [1] and torch.equal(part.cpu(), got.cpu()[3:103, 130:220])
    with pytest.raises(ValueError, match="decode_tiled"):
        codec.decode_images(net_vbr, [data])


def test_code_image_with_tiles(net_s, coded):
    img, data, _, full, dinfo = coded
    x = img.permute(2, 0, 1).unsqueeze(0).float().div(255).to(DEV)
    r = bitstream.code_image(net_s, x, tile=T, overlap=32)
    assert r["bytes"] == len(data) and r["psnr"] == dinfo["psnr"] and r["grid"] == (2, 4)
    assert torch.equal(bitstream.to_u8(r["x_hat"])[0].permute(1, 2, 0).cpu(), full)


def test_cli_round_trip(tmp_path, capsys, coded):
    img, data, _, full, _ = coded
    spec = importlib.util.spec_from_file_location("mlic_codec_tiled_gpu_cli", os.path.join(ROOT, "tools", "mlic_codec.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    src, bit, out, part = (str(tmp_path / n) for n in ("a.ppm", "a.bit", "full.ppm", "part.ppm"))
    with open(src, "wb") as f:
        f.write(cli.write_ppm(img.numpy()))
    model = ["--model", "MLICPP_S", "--synthetic", "0"]
    cli.main(["encode", src, bit, "--tile", "128"] + model)
    with open(bit, "rb") as f:
        assert f.read() == data  # --overlap defaults to 32: the file of encode_tiled
    cli.main(["info", bit, "--model", "MLICPP_S"])
    text = capsys.readouterr().out
    assert "tile 128, overlap 32, grid 2 x 4" in text and text.count("\n  tile ") == 8
    cli.main(["decode", bit, out] + model)
    cli.main(["decode", bit, part, "--region", "90", "91", "45", "43"] + model)
    assert "4 of 8 tiles decoded" in capsys.readouterr().out
    with open(out, "rb") as f:
        whole = cli.read_ppm(f.read())
    with open(part, "rb") as f:
        crop = cli.read_ppm(f.read())
    assert np.array_equal(whole, full.numpy()) and np.array_equal(crop, whole[90:135, 91:134])
