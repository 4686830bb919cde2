"""Bitstream file format and the per-image evaluation harness.

File layout (utils/utils.py:28-83, utils/testing.py:203-262):
    >II   H, W of the unpadded image            (VBR: >III H, W, level)
    >III  h_z, w_z, n_strings (= 2)
    n_strings x ( >I length, bytes )            y stream, then z stream (image 0 only: B = 1)
An ROI file (codec.encode_images(roi=...), *_VBR models) has n_strings = 3: the third string is the level map on
the z grid, one version byte 0 and h_z * w_z levels of 4 bits each (codec.write_container_roi).
Harness semantics (utils/testing.py:338-424; the NAIC "bpp > 0.1 => blur and retry" loop is code_image's
max_bpp=, off by default):
pad right/bottom with zeros to a multiple of 64, compress, write, read, decompress, crop;
bpp = 8 * filesize / (H * W) of the unpadded image; PSNR on uint8 images made by clamp(0,1)*255 and
truncation (torchvision ToPILImage), max 255 (utils/metrics.py:32-33).
"""
from __future__ import annotations

import io
import math
import struct
import time
from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F


def file_bytes(y_len: int, z_len: int, vbr: bool = False) -> int:
    """Size of the file write_stream produces for one image's y and z streams (the header included:
    bpp_file = 8 * file_bytes / (H * W), utils/utils.py:71-83)."""
    return (12 if vbr else 8) + 12 + (4 + y_len) + (4 + z_len)


def write_stream(fd, H: int, W: int, shape, strings, level=None) -> int:
    n = 0
    if level is None:
        fd.write(struct.pack(">2I", H, W))
        n += 8
    else:
        fd.write(struct.pack(">3I", H, W, int(level)))
        n += 12
    fd.write(struct.pack(">3I", int(shape[0]), int(shape[1]), len(strings)))
    n += 12
    for s in strings:
        b = s[0]
        fd.write(struct.pack(">I", len(b)))
        fd.write(b)
        n += 4 + len(b)
    return n


def read_stream(fd, vbr: bool = False):
    hdr = struct.unpack(">3I" if vbr else ">2I", fd.read(12 if vbr else 8))
    hz, wz, n = struct.unpack(">3I", fd.read(12))
    strings: List[List[bytes]] = []
    for _ in range(n):
        (ln,) = struct.unpack(">I", fd.read(4))
        strings.append([fd.read(ln)])
    return hdr, strings, (hz, wz)


def read_stream_checked(fd, vbr: bool = False, n_levels=None, max_pixels: int = 1 << 28):
    """read_stream through the library's validating parser (csrc/container.cpp): the same return value for a
    well-formed file, _lib.MlicError for a truncated or inconsistent one (a length past the end, h_z / w_z that
    do not belong to H / W, a padded size above max_pixels, a level >= n_levels, trailing bytes).  fd: a binary
    file object (read to its end) or the file's bytes."""
    from . import codec
    data = fd if isinstance(fd, (bytes, bytearray, memoryview)) else fd.read()
    data = bytes(data)
    c = codec.parse_container(data, vbr, n_levels, max_pixels)
    hdr = (c.H, c.W, c.level) if vbr else (c.H, c.W)
    return hdr, [[data[c.y_off:c.y_off + c.y_len]], [data[c.z_off:c.z_off + c.z_len]]], (c.hz, c.wz)


def write_file(path: str, H: int, W: int, out: Dict, level=None) -> int:
    with open(path, "wb") as f:
        return write_stream(f, H, W, out["shape"], out["strings"], level)


def read_file(path: str, vbr: bool = False):
    with open(path, "rb") as f:
        return read_stream(f, vbr)


def pad64(x: torch.Tensor) -> torch.Tensor:
    H, W = x.shape[-2:]
    ph = (64 - H % 64) % 64
    pw = (64 - W % 64) % 64
    return F.pad(x, (0, pw, 0, ph), mode="constant", value=0) if (ph or pw) else x


def to_u8(x: torch.Tensor) -> torch.Tensor:
    return (x.clamp(0, 1) * 255).to(torch.uint8)


def psnr_u8(a: torch.Tensor, b: torch.Tensor) -> float:
    mse = torch.mean((to_u8(a).float() - to_u8(b).float()) ** 2).item()
    return 20 * math.log10(255.0) - 10 * math.log10(mse) if mse > 0 else float("inf")


@torch.no_grad()
def code_image(net, img: torch.Tensor, ms_ssim: bool = False, max_bpp=None, max_passes: int = 8, lpips=None,
               dists=None, roi=None, roi_levels=None, tile=None, overlap: int = 32, yuv=None, rate_map: bool = False,
               progressive: bool = False, max_error=None, residual_segment=None, **kw) -> Dict:
    """One image [1,3,H,W] in [0,1] through pad -> compress -> file bytes -> decompress -> crop.
    ms_ssim=True adds "ms_ssim" (metrics.ms_ssim_u8 of img against the cropped x_hat, utils/testing.py:397-421;
    None when the image is too small for the five levels).
    lpips=metric (a metrics.LPIPS, or any callable (a, b) -> [B] tensor) adds "lpips": metric(img, cropped x_hat)
    as a float, None when min(H, W) < 16; off by default.
    dists=metric (a metrics.DISTS, or any such callable) adds "dists" in the same way.
    max_bpp: the reference's rate constraint (utils/testing.py:363-390) through codec.rate_loop on the float
    image: while the file is above max_bpp and fewer than max_passes filter passes were made, filter and code
    again.  The record then also holds "passes" and "met" (bpp <= max_bpp); psnr stays against the unfiltered
    img, and enc_s covers the whole loop.
    roi=mask (uint8 / bool [H,W] or [1,H,W], nonzero = inside) with roi_levels=(lo, hi), a *_VBR model: ROI coding
    (codec.roi_levels -> codec.gain_plane -> compress(gain_map=)); the file is the ROI file with its level map,
    the decoder rebuilds the plane from the file alone, and the record also holds "psnr_roi" and "psnr_bg" (PSNR
    inside and outside the mask; None for a side without pixels) and "roi_levels", the map.  Not together with
    max_bpp or s=; off by default.
    tile=T (with overlap=V): tiled coding (codec.encode_tiled / decode_tiled, DESIGN.md §5 "Tiled coding") of
    to_u8(img): the file is the tiled file, x_hat the decoded uint8 image / 255, psnr comes from the decode's
    exact squared error, and the record also holds "tile", "overlap", "grid" and "tile_bytes".  s= is the one
    level of the image; not together with max_bpp or roi=; off by default.
    yuv=fmt (a codec.YuvFormat): the record also holds "sq_err_yuv" (three ints), "psnr_y", "psnr_u", "psnr_v" and
    "psnr_yuv" = (6 Y + U + V) / 8 of codec.egress_yuv(x_hat, fmt) against the source planes, which are taken as
    codec.egress_yuv(img, fmt): the RGB image's 4:4:4 conversion through the same formula, filtered as fmt says.
    Not together with tile=, and refused for a format of depth > 8; off by default.
    rate_map=True: the record also holds "slice_bits" (one float per slice: the sum of -log2 of that slice's y
    likelihoods) and "z_bits" (the same for z), codec.rate_maps' slice_bits of one extra forward() of the padded
    image with the coder's arguments (s=, or the ROI gain plane).  Not together with tile=, yuv=, max_bpp= (the loop
    codes a filtered image), scale= / coded_size= or depth=; off by default, and the file bytes are the same either
    way.
    progressive=True: the file is the layered file (codec.write_container_layered of compress(layered=True): one
    rANS string per channel slice), decoded from its layers, and the record also holds "layer_bytes" (S ints: the
    exact coded bytes per slice) and "prefix_psnr" (S + 1 floats: PSNR of the mean-fill decode of the first K
    layers, K = 0..S).  Not together with tile=, roi=, max_bpp=, scale= / coded_size= or batch_stream; off by
    default.
    max_error=tau: the record also holds "residual_bytes" (the residual string that brings every sample of to_u8(img)
    within tau of the decode; codec.encode_images(max_error=tau) of to_u8(img), decoded again) and "max_abs_err"
    (the largest error of that decode, measured: <= tau).  bytes, bpp, psnr and x_hat stay those of the base file.
    Not together with tile=, roi=, max_bpp=, progressive=, yuv=, scale= / coded_size=, depth= or batch_stream; off
    by default.  residual_segment=L (with max_error=) passes through to encode_images: the file is the segmented
    residual file, and the record's "residual_kind" says which was written ("MLR1" or "MLR2")."""
    assert img.dim() == 4 and img.size(0) == 1
    if residual_segment is not None and max_error is None:
        raise ValueError("code_image: residual_segment= needs max_error=")
    H, W = img.shape[-2:]
    if max_error is not None:
        given = {"tile": tile, "roi": roi, "roi_levels": roi_levels, "max_bpp": max_bpp, "yuv": yuv,
                 "progressive": progressive or None, "scale": kw.get("scale"), "coded_size": kw.get("coded_size"),
                 "depth": kw.get("depth"), "batch_stream": kw.get("batch_stream") or None}
        for k, v in given.items():
            if v is not None:
                raise ValueError(f"code_image: max_error= together with {k}= is not supported")
    if progressive:
        given = {"tile": tile, "roi": roi, "roi_levels": roi_levels, "max_bpp": max_bpp, "scale": kw.get("scale"),
                 "coded_size": kw.get("coded_size"), "batch_stream": kw.get("batch_stream") or None}
        for k, v in given.items():
            if v is not None:
                raise ValueError(f"code_image: progressive=True together with {k}= is not supported")
    if rate_map:
        given = {"tile": tile, "yuv": yuv, "max_bpp": max_bpp, "scale": kw.get("scale"),
                 "coded_size": kw.get("coded_size"), "depth": kw.get("depth")}
        for k, v in given.items():
            if v is not None:
                raise ValueError(f"code_image: rate_map=True together with {k}= is not supported")
    if yuv is not None and tile is not None:
        raise ValueError("code_image: yuv= together with tile= is not supported")
    if yuv is not None and getattr(yuv, "depth", 8) > 8:
        raise ValueError(f"code_image: yuv= at depth {yuv.depth} is not supported: the record's PSNR fields are "
                         f"defined on 8-bit planes (score a high-depth decode with codec.decode_yuv(ref=))")
    if tile is not None:
        from . import codec
        if max_bpp is not None or roi is not None or roi_levels is not None or set(kw) - {"s"}:
            raise ValueError("code_image: tile= goes with overlap= and the level s= alone, not with max_bpp or roi=")
        lv = kw.get("s")
        if isinstance(lv, (list, tuple)):
            if len(lv) != 1:
                raise ValueError("code_image: tile= takes one level for the image")
            lv = lv[0]
        u8 = to_u8(img[0]).permute(1, 2, 0).contiguous()
        t0 = time.time()
        data, einfo = codec.encode_tiled(net, u8, tile=tile, overlap=overlap, level=lv, layout="hwc", return_info=True)
        enc = time.time() - t0
        t0 = time.time()
        dec_u8, dinfo = codec.decode_tiled(net, data, ref=u8)
        dect = time.time() - t0
        x_hat = dec_u8.permute(2, 0, 1).unsqueeze(0).float().div(255)
        r = {"H": H, "W": W, "bytes": len(data), "bpp": 8.0 * len(data) / (H * W), "psnr": dinfo["psnr"], "enc_s": enc,
             "dec_s": dect, "x_hat": x_hat, "tile": einfo["tile"], "overlap": einfo["overlap"], "grid": einfo["grid"],
             "tile_bytes": einfo["tile_bytes"]}
        if ms_ssim:
            from . import metrics
            r["ms_ssim"] = metrics.ms_ssim_u8(img, x_hat).item() if min(H, W) > metrics.MIN_SIDE else None
        if lpips is not None:
            from . import metrics
            r["lpips"] = lpips(img, x_hat).item() if min(H, W) >= metrics.LPIPS_MIN_SIDE else None
        if dists is not None:
            from . import metrics
            r["dists"] = dists(img, x_hat).item() if min(H, W) >= metrics.DISTS_MIN_SIDE else None
        return r
    x = pad64(img)
    level = kw.get("s") if kw else None
    buf = io.BytesIO()
    passes = None
    if (roi is None) != (roi_levels is None):
        raise ValueError("code_image: roi= and roi_levels=(lo, hi) go together")
    if roi is not None:
        from . import codec
        if max_bpp is not None or kw:
            raise ValueError("code_image: roi= goes with roi_levels=(lo, hi) alone, not with max_bpp or s=")
        lo, hi = roi_levels
        mask = codec._mask_batch(roi, "code_image roi")
        if tuple(mask.shape) != (1, H, W):
            raise ValueError(f"code_image: roi must be a mask of shape {(H, W)}, got {tuple(mask.shape)}")
        mask = mask.to(img.device)
        t0 = time.time()
        lmap = codec.roi_levels(mask, lo, hi)
        out = net.compress(x, gain_map=codec.gain_plane(net, lmap))
        enc = time.time() - t0
        data = codec.write_container_roi(H, W, out["shape"], out["strings"][0][0], out["strings"][1][0], hi, lmap[0])
        nbytes = len(data)
        c, fmap = codec.parse_container_roi(data, min(int(net.levels), 16))
        t0 = time.time()
        dec = net.decompress([[data[c.y_off:c.y_off + c.y_len]], [data[c.z_off:c.z_off + c.z_len]]], (c.hz, c.wz),
                             gain_map=codec.gain_plane(net, torch.from_numpy(fmap)))
        dect = time.time() - t0
    elif progressive:
        from . import codec
        lv = level[0] if isinstance(level, (list, tuple)) else level
        t0 = time.time()
        out = net.compress(x, layered=True, **kw)
        enc = time.time() - t0
        data = codec.write_container_layered(H, W, out["shape"], out["strings"][1][0], out["layers"][0], lv)
        nbytes = len(data)
        c = codec.parse_container_layered(data, getattr(net, "levels", None))
        layers, zstr = codec._layers(data, c), data[c.z_off:c.z_off + c.z_len]
        t0 = time.time()
        dec = net.decompress_layers([layers], [zstr], (c.hz, c.wz), **kw)
        dect = time.time() - t0
        prefix_psnr = []  # K = 0 .. S - 1 (K = S is the decode above)
        for k in range(len(layers)):
            part = net.decompress_layers([layers[:k]], [zstr], (c.hz, c.wz), **kw)["x_hat"]
            prefix_psnr.append(psnr_u8(img, part[:, :, :H, :W]))
    elif max_bpp is None:
        t0 = time.time()
        out = net.compress(x, **kw)
        enc = time.time() - t0
        nbytes = write_stream(buf, H, W, out["shape"], out["strings"], level)
    else:
        from . import codec
        if set(kw) - {"s"}:
            raise ValueError(f"code_image: max_bpp goes with the level s= only, got {sorted(kw)}")
        t0 = time.time()
        files, ps, _ = codec.rate_loop(net, x.contiguous().float(), H, W, level, max_bpp, max_passes)
        enc = time.time() - t0
        nbytes, passes = buf.write(files[0]), ps[0]
    if roi is None and not progressive:
        buf.seek(0)
        hdr, strings, shape = read_stream(buf, vbr=level is not None)
        t0 = time.time()
        dec = net.decompress(strings, shape, **kw)
        dect = time.time() - t0
    x_hat = dec["x_hat"][:, :, :H, :W]
    r = {"H": H, "W": W, "bytes": nbytes, "bpp": 8.0 * nbytes / (H * W), "psnr": psnr_u8(img, x_hat),
         "enc_s": enc, "dec_s": dect, "x_hat": x_hat}
    if passes is not None:
        r["passes"], r["met"] = passes, r["bpp"] <= max_bpp
    if progressive:
        r["layer_bytes"] = [len(l) for l in layers]
        r["prefix_psnr"] = prefix_psnr + [r["psnr"]]
    if roi is not None:
        p = codec.psnr_roi(to_u8(img), to_u8(x_hat), mask, layout="chw")[0]
        r["psnr_roi"], r["psnr_bg"], r["roi_levels"] = p["psnr_roi"], p["psnr_bg"], fmap
    if rate_map:
        from . import codec
        fkw = {"gain_map": codec.gain_plane(net, lmap)} if roi is not None else \
            {k: v for k, v in kw.items() if k != "batch_stream"}
        sb = net.rate_map(x.contiguous().float(), **fkw)["slice_bits"][0].cpu().tolist()
        r["slice_bits"], r["z_bits"] = sb[:-1], sb[-1]
    if max_error is not None:
        from . import codec
        u8 = to_u8(img[0]).permute(1, 2, 0).contiguous()
        files, einfo = codec.encode_images(net, u8, level=level, layout="hwc", max_error=max_error, return_info=True,
                                           residual_segment=residual_segment)
        _, dinfo = codec.decode_images(net, files, ref=u8.unsqueeze(0))
        r["residual_bytes"], r["max_abs_err"] = einfo[0]["residual_bytes"], dinfo[0]["max_abs_err"]
        r["residual_kind"] = files[0][:4].decode()
        if residual_segment is not None:
            r["residual_segment"], r["segments"] = einfo[0]["residual_segment"], einfo[0]["segments"]
    if yuv is not None:
        from . import codec
        src = codec.egress_yuv(img.float().contiguous(), H, W, yuv)
        p = codec.psnr_yuv_from_sq_err(codec.egress_yuv(x_hat.float(), H, W, yuv, ref=src)[3][0].cpu().tolist(), H, W, yuv)
        r["sq_err_yuv"] = p.pop("sq_err")
        r.update(p)
    if ms_ssim:
        from . import metrics
        r["ms_ssim"] = metrics.ms_ssim_u8(img, x_hat).item() if min(H, W) > metrics.MIN_SIDE else None
    if lpips is not None:
        from . import metrics
        r["lpips"] = lpips(img, x_hat).item() if min(H, W) >= metrics.LPIPS_MIN_SIDE else None
    if dists is not None:
        from . import metrics
        r["dists"] = dists(img, x_hat).item() if min(H, W) >= metrics.DISTS_MIN_SIDE else None
    return r
