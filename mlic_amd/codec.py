"""uint8 images in, bitstream files out, uint8 images back (utils/testing.py:338-424, submit/decode.py):

    PIL image -> ToTensor -> pad to 64 -> compress -> file  |  file -> decompress -> crop -> uint8 image

`ingest_u8` is ToTensor + pad in one kernel launch (uint8 of any layout / strides -> fp32 [B,3,Hp,Wp], v / 255
exactly as torch's CPU `u8.float().div(255)`, zeros in the padding), `egress_u8` is crop + clamp * 255 + cast in
one launch (optionally with the exact per-image sum of squared uint8 differences against a reference, so PSNR
comes with the decode).  The file is the layout documented in bitstream.py, written and parsed by the library
(csrc/container.cpp); the parser validates every field before anything is sized from it.

`encode_images(max_bpp=...)` adds the reference's rate constraint (utils/testing.py:363-390): while a file is
above the budget, the float image goes through the 3x3 Gaussian prefilter `blur3_pad` (one launch that also
compacts the images of a batch still over budget) and is coded again; `level="auto"` picks a *_VBR model's level
from the budget.  Off by default.

`encode_images(roi=masks, roi_levels=(lo, hi))` codes a *_VBR model with a gain per latent pixel (DESIGN.md §5
"ROI coding"): `roi_levels` turns the mask into a level map on the z grid (one cell per 64 x 64 pixels, lo outside
the ROI, hi inside), `gain_plane` expands it to the latent grid, and the map travels in the file as a third
string, so `decode_images` needs nothing but the file.  `sq_err_roi` / `psnr_roi` score a decode inside and
outside the mask.

`encode_tiled` / `decode_tiled` code one image of any size as independent tiles (DESIGN.md §5 "Tiled coding"): the
grid of `tile_grid`, each tile's file byte for byte `encode_images` of that crop, a tiled container with an index,
a decoder that touches only the tiles a region needs, and `blend_tiles`, one launch that assembles the region from
the overlapping tiles with feathered seams.

`ingest_u16` / `egress_u16`, `encode_images(depth=)` / `decode_images(depth=)` and `YuvFormat(depth=, msb=)` are
the same front doors for samples of 9 to 16 bits in uint16 words (DESIGN.md §5 "High-bit-depth I/O",
csrc/image_io16.hip): nothing is rounded to 8 bits on the way, the file does not know its depth, and PSNR is
computed at the peak 2^depth - 1.  uint16 tensors are only moved and viewed on the device, never computed with.

`rate_maps` / `rate_map` say where the entropy model's bits lie (DESIGN.md §5 "Rate maps", csrc/ratemap.hip): per
latent pixel and slice the sum of -log2 of forward()'s likelihoods, the per-cell total with z's share, and the
per-slice totals; `sq_err_blocks` is the matching error map (squared uint8 error per block) and `heat_u8` draws either
as a heat map, optionally blended over the image.

`encode_images(max_error=tau)` adds a second layer that bounds the error of every sample (DESIGN.md §5 "Residual
coding", csrc/residual.hip): the image is coded as before, its own strings are decoded to the base image, and
`residual_front` gives the quantised difference with a context per sample that reads the base image alone, the
histograms the tables are built from and a digest of the base image; the residual file wraps the unchanged plain
file.  `decode_images` checks the digest, decodes the residual string and `residual_apply` adds it back: no sample
is off by more than tau, and at tau = 0 the decode is the original.  `strip_residual` returns the plain file.
With `residual_segment=L` the residual string is cut into independently coded segments ("MLR2" file; DESIGN.md §5
"Segments", csrc/residual_coder.hip) that `residual_encode_segments` / `residual_decode_segments` code on the device.
Deep RGB (`encode_residual16`, "MLR3") and Y'CbCr frames (`encode_residual_yuv`, "MLR4") go through the same encoder
and decoder (`_encode_residual_layer`, `_decode_residual_layer`); a `_ResidualKind` supplies what differs.

CUDA tensors run the HIP kernels (csrc/image_io.hip, csrc/roi.hip) on the current stream; CPU tensors run a torch
restatement, so everything but the model also works without a GPU (as metrics.py does).
"""
from __future__ import annotations

import ctypes as C
import math
import re
import struct
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib, bitstream, entropy

MAX_PIXELS = 1 << 28  # default bound on a file's padded Hp * Wp (a 16384 x 16384 image)
_NO_LEVEL_LIMIT = 0x7FFFFFFF


# ------------------------------------------------------------------------------------------ layouts
def _layout(t: torch.Tensor, layout: Optional[str]) -> str:
    if layout is None:
        if t.shape[-1] == 3:
            return "hwc"
        if t.shape[-3] == 3:
            return "chw"
        raise ValueError(f"cannot tell the layout of an image tensor of shape {tuple(t.shape)}: pass layout=")
    if layout not in ("hwc", "chw"):
        raise ValueError(f"layout must be 'hwc' or 'chw', got {layout!r}")
    return layout


def _u8_batch(img, layout: Optional[str], what: str):
    """-> (4-dim uint8 tensor, layout): a single image gains the batch dimension."""
    if isinstance(img, np.ndarray):
        img = torch.from_numpy(np.ascontiguousarray(img))
    if not torch.is_tensor(img) or img.dtype != torch.uint8 or img.dim() not in (3, 4):
        raise ValueError(f"{what}: a uint8 tensor or array [B,H,W,3] / [B,3,H,W] (or one image) expected")
    if img.dim() == 3:
        img = img.unsqueeze(0)
    layout = _layout(img, layout)
    if img.size(3 if layout == "hwc" else 1) != 3:
        raise ValueError(f"{what}: {layout} image with 3 channels expected, got shape {tuple(img.shape)}")
    if 0 in img.shape:
        raise ValueError(f"{what}: empty image {tuple(img.shape)}")
    return img, layout


def _hw(t: torch.Tensor, layout: str):
    return (t.size(1), t.size(2)) if layout == "hwc" else (t.size(2), t.size(3))


def _strides(t: torch.Tensor, layout: str):
    """Element strides {image, row, column, channel} of a 4-dim image tensor."""
    s = t.stride()
    return (s[0], s[1], s[2], s[3]) if layout == "hwc" else (s[0], s[2], s[3], s[1])


def _in_place(t: torch.Tensor, layout: str) -> torch.Tensor:
    """The kernels read any strides but zero column / channel strides (an expanded tensor)."""
    _, _, col, ch = _strides(t, layout)
    return t.contiguous() if col == 0 or ch == 0 else t


def _nchw(t: torch.Tensor, layout: str) -> torch.Tensor:
    return t.permute(0, 3, 1, 2) if layout == "hwc" else t


def _pad64(n: int) -> int:
    return (n + 63) // 64 * 64


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------ kernels
def ingest_u8(img, layout: Optional[str] = "hwc") -> torch.Tensor:
    """uint8 images [B,H,W,3] (layout "hwc") or [B,3,H,W] ("chw"), or one image, with any strides (a crop, a
    row-padded buffer, the RGB of an RGBA array are read in place) -> the model's input: contiguous fp32
    [B,3,Hp,Wp], Hp / Wp the next multiples of 64; v / 255 inside the image (true division: the value
    torchvision's ToTensor produces) and exactly 0 in the right / bottom padding."""
    img, layout = _u8_batch(img, layout, "ingest_u8")
    B = img.size(0)
    H, W = _hw(img, layout)
    if not img.is_cuda:
        return bitstream.pad64(_nchw(img, layout).float().div(255)).contiguous()
    img = _in_place(img, layout)
    Hp, Wp = _pad64(H), _pad64(W)
    with torch.cuda.device(img.device):
        x = torch.empty(B, 3, Hp, Wp, dtype=torch.float32, device=img.device)
        if _lib.poison():
            x.fill_(float("nan"))
        _lib.call("mlic_image_ingest_u8", _stream(), C.c_void_p(img.data_ptr()), (C.c_int64 * 4)(*_strides(img, layout)),
                  B, H, W, C.c_void_p(x.data_ptr()), Hp, Wp)
    return x


def egress_u8(x_hat: torch.Tensor, H: int, W: int, layout: str = "hwc", ref=None, out: Optional[torch.Tensor] = None):
    """The top-left H x W crop of fp32 [B,3,>=H,>=W] (a padded x_hat, read in place) as uint8
    floor(clamp(v, 0, 1) * 255) -- bitstream.to_u8; a NaN gives 0 on the device -- in `layout`: [B,H,W,3] or
    [B,3,H,W].  out: an optional uint8 tensor of that shape with any strides (a window of a larger canvas); only
    the crop's bytes are written.  ref: a uint8 image batch of that shape (any strides): returns (image, sq_err)
    with sq_err int64 [B], the exact per-image sum of squared uint8 differences."""
    layout = _layout(x_hat, layout)
    if x_hat.dim() != 4 or x_hat.size(1) != 3 or x_hat.dtype != torch.float32:
        raise ValueError(f"egress_u8: fp32 [B,3,h,w] expected, got {x_hat.dtype} {tuple(x_hat.shape)}")
    B = x_hat.size(0)
    if not (1 <= H <= x_hat.size(2) and 1 <= W <= x_hat.size(3)) or B < 1:
        raise ValueError(f"egress_u8: crop {H} x {W} of {tuple(x_hat.shape)}")
    shape = (B, H, W, 3) if layout == "hwc" else (B, 3, H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=x_hat.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != x_hat.device:
        raise ValueError(f"egress_u8: out must be uint8 {shape} on {x_hat.device}")
    if ref is not None:
        ref, _ = _u8_batch(ref, layout, "egress_u8 ref")
        if tuple(ref.shape) != shape:
            raise ValueError(f"egress_u8: ref must have shape {shape}, got {tuple(ref.shape)}")
        ref = ref.to(x_hat.device)
    if not x_hat.is_cuda:
        u = bitstream.to_u8(x_hat[:, :, :H, :W])
        out.copy_(u.permute(0, 2, 3, 1) if layout == "hwc" else u)
        if ref is None:
            return out
        d = out.to(torch.int64) - ref.to(torch.int64)
        return out, (d * d).flatten(1).sum(1)
    if x_hat.stride(3) != 1:
        x_hat = x_hat.contiguous()
    if 0 in _strides(out, layout)[2:]:
        raise ValueError("egress_u8: out has a zero column or channel stride")
    with torch.cuda.device(x_hat.device):
        sq = None
        if ref is not None:
            ref = _in_place(ref, layout)
            sq = torch.full((B,), -1, dtype=torch.int64, device=x_hat.device)
        _lib.call("mlic_image_egress_u8", _stream(), C.c_void_p(x_hat.data_ptr()), (C.c_int64 * 3)(*x_hat.stride()[:3]),
                  B, H, W, C.c_void_p(out.data_ptr()), (C.c_int64 * 4)(*_strides(out, layout)),
                  None if ref is None else C.c_void_p(ref.data_ptr()),
                  None if ref is None else (C.c_int64 * 4)(*_strides(ref, layout)),
                  None if sq is None else C.c_void_p(sq.data_ptr()))
    return out if ref is None else (out, sq)


# --------------------------------------------------------------------------- samples deeper than a byte
def _check_depth(depth, what: str, lo: int = 8) -> int:
    if isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) or not lo <= depth <= 16:
        raise ValueError(f"{what}: depth must be an integer in [{lo}, 16], got {depth!r}")
    return int(depth)


def _check_msb(msb, what: str) -> bool:
    if not isinstance(msb, (bool, np.bool_)):
        raise ValueError(f"{what}: msb must be a bool (False: LSB-aligned samples, True: MSB-aligned, P010 style), "
                         f"got {msb!r}")
    return bool(msb)


def _as_u16(t, what: str) -> torch.Tensor:
    """A numpy uint16 array or torch.uint16 tensor -> torch.uint16 tensor sharing the memory."""
    if isinstance(t, np.ndarray):
        if t.dtype != np.uint16:
            raise ValueError(f"{what}: a uint16 array expected, got {t.dtype}")
        t = torch.from_numpy(t if t.flags.writeable else t.copy())
    if not torch.is_tensor(t) or t.dtype != torch.uint16:
        raise ValueError(f"{what}: a uint16 tensor or array expected, got "
                         f"{t.dtype if torch.is_tensor(t) else type(t).__name__}")
    return t


def _u16_batch(img, layout: Optional[str], what: str):
    """_u8_batch for uint16 images."""
    img = _as_u16(img, what)
    if img.dim() not in (3, 4):
        raise ValueError(f"{what}: a uint16 tensor or array [B,H,W,3] / [B,3,H,W] (or one image) expected")
    if img.dim() == 3:
        img = img.unsqueeze(0)
    layout = _layout(img, layout)
    if img.size(3 if layout == "hwc" else 1) != 3:
        raise ValueError(f"{what}: {layout} image with 3 channels expected, got shape {tuple(img.shape)}")
    if 0 in img.shape:
        raise ValueError(f"{what}: empty image {tuple(img.shape)}")
    return img, layout


def samples_of_words(w: torch.Tensor, depth: int, msb: bool = False) -> torch.Tensor:
    """uint16 words (CPU) -> int32 samples: min(word, 2^depth - 1), or word >> (16 - depth) for msb."""
    w = w.to(torch.int32)
    return w >> (16 - depth) if msb else w.clamp(max=(1 << depth) - 1)


def words_of_samples(s: torch.Tensor, depth: int, msb: bool = False) -> torch.Tensor:
    """Integer samples in [0, 2^depth - 1] (CPU) -> uint16 words (shifted up for msb, the low bits zero)."""
    s = s.to(torch.int32)
    return (s << (16 - depth) if msb else s).to(torch.uint16)


def _dense_u16(t: torch.Tensor, zero_dims) -> torch.Tensor:
    """A contiguous copy when one of the dims in zero_dims has stride 0 (an expanded tensor); through the host for
    a device tensor, where uint16 is only moved."""
    if not any(t.stride(d) == 0 for d in zero_dims):
        return t
    return t.cpu().contiguous().to(t.device) if t.is_cuda else t.contiguous()


def ingest_u16(img, depth: int, layout: Optional[str] = None, msb: bool = False) -> torch.Tensor:
    """ingest_u8 for samples of `depth` bits (8..16) in uint16 words (numpy uint16 arrays or torch.uint16 tensors,
    [B,H,W,3] / [B,3,H,W] or one image, any strides): the model's input, contiguous fp32 [B,3,Hp,Wp], sample /
    (2^depth - 1) inside the image as a true division (torch's CPU `t.to(torch.float32).div(maxv)` bit for bit) and
    +0 in the padding.  msb=False: the samples are LSB-aligned (PPM, y4m p10), a word above maxv reads as maxv;
    msb=True: MSB-aligned (P010 / P016 style), the low 16 - depth bits of a word are ignored.  CUDA tensors run the
    kernel (csrc/image_io16.hip) on the current stream, CPU tensors the torch restatement (the same bits)."""
    depth, msb = _check_depth(depth, "ingest_u16"), _check_msb(msb, "ingest_u16")
    img, layout = _u16_batch(img, layout, "ingest_u16")
    B = img.size(0)
    H, W = _hw(img, layout)
    if not img.is_cuda:
        s = samples_of_words(_nchw(img, layout), depth, msb)
        return bitstream.pad64(s.to(torch.float32).div((1 << depth) - 1)).contiguous()
    img = _dense_u16(img, (2, 3) if layout == "hwc" else (3, 1))
    Hp, Wp = _pad64(H), _pad64(W)
    with torch.cuda.device(img.device):
        x = torch.empty(B, 3, Hp, Wp, dtype=torch.float32, device=img.device)
        if _lib.poison():
            x.fill_(float("nan"))
        _lib.call("mlic_image_ingest_u16", _stream(), C.c_void_p(img.data_ptr()), (C.c_int64 * 4)(*_strides(img, layout)),
                  depth, int(msb), B, H, W, C.c_void_p(x.data_ptr()), Hp, Wp)
    return x


def egress_u16(x_hat: torch.Tensor, H: int, W: int, depth: int, layout: str = "hwc", msb: bool = False, ref=None,
               out: Optional[torch.Tensor] = None):
    """egress_u8 for samples of `depth` bits: the top-left H x W crop of fp32 [B,3,>=H,>=W] as uint16 words,
    sample = floor(clamp(v, 0, 1) * (2^depth - 1)) (a NaN gives 0), shifted up by 16 - depth for msb=True.  out: an
    optional uint16 tensor of the result's shape with any strides; only the crop's words are written.  ref: a uint16
    image batch of that shape in the same sample format: returns (image, sq_err) with sq_err int64 [B], the exact
    per-image sum of squared sample differences."""
    depth, msb = _check_depth(depth, "egress_u16"), _check_msb(msb, "egress_u16")
    layout = _layout(x_hat, layout)
    if x_hat.dim() != 4 or x_hat.size(1) != 3 or x_hat.dtype != torch.float32:
        raise ValueError(f"egress_u16: fp32 [B,3,h,w] expected, got {x_hat.dtype} {tuple(x_hat.shape)}")
    B = x_hat.size(0)
    if not (1 <= H <= x_hat.size(2) and 1 <= W <= x_hat.size(3)) or B < 1:
        raise ValueError(f"egress_u16: crop {H} x {W} of {tuple(x_hat.shape)}")
    shape = (B, H, W, 3) if layout == "hwc" else (B, 3, H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.int16, device=x_hat.device)  # uint16 is only viewed on the device
        if x_hat.is_cuda and _lib.poison():
            out.fill_(-1)
        out = out.view(torch.uint16)
    elif out.dtype != torch.uint16 or tuple(out.shape) != shape or out.device != x_hat.device:
        raise ValueError(f"egress_u16: out must be uint16 {shape} on {x_hat.device}")
    if ref is not None:
        ref, _ = _u16_batch(ref, layout, "egress_u16 ref")
        if tuple(ref.shape) != shape:
            raise ValueError(f"egress_u16: ref must have shape {shape}, got {tuple(ref.shape)}")
        ref = ref.to(x_hat.device)  # uint16 is only moved and viewed on the device, never computed with
    maxv = (1 << depth) - 1
    if not x_hat.is_cuda:
        x = x_hat[:, :, :H, :W]
        s = (torch.where(torch.isnan(x), torch.zeros_like(x), x).clamp(0, 1) * maxv).floor().to(torch.int32)
        out.copy_(words_of_samples(s.permute(0, 2, 3, 1) if layout == "hwc" else s, depth, msb))
        if ref is None:
            return out
        d = (s.permute(0, 2, 3, 1) if layout == "hwc" else s).to(torch.int64) - samples_of_words(ref, depth, msb).to(torch.int64)
        return out, (d * d).flatten(1).sum(1)
    if x_hat.stride(3) != 1:
        x_hat = x_hat.contiguous()
    if 0 in _strides(out, layout)[2:]:
        raise ValueError("egress_u16: out has a zero column or channel stride")
    with torch.cuda.device(x_hat.device):
        sq = None
        if ref is not None:
            ref = _dense_u16(ref, (2, 3) if layout == "hwc" else (3, 1))
            sq = torch.full((B,), -1, dtype=torch.int64, device=x_hat.device)
        _lib.call("mlic_image_egress_u16", _stream(), C.c_void_p(x_hat.data_ptr()), (C.c_int64 * 3)(*x_hat.stride()[:3]),
                  B, H, W, depth, int(msb), C.c_void_p(out.data_ptr()), (C.c_int64 * 4)(*_strides(out, layout)),
                  None if ref is None else C.c_void_p(ref.data_ptr()),
                  None if ref is None else (C.c_int64 * 4)(*_strides(ref, layout)),
                  None if sq is None else C.c_void_p(sq.data_ptr()))
        if ref is not None:
            ref.record_stream(torch.cuda.current_stream())
    return out if ref is None else (out, sq)


def _f32(hexfloat: str) -> float:
    v = float.fromhex(hexfloat)
    assert float(np.float32(v)) == v
    return v


# The rate loop's 3x3 Gaussian, sigma = 0.5 (utils/testing.py:264-284): exp(-d2 / (2 sigma^2)) over the grid's
# squared distances from the centre, scaled by 1 / (2 pi sigma^2) and divided by its sum, as torch evaluates it
# in fp32.  Row-major, dy = -1..1 then dx = -1..1; the same constants are the kernel's default.
_CORNER, _EDGE, _CENTRE = _f32("0x1.73b62cp-7"), _f32("0x1.575320p-4"), _f32("0x1.3d1b0ep-1")
BLUR3_WEIGHTS = (_CORNER, _EDGE, _CORNER, _EDGE, _CENTRE, _EDGE, _CORNER, _EDGE, _CORNER)


def blur3_pad(x: torch.Tensor, H: int, W: int, index=None, weights=None) -> torch.Tensor:
    """The rate loop's prefilter on the model's padded input (utils/testing.py:363-390: crop to H x W, 3x3
    depthwise conv with padding 1, pad to 64 again) in one launch.  x: contiguous fp32 [B,3,Hp,Wp] (Hp, Wp
    multiples of 64, as ingest_u8 returns it).  index: n image indices into x (a sequence or an integer tensor;
    duplicates allowed; None = every image in order): output image i is the filter of x[index[i]], so the images
    still over a budget are filtered and compacted together.  Returns a new fp32 [n,3,Hp,Wp]: inside the image
    acc = 0; acc = acc + w[t] * v[t] over the 3x3 taps in row-major order, v = 0 outside the H x W image, each
    product and sum rounded once; +0 in the padding.  weights: nine floats, row-major (None = BLUR3_WEIGHTS).
    CUDA tensors run the kernel on the current stream, CPU tensors the torch loop with the same arithmetic."""
    if not torch.is_tensor(x) or x.dim() != 4 or x.size(1) != 3 or x.dtype != torch.float32 or x.size(0) < 1:
        raise ValueError("blur3_pad: fp32 [B,3,Hp,Wp] expected")
    B, _, Hp, Wp = x.shape
    H, W = int(H), int(W)
    if Hp % 64 or Wp % 64 or not (1 <= H <= Hp and 1 <= W <= Wp):
        raise ValueError(f"blur3_pad: {H} x {W} image in a {Hp} x {Wp} buffer: multiples of 64 that cover it expected")
    w = [float(v) for v in (BLUR3_WEIGHTS if weights is None else
                            weights.reshape(-1).tolist() if torch.is_tensor(weights) else
                            np.asarray(weights, dtype=np.float64).reshape(-1).tolist())]
    if len(w) != 9:
        raise ValueError("blur3_pad: nine weights expected")
    idx = None
    if index is not None:
        idx = [int(v) for v in (index.reshape(-1).tolist() if torch.is_tensor(index) else list(index))]
        if not idx or any(not 0 <= v < B for v in idx):
            raise ValueError(f"blur3_pad: index must name at least one image, each in [0, {B})")
    n = B if idx is None else len(idx)
    x = x.contiguous()
    if not x.is_cuda:
        w32 = torch.tensor(w, dtype=torch.float32)
        src = x if idx is None else x.index_select(0, torch.tensor(idx, dtype=torch.int64))
        xp = torch.nn.functional.pad(src[:, :, :H, :W], (1, 1, 1, 1))
        acc = torch.zeros(n, 3, H, W, dtype=torch.float32)
        for t in range(9):
            dy, dx = divmod(t, 3)
            acc = acc + w32[t] * xp[:, :, dy:dy + H, dx:dx + W]
        out = torch.zeros(n, 3, Hp, Wp, dtype=torch.float32)
        out[:, :, :H, :W] = acc
        return out
    with torch.cuda.device(x.device):
        out = torch.empty(n, 3, Hp, Wp, dtype=torch.float32, device=x.device)
        if _lib.poison():
            out.fill_(float("nan"))
        ix = None if idx is None else torch.tensor(idx, dtype=torch.int32).to(x.device)
        _lib.call("mlic_image_blur3_pad", _stream(), C.c_void_p(x.data_ptr()),
                  None if ix is None else C.c_void_p(ix.data_ptr()), n, H, W, Hp, Wp,
                  None if weights is None else (C.c_float * 9)(*w), C.c_void_p(out.data_ptr()))
        if ix is not None:
            ix.record_stream(torch.cuda.current_stream())
    return out


# ---------------------------------------------------------------------------------------- container
def container_bytes(y_len: int, z_len: int, vbr: bool = False) -> int:
    n = C.c_size_t()
    _lib.call("mlic_container_bytes", y_len, z_len, int(vbr), C.byref(n))
    return n.value


def write_container(H: int, W: int, shape, y: bytes, z: bytes, level: Optional[int] = None) -> bytes:
    """One image's file (byte-identical to bitstream.write_stream(fd, H, W, shape, [[y], [z]], level))."""
    n = C.c_size_t()
    lv = -1 if level is None else int(level)
    if level is not None and lv < 0:
        raise ValueError("write_container: negative level")
    buf = C.create_string_buffer(max(1, container_bytes(len(y), len(z), level is not None)))
    _lib.call("mlic_container_write", H, W, lv, int(shape[0]), int(shape[1]), y, len(y), z, len(z), buf, len(buf),
              C.byref(n))
    return C.string_at(buf, n.value)


def parse_container(data: bytes, vbr: bool = False, n_levels: Optional[int] = None,
                    max_pixels: int = MAX_PIXELS) -> _lib.ContainerInfo:
    """The validating parser (mlic_container_parse): raises _lib.MlicError on any malformed input.  vbr says
    whether the file has a level word (the format cannot tell); n_levels bounds it (None: any level)."""
    data = bytes(data)
    info = _lib.ContainerInfo()
    nl = (_NO_LEVEL_LIMIT if n_levels is None else int(n_levels)) if vbr else 0
    _lib.call("mlic_container_parse", data, len(data), int(vbr), nl, int(max_pixels), C.byref(info))
    return info


def peek(data: bytes, vbr: bool = False, n_levels: Optional[int] = None, max_pixels: Optional[int] = None) -> Dict:
    """What a file says about itself, validated: H, W, level (None without one), the z grid `shape`, the
    padded size, the string lengths and the bpp of the whole file; for an ROI file also "roi_levels", its level
    map (uint8 numpy [hz, wz]).  A tiled file (is_tiled_file; its flags say whether the tiles carry a level word,
    and max_pixels bounds the whole image's H * W) gives {"tiled": True, H, W,
    tile, overlap, grid (ny, nx), vbr, level, bytes, bpp, "tiles": per tile index, y0, x0, H, W, level, bytes,
    bpp}.  A scaled file (is_scaled_file; its flags say whether the inner file has a level word) gives {"scaled":
    True, H, W (the display size), "coded" (h, w), "filter", vbr, level, shape, Hp, Wp (of the coded image), y_len,
    z_len, bytes, bpp (the whole file over the display pixels)}.  A layered file (is_layered_file; whole or
    truncated; its flags say whether it has a level word) gives {"layered": True, H, W, level, vbr, shape, Hp, Wp,
    "slices" (S), "layers_present", "layer_bytes" (the whole layers' lengths: exact coded bytes per slice), z_len,
    "header_bytes" (everything before the z string), bytes, bpp}: a whole file's bytes are header_bytes + z_len +
    sum(layer_bytes) + 4 per layer.  A residual file (is_residual_file; its flags say whether the inner file has a
    level word) gives {"residual": True, H, W, "max_error" (tau), vbr, level, shape, Hp, Wp, y_len, z_len, "digest",
    "base_bytes" (the inner file), "residual_bytes" (the residual string), "header_bytes" (the rest: header, tables
    and the two length words), bytes, bpp}; a segmented one ("MLR2") also "residual_segment" and "segments", and its
    "residual_bytes" are the index and the segments; a deep one ("MLR3", is_residual_deep_file) besides those
    "depth", "shift" and "low_bytes" (the low-bit plane); a Y'CbCr one ("MLR4", is_residual_yuv_file) besides those
    "sub", "matrix", "full_range" and "site_x" (H, W are the luma size)."""
    data = bytes(data)
    if is_residual_file(data) or is_residual_deep_file(data) or bytes(data[:4]) == b"MLR4":
        return _peek_residual(data, n_levels, MAX_PIXELS if max_pixels is None else max_pixels)
    if is_layered_file(data):
        return _peek_layered(data, n_levels, MAX_PIXELS if max_pixels is None else max_pixels)
    if is_tiled_file(data):
        return _peek_tiled(data, n_levels, MAX_IMAGE_PIXELS if max_pixels is None else max_pixels)
    if is_scaled_file(data):
        return _peek_scaled(data, n_levels, MAX_PIXELS if max_pixels is None else max_pixels)
    max_pixels = MAX_PIXELS if max_pixels is None else max_pixels
    lv = None
    if vbr and is_roi_file(data):
        c, lv = parse_container_roi(data, 16 if n_levels is None else n_levels, max_pixels)
    else:
        c = parse_container(data, vbr, n_levels, max_pixels)
    d = {"H": c.H, "W": c.W, "level": c.level if vbr else None, "shape": (c.hz, c.wz), "Hp": 64 * c.hz,
         "Wp": 64 * c.wz, "y_len": c.y_len, "z_len": c.z_len, "bytes": len(data),
         "bpp": 8.0 * len(data) / (c.H * c.W)}
    if lv is not None:
        d["roi_levels"] = lv  # uint8 [hz, wz]: the file's level map (ROI files only)
    return d


def is_roi_file(data: bytes) -> bool:
    """Whether a VBR file's n_strings word says 3 (H, W, level, h_z, w_z come before it)."""
    return len(data) >= 24 and int.from_bytes(data[20:24], "big") == 3


def write_container_roi(H: int, W: int, shape, y: bytes, z: bytes, level: int, levels) -> bytes:
    """One image's ROI file (mlic_container_write_roi): the VBR file with the level map as a third string.
    level: the header's level word (the map's upper level); levels: [hz, wz] integers, each <= 15."""
    hz, wz = int(shape[0]), int(shape[1])
    lv = np.ascontiguousarray(np.asarray(levels.cpu() if torch.is_tensor(levels) else levels).reshape(-1))
    if lv.size != hz * wz or lv.min() < 0 or lv.max() > 15:
        raise ValueError(f"write_container_roi: {hz} x {wz} levels in [0, 15] expected")
    lv = lv.astype(np.uint8)
    n = C.c_size_t()
    _lib.call("mlic_container_write_roi", H, W, int(level), hz, wz, y, len(y), z, len(z), None, None, 0, C.byref(n))
    buf = C.create_string_buffer(max(1, n.value))
    _lib.call("mlic_container_write_roi", H, W, int(level), hz, wz, y, len(y), z, len(z), C.c_void_p(lv.ctypes.data),
              buf, len(buf), C.byref(n))
    return C.string_at(buf, n.value)


def parse_container_roi(data: bytes, n_levels: int = 16, max_pixels: int = MAX_PIXELS):
    """The validating parser of a VBR file with or without a level map (mlic_container_parse_roi) ->
    (ContainerInfo, levels): levels is a uint8 numpy array [hz, wz], or None for a 2-string file.  Raises
    _lib.MlicError on any malformed input; n_levels (<= 16) bounds the level word and every level of the map."""
    data = bytes(data)
    info = _lib.ContainerRoiInfo()
    _lib.call("mlic_container_parse_roi", data, len(data), int(n_levels), int(max_pixels), C.byref(info), None, 0)
    c = info.file
    if info.map_len == 0:
        return c, None
    lv = np.zeros(c.hz * c.wz, np.uint8)
    _lib.call("mlic_container_parse_roi", data, len(data), int(n_levels), int(max_pixels), C.byref(info),
              C.c_void_p(lv.ctypes.data), lv.size)
    return info.file, lv.reshape(c.hz, c.wz)


def _strings(data: bytes, c: _lib.ContainerInfo):
    return data[c.y_off:c.y_off + c.y_len], data[c.z_off:c.z_off + c.z_len]


# ------------------------------------------------------------------------------- progressive coding
LAYERED_MAGIC = b"MLL1"
MAX_LAYERS = 32  # the file's S byte


def is_layered_file(data: bytes) -> bool:
    """Whether the bytes begin with the layered file's magic (DESIGN.md §5 "Progressive coding")."""
    return bytes(data[:4]) == LAYERED_MAGIC


def container_layered_bytes(z_len: int, layer_lens, vbr: bool = False) -> int:
    lens = [int(n) for n in layer_lens]
    n = C.c_size_t()
    _lib.call("mlic_container_layered_bytes", int(z_len), (C.c_size_t * max(1, len(lens)))(*lens), len(lens), int(vbr),
              C.byref(n))
    return n.value


def write_container_layered(H: int, W: int, shape, z: bytes, layers: Sequence[bytes],
                            level: Optional[int] = None) -> bytes:
    """One image's layered file: "MLL1", version, flags, S, a reserved byte, H, W, the level word of a VBR file,
    the z grid, the z string, then S length-prefixed layer strings (one rANS string per channel slice,
    compress(layered=True)["layers"][b]).  Pure Python, byte-identical to mlic_container_write_layered."""
    layers = [bytes(l) for l in layers]
    if not 1 <= len(layers) <= MAX_LAYERS:
        raise ValueError(f"write_container_layered: 1..{MAX_LAYERS} layers expected, got {len(layers)}")
    if level is not None and int(level) < 0:
        raise ValueError("write_container_layered: negative level")
    out = [LAYERED_MAGIC, struct.pack(">BBBB", 0, 0 if level is None else 1, len(layers), 0),
           struct.pack(">II", H, W)]
    if level is not None:
        out.append(struct.pack(">I", int(level)))
    out += [struct.pack(">II", int(shape[0]), int(shape[1])), struct.pack(">I", len(z)), bytes(z)]
    for l in layers:
        out += [struct.pack(">I", len(l)), l]
    return b"".join(out)


def _write_container_layered_c(H: int, W: int, shape, z: bytes, layers: Sequence[bytes],
                               level: Optional[int] = None) -> bytes:
    """write_container_layered through the library's writer (the test of the two against each other)."""
    layers = [bytes(l) for l in layers]
    S = len(layers)
    bufs = [C.create_string_buffer(l, max(1, len(l))) for l in layers]
    ptrs = (C.c_void_p * max(1, S))(*[C.cast(b, C.c_void_p) for b in bufs])
    lens = (C.c_size_t * max(1, S))(*[len(l) for l in layers])
    lv = -1 if level is None else int(level)
    n = C.c_size_t()
    _lib.call("mlic_container_write_layered", H, W, lv, int(shape[0]), int(shape[1]), z, len(z), ptrs, lens, S, None, 0,
              C.byref(n))
    buf = C.create_string_buffer(max(1, n.value))
    _lib.call("mlic_container_write_layered", H, W, lv, int(shape[0]), int(shape[1]), z, len(z), ptrs, lens, S, buf,
              len(buf), C.byref(n))
    return C.string_at(buf, n.value)


def parse_container_layered(data: bytes, n_levels: Optional[int] = None, max_pixels: int = MAX_PIXELS,
                            allow_truncated: bool = False) -> _lib.ContainerLayeredInfo:
    """The validating parser of a layered file (mlic_container_parse_layered): raises _lib.MlicError on any
    malformed input.  allow_truncated: a file cut at any byte after its complete z string is accepted, and
    layers_present counts its whole layers.  The file's flags say whether it has a level word (level = -1
    without one); n_levels bounds it (None: any level).  That S is the model's is the caller's check."""
    data = bytes(data)
    info = _lib.ContainerLayeredInfo()
    nl = _NO_LEVEL_LIMIT if n_levels is None else int(n_levels)
    _lib.call("mlic_container_parse_layered", data, len(data), nl, int(max_pixels), int(bool(allow_truncated)),
              C.byref(info))
    return info


def _layers(data: bytes, c: _lib.ContainerLayeredInfo) -> List[bytes]:
    return [data[c.layer_off[k]:c.layer_off[k] + c.layer_len[k]] for k in range(c.layers_present)]


def truncate_layered(data: bytes, K: int) -> bytes:
    """The first bytes of a layered file up to the end of layer K - 1 (K = 0: up to the end of z): the
    shortest file whose first K layers decode."""
    data = bytes(data)
    c = parse_container_layered(data, None, MAX_IMAGE_PIXELS, allow_truncated=True)
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 0 <= K <= c.layers_present:
        raise ValueError(f"truncate_layered: K must be in [0, {c.layers_present}] (the layers present), got {K!r}")
    if K == 0:
        return data[:c.z_off + c.z_len]
    return data[:c.layer_off[K - 1] + c.layer_len[K - 1]]


def _peek_layered(data: bytes, n_levels, max_pixels) -> Dict:
    c = parse_container_layered(data, n_levels, max_pixels, allow_truncated=True)
    lb = [int(c.layer_len[k]) for k in range(c.layers_present)]
    return {"layered": True, "H": c.H, "W": c.W, "level": None if c.level < 0 else c.level, "vbr": c.level >= 0,
            "shape": (c.hz, c.wz), "Hp": 64 * c.hz, "Wp": 64 * c.wz, "slices": c.S, "layers_present": c.layers_present,
            "layer_bytes": lb, "z_len": int(c.z_len), "header_bytes": int(c.z_off), "bytes": len(data),
            "bpp": 8.0 * len(data) / (c.H * c.W)}


def _check_prefix(net, slices, fill, what: str):
    """slices= / fill= of a decode, refused before any library call."""
    if fill not in ("mean", "zero"):
        raise ValueError(f"{what}: fill must be 'mean' or 'zero', got {fill!r}")
    if slices is None:
        return None
    S = int(net.slice_num)
    if isinstance(slices, bool) or not isinstance(slices, (int, np.integer)) or not 0 <= slices <= S:
        raise ValueError(f"{what}: slices must be an integer in [0, {S}], got {slices!r}")
    return int(slices)


def _refuse_layered(what: str, **given):
    """layered= composes with none of these: each is refused by name."""
    why = {"roi": "ROI coding has no layered form", "max_bpp": "the rate loop codes plain files",
           "level='auto'": "the level choice runs inside the rate loop", "scale": "scaled coding has no layered form",
           "coded_size": "scaled coding has no layered form", "tiles": "tiled coding has no layered form"}
    for name, v in given.items():
        if v:
            raise ValueError(f"{what}: layered=True together with {name} is not supported ({why[name]})")


# ------------------------------------------------------------------------------------ scaled coding
FILTERS = ("lanczos3", "bicubic", "triangle")  # the file's filter byte is the index
SCALED_MAGIC = b"MLS1"
MAX_SCALE_RATIO = 8  # per axis, 1/8 <= output / input <= 8


def _filter_id(filter, what: str) -> int:
    if filter not in FILTERS:
        raise ValueError(f"{what}: filter must be one of {FILTERS}, got {filter!r}")
    return FILTERS.index(filter)


def _check_size(size, what: str):
    try:
        h, w = size
    except (TypeError, ValueError):
        raise ValueError(f"{what}: a pair (height, width) expected, got {size!r}") from None
    for v in (h, w):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"{what}: a pair of positive integers (height, width) expected, got {size!r}")
    return int(h), int(w)


def _check_ratio(Li: int, Lo: int, what: str):
    if Lo > MAX_SCALE_RATIO * Li or Li > MAX_SCALE_RATIO * Lo:
        raise ValueError(f"{what}: {Li} -> {Lo} leaves the ratio range [1/{MAX_SCALE_RATIO}, {MAX_SCALE_RATIO}]")


def resample_table(filter: str, Li: int, Lo: int):
    """One axis' table of the resampler (mlic_resample_table; the definition is in DESIGN.md §5 "Scaled coding" and
    csrc/resample_table.h) -> (start int32 [Lo], count int32 [Lo], weights float32 [Lo, taps]): output o is
    sum_j weights[o, j] * input[start[o] + j] over j < count[o]; weights[o, count[o]:] is 0.  1/8 <= Lo / Li <= 8."""
    f = _filter_id(filter, "resample_table")
    taps = C.c_int()
    _lib.call("mlic_resample_table", f, int(Li), int(Lo), None, None, None, 0, C.byref(taps))
    start, count = np.zeros(Lo, np.int32), np.zeros(Lo, np.int32)
    w = np.zeros((Lo, taps.value), np.float32)
    _lib.call("mlic_resample_table", f, int(Li), int(Lo), C.c_void_p(start.ctypes.data), C.c_void_p(count.ctypes.data),
              C.c_void_p(w.ctypes.data), taps.value, C.byref(taps))
    return start, count, w


def _resample_axis_cpu(v: torch.Tensor, table) -> torch.Tensor:
    """The last axis of fp32 v through one table: acc = +0; acc = acc + w * v over the taps in ascending order,
    the product and the sum rounded once each (two torch operations), taps j >= count left out of the sum."""
    start, count, w = (torch.from_numpy(a) for a in table)
    start, count = start.long(), count.long()
    Li = v.size(-1)
    acc = torch.zeros(v.shape[:-1] + (w.size(0),), dtype=torch.float32)
    for j in range(w.size(1)):
        live = count > j
        term = w[:, j] * v[..., (start + j).clamp(max=Li - 1)]
        acc = torch.where(live, acc + term, acc)
    return acc


def _resample_cpu(v: torch.Tensor, size, filter: str) -> torch.Tensor:
    """fp32 [..., Hi, Wi] -> [..., Ho, Wo]: the horizontal pass, then the vertical one (the kernels' arithmetic)."""
    t = _resample_axis_cpu(v, resample_table(filter, v.size(-1), size[1]))
    return _resample_axis_cpu(t.transpose(-1, -2), resample_table(filter, v.size(-2), size[0])).transpose(-1, -2)


def ingest_u8_scaled(img, size, filter: str = "lanczos3", layout: Optional[str] = "hwc") -> torch.Tensor:
    """ingest_u8 with the resampler in the same launch: uint8 images of any strides -> v / 255, resampled to
    size = (h, w) with `filter` (horizontal pass first, fp32, nothing rounded to 8 bits), clamped to [0, 1] ->
    contiguous fp32 [B,3,pad64(h),pad64(w)] with exactly 0 in the padding.  size equal to the image's size gives
    ingest_u8's tensor bit for bit."""
    img, layout = _u8_batch(img, layout, "ingest_u8_scaled")
    f = _filter_id(filter, "ingest_u8_scaled")
    h, w = _check_size(size, "ingest_u8_scaled size")
    B = img.size(0)
    H, W = _hw(img, layout)
    _check_ratio(H, h, "ingest_u8_scaled")
    _check_ratio(W, w, "ingest_u8_scaled")
    if not img.is_cuda:
        v = _resample_cpu(_nchw(img, layout).float().div(255), (h, w), filter).clamp(0, 1)
        return bitstream.pad64(v).contiguous()
    img = _in_place(img, layout)
    Hp, Wp = _pad64(h), _pad64(w)
    with torch.cuda.device(img.device):
        x = torch.empty(B, 3, Hp, Wp, dtype=torch.float32, device=img.device)
        if _lib.poison():
            x.fill_(float("nan"))
        _lib.call("mlic_image_ingest_u8_scaled", _stream(), C.c_void_p(img.data_ptr()),
                  (C.c_int64 * 4)(*_strides(img, layout)), B, H, W, f, h, w, C.c_void_p(x.data_ptr()), Hp, Wp)
    return x


def egress_u8_scaled(x_hat: torch.Tensor, h: int, w: int, size, filter: str = "lanczos3", layout: str = "hwc", ref=None,
                     out: Optional[torch.Tensor] = None):
    """egress_u8 with the resampler in the same launch: the top-left h x w crop of fp32 [B,3,>=h,>=w], clamped to
    [0, 1] (a NaN gives 0), resampled to size = (Ho, Wo), then floor(clamp(v, 0, 1) * 255) as uint8 in `layout`.
    out / ref as in egress_u8, both of the output size; with ref returns (image, sq_err).  size == (h, w) gives
    egress_u8's bytes."""
    layout = _layout(x_hat, layout)
    f = _filter_id(filter, "egress_u8_scaled")
    if x_hat.dim() != 4 or x_hat.size(1) != 3 or x_hat.dtype != torch.float32:
        raise ValueError(f"egress_u8_scaled: fp32 [B,3,h,w] expected, got {x_hat.dtype} {tuple(x_hat.shape)}")
    B = x_hat.size(0)
    if not (1 <= h <= x_hat.size(2) and 1 <= w <= x_hat.size(3)) or B < 1:
        raise ValueError(f"egress_u8_scaled: crop {h} x {w} of {tuple(x_hat.shape)}")
    Ho, Wo = _check_size(size, "egress_u8_scaled size")
    _check_ratio(h, Ho, "egress_u8_scaled")
    _check_ratio(w, Wo, "egress_u8_scaled")
    shape = (B, Ho, Wo, 3) if layout == "hwc" else (B, 3, Ho, Wo)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=x_hat.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != x_hat.device:
        raise ValueError(f"egress_u8_scaled: out must be uint8 {shape} on {x_hat.device}")
    if ref is not None:
        ref, _ = _u8_batch(ref, layout, "egress_u8_scaled ref")
        if tuple(ref.shape) != shape:
            raise ValueError(f"egress_u8_scaled: ref must have shape {shape}, got {tuple(ref.shape)}")
        ref = ref.to(x_hat.device)
    if not x_hat.is_cuda:
        v = x_hat[:, :, :h, :w]
        v = torch.where(torch.isnan(v), torch.zeros((), dtype=v.dtype), v).clamp(0, 1)
        u = bitstream.to_u8(_resample_cpu(v, (Ho, Wo), filter))
        out.copy_(u.permute(0, 2, 3, 1) if layout == "hwc" else u)
        if ref is None:
            return out
        d = out.to(torch.int64) - ref.to(torch.int64)
        return out, (d * d).flatten(1).sum(1)
    if x_hat.stride(3) != 1:
        x_hat = x_hat.contiguous()
    if 0 in _strides(out, layout)[2:]:
        raise ValueError("egress_u8_scaled: out has a zero column or channel stride")
    with torch.cuda.device(x_hat.device):
        sq = None
        if ref is not None:
            ref = _in_place(ref, layout)
            sq = torch.full((B,), -1, dtype=torch.int64, device=x_hat.device)
        _lib.call("mlic_image_egress_u8_scaled", _stream(), C.c_void_p(x_hat.data_ptr()),
                  (C.c_int64 * 3)(*x_hat.stride()[:3]), B, h, w, f, Ho, Wo, C.c_void_p(out.data_ptr()),
                  (C.c_int64 * 4)(*_strides(out, layout)), None if ref is None else C.c_void_p(ref.data_ptr()),
                  None if ref is None else (C.c_int64 * 4)(*_strides(ref, layout)),
                  None if sq is None else C.c_void_p(sq.data_ptr()))
    return out if ref is None else (out, sq)


def is_scaled_file(data: bytes) -> bool:
    return bytes(data[:4]) == SCALED_MAGIC


def write_container_scaled(H: int, W: int, inner: bytes, filter: str = "lanczos3", vbr: bool = False) -> bytes:
    """The scaled file (mlic_container_write_scaled): a 16-byte header -- "MLS1", version, flags (bit 0: vbr),
    filter, reserved, the display size H, W -- around `inner`, the coded image's plain or VBR file, unchanged."""
    inner = bytes(inner)
    f = _filter_id(filter, "write_container_scaled")
    n = C.c_size_t()
    buf = C.create_string_buffer(16 + max(1, len(inner)))
    _lib.call("mlic_container_write_scaled", H, W, int(bool(vbr)), f, inner, len(inner), buf, len(buf), C.byref(n))
    return C.string_at(buf, n.value)


def parse_container_scaled(data: bytes, n_levels: Optional[int] = None,
                           max_pixels: int = MAX_PIXELS) -> _lib.ContainerScaledInfo:
    """The validating parser of a scaled file (mlic_container_parse_scaled): raises _lib.MlicError on any malformed
    input.  The file's flags say whether the inner file has a level word; n_levels bounds it (None: any level).
    info.inner is the inner file's ContainerInfo, its offsets relative to data[info.inner_off:]."""
    data = bytes(data)
    info = _lib.ContainerScaledInfo()
    nl = _NO_LEVEL_LIMIT if n_levels is None else int(n_levels)
    _lib.call("mlic_container_parse_scaled", data, len(data), nl, int(max_pixels), C.byref(info))
    return info


def coded_size(H: int, W: int, scale):
    """The coded size of an H x W image at `scale` (a Fraction, an int, a string "N/D", or a float taken at its
    exact binary value): per axis max(1, floor(L * scale + 1/2)) in exact rational arithmetic -- round to nearest,
    a tie goes up."""
    from fractions import Fraction
    if isinstance(scale, bool):
        raise ValueError(f"scale: a positive rational expected, got {scale!r}")
    try:
        s = Fraction(scale)
    except (TypeError, ValueError, ZeroDivisionError):
        raise ValueError(f"scale: a positive rational (Fraction, int, 'N/D') expected, got {scale!r}") from None
    if s <= 0:
        raise ValueError(f"scale: a positive rational expected, got {scale!r}")
    return tuple(max(1, math.floor(L * s + Fraction(1, 2))) for L in (H, W))


_scaled_size = coded_size  # encode_images has a parameter of that name


def _peek_scaled(data: bytes, n_levels, max_pixels) -> Dict:
    s = parse_container_scaled(data, n_levels, max_pixels)
    c = s.inner
    return {"scaled": True, "H": s.H, "W": s.W, "coded": (c.H, c.W), "filter": FILTERS[s.filter], "vbr": bool(s.vbr),
            "level": c.level if s.vbr else None, "shape": (c.hz, c.wz), "Hp": 64 * c.hz, "Wp": 64 * c.wz,
            "y_len": c.y_len, "z_len": c.z_len, "bytes": len(data), "bpp": 8.0 * len(data) / (s.H * s.W)}


# ---------------------------------------------------------------------------------- residual coding
RESIDUAL_MAGIC = b"MLR1"
RESIDUAL_SEG_MAGIC = b"MLR2"  # the segmented residual file (DESIGN.md §5 "Residual coding", "Segments")
RES_SEG_MIN, RES_SEG_MAX, RES_SEG_SLACK = 256, 65536, 4
RES_SEG_MAX_N = 1 << 29  # samples of one string (csrc/residual_seg.h)
DEFAULT_RESIDUAL_SEGMENT = 4096
MAX_TAU = 127
RES_CTX, RES_BINS, RES_MAX_M, RES_ABSENT, RES_CDF_STRIDE = 24, 128, 63, 0xFF, 129
_DIGEST_K = 0x9E3779B97F4A7C15
_CLASS_OF = np.array([0 if a < 2 else a.bit_length() - 1 for a in range(256)], np.uint8)  # class of a = max - min


def _check_tau(tau, what: str) -> int:
    if isinstance(tau, bool) or not isinstance(tau, (int, np.integer)) or not 0 <= tau <= MAX_TAU:
        raise ValueError(f"{what}: max_error must be an integer in [0, {MAX_TAU}], got {tau!r}")
    return int(tau)


def _quantise_np(x: np.ndarray, base: np.ndarray, tau: int):
    """(q, rec) of integer arrays: r = x - base, q = sign(r) floor((|r| + tau) / (2 tau + 1)), rec = clamp(base +
    q (2 tau + 1), 0, 255)."""
    step = 2 * tau + 1
    r = x - base
    q = np.sign(r) * ((np.abs(r) + tau) // step)
    return q, np.clip(base + q * step, 0, 255)


def _residual_images(base, x, layout, x_layout, what: str):
    base, layout = _u8_batch(base, layout, f"{what} base")
    if x is not None:
        x, x_layout = _u8_batch(x, layout if x_layout is None else x_layout, f"{what} x")
        if x.size(0) != base.size(0) or _hw(x, x_layout) != _hw(base, layout):
            raise ValueError(f"{what}: x {tuple(x.shape)} ({x_layout}) does not match base {tuple(base.shape)} ({layout})")
        if x.device != base.device:
            raise ValueError(f"{what}: base and x are on different devices")
    return base, layout, x, x_layout


def _residual_front_cpu(base, x=None, tau: int = 0, layout: Optional[str] = None, x_layout: Optional[str] = None) -> Dict:
    """residual_front in NumPy integers: the definition written out (csrc/residual.h).  Samples in the canonical
    order i = (c H + y) W + x.  Context 8 c + class from a = max - min of channel c of base over the 3 x 3
    neighbourhood (edge replication); class 0 for a < 2, else floor(log2 a).  Digest = the sum over i of
    (base_i + 1) ((i + 1) K) mod 2^64.  With x: r = x - base, q = sign(r) floor((|r| + tau) / (2 tau + 1)), rec =
    clamp(base + q (2 tau + 1), 0, 255), bin q + 63 for |q| <= 63, else the escape bin 127."""
    tau = _check_tau(tau, "residual_front")
    base, layout, x, x_layout = _residual_images(base, x, layout, x_layout, "residual_front")
    b = _nchw(base.cpu(), layout).numpy().astype(np.int64)
    B, _, H, W = b.shape
    p = np.pad(b, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge")
    win = [p[:, :, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)]
    a = np.maximum.reduce(win) - np.minimum.reduce(win)
    ctx = (_CLASS_OF[a] + 8 * np.arange(3, dtype=np.uint8).reshape(1, 3, 1, 1)).astype(np.uint8)
    count = np.stack([np.bincount(ctx[i].reshape(-1), minlength=RES_CTX) for i in range(B)])
    with np.errstate(over="ignore"):
        w = np.arange(1, 3 * H * W + 1, dtype=np.uint64) * np.uint64(_DIGEST_K)
        digest = ((b.reshape(B, -1) + 1).astype(np.uint64) * w).sum(1, dtype=np.uint64)
    out = {"ctx": torch.from_numpy(ctx), "ctx_count": torch.from_numpy(count.astype(np.int64)),
           "digest": torch.from_numpy(digest.view(np.int64).copy())}
    if x is not None:
        xv = _nchw(x.cpu(), x_layout).numpy().astype(np.int64)
        q, rec = _quantise_np(xv, b, tau)
        bins = np.where(np.abs(q) <= RES_MAX_M, q + RES_MAX_M, RES_BINS - 1)
        key = ctx.astype(np.int64) * RES_BINS + bins
        hist = np.stack([np.bincount(key[i].reshape(-1), minlength=RES_CTX * RES_BINS) for i in range(B)])
        out.update(sym=torch.from_numpy(q.astype(np.int16)),
                   hist=torch.from_numpy(hist.reshape(B, RES_CTX, RES_BINS).astype(np.int64)),
                   max_err=torch.from_numpy(np.abs(xv - rec).reshape(B, -1).max(1).astype(np.int64)))
    return out


def _residual_apply_cpu(base, sym, tau: int, layout: Optional[str] = None, ref=None, out=None):
    """residual_apply in NumPy integers: out = clamp(base + sym (2 tau + 1), 0, 255); with ref also the exact squared
    error and the largest absolute error against it, per image."""
    tau = _check_tau(tau, "residual_apply")
    base, layout = _u8_batch(base, layout, "residual_apply base")
    b = _nchw(base.cpu(), layout).numpy().astype(np.int64)
    q = np.asarray(sym.cpu() if torch.is_tensor(sym) else sym).astype(np.int64).reshape(b.shape)
    rec = np.clip(b + q * (2 * tau + 1), 0, 255)
    img = torch.from_numpy(rec.astype(np.uint8))
    img = img.permute(0, 2, 3, 1).contiguous() if layout == "hwc" else img
    if out is not None:
        out.copy_(img)
        img = out
    if ref is None:
        return img
    ref, _ = _u8_batch(ref, layout, "residual_apply ref")
    d = rec - _nchw(ref.cpu(), layout).numpy().astype(np.int64)
    B = b.shape[0]
    return img, torch.from_numpy((d * d).reshape(B, -1).sum(1)), torch.from_numpy(np.abs(d).reshape(B, -1).max(1))


def _ptr(t):
    return None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())


def _front_buffers(dev, shape, with_x: bool, plane_words: Optional[int] = None) -> Dict:
    """What a front launch writes, on `dev`: ctx (of `shape`, B first), count and digest; with x also sym, hist and
    merr, and for the kinds with a low-bit plane (plane_words given) plane, mq and sq.  None where not asked for."""
    B = shape[0]
    o = dict.fromkeys(("sym", "plane", "hist", "merr", "mq", "sq"))
    o.update(ctx=torch.empty(shape, dtype=torch.uint8, device=dev),
             count=torch.empty(B, RES_CTX, dtype=torch.int32, device=dev),
             digest=torch.empty(B, dtype=torch.int64, device=dev))
    if with_x:
        o.update(sym=torch.empty(shape, dtype=torch.int16, device=dev),
                 hist=torch.empty(B, RES_CTX, RES_BINS, dtype=torch.int32, device=dev),
                 merr=torch.empty(B, dtype=torch.int32, device=dev))
        if plane_words is not None:
            o.update(plane=torch.empty(B, plane_words, dtype=torch.int64, device=dev),
                     mq=torch.empty(B, dtype=torch.int32, device=dev), sq=torch.empty(B, dtype=torch.int64, device=dev))
    if _lib.poison():  # what the kernel does not write shows
        o["ctx"].fill_(0xEE)
        for k in ("count", "digest", "hist", "merr", "mq", "sq", "plane"):
            if o[k] is not None:
                o[k].fill_(-1)
        if with_x:
            o["sym"].fill_(-0x1112)
    return o


def _front_result(o: Dict) -> Dict:
    """A front wrapper's result from its buffers: the counts as int64."""
    out = {"ctx": o["ctx"], "ctx_count": o["count"].to(torch.int64), "digest": o["digest"]}
    if o["sym"] is not None:
        out.update(sym=o["sym"], hist=o["hist"].to(torch.int64), max_err=o["merr"].to(torch.int64))
        if o["plane"] is not None:
            out.update(plane=o["plane"], max_abs_q=o["mq"].to(torch.int64), sum_abs_q=o["sq"])
    return out


def _apply_out(shape, deep: bool, dev) -> torch.Tensor:
    """An apply wrapper's default `out`: uint8, or uint16 words (made as int16, which fill_ takes), poison filled."""
    out = torch.empty(tuple(shape), dtype=torch.int16 if deep else torch.uint8, device=dev)
    if _lib.poison():
        out.fill_(-1 if deep else 0xFF)
    return out.view(torch.uint16) if deep else out


def _apply_buffers(dev, B: int, ref, sq_shape):
    """(sq, merr, status) of an apply launch: the error sums go with ref, the status is one word per image."""
    sq = merr = None
    if ref is not None:
        sq = torch.full(sq_shape, -1, dtype=torch.int64, device=dev)
        merr = torch.full((B,), -1, dtype=torch.int32, device=dev)
    return sq, merr, torch.full((B,), -1, dtype=torch.int32, device=dev)


def _apply_refusal(what: str, noun: str, status, refs):
    """After an apply launch: reads the status back and refuses the first image with a symbol outside [-255, 255];
    `refs` (moved to the device by the caller) stay alive until the stream has read them."""
    bad = torch.nonzero(status).flatten().cpu().tolist()
    for t in refs:
        t.record_stream(torch.cuda.current_stream())
    if bad:
        raise ValueError(f"{what}: {noun} {bad[0]} holds a symbol outside [-255, 255]")


def residual_front(base, x=None, tau: int = 0, layout: Optional[str] = None, x_layout: Optional[str] = None) -> Dict:
    """The encoder's and the decoder's first pass over the base image (csrc/residual.hip, one launch; DESIGN.md §5
    "Residual coding").  base: uint8 [B,H,W,3] / [B,3,H,W] (or one image), any strides; x: the original, the same
    size, in x_layout (default: base's layout).  Returns {"ctx" uint8 [B,3,H,W] (the context of every sample, in
    the canonical order), "ctx_count" int64 [B,24], "digest" int64 [B] (the uint64's bits)} and, with x, {"sym"
    int16 [B,3,H,W] (the quantised residual), "hist" int64 [B,24,128], "max_err" int64 [B] (the largest |x - rec|)}.
    CPU tensors take the NumPy restatement."""
    tau = _check_tau(tau, "residual_front")
    base, layout, x, x_layout = _residual_images(base, x, layout, x_layout, "residual_front")
    if not base.is_cuda:
        return _residual_front_cpu(base, x, tau, layout, x_layout)
    B = base.size(0)
    H, W = _hw(base, layout)
    base = _in_place(base, layout)
    dev = base.device
    with torch.cuda.device(dev):
        if x is not None:
            x = _in_place(x, x_layout)
        o = _front_buffers(dev, (B, 3, H, W), x is not None)
        _lib.call("mlic_image_residual_front_u8", _stream(), _ptr(base), (C.c_int64 * 4)(*_strides(base, layout)), _ptr(x),
                  None if x is None else (C.c_int64 * 4)(*_strides(x, x_layout)), B, H, W, tau, _ptr(o["ctx"]),
                  _ptr(o["count"]), _ptr(o["digest"]), _ptr(o["sym"]), _ptr(o["hist"]), _ptr(o["merr"]))
        return _front_result(o)


def residual_apply(base, sym, tau: int, layout: Optional[str] = None, ref=None, out: Optional[torch.Tensor] = None):
    """The decoder's last pass (csrc/residual.hip, one launch): out = clamp(base + sym (2 tau + 1), 0, 255) in base's
    layout.  sym: int16 [B,3,H,W], dense, on base's device.  out: an optional uint8 tensor of base's shape with any
    strides.  ref (uint8, base's shape, any strides): returns (out, sq_err int64 [B], max_abs_err int64 [B]), exact,
    on egress_u8's terms.  CPU tensors take the NumPy restatement."""
    tau = _check_tau(tau, "residual_apply")
    base, layout = _u8_batch(base, layout, "residual_apply base")
    B = base.size(0)
    H, W = _hw(base, layout)
    if not torch.is_tensor(sym) or sym.dtype != torch.int16 or tuple(sym.shape) != (B, 3, H, W):
        raise ValueError(f"residual_apply: sym must be an int16 tensor {(B, 3, H, W)}")
    if sym.device != base.device:
        raise ValueError("residual_apply: base and sym are on different devices")
    if out is not None and (out.dtype != torch.uint8 or tuple(out.shape) != tuple(base.shape) or out.device != base.device):
        raise ValueError(f"residual_apply: out must be uint8 {tuple(base.shape)} on {base.device}")
    if ref is not None:
        ref, _ = _u8_batch(ref, layout, "residual_apply ref")
        if tuple(ref.shape) != tuple(base.shape):
            raise ValueError(f"residual_apply: ref must have shape {tuple(base.shape)}, got {tuple(ref.shape)}")
        ref = ref.to(base.device)
    if not base.is_cuda:
        return _residual_apply_cpu(base, sym, tau, layout, ref, out)
    base = _in_place(base, layout)
    sym = sym.contiguous()
    dev = base.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(tuple(base.shape), dtype=torch.uint8, device=dev)
        elif 0 in _strides(out, layout)[2:]:
            raise ValueError("residual_apply: out has a zero column or channel stride")
        sq = merr = None
        if ref is not None:
            ref = _in_place(ref, layout)
            sq = torch.full((B,), -1, dtype=torch.int64, device=dev)
            merr = torch.full((B,), -1, dtype=torch.int32, device=dev)
        _lib.call("mlic_image_residual_apply_u8", _stream(), _ptr(base), (C.c_int64 * 4)(*_strides(base, layout)),
                  _ptr(sym), B, H, W, tau, _ptr(out), (C.c_int64 * 4)(*_strides(out, layout)), _ptr(ref),
                  None if ref is None else (C.c_int64 * 4)(*_strides(ref, layout)), _ptr(sq), _ptr(merr))
    return out if ref is None else (out, sq, merr.to(torch.int64))


def residual_tables(hist) -> Dict:
    """One image's tables from its histograms [24,128] (mlic_residual_tables): per context with a nonzero count,
    m = the largest |q| <= 63 seen, and the symbols -m..m plus the escape through pmf_to_quantized_cdf at precision
    16 on float32 count / total.  -> {"m" uint8 [24] (0xFF = no table), "freq" uint16 [24,128] (the file's 2 m + 2
    frequencies per table), "cdf" int32 [24,129], "length" int32 [24], "offset" int32 [24]} (the rANS tables)."""
    h = np.asarray(hist.cpu() if torch.is_tensor(hist) else hist)
    if h.shape != (RES_CTX, RES_BINS) or h.min() < 0 or h.max() > 0xFFFFFFFF:
        raise ValueError(f"residual_tables: a [{RES_CTX}, {RES_BINS}] histogram of counts expected")
    h = np.ascontiguousarray(h, dtype=np.uint32)
    m = np.zeros(RES_CTX, np.uint8)
    freq = np.zeros((RES_CTX, RES_BINS), np.uint16)
    cdf = np.zeros((RES_CTX, RES_CDF_STRIDE), np.int32)
    length, offset = np.zeros(RES_CTX, np.int32), np.zeros(RES_CTX, np.int32)
    _lib.call("mlic_residual_tables", h.ctypes.data, m.ctypes.data, freq.ctypes.data, cdf.ctypes.data, length.ctypes.data,
              offset.ctypes.data)
    return {"m": m, "freq": freq, "cdf": cdf, "length": length, "offset": offset}


def _tables_of_freq(m, freqs) -> Dict:
    """The rANS tables of a file's frequencies: integer sums, nothing rebuilt from floats."""
    cdf = np.zeros((RES_CTX, RES_CDF_STRIDE), np.int32)
    length, offset = np.zeros(RES_CTX, np.int32), np.zeros(RES_CTX, np.int32)
    for k in range(RES_CTX):
        if m[k] == RES_ABSENT:
            continue
        n = 2 * int(m[k]) + 2
        cdf[k, 1:n + 1] = np.cumsum(np.asarray(freqs[k][:n], np.int64))
        length[k], offset[k] = n + 1, -int(m[k])
    freq = np.zeros((RES_CTX, RES_BINS), np.uint16)
    for k in range(RES_CTX):
        if m[k] != RES_ABSENT:
            freq[k, :2 * int(m[k]) + 2] = freqs[k][:2 * int(m[k]) + 2]
    return {"m": np.asarray(m, np.uint8), "freq": freq, "cdf": cdf, "length": length, "offset": offset}


def _coder_tables(t: Dict):
    """(cdf, length, offset) as the rANS coder takes them: it wants every table well-formed, so a context without a
    table gets a two-symbol placeholder that no symbol is coded with (the callers check that no sample has it)."""
    cdf, length, offset = t["cdf"].copy(), t["length"].copy(), t["offset"].copy()
    for k in np.flatnonzero(length == 0):
        cdf[k, :3], length[k], offset[k] = (0, 32768, 65536), 3, 0
    return cdf, length, offset


def is_residual_file(data: bytes) -> bool:
    """A residual file of either kind: "MLR1" (one serial string) or "MLR2" (segments)."""
    return bytes(data[:4]) in (RESIDUAL_MAGIC, RESIDUAL_SEG_MAGIC)


def is_residual_seg_file(data: bytes) -> bool:
    return bytes(data[:4]) == RESIDUAL_SEG_MAGIC


def _write_residual(sfx: str, H, W, vbr, tau, own, digest, m, freq, seg, blobs) -> bytes:
    """The body of write_container_residual<sfx>: H, W, vbr, tau and `own` (the kind's own integer fields), the
    digest and the tables, seg = (segment, seg_bytes) of a segmented kind or None, then `blobs`, each behind its
    length.  Arguments are converted and checked in the order the four functions always had: m, freq, seg_bytes,
    the shapes, the lengths' range, then the integers.  The library is called twice: for the size, then to write."""
    what = "write_container_residual" + sfx
    m = np.ascontiguousarray(m, dtype=np.uint8)
    freq = np.ascontiguousarray(freq, dtype=np.uint16)
    if seg is not None:
        sb = np.ascontiguousarray(np.asarray(seg[1], np.int64).reshape(-1))
    if m.shape != (RES_CTX,) or freq.shape != (RES_CTX, RES_BINS):
        raise ValueError(f"{what}: m [{RES_CTX}] and freq [{RES_CTX}, {RES_BINS}] expected")
    if seg is not None and (sb.size > 0xFFFFFFFF or (sb.size and (sb.min() < 0 or sb.max() > 0xFFFFFFFF))):
        raise ValueError(f"{what}: segment lengths must fit 32 bits")
    args = (H, W, int(bool(vbr)), int(tau), *[int(v) for v in own], int(digest) & 0xFFFFFFFFFFFFFFFF, m.ctypes.data,
            freq.ctypes.data)
    if seg is not None:
        sb = sb.astype(np.uint32)
        args += (int(seg[0]) & 0xFFFFFFFF, sb.size, sb.ctypes.data)
    for blob in blobs:
        args += (blob, len(blob))
    n = C.c_size_t()
    _lib.call("mlic_container_write_residual" + sfx, *args, None, 0, C.byref(n))
    buf = C.create_string_buffer(max(1, n.value))
    _lib.call("mlic_container_write_residual" + sfx, *args, buf, len(buf), C.byref(n))
    return C.string_at(buf, n.value)


def _parse_residual(entry: str, info, data: bytes, n_levels, max_pixels):
    """The body of the four parse_container_residual* functions: `entry` fills `info`, the kind's info struct."""
    data = bytes(data)
    nl = _NO_LEVEL_LIMIT if n_levels is None else int(n_levels)
    _lib.call(entry, data, len(data), nl, int(max_pixels), C.byref(info))
    return info


def write_container_residual(H: int, W: int, inner: bytes, res: bytes, tau: int, digest: int, m, freq,
                             vbr: bool = False) -> bytes:
    """The residual file (mlic_container_write_residual): "MLR1", version, flags (bit 0: vbr), tau, n_ctx, H, W, the
    digest of the base image, the 24 tables (m and 2 m + 2 frequencies each, or 0xFF), then `inner`, the image's
    plain or VBR file, unchanged, and `res`, the residual string, each behind its length."""
    inner, res = bytes(inner), bytes(res)
    return _write_residual("", H, W, vbr, tau, (), digest, m, freq, None, (inner, res))


def parse_container_residual(data: bytes, n_levels: Optional[int] = None,
                             max_pixels: int = MAX_PIXELS) -> _lib.ContainerResidualInfo:
    """The validating parser of a residual file (mlic_container_parse_residual): raises _lib.MlicError on any
    malformed input.  The flags say whether the inner file has a level word; n_levels bounds it (None: any level).
    info.inner is the inner file's ContainerInfo, its offsets relative to data[info.inner_off:]."""
    return _parse_residual("mlic_container_parse_residual", _lib.ContainerResidualInfo(), data, n_levels, max_pixels)


def _file_tables(data: bytes, s: _lib.ContainerResidualInfo) -> Dict:
    freqs = []
    for k in range(RES_CTX):
        n = 0 if s.m[k] == RES_ABSENT else 2 * s.m[k] + 2
        freqs.append(np.frombuffer(data, ">u2", n, s.freq_off[k]))
    return _tables_of_freq(list(s.m), freqs)


def strip_residual(data: bytes, n_levels: Optional[int] = None, max_pixels: int = MAX_PIXELS) -> bytes:
    """The inner file of a residual file ("MLR1", "MLR2", "MLR3" or "MLR4"): byte for byte what encode_images writes
    without max_error= (for "MLR3": what encode_images(depth=) writes; for "MLR4": what encode_yuv writes)."""
    data = bytes(data)
    s = _parse_residual_any(data, n_levels, max_pixels)
    return data[s.inner_off:s.inner_off + s.inner_len]


_RESIDUAL_PARSERS = {RESIDUAL_MAGIC: ("mlic_container_parse_residual", _lib.ContainerResidualInfo),
                     RESIDUAL_SEG_MAGIC: ("mlic_container_parse_residual_seg", _lib.ContainerResidualSegInfo),
                     b"MLR3": ("mlic_container_parse_residual_deep", _lib.ContainerResidualDeepInfo),
                     b"MLR4": ("mlic_container_parse_residual_yuv", _lib.ContainerResidualYuvInfo)}


def _parse_residual_any(data: bytes, n_levels, max_pixels):
    """The parse of a residual file of any kind (told apart by the magic; "MLR1"'s parser refuses any other)."""
    entry, info = _RESIDUAL_PARSERS.get(bytes(data[:4]), _RESIDUAL_PARSERS[RESIDUAL_MAGIC])
    return _parse_residual(entry, info(), data, n_levels, max_pixels)


def _peek_residual(data: bytes, n_levels, max_pixels) -> Dict:
    s = _parse_residual_any(data, n_levels, max_pixels)
    c = s.inner
    out = {"residual": True, "H": s.H, "W": s.W, "max_error": s.tau, "vbr": bool(s.vbr),
           "level": c.level if s.vbr else None, "shape": (c.hz, c.wz), "Hp": 64 * c.hz, "Wp": 64 * c.wz,
           "y_len": c.y_len, "z_len": c.z_len, "digest": int(s.digest), "base_bytes": int(s.inner_len),
           "residual_bytes": int(s.res_len), "header_bytes": len(data) - int(s.inner_len) - int(s.res_len),
           "bytes": len(data), "bpp": 8.0 * len(data) / (s.H * s.W)}
    magic = bytes(data[:4])
    if magic != RESIDUAL_MAGIC:  # every kind but "MLR1" has segments
        out.update(residual_segment=int(s.seg_len), segments=int(s.n_seg))
    if magic in (b"MLR3", b"MLR4"):  # the low-bit plane
        out.update(depth=int(s.depth), shift=int(s.shift), low_bytes=int(s.lo_len))
        out["header_bytes"] -= int(s.lo_len)
    if magic == b"MLR4":
        out.update(sub=(int(s.sub_x), int(s.sub_y)), matrix={0: "bt601", 1: "bt709", 2: "bt2020"}[int(s.matrix)],
                   full_range=bool(s.full_range), site_x="left" if s.site_x else "centre")
    return out


# ---- segmented residual strings (csrc/residual_seg.h, csrc/residual_coder.hip)
class ResidualSegmentError(ValueError):
    """A coder refused a segment: .image (index in the call's batch), .segment, .reason."""

    def __init__(self, what: str, image: int, segment: int, reason: str):
        super().__init__(f"{what}: image {image}, segment {segment}: {reason}")
        self.image, self.segment, self.reason = image, segment, reason


def _check_segment(segment, what: str) -> int:
    if isinstance(segment, bool) or not isinstance(segment, (int, np.integer)) or not RES_SEG_MIN <= segment <= RES_SEG_MAX:
        raise ValueError(f"{what}: residual_segment must be an integer in [{RES_SEG_MIN}, {RES_SEG_MAX}], got {segment!r}")
    return int(segment)


def _check_coder(coder, what: str) -> str:
    if coder not in ("device", "host"):
        raise ValueError(f"{what}: residual_coder must be 'device' or 'host', got {coder!r}")
    return coder


def _seg_tables(tables, B: int, what: str):
    """(m uint8 [B,24], freq uint16 [B,24,128]) of B table dicts (residual_tables' or a file's); one dict serves all."""
    tables = [tables] * B if isinstance(tables, dict) else list(tables)
    if len(tables) != B:
        raise ValueError(f"{what}: {B} images but {len(tables)} table sets")
    m = np.ascontiguousarray(np.stack([np.asarray(t["m"], np.uint8) for t in tables]))
    freq = np.ascontiguousarray(np.stack([np.asarray(t["freq"], np.uint16) for t in tables]))
    if m.shape != (B, RES_CTX) or freq.shape != (B, RES_CTX, RES_BINS):
        raise ValueError(f"{what}: tables with m [{RES_CTX}] and freq [{RES_CTX}, {RES_BINS}] expected")
    return m, freq


def _seg_call(name: str, what: str, *args):
    """_lib.call, with a coder's refusal of a segment turned into ResidualSegmentError."""
    try:
        _lib.call(name, *args)
    except _lib.MlicError as e:
        hit = re.search(r"image (\d+), segment (\d+): (.*)$", str(e))
        if hit is None:
            raise
        raise ResidualSegmentError(what, int(hit.group(1)), int(hit.group(2)), hit.group(3)) from None


def _seg_scratch(B: int, n_seg: int, dev) -> torch.Tensor:
    n = C.c_size_t()
    _lib.call("mlic_residual_segments_scratch_bytes", B, n_seg, C.byref(n))
    return torch.empty(n.value, dtype=torch.uint8, device=dev)


def residual_segment_cap(H: int, W: int, segment: int) -> int:
    """Bytes that the segments of one H x W image cannot exceed: 4 (n + 4) per segment of n samples."""
    N = 3 * H * W
    return 4 * (N + RES_SEG_SLACK * -(-N // segment))


def _seg_images(sym, ctx, what: str):
    """-> (B, N, (H, W) or None): [B,3,H,W] planes of an RGB image, or [B,N] strings of N samples (a Y'CbCr frame's
    canonical order), which take the entries with N in place of H, W."""
    ok = lambda t, dt: torch.is_tensor(t) and t.dtype == dt and (t.dim() == 2 or (t.dim() == 4 and t.size(1) == 3))  # noqa: E731
    if sym is not None and not ok(sym, torch.int16):
        raise ValueError(f"{what}: sym must be an int16 tensor [B,3,H,W] (or [B,N])")
    if not ok(ctx, torch.uint8):
        raise ValueError(f"{what}: ctx must be a uint8 tensor [B,3,H,W] (or [B,N])")
    if sym is not None and (tuple(sym.shape) != tuple(ctx.shape) or sym.device != ctx.device):
        raise ValueError(f"{what}: sym {tuple(sym.shape)} and ctx {tuple(ctx.shape)} must match, on one device")
    if ctx.dim() == 2:
        if not 1 <= ctx.size(1) <= RES_SEG_MAX_N:
            raise ValueError(f"{what}: N must be in [1, 2^29], got {ctx.size(1)}")
        return ctx.size(0), ctx.size(1), None
    return ctx.size(0), 3 * ctx.size(2) * ctx.size(3), (ctx.size(2), ctx.size(3))



def residual_encode_segments(sym, ctx, tables, segment: int, coder: str = "device", cap: Optional[int] = None,
                             out: Optional[torch.Tensor] = None):
    """The segmented residual strings of B images (csrc/residual_coder.hip; mlic_residual_encode_segments): sym int16
    and ctx uint8 [B,3,H,W] (residual_front's), tables: B dicts with "m" and "freq" (residual_tables'), segment: the
    samples per segment.  -> [(bytes, seg_bytes uint32 [n_seg])] per image; bytes is the concatenation of the
    segments, each exactly entropy.rans_encode of its slice.  CUDA tensors with coder="device" run the kernels (a
    counting pass, a scan, a writing pass; only the bytes and their lengths come back); CPU tensors or coder="host"
    take the host entry, which gives the same bytes.  cap: the bytes allowed per image (default: the bound
    residual_segment_cap); out: an optional uint8 device buffer of at least B cap bytes to code into."""
    what = "residual_encode_segments"
    B, N, hw = _seg_images(sym, ctx, what)
    L, coder = _check_segment(segment, what), _check_coder(coder, what)
    n_seg = -(-N // L)
    size = hw if hw is not None else (N,)  # H, W of an RGB image, or N alone (the _n entries)
    sfx = "" if hw is not None else "_n"
    m, freq = _seg_tables(tables, B, what)
    cap = 4 * (N + RES_SEG_SLACK * n_seg) if cap is None else int(cap)
    lens = (C.c_uint64 * B)()
    if sym.is_cuda and coder == "device":
        sym, ctx = sym.contiguous(), ctx.contiguous()
        dev = sym.device
        with torch.cuda.device(dev):
            if out is None:
                out = torch.empty(B * cap, dtype=torch.uint8, device=dev)
            elif out.dtype != torch.uint8 or out.device != dev or not out.is_contiguous() or out.numel() < B * cap:
                raise ValueError(f"{what}: out must be a contiguous uint8 tensor of at least {B * cap} bytes on {dev}")
            segb = torch.empty(B, n_seg, dtype=torch.int32, device=dev)
            scratch = _seg_scratch(B, n_seg, dev)
            _seg_call("mlic_residual_encode_segments" + sfx, what, _stream(), C.c_void_p(sym.data_ptr()),
                      C.c_void_p(ctx.data_ptr()), B, *size, m.ctypes.data, freq.ctypes.data, L, n_seg,
                      C.c_void_p(out.data_ptr()), cap, C.c_void_p(segb.data_ptr()), lens, C.c_void_p(scratch.data_ptr()),
                      scratch.numel(), None)
            top = max(lens)
            data = out[:B * cap].view(B, cap)[:, :top].cpu().numpy()
            segb = segb.cpu().numpy().view(np.uint32)
    else:
        s = np.ascontiguousarray(sym.cpu().numpy())
        c = np.ascontiguousarray(ctx.cpu().numpy())
        data = np.empty((B, cap), np.uint8)
        segb = np.empty((B, n_seg), np.uint32)
        _seg_call("mlic_residual_encode_segments_host" + sfx, what, s.ctypes.data, c.ctypes.data, B, *size, m.ctypes.data,
                  freq.ctypes.data, L, n_seg, data.ctypes.data, cap, segb.ctypes.data, lens)
    return [(data[b, :lens[b]].tobytes(), segb[b].copy()) for b in range(B)]


def residual_decode_segments(data, seg_bytes, ctx, tables, segment: int, coder: str = "device",
                             out: Optional[torch.Tensor] = None):
    """The symbols of B images' segmented residual strings (mlic_residual_decode_segments): data: B byte strings,
    seg_bytes: B arrays of n_seg lengths, ctx uint8 [B,3,H,W], tables: B dicts with "m" and "freq".  -> int16
    [B,3,H,W] on ctx's device, straight into the buffer residual_apply reads: on the device path no symbol and no
    context crosses to the host.  Every segment must consume exactly its words and end at the state 2^31; a segment
    that does not, or that holds what a well-formed one cannot, raises ResidualSegmentError.  out: an optional
    contiguous int16 device tensor of at least B 3 H W elements to decode into (the result is a view of it)."""
    what = "residual_decode_segments"
    B, N, hw = _seg_images(None, ctx, what)
    L, coder = _check_segment(segment, what), _check_coder(coder, what)
    n_seg = -(-N // L)
    size = hw if hw is not None else (N,)
    sfx = "" if hw is not None else "_n"
    shape = tuple(ctx.shape)
    m, freq = _seg_tables(tables, B, what)
    data = [bytes(d) for d in data]
    if len(data) != B or len(seg_bytes) != B:
        raise ValueError(f"{what}: {B} images but {len(data)} strings and {len(seg_bytes)} length arrays")
    segb = np.ascontiguousarray(np.stack([np.asarray(v, np.int64).reshape(-1) for v in seg_bytes]))
    if segb.shape != (B, n_seg) or segb.min() < 0 or segb.max() > 0xFFFFFFFF:
        raise ValueError(f"{what}: {n_seg} segment lengths per image expected")
    segb = segb.astype(np.uint32)
    stride = (max(len(d) for d in data) + 3) // 4 * 4
    buf = np.zeros((B, max(stride, 4)), np.uint8)
    for b, d in enumerate(data):
        buf[b, :len(d)] = np.frombuffer(d, np.uint8)
    lens = (C.c_uint64 * B)(*[len(d) for d in data])
    if ctx.is_cuda and coder == "device":
        ctx = ctx.contiguous()
        dev = ctx.device
        with torch.cuda.device(dev):
            if out is None:
                sym = torch.empty(shape, dtype=torch.int16, device=dev)
                if _lib.poison():
                    sym.fill_(-0x1112)
            elif out.dtype != torch.int16 or out.device != dev or not out.is_contiguous() or out.numel() < B * N:
                raise ValueError(f"{what}: out must be a contiguous int16 tensor of at least {B * N} elements on {dev}")
            else:
                sym = out.view(-1)[:B * N].view(shape)
            scratch = _seg_scratch(B, n_seg, dev)
            d_dev = torch.from_numpy(buf).to(dev)
            _seg_call("mlic_residual_decode_segments" + sfx, what, _stream(), C.c_void_p(d_dev.data_ptr()), buf.shape[1],
                      lens, segb.ctypes.data, C.c_void_p(ctx.data_ptr()), B, *size, m.ctypes.data, freq.ctypes.data, L, n_seg,
                      C.c_void_p(sym.data_ptr()), C.c_void_p(scratch.data_ptr()), scratch.numel(), None)
        return sym
    c = np.ascontiguousarray(ctx.cpu().numpy())
    q = np.empty(shape, np.int16)
    _seg_call("mlic_residual_decode_segments_host" + sfx, what, buf.ctypes.data, buf.shape[1], lens, segb.ctypes.data,
              c.ctypes.data, B, *size, m.ctypes.data, freq.ctypes.data, L, n_seg, q.ctypes.data)
    return torch.from_numpy(q).to(ctx.device)


def write_container_residual_seg(H: int, W: int, inner: bytes, segs: bytes, seg_bytes, segment: int, tau: int,
                                 digest: int, m, freq, vbr: bool = False) -> bytes:
    """The segmented residual file (mlic_container_write_residual_seg): "MLR2", then the header and the tables of
    the "MLR1" file, seg_len, n_seg, `inner` behind its length, and behind res_len the n_seg segment byte lengths
    and `segs`, the concatenated segments."""
    inner, segs = bytes(inner), bytes(segs)
    return _write_residual("_seg", H, W, vbr, tau, (), digest, m, freq, (segment, seg_bytes), (inner, segs))


def parse_container_residual_seg(data: bytes, n_levels: Optional[int] = None,
                                 max_pixels: int = MAX_PIXELS) -> _lib.ContainerResidualSegInfo:
    """The validating parser of a segmented residual file (mlic_container_parse_residual_seg): raises _lib.MlicError
    on any malformed input.  info.index_off: the n_seg big-endian u32 lengths; info.data_off / data_len: the
    segments."""
    return _parse_residual("mlic_container_parse_residual_seg", _lib.ContainerResidualSegInfo(), data, n_levels,
                           max_pixels)


def _seg_cap_of_hist(hist, t, n_seg: int) -> int:
    """An upper bound of one image's segment bytes from its histograms and tables: a symbol of frequency f grows the
    coder's state by less than 16 - log2 f + 2^-14 bits and an escape by 16 more (csrc/residual_seg.h), and a
    segment adds its flush and less than a word of rounding.  Far below one word per sample on real pictures."""
    bits = 0.0
    for k in range(RES_CTX):
        if t["m"][k] == RES_ABSENT:
            continue
        cnt = 2 * int(t["m"][k]) + 2
        h = np.zeros(cnt, np.float64)
        mk = int(t["m"][k])
        h[:cnt - 1] = hist[k, RES_MAX_M - mk:RES_MAX_M + mk + 1]
        h[cnt - 1] = hist[k, RES_BINS - 1]
        bits += float((h * (16.0 + 2.0 ** -14 - np.log2(t["freq"][k, :cnt].astype(np.float64)))).sum())
        bits += (16.0 + 4 * 2.0 ** -14) * float(h[cnt - 1])
    return (int(bits / 8.0) + 16 * n_seg + 64) // 4 * 4


def _refuse_residual(what: str, **given):
    """max_error= composes with nothing but level=: each other feature is refused by name."""
    for name, on in given.items():
        if on:
            raise ValueError(f"{what}: max_error= (residual coding) together with {name} is not supported")


def _base_x_hat(net, strings, shape, kw, B):
    """x_hat of the strings just made, as a decoder of each file alone will have it.  The fp16 range guard re-runs
    g_s in fp32 for a whole lane when any image of it overflows, so after a batch decode that took that path each
    image is decoded alone."""
    counters = getattr(net, "range_fallbacks", None)
    before = counters()["decompress_gs"] if counters else 0
    x_hat = net.decompress(strings, shape, **kw)["x_hat"]
    if B > 1 and counters and counters()["decompress_gs"] != before:
        one = [net.decompress([[strings[0][b]], [strings[1][b]]], shape, **{k: [v[b]] for k, v in kw.items()})["x_hat"]
               for b in range(B)]
        x_hat = torch.cat(one, 0)
    return x_hat


class _ResidualKind(NamedTuple):
    """What differs between the kinds of residual layer (8-bit RGB, deep RGB, Y'CbCr planes): everything else is in
    _encode_residual_layer and _decode_residual_layer.  A batch is a tensor [B,H,W,3] or three planes."""
    entry: str  # the decoder's name in messages
    noun: str  # "image" or "frame"
    base_word: str  # "base image" or "base planes"
    low: bool  # whether the files carry a shift and a low-bit plane
    front: Callable  # (base, x or None, tau, shift) -> residual_front*'s dictionary
    stats: Optional[Callable]  # (base, x, tau) -> residual_stats*'s dictionary
    apply: Callable  # (base, sym, plane, tau, shift, ref, out) -> None, or with ref (sq_err [B...], max_abs_err [B])
    decode_inner: Callable  # (net, inner files, ref, max_pixels) -> (batch, info): the kind's plain decode
    size: Callable  # batch -> (H, W, device)
    crop: Callable  # (batch, slice of the batch, h, w) -> a view; h=None: whole pictures
    paste: Callable  # (view of one picture, the same picture decoded alone): copies it in
    canvas: Callable  # (base, zero) -> an output batch like base
    check_ref: Callable  # (ref, B, H, W, device) -> ref on the device, or ValueError
    samples: Callable  # (h, w) -> N
    plane_words: Callable  # (h, w, shift) -> 64-bit words of the low-bit plane
    check_low: Callable  # (file index, the plane's words, h, w, shift): ValueError if a padding bit is set
    score: Callable  # (sq_err of one picture, h, w) -> the info fields
    extra: Callable  # shift -> the info fields a kind adds
    write: Callable  # (H, W, inner, segs, seg_bytes, segment, tau, shift, low, digest, m, freq, vbr) -> the file


def _copy_words(dst: torch.Tensor, src: torch.Tensor):
    if dst.dtype == torch.uint16:  # copy_ takes int16
        dst, src = dst.view(torch.int16), src.view(torch.int16)
    dst.copy_(src)


def _like(t: torch.Tensor, zero: bool) -> torch.Tensor:
    deep = t.dtype == torch.uint16
    out = (torch.zeros if zero else torch.empty)(tuple(t.shape), dtype=torch.int16 if deep else torch.uint8, device=t.device)
    return out.view(torch.uint16) if deep else out


def _rgb_kind(depth: Optional[int] = None, x_layout: Optional[str] = None) -> _ResidualKind:
    """The kind of 8-bit RGB images (depth=None: "MLR1", "MLR2") or of deep ones ("MLR3"), base in HWC."""
    deep = depth is not None
    word = "uint16" if deep else "uint8"

    def check_ref(ref, B, H, W, dev):
        if not deep:  # _decode_residual16 has made a batch of it before it split the depths
            ref, _ = _u8_batch(ref, "hwc", "decode_images ref")
        if tuple(ref.shape) != (B, H, W, 3):
            raise ValueError(f"decode_images: ref must be {word} {(B, H, W, 3)}, got {tuple(ref.shape)}")
        return ref.to(dev)

    def check_low(b, pl, h, w, sh):
        if sh and w % 64 and (pl.reshape(3 * h, -(-w // 64), sh)[:, -1, :] >> np.uint64(w % 64)).any():
            raise ValueError(f"decode_images: file {b}: the low-bit plane has bits set beyond column {w} (its "
                             f"padding bits must be zero)")

    def apply(base, sym, plane, tau, sh, ref, out):
        if deep:
            r = residual_apply16(base, sym, plane, depth, tau, sh, "hwc", ref=ref, out=out)
        else:
            r = residual_apply(base, sym, tau, "hwc", ref=ref, out=out)
        return None if ref is None else r[1:]

    def front(base, x, tau, sh):
        if deep:
            return residual_front16(base, x, depth, tau, sh, "hwc", x_layout)
        return residual_front(base, x, tau, "hwc", x_layout)

    def write(H, W, inner, segs, seg_bytes, L, tau, sh, low, digest, m, freq, vbr):
        if deep:
            return write_container_residual_deep(H, W, inner, segs, seg_bytes, L, tau, depth, sh, low, digest, m, freq,
                                                 vbr=vbr)
        return write_container_residual_seg(H, W, inner, segs, seg_bytes, L, tau, digest, m, freq, vbr=vbr)

    kw = {"depth": depth} if deep else {}
    peak = (1 << depth) - 1 if deep else 255
    return _ResidualKind(
        entry="decode_images", noun="image", base_word="base image", low=deep, front=front,
        stats=(lambda base, x, tau: residual_stats16(base, x, depth, tau, "hwc", x_layout)) if deep else None, apply=apply,
        decode_inner=lambda net, inner, ref, max_pixels: decode_images(net, inner, ref=ref, max_pixels=max_pixels, **kw),
        size=lambda t: (t.size(1), t.size(2), t.device),
        crop=lambda t, sl, h=None, w=None: t[sl] if h is None else t[sl, :h, :w],
        paste=_copy_words, canvas=_like, check_ref=check_ref, samples=lambda h, w: 3 * h * w,
        plane_words=residual_plane_words, check_low=check_low,
        score=lambda sq, h, w: {"sq_err": int(sq), "psnr": psnr_from_sq_err(int(sq), 3 * h * w, peak)},
        extra=lambda sh: {"depth": depth, "shift": sh} if deep else {}, write=write)


def _residual_shifts(what: str, name: str, kind: _ResidualKind, depth: int, N: int, stats: Dict, shift, B: int):
    """The shift of every image of a batch from residual_stats*'s figures: by the rule (residual_shift), or the
    explicit `shift` (the caller's argument `name`), refused if it does not fit an image."""
    mq, sq = stats["max_abs_q"].cpu().tolist(), stats["sum_abs_q"].cpu().tolist()
    if shift is None:
        return [residual_shift(depth, N, mq[b], sq[b]) for b in range(B)]
    for b in range(B):
        if not residual_shift_fits(mq[b], shift):
            raise ValueError(f"{what}: {name}={shift} does not fit {kind.noun} {b} (its largest |q| is {mq[b]}): the "
                             f"smallest shift that fits is {residual_min_shift(depth, mq[b])}")
    return [shift] * B


def _inner_x_hat(net, inner):
    """(x_hat, vbr) of the plain or VBR files just written, as a decoder of each file alone will have it."""
    vbr = hasattr(net, "levels")
    cs = [parse_container(f, vbr, net.levels if vbr else None) for f in inner]
    pairs = [_strings(f, c) for f, c in zip(inner, cs)]
    kw = {"s": [c.level for c in cs]} if vbr else {}
    x_hat = _base_x_hat(net, [[p[0] for p in pairs], [p[1] for p in pairs]], (cs[0].hz, cs[0].wz), kw, len(inner))
    return x_hat, vbr


def _encode_residual_layer(kind: _ResidualKind, what: str, base, x, H: int, W: int, tau: int, shifts, segment, coder,
                           inner, vbr: bool):
    """The residual files of `inner` (the pictures' plain or VBR files) for the originals x over the base pictures
    `base`, and the info fields they add -> (files, extra).  Runs of pictures with one shift take one front launch
    each; the bound is checked on the device value; the tables come from the histograms.  segment=L: segmented
    strings through residual_encode_segments (coder="device": sym and ctx stay on the device, the histograms alone
    go to the host); segment=None (8-bit RGB only): one serial string per image, coded on the host ("MLR1")."""
    B = len(inner)
    N = kind.samples(H, W)
    files, extra = [None] * B, [None] * B
    a = 0
    while a < B:  # runs of pictures with one shift: one front launch each
        e = a + 1
        while e < B and shifts[e] == shifts[a]:
            e += 1
        s = shifts[a]
        front = kind.front(kind.crop(base, slice(a, e)), kind.crop(x, slice(a, e)), tau, s)
        worst = int(front["max_err"].max())  # computed on the device, beside the symbols
        if worst > tau:
            raise RuntimeError(f"{what}: the residual layer leaves an error of {worst} > max_error {tau}")
        hist = front["hist"].cpu().numpy()
        digest = front["digest"].cpu().tolist()
        tabs = [residual_tables(hist[j]) for j in range(e - a)]
        if segment is None:
            sym = front["sym"].cpu().numpy().reshape(e - a, -1)
            ctx = front["ctx"].cpu().numpy().reshape(e - a, -1)
            for j, t in enumerate(tabs):
                res = entropy.rans_encode(sym[j].astype(np.int32), ctx[j].astype(np.int32), *_coder_tables(t))
                files[a + j] = write_container_residual(H, W, inner[a + j], res, tau, digest[j], t["m"], t["freq"], vbr=vbr)
                extra[a + j] = {"max_error": tau, "base_bytes": len(inner[a + j]), "residual_bytes": len(res)}
            a = e
            continue
        n_seg = -(-N // segment)
        plane = front["plane"].cpu().numpy() if kind.low else None
        cap = min(max(_seg_cap_of_hist(hist[j], tabs[j], n_seg) for j in range(e - a)), 4 * (N + RES_SEG_SLACK * n_seg))
        coded = residual_encode_segments(front["sym"], front["ctx"], tabs, segment, coder, cap=cap)
        for j, (segs, seg_bytes) in enumerate(coded):
            b, t = a + j, tabs[j]
            low = plane[j].astype("<i8").tobytes() if kind.low else b""
            files[b] = kind.write(H, W, inner[b], segs, seg_bytes, segment, tau, s, low, digest[j], t["m"], t["freq"], vbr)
            extra[b] = {"max_error": tau, **kind.extra(s), "base_bytes": len(inner[b]),
                        "residual_bytes": len(segs) + 4 * n_seg, **({"low_bytes": len(low)} if kind.low else {}),
                        "residual_segment": segment, "segments": n_seg}
        a = e
    return files, extra


def _encode_residual(net, img, layout, files, strings, shape, lv, tau, segment=None, coder="device"):
    """encode_images' second layer: the residual files of `files` (the images' plain or VBR files) and the info.
    segment=None: the serial file ("MLR1"); segment=L: the segmented file ("MLR2").  Both code the same symbols."""
    B = img.size(0)
    H, W = _hw(img, layout)
    kw = {} if lv is None else {"s": list(lv)}
    base = egress_u8(_base_x_hat(net, strings, shape, kw, B), H, W, "hwc")
    return _encode_residual_layer(_rgb_kind(x_layout=layout), "encode_images", base, img, H, W, tau, [0] * B, segment,
                                  coder, files, lv is not None)


def _digest_error(b: int, want: int, got: int, net) -> RuntimeError:
    return RuntimeError(
        f"decode_images: file {b}: the digest of the decoded base image is {got & 0xFFFFFFFFFFFFFFFF:#018x}, the file "
        f"says {want:#018x}: this decoder's base image is not the encoder's, so the residual cannot be applied and no "
        f"error bound holds.  The base image depends on the synthesis arithmetic: decode with the encoder's "
        f"set_synthesis_precision and precision mode (here set_synthesis_precision "
        f"{getattr(net, '_synth_precision', '?')}, precision mode {getattr(net, '_precision', '?')}), or decode the "
        f"base image alone with enhance=False")


def _parse_residual_files(entry: str, net, files, max_pixels, check=None):
    """Every file parsed and its level word checked against the model; check(b, info): the kind's own checks."""
    vbr = hasattr(net, "levels")
    ss = [_parse_residual_any(f, net.levels if vbr else None, max_pixels) for f in files]
    for b, s in enumerate(ss):
        if bool(s.vbr) != vbr:
            raise ValueError(f"{entry}: the residual file's inner file {'carries a' if s.vbr else 'has no'} "
                             f"level word, the model is {'variable' if vbr else 'fixed'}-rate")
        if check is not None:
            check(b, s)
    return ss


def _decode_residual_layer(kind: _ResidualKind, net, files, ss, ref, max_pixels, enhance, coder):
    """The decoder of every kind of residual file, after _parse_residual_files: the inner files through the kind's
    plain decode, then the residual layer.  Files of one size, tau, shift and segment length go through the kernels
    as one batch, others one by one.  The base of a file is defined as the decode of that file alone: where the
    batch's base has another digest (the range guard's fp32 re-run takes a whole lane) the file is decoded alone and
    that base pasted in; if its digest differs too, no picture is returned (_digest_error).  "MLR1" files decode
    their string on the host; the others go through residual_decode_segments (coder="device": the kernel, on a GPU
    model; "host": the host entry), whose int16 output the apply kernel reads in place."""
    B = len(files)
    inner = [f[s.inner_off:s.inner_off + s.inner_len] for f, s in zip(files, ss)]
    keys, extra = [], []
    for f, s in zip(files, ss):
        sh, L = int(s.shift) if kind.low else 0, int(getattr(s, "seg_len", 0))  # L = 0: the serial kind
        keys.append((int(s.tau), sh, L))
        extra.append({"max_error": int(s.tau), **kind.extra(sh), "residual_bytes": int(s.res_len),
                      "base_bytes": int(s.inner_len), **({"low_bytes": int(s.lo_len)} if kind.low else {}),
                      **({"residual_segment": L, "segments": int(s.n_seg)} if L else {}), "bytes": len(f),
                      "bpp": 8.0 * len(f) / (s.H * s.W)})
    if not enhance:
        img, info = kind.decode_inner(net, inner, ref, max_pixels)
        for d, e in zip(info, extra):
            d.update(e, enhanced=False)
        return img, info
    base, info = kind.decode_inner(net, inner, None, max_pixels)
    H, W, dev = kind.size(base)
    if ref is not None:
        ref = kind.check_ref(ref, B, H, W, dev)
    same = all((s.H, s.W) == (H, W) for s in ss)
    one = same and len(set(keys)) == 1
    groups = [list(range(B))] if one else [[b] for b in range(B)]
    img = kind.canvas(base, not same)  # files of differing sizes come back in a zeroed canvas
    for g in groups:
        h, w = ss[g[0]].H, ss[g[0]].W
        tau, sh, L = keys[g[0]]
        sl = slice(g[0], g[-1] + 1)
        view = kind.crop(base, sl, h, w)
        front = kind.front(view, None, tau, 0)
        digest = front["digest"].cpu().tolist()
        for j, b in enumerate(g):
            if (digest[j] & 0xFFFFFFFFFFFFFFFF) == ss[b].digest:
                continue
            alone, _ = kind.decode_inner(net, [inner[b]], None, max_pixels)
            again = int(kind.front(alone, None, tau, 0)["digest"].cpu()[0])
            if (again & 0xFFFFFFFFFFFFFFFF) != ss[b].digest:
                raise _digest_error(b, int(ss[b].digest), again, net)
            kind.paste(kind.crop(base, slice(b, b + 1), h, w), alone)
            front = None
        if front is None:
            front = kind.front(view, None, tau, 0)
        count = front["ctx_count"].cpu().numpy()
        tabs = [_file_tables(files[b], ss[b]) for b in g]
        planes = []
        for j, b in enumerate(g):
            missing = [k for k in range(RES_CTX) if count[j, k] > 0 and tabs[j]["m"][k] == RES_ABSENT]
            if missing:
                raise ValueError(f"{kind.entry}: file {b}: contexts {missing} occur in the {kind.base_word} but the "
                                 f"file has no table for them")
            if kind.low:
                pl = np.frombuffer(files[b], "<u8", kind.plane_words(h, w, sh), ss[b].lo_off)
                kind.check_low(b, pl, h, w, sh)
                planes.append(pl.view(np.int64))
        if L:  # segments: no symbol and no context crosses to the host on the device path
            try:
                sym_d = residual_decode_segments(
                    [files[b][ss[b].data_off:ss[b].data_off + ss[b].data_len] for b in g],
                    [np.frombuffer(files[b], ">u4", ss[b].n_seg, ss[b].index_off) for b in g], front["ctx"], tabs, L, coder)
            except ResidualSegmentError as e:
                raise ValueError(f"{kind.entry}: file {g[e.image]}: segment {e.segment} of the residual string is "
                                 f"corrupt: {e.reason}") from None
        else:
            ctx = front["ctx"].cpu().numpy().reshape(len(g), -1)
            sym = np.empty(ctx.shape, np.int16)
            for j, b in enumerate(g):
                res = files[b][ss[b].res_off:ss[b].res_off + ss[b].res_len]
                q = entropy.rans_decode(res, ctx[j].astype(np.int32), *_coder_tables(tabs[j]))
                if q.size and (q.min() < -255 or q.max() > 255):
                    raise ValueError(f"{kind.entry}: file {b}: the residual string holds a symbol outside [-255, 255]")
                sym[j] = q
            sym_d = torch.from_numpy(sym.reshape(tuple(front["ctx"].shape))).to(dev)
        plane_d = torch.from_numpy(np.stack(planes).reshape(len(g), -1).copy()).to(dev) if kind.low else None
        try:
            r = kind.apply(view, sym_d, plane_d, tau, sh, None if ref is None else kind.crop(ref, sl, h, w),
                           kind.crop(img, sl, h, w))
        except ValueError as e:
            if not kind.low:  # only the kinds with a status word refuse a symbol here, and name the files
                raise
            raise ValueError(f"{kind.entry}: files {g[0]}..{g[-1]}: {e}") from None
        if ref is not None:
            sq, me = r[0].cpu().tolist(), r[1].cpu().tolist()
            for j, b in enumerate(g):
                extra[b].update(kind.score(sq[j], h, w), max_abs_err=int(me[j]))
    for d, e in zip(info, extra):
        d.update(e)
    return img, info


def _decode_residual(net, files, ref, max_pixels, enhance, coder="device"):
    """decode_images for "MLR1" and "MLR2" files."""
    ss = _parse_residual_files("decode_images", net, files, max_pixels)
    return _decode_residual_layer(_rgb_kind(), net, files, ss, ref, max_pixels, enhance, coder)


# ---- residual coding of 9..16-bit samples (csrc/residual16.h, csrc/residual16.hip; DESIGN.md §5 "Deep samples")
RESIDUAL_DEEP_MAGIC = b"MLR3"
RES16_MIN_DEPTH, RES16_MAX_HI = 9, 255


def is_residual_deep_file(data: bytes) -> bool:
    return bytes(data[:4]) == RESIDUAL_DEEP_MAGIC


def _check_shift(shift, depth: int, what: str) -> int:
    if isinstance(shift, bool) or not isinstance(shift, (int, np.integer)) or not 0 <= shift <= depth - 7:
        raise ValueError(f"{what}: shift must be an integer in [0, depth - 7 = {depth - 7}], got {shift!r}")
    return int(shift)


def residual_shift_fits(max_abs_q: int, shift: int) -> bool:
    """Whether `shift` keeps every |hi| within 255 for an image whose largest |q| is max_abs_q."""
    return (int(max_abs_q) + (1 << shift) - 1) >> shift <= RES16_MAX_HI


def residual_min_shift(depth: int, max_abs_q: int) -> int:
    """The smallest shift that fits (depth - 7 always does)."""
    return next(s for s in range(depth - 6) if residual_shift_fits(max_abs_q, s))


def residual_shift(depth: int, n: int, max_abs_q: int, sum_abs_q: int) -> int:
    """The shift rule (mlic_residual_shift; host integers): the smallest s in 0..depth-7 with (max_abs_q + 2^s - 1)
    >> s <= 255 and sum_abs_q <= 8 n 2^s, n = 3 H W the image's samples; depth - 7 if there is none."""
    depth = _check_depth(depth, "residual_shift", RES16_MIN_DEPTH)
    s = C.c_int()
    _lib.call("mlic_residual_shift", depth, int(n), int(max_abs_q), int(sum_abs_q), C.byref(s))
    return s.value


def residual_plane_words(H: int, W: int, shift: int) -> int:
    """64-bit words of one image's low-bit plane: 3 H ceil(W / 64) shift."""
    return 3 * H * -(-W // 64) * shift


def _residual16_images(base, x, layout, x_layout, what: str):
    base, layout = _u16_batch(base, layout, f"{what} base")
    if x is not None:
        x, x_layout = _u16_batch(x, layout if x_layout is None else x_layout, f"{what} x")
        if x.size(0) != base.size(0) or _hw(x, x_layout) != _hw(base, layout):
            raise ValueError(f"{what}: x {tuple(x.shape)} ({x_layout}) does not match base {tuple(base.shape)} ({layout})")
        if x.device != base.device:
            raise ValueError(f"{what}: base and x are on different devices")
    return base, layout, x, x_layout


def _samples_np(t: torch.Tensor, layout: str, depth: int) -> np.ndarray:
    """uint16 words (any device) -> int64 samples [B,3,H,W]; a word above maxv reads as maxv."""
    return samples_of_words(_nchw(t.cpu(), layout), depth).numpy().astype(np.int64)


def _pack_plane_np(lo: np.ndarray, shift: int) -> np.ndarray:
    """lo int64 [B,3,H,W] in 0..2^shift-1 -> the low-bit planes, uint64 [B, 3 H G shift]: word ((c H + y) G + g) shift
    + j holds bit j of lo(c, y, x) at bit x mod 64, zero beyond column W."""
    B, _, H, W = lo.shape
    G = -(-W // 64)
    p = np.zeros((B, 3, H, 64 * G), np.uint64)
    p[..., :W] = lo.astype(np.uint64)
    p = p.reshape(B, 3, H, G, 64)
    bit = np.uint64(1) << np.arange(64, dtype=np.uint64)
    out = np.zeros((B, 3, H, G, shift), np.uint64)
    for j in range(shift):
        out[..., j] = (((p >> np.uint64(j)) & np.uint64(1)) * bit).sum(-1, dtype=np.uint64)
    return out.reshape(B, -1)


def _unpack_plane_np(plane: np.ndarray, H: int, W: int, shift: int) -> np.ndarray:
    """The inverse of _pack_plane_np: uint64 [B, 3 H G shift] -> lo int64 [B,3,H,W]."""
    B = plane.shape[0]
    G = -(-W // 64)
    if shift == 0:
        return np.zeros((B, 3, H, W), np.int64)
    w = plane.reshape(B, 3, H, G, shift, 1) >> np.arange(64, dtype=np.uint64).reshape(1, 1, 1, 1, 1, 64)
    bits = (w & np.uint64(1)).astype(np.int64)  # [B,3,H,G,shift,64]
    lo = (bits << np.arange(shift, dtype=np.int64).reshape(1, 1, 1, 1, shift, 1)).sum(4)
    return lo.reshape(B, 3, H, 64 * G)[..., :W]


def _residual_front16_cpu(base, x, depth: int, tau: int, shift: int, layout: str, x_layout, stats: bool = False) -> Dict:
    """residual_front16 / residual_stats16 in NumPy integers: the definitions of csrc/residual16.h written out."""
    b = _samples_np(base, layout, depth)
    B, _, H, W = b.shape
    out = {}
    if not stats:
        p = np.pad(b, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge")
        win = [p[:, :, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)]
        a = (np.maximum.reduce(win) - np.minimum.reduce(win)) >> (depth - 8)
        ctx = (_CLASS_OF[a] + 8 * np.arange(3, dtype=np.uint8).reshape(1, 3, 1, 1)).astype(np.uint8)
        count = np.stack([np.bincount(ctx[i].reshape(-1), minlength=RES_CTX) for i in range(B)])
        with np.errstate(over="ignore"):
            w = np.arange(1, 3 * H * W + 1, dtype=np.uint64) * np.uint64(_DIGEST_K)
            digest = ((b.reshape(B, -1) + 1).astype(np.uint64) * w).sum(1, dtype=np.uint64)
        out = {"ctx": torch.from_numpy(ctx), "ctx_count": torch.from_numpy(count.astype(np.int64)),
               "digest": torch.from_numpy(digest.view(np.int64).copy())}
    if x is None:
        return out
    xv = _samples_np(x, x_layout, depth)
    step, maxv = 2 * tau + 1, (1 << depth) - 1
    r = xv - b
    q = np.sign(r) * ((np.abs(r) + tau) // step)
    aq = np.abs(q).reshape(B, -1)
    out.update(max_abs_q=torch.from_numpy(aq.max(1)), sum_abs_q=torch.from_numpy(aq.sum(1)))
    if stats:
        return out
    rec = np.clip(b + q * step, 0, maxv)
    hi = q >> shift
    lo = q - (hi << shift)
    bins = np.where(np.abs(hi) <= RES_MAX_M, hi + RES_MAX_M, RES_BINS - 1)
    key = ctx.astype(np.int64) * RES_BINS + bins
    hist = np.stack([np.bincount(key[i].reshape(-1), minlength=RES_CTX * RES_BINS) for i in range(B)])
    out.update(sym=torch.from_numpy(np.clip(hi, -32768, 32767).astype(np.int16)),
               plane=torch.from_numpy(_pack_plane_np(lo, shift).view(np.int64).copy()),
               hist=torch.from_numpy(hist.reshape(B, RES_CTX, RES_BINS).astype(np.int64)),
               max_err=torch.from_numpy(np.abs(xv - rec).reshape(B, -1).max(1).astype(np.int64)))
    return out


def _u16_in_place(t: torch.Tensor, layout: str) -> torch.Tensor:
    return _dense_u16(t, (2, 3) if layout == "hwc" else (3, 1))


def residual_front16(base, x=None, depth: int = 16, tau: int = 0, shift: int = 0, layout: Optional[str] = None,
                     x_layout: Optional[str] = None) -> Dict:
    """residual_front for samples of `depth` bits (9..16) in uint16 words, LSB-aligned (csrc/residual16.hip, one
    launch; DESIGN.md §5 "Residual coding", "Deep samples").  base: uint16 [B,H,W,3] / [B,3,H,W] (or one image), any
    strides; x: the original, the same size, in x_layout.  Returns {"ctx" uint8 [B,3,H,W], "ctx_count" int64 [B,24],
    "digest" int64 [B]} and, with x, {"sym" int16 [B,3,H,W] (hi = q >> shift, saturated to int16), "plane" int64
    [B, 3 H ceil(W/64) shift] (the low-bit plane's 64-bit words), "hist" int64 [B,24,128] (of hi), "max_err" int64
    [B], "max_abs_q" int64 [B], "sum_abs_q" int64 [B]}.  sym fits the 8-bit layer's tables and coders when
    residual_shift_fits(max_abs_q, shift).  CPU tensors take the NumPy restatement (the same bits)."""
    what = "residual_front16"
    depth, tau = _check_depth(depth, what, RES16_MIN_DEPTH), _check_tau(tau, what)
    shift = _check_shift(shift, depth, what)
    base, layout, x, x_layout = _residual16_images(base, x, layout, x_layout, what)
    if not base.is_cuda:
        return _residual_front16_cpu(base, x, depth, tau, shift, layout, x_layout)
    B = base.size(0)
    H, W = _hw(base, layout)
    base = _u16_in_place(base, layout)
    dev = base.device
    with torch.cuda.device(dev):
        if x is not None:
            x = _u16_in_place(x, x_layout)
        o = _front_buffers(dev, (B, 3, H, W), x is not None, residual_plane_words(H, W, shift))
        _lib.call("mlic_image_residual_front_u16", _stream(), _ptr(base), (C.c_int64 * 4)(*_strides(base, layout)),
                  _ptr(x), None if x is None else (C.c_int64 * 4)(*_strides(x, x_layout)), B, H, W, depth, tau, shift,
                  _ptr(o["ctx"]), _ptr(o["count"]), _ptr(o["digest"]), _ptr(o["sym"]), _ptr(o["plane"]), _ptr(o["hist"]),
                  _ptr(o["merr"]), _ptr(o["mq"]), _ptr(o["sq"]))
        return _front_result(o)


def residual_stats16(base, x, depth: int, tau: int = 0, layout: Optional[str] = None,
                     x_layout: Optional[str] = None) -> Dict:
    """{"max_abs_q" int64 [B], "sum_abs_q" int64 [B]} of the quantised residual of x against base: what the shift is
    chosen from (residual_shift), by a statistics launch of the front kernel (mlic_image_residual_stats_u16)."""
    what = "residual_stats16"
    depth, tau = _check_depth(depth, what, RES16_MIN_DEPTH), _check_tau(tau, what)
    if x is None:
        raise ValueError(f"{what}: x is needed")
    base, layout, x, x_layout = _residual16_images(base, x, layout, x_layout, what)
    if not base.is_cuda:
        return _residual_front16_cpu(base, x, depth, tau, 0, layout, x_layout, stats=True)
    B = base.size(0)
    H, W = _hw(base, layout)
    base, x = _u16_in_place(base, layout), _u16_in_place(x, x_layout)
    dev = base.device
    with torch.cuda.device(dev):
        mq = torch.full((B,), -1, dtype=torch.int32, device=dev)
        sq = torch.full((B,), -1, dtype=torch.int64, device=dev)
        _lib.call("mlic_image_residual_stats_u16", _stream(), C.c_void_p(base.data_ptr()),
                  (C.c_int64 * 4)(*_strides(base, layout)), C.c_void_p(x.data_ptr()),
                  (C.c_int64 * 4)(*_strides(x, x_layout)), B, H, W, depth, tau, C.c_void_p(mq.data_ptr()),
                  C.c_void_p(sq.data_ptr()))
    return {"max_abs_q": mq.to(torch.int64), "sum_abs_q": sq}


def _residual_apply16_cpu(base, sym, plane, depth, tau, shift, layout, ref, out):
    b = _samples_np(base, layout, depth)
    B, _, H, W = b.shape
    hi = np.asarray(sym.cpu()).astype(np.int64).reshape(b.shape)
    bad = np.flatnonzero((np.abs(hi) > RES16_MAX_HI).reshape(B, -1).any(1))
    if bad.size:
        raise ValueError(f"residual_apply16: image {int(bad[0])} holds a symbol outside [-255, 255]")
    lo = _unpack_plane_np(np.ascontiguousarray(plane.cpu().numpy()).view(np.uint64).reshape(B, -1), H, W, shift)
    rec = np.clip(b + ((hi << shift) + lo) * (2 * tau + 1), 0, (1 << depth) - 1)
    img = torch.from_numpy(rec.astype(np.uint16))
    img = img.permute(0, 2, 3, 1).contiguous() if layout == "hwc" else img
    if out is not None:
        out.copy_(img)
        img = out
    if ref is None:
        return img
    d = rec - _samples_np(ref, layout, depth)
    return img, torch.from_numpy((d * d).reshape(B, -1).sum(1)), torch.from_numpy(np.abs(d).reshape(B, -1).max(1))


def residual_apply16(base, sym, plane, depth: int, tau: int, shift: int, layout: Optional[str] = None, ref=None,
                     out: Optional[torch.Tensor] = None):
    """The deep decoder's last pass (csrc/residual16.hip, one launch): out = clamp(base + ((sym << shift) + lo)
    (2 tau + 1), 0, 2^depth - 1) as uint16 words in base's layout, lo read from `plane` (int64 [B, 3 H ceil(W/64)
    shift], residual_front16's).  sym: int16 [B,3,H,W], dense, on base's device; a sym outside [-255, 255] is
    refused (ValueError naming the image).  out: an optional uint16 tensor of base's shape with any strides.  ref
    (uint16, base's shape): returns (out, sq_err int64 [B], max_abs_err int64 [B]), exact.  CPU tensors take the
    NumPy restatement."""
    what = "residual_apply16"
    depth, tau = _check_depth(depth, what, RES16_MIN_DEPTH), _check_tau(tau, what)
    shift = _check_shift(shift, depth, what)
    base, layout = _u16_batch(base, layout, f"{what} base")
    B = base.size(0)
    H, W = _hw(base, layout)
    if not torch.is_tensor(sym) or sym.dtype != torch.int16 or tuple(sym.shape) != (B, 3, H, W):
        raise ValueError(f"{what}: sym must be an int16 tensor {(B, 3, H, W)}")
    words = residual_plane_words(H, W, shift)
    if not torch.is_tensor(plane) or plane.dtype != torch.int64 or tuple(plane.shape) != (B, words):
        raise ValueError(f"{what}: plane must be an int64 tensor {(B, words)}")
    if sym.device != base.device or plane.device != base.device:
        raise ValueError(f"{what}: base, sym and plane must be on one device")
    if out is not None and (out.dtype != torch.uint16 or tuple(out.shape) != tuple(base.shape) or out.device != base.device):
        raise ValueError(f"{what}: out must be uint16 {tuple(base.shape)} on {base.device}")
    if ref is not None:
        ref, _ = _u16_batch(ref, layout, f"{what} ref")
        if tuple(ref.shape) != tuple(base.shape):
            raise ValueError(f"{what}: ref must have shape {tuple(base.shape)}, got {tuple(ref.shape)}")
        ref = ref.to(base.device)
    if not base.is_cuda:
        return _residual_apply16_cpu(base, sym, plane, depth, tau, shift, layout, ref, out)
    base = _u16_in_place(base, layout)
    sym, plane = sym.contiguous(), plane.contiguous()
    dev = base.device
    with torch.cuda.device(dev):
        if out is None:
            out = _apply_out(base.shape, True, dev)
        elif 0 in _strides(out, layout)[2:]:
            raise ValueError(f"{what}: out has a zero column or channel stride")
        if ref is not None:
            ref = _u16_in_place(ref, layout)
        sq, merr, status = _apply_buffers(dev, B, ref, (B,))
        _lib.call("mlic_image_residual_apply_u16", _stream(), _ptr(base), (C.c_int64 * 4)(*_strides(base, layout)),
                  _ptr(sym), _ptr(plane), B, H, W, depth, tau, shift, _ptr(out), (C.c_int64 * 4)(*_strides(out, layout)),
                  _ptr(ref), None if ref is None else (C.c_int64 * 4)(*_strides(ref, layout)), _ptr(sq), _ptr(merr),
                  _ptr(status))
        _apply_refusal(what, "image", status, () if ref is None else (ref,))
    return out if ref is None else (out, sq, merr.to(torch.int64))


def write_container_residual_deep(H: int, W: int, inner: bytes, segs: bytes, seg_bytes, segment: int, tau: int,
                                  depth: int, shift: int, low: bytes, digest: int, m, freq, vbr: bool = False) -> bytes:
    """The deep residual file (mlic_container_write_residual_deep): "MLR3", the header and the tables of the "MLR2"
    file, depth and shift, seg_len, n_seg, `inner`, the index and `segs`, and behind lo_len the low-bit plane `low`
    (8 * 3 H ceil(W / 64) shift bytes, little-endian 64-bit words)."""
    inner, segs, low = bytes(inner), bytes(segs), bytes(low)
    return _write_residual("_deep", H, W, vbr, tau, (depth, shift), digest, m, freq, (segment, seg_bytes),
                           (inner, segs, low))


def parse_container_residual_deep(data: bytes, n_levels: Optional[int] = None,
                                  max_pixels: int = MAX_PIXELS) -> _lib.ContainerResidualDeepInfo:
    """The validating parser of a deep residual file (mlic_container_parse_residual_deep): raises _lib.MlicError on any
    malformed input.  The fields of the "MLR2" parse, and depth, shift, lo_off / lo_len (the low-bit plane)."""
    return _parse_residual("mlic_container_parse_residual_deep", _lib.ContainerResidualDeepInfo(), data, n_levels,
                           max_pixels)


@torch.no_grad()
def encode_residual16(net, imgs_u16, depth: int, max_error: int = 0, level=None, layout: Optional[str] = None,
                      residual_segment: int = DEFAULT_RESIDUAL_SEGMENT, residual_coder: str = "device",
                      shift: Optional[int] = None, return_info: bool = False):
    """Lossless (max_error=0) and near-lossless coding of uint16 images of `depth` bits (9..16, LSB-aligned; DESIGN.md
    §5 "Residual coding", "Deep samples") -> one "MLR3" file per image.  The images are ingested and compressed
    exactly as encode_images(depth=) does (the inner file is that file, byte for byte); the base image is the decode
    of that file alone through egress_u16.  residual_stats16 gives max|q| and sum|q| per image, the shift rule
    (residual_shift) or `shift` the split, residual_front16 the high parts with their contexts and histograms and the
    low-bit plane; the bound is checked on the device, the high parts go through residual_tables and
    residual_encode_segments (residual_coder as in encode_images), the low bits are stored raw.  An explicit shift=
    that does not fit an image is refused, naming the smallest that fits.  return_info=True: (files, info), info[b] =
    encode_images' fields and "max_error", "depth", "shift", "base_bytes", "residual_bytes", "low_bytes",
    "residual_segment", "segments"."""
    what = "encode_residual16"
    depth, tau = _check_depth(depth, what, RES16_MIN_DEPTH), _check_tau(max_error, what)
    L, coder = _check_segment(residual_segment, what), _check_coder(residual_coder, what)
    if shift is not None:
        shift = _check_shift(shift, depth, what)
    img, layout = _u16_batch(imgs_u16, layout, what)
    inner, info = encode_images(net, img, level=level, layout=layout, depth=depth, return_info=True)
    B = img.size(0)
    H, W = _hw(img, layout)
    x_hat, vbr = _inner_x_hat(net, inner)
    base = egress_u16(x_hat.float(), H, W, depth, "hwc")
    img = img.to(base.device)
    kind = _rgb_kind(depth, layout)
    shifts = _residual_shifts(what, "shift", kind, depth, 3 * H * W, kind.stats(base, img, tau), shift, B)
    files, extra = _encode_residual_layer(kind, what, base, img, H, W, tau, shifts, L, coder, inner, vbr)
    for d, f, e in zip(info, files, extra):
        d.update(e, bytes=len(f), bpp=8.0 * len(f) / (H * W))
    return (files, info) if return_info else files


def _decode_residual16(net, files, ref, max_pixels, enhance, coder, depth):
    """decode_images for "MLR3" files: the inner files decoded at the file's depth, then the deep residual layer."""
    def check(b, s):
        if depth is not None and depth != s.depth:
            raise ValueError(f"decode_images: depth={depth}, but file {b} (MLR3) holds samples of depth {s.depth}")

    ss = _parse_residual_files("decode_images", net, files, max_pixels, check)
    B = len(files)
    if ref is not None:
        ref, _ = _u16_batch(ref, "hwc", "decode_images ref")
    depths = sorted({int(s.depth) for s in ss})
    if len(depths) > 1:  # one depth at a time, pasted into one canvas
        parts = {}
        for d in depths:
            idx = [b for b in range(B) if ss[b].depth == d]
            r = None if ref is None else torch.stack([ref.cpu().view(torch.int16)[b] for b in idx]).view(torch.uint16)
            parts[d] = (idx, _decode_residual16(net, [files[b] for b in idx], r, max_pixels, enhance, coder, None))
        dev = next(iter(parts.values()))[1][0].device
        Hm, Wm = max(s.H for s in ss), max(s.W for s in ss)
        img = torch.zeros(B, Hm, Wm, 3, dtype=torch.int16, device=dev)
        info = [None] * B
        for idx, (im, inf) in parts.values():
            for j, b in enumerate(idx):
                h, w = min(im.size(1), Hm), min(im.size(2), Wm)
                img[b, :h, :w].copy_(im[j, :h, :w].view(torch.int16))
                info[b] = inf[j]
        return img.view(torch.uint16), info
    return _decode_residual_layer(_rgb_kind(depths[0]), net, files, ss, ref, max_pixels, enhance, coder)


# ---------------------------------------------------------------------------------------------- ROI
def _mask_batch(mask, what: str) -> torch.Tensor:
    """-> 3-dim uint8 tensor [B,H,W] (a bool mask is viewed as bytes; one mask gains the batch dimension)."""
    if isinstance(mask, np.ndarray):
        mask = torch.from_numpy(np.ascontiguousarray(mask))
    if not torch.is_tensor(mask) or mask.dtype not in (torch.uint8, torch.bool) or mask.dim() not in (2, 3):
        raise ValueError(f"{what}: a uint8 or bool mask [B,H,W] (or one [H,W]) expected")
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    if mask.dim() == 2:
        mask = mask.unsqueeze(0)
    if 0 in mask.shape:
        raise ValueError(f"{what}: empty mask {tuple(mask.shape)}")
    return mask


def _check_roi_levels(lo, hi, what: str):
    ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (lo, hi))
    if not ok or not 0 <= lo <= hi <= 255:
        raise ValueError(f"{what}: integer levels 0 <= lo <= hi expected, got ({lo!r}, {hi!r})")


def roi_levels(mask, lo: int, hi: int) -> torch.Tensor:
    """mask (uint8 / bool [B,H,W] or [H,W], nonzero = inside the ROI, any strides: read in place) -> the level map
    uint8 [B,hz,wz] on the z grid (hz = ceil(H / 64), wz = ceil(W / 64)), one cell per 64 x 64 pixel block
    clipped to the image: level = lo + ceil((hi - lo) * count / area) in integers, count the cell's nonzero mask
    pixels and area its pixels inside the image.  One launch on the mask's device (CPU: the same rule in torch)."""
    mask = _mask_batch(mask, "roi_levels")
    _check_roi_levels(lo, hi, "roi_levels")
    B, H, W = mask.shape
    hz, wz = (H + 63) // 64, (W + 63) // 64
    if not mask.is_cuda:
        m = torch.zeros(B, 64 * hz, 64 * wz, dtype=torch.int64)
        m[:, :H, :W] = (mask != 0)
        cnt = m.reshape(B, hz, 64, wz, 64).sum((2, 4))
        ys = torch.clamp(H - 64 * torch.arange(hz), max=64)
        xs = torch.clamp(W - 64 * torch.arange(wz), max=64)
        area = ys[:, None] * xs[None, :]
        return (lo + ((hi - lo) * cnt + area - 1) // area).to(torch.uint8)
    with torch.cuda.device(mask.device):
        out = torch.full((B, hz, wz), 255, dtype=torch.uint8, device=mask.device)
        _lib.call("mlic_image_roi_levels_u8", _stream(), C.c_void_p(mask.data_ptr()), (C.c_int64 * 3)(*mask.stride()),
                  B, H, W, int(lo), int(hi), C.c_void_p(out.data_ptr()))
    return out


_roi_level_map = roi_levels  # encode_images has a parameter of that name


def gain_plane(net, levels) -> torch.Tensor:
    """Level map (integer [B,hz,wz] or [hz,wz], each level below net.levels) -> the gain plane fp32
    [B,1,4 hz,4 wz] on the model's device that `gain_map=` takes: latent pixel (i, j) gets
    |net.Gain|[levels[b][i >> 2][j >> 2]] (the coder paths' gain).  Encoder and decoder both come through here."""
    if not hasattr(net, "levels"):
        raise ValueError("gain_plane: a *_VBR model expected (ROI coding needs the Gain table)")
    if isinstance(levels, np.ndarray):
        levels = torch.from_numpy(np.ascontiguousarray(levels))
    if not torch.is_tensor(levels) or levels.is_floating_point() or levels.dim() not in (2, 3) or 0 in levels.shape:
        raise ValueError("gain_plane: an integer level map [B,hz,wz] (or one [hz,wz]) expected")
    if levels.dim() == 2:
        levels = levels.unsqueeze(0)
    n = int(net.levels)
    if n > 16:
        raise ValueError(f"gain_plane: at most 16 levels fit the file's map, the model has {n}")
    if int(levels.min()) < 0 or int(levels.max()) >= n:
        raise ValueError(f"gain_plane: levels in [0, {n}) expected")
    gains = net.Gain.detach().float().abs().cpu().reshape(-1)[:n].contiguous()
    B, hz, wz = levels.shape
    dev = net.device
    levels = levels.to(torch.uint8).to(dev).contiguous()
    if dev.type != "cuda":
        return gains[levels.long()].repeat_interleave(4, 1).repeat_interleave(4, 2).unsqueeze(1).contiguous()
    with torch.cuda.device(dev):
        g = torch.empty(B, 1, 4 * hz, 4 * wz, dtype=torch.float32, device=dev)
        if _lib.poison():
            g.fill_(float("nan"))
        _lib.call("mlic_roi_gain_plane", _stream(), C.c_void_p(levels.data_ptr()), B, hz, wz,
                  (C.c_float * n)(*gains.tolist()), n, C.c_void_p(g.data_ptr()))
        levels.record_stream(torch.cuda.current_stream())
    return g


def sq_err_roi(a, b, mask, layout: Optional[str] = None) -> torch.Tensor:
    """Two uint8 image batches (any strides, read in place) and a mask [B,H,W] -> int64 [B,4] on their device:
    {squared error inside the ROI, pixels inside, squared error outside, pixels outside}; the squared error is
    summed over the three channels, in integers (exact).  Inside + outside is egress_u8's sq_err."""
    a, layout = _u8_batch(a, layout, "sq_err_roi")
    b, _ = _u8_batch(b, layout, "sq_err_roi")
    mask = _mask_batch(mask, "sq_err_roi")
    B = a.size(0)
    H, W = _hw(a, layout)
    if tuple(b.shape) != tuple(a.shape) or tuple(mask.shape) != (B, H, W):
        raise ValueError(f"sq_err_roi: images of one shape and a mask {(B, H, W)} expected, got {tuple(a.shape)}, "
                         f"{tuple(b.shape)}, {tuple(mask.shape)}")
    b, mask = b.to(a.device), mask.to(a.device)
    if not a.is_cuda:
        d = _nchw(a, layout).to(torch.int64) - _nchw(b, layout).to(torch.int64)
        sq = (d * d).sum(1)
        inside = mask != 0
        return torch.stack([(sq * inside).flatten(1).sum(1), inside.flatten(1).sum(1),
                            (sq * ~inside).flatten(1).sum(1), (~inside).flatten(1).sum(1)], 1)
    with torch.cuda.device(a.device):
        out = torch.full((B, 4), -1, dtype=torch.int64, device=a.device)
        _lib.call("mlic_image_sq_err_roi_u8", _stream(), C.c_void_p(a.data_ptr()), (C.c_int64 * 4)(*_strides(a, layout)),
                  C.c_void_p(b.data_ptr()), (C.c_int64 * 4)(*_strides(b, layout)), C.c_void_p(mask.data_ptr()),
                  (C.c_int64 * 3)(*mask.stride()), B, H, W, C.c_void_p(out.data_ptr()))
        for t in (b, mask):
            t.record_stream(torch.cuda.current_stream())
    return out


def psnr_roi(a, b, mask, layout: Optional[str] = None) -> List[Dict]:
    """Per image {"psnr_roi", "psnr_bg", "sq_err_roi", "n_roi", "sq_err_bg", "n_bg"}: PSNR (max 255) inside and
    outside the mask from sq_err_roi's exact sums; None for a side that holds no pixel."""
    out = []
    for si, ni, so, no in sq_err_roi(a, b, mask, layout).cpu().tolist():
        out.append({"psnr_roi": psnr_from_sq_err(si, 3 * ni) if ni else None,
                    "psnr_bg": psnr_from_sq_err(so, 3 * no) if no else None,
                    "sq_err_roi": si, "n_roi": ni, "sq_err_bg": so, "n_bg": no})
    return out


def _roi_map(net, roi, roi_levels, shape, what: str):
    """roi= / roi_levels= of a *_VBR model, checked -> (the level map on the model's device, hi)."""
    if not hasattr(net, "levels"):
        raise ValueError("roi= given for a fixed-rate model: ROI coding needs a *_VBR model")
    try:
        lo, hi = roi_levels
    except (TypeError, ValueError):
        raise ValueError(f"roi_levels: a pair (lo, hi) expected, got {roi_levels!r}") from None
    _check_roi_levels(lo, hi, "roi_levels")
    if hi >= min(int(net.levels), 16):
        raise ValueError(f"roi_levels: levels in [0, {min(int(net.levels), 16)}) expected, got ({lo}, {hi})")
    mask = _mask_batch(roi, f"{what} roi")
    if tuple(mask.shape) != tuple(shape):
        raise ValueError(f"{what}: roi must be a mask of shape {tuple(shape)}, got {tuple(mask.shape)}")
    return _roi_level_map(mask.to(net.device), int(lo), int(hi)), hi


# ---------------------------------------------------------------------------------------- rate maps
CMAPS = ("gray", "hot")  # heat_u8's colour maps; the library's cmap argument is the index
MAP_BLOCKS = (8, 16, 32, 64)  # sq_err_blocks' block sizes and heat_u8's cell sizes


def _lik_batch(t, what: str) -> torch.Tensor:
    """A likelihood tensor the kernel can read in place: fp32 [B,C,h,w], every image dense (any batch stride)."""
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 4 or 0 in t.shape:
        raise ValueError(f"rate_maps: {what}: a float32 tensor [B,C,h,w] expected")
    return t if t[0].is_contiguous() and t.stride(0) >= t[0].numel() else t.contiguous()


def _cell_bits_cpu(y_map: torch.Tensor, z_map: torch.Tensor) -> torch.Tensor:
    """cell_bits [B,h,w] from y_map [B,S,h,w] and z_map [B,h/4,w/4], the kernel's sequence in CPU doubles:
    ((z / 16 + y[0]) + y[1]) + ... + y[S-1], a z pixel standing for its 4 x 4 latent pixels."""
    y, z = y_map.detach().cpu().double(), z_map.detach().cpu().double()
    v = z.repeat_interleave(4, 1).repeat_interleave(4, 2) / 16.0
    for s in range(y.size(1)):
        v = v + y[:, s]
    return v


def _plane_sum_cpu(p: torch.Tensor) -> torch.Tensor:
    """[..., ph, pw] doubles -> [...]: the kernel's order.  Per row, lane l of 64 adds the elements l, l + 64, ... from
    +0.0, the 64 lane sums are folded in halves (l += l + 32, then 16, 8, 4, 2, 1), and the row sums are added top
    to bottom from +0.0."""
    p = p.detach().cpu().double()
    lead, (ph, pw) = p.shape[:-2], p.shape[-2:]
    n = (pw + 63) // 64
    q = torch.zeros(*lead, ph, n * 64, dtype=torch.float64)  # a lane past the row's end adds nothing: + 0.0 is exact
    q[..., :pw] = p
    q = q.reshape(*lead, ph, n, 64)
    v = torch.zeros(*lead, ph, 64, dtype=torch.float64)
    for k in range(n):
        v = v + q[..., k, :]
    for off in (32, 16, 8, 4, 2, 1):
        v = v[..., :off] + v[..., off:2 * off]
    total = torch.zeros(lead, dtype=torch.float64)
    for r in range(ph):
        total = total + v[..., r, 0]
    return total


def _slice_bits_cpu(y_map: torch.Tensor, z_map: torch.Tensor) -> torch.Tensor:
    """slice_bits [B,S+1] from the two maps: _plane_sum_cpu of each y_map[s], then of z_map."""
    return torch.cat([_plane_sum_cpu(y_map), _plane_sum_cpu(z_map).unsqueeze(1)], 1)


def rate_maps(y_lik: torch.Tensor, z_lik: torch.Tensor, slices: int) -> Dict[str, torch.Tensor]:
    """Where the entropy model's bits lie (DESIGN.md §5 "Rate maps").  y_lik fp32 [B,M,h,w] and z_lik fp32
    [B,N,h/4,w/4] -- forward()'s likelihood tensors, or batch-strided views of them, read in place -> float64
    tensors on their device:
        "y_map" [B,S,h,w]    per latent pixel and slice (M / S channels each), the sum in ascending channel order of
                             -(double)log2f(lik), the term mlic_encoded_bits / likelihood_bits sum
        "z_map" [B,h/4,w/4]  the same over z's N channels
        "cell_bits" [B,h,w]  z_map / 16 (a z pixel covers 4 x 4 latent pixels) + y_map[0] + ... + y_map[S-1]
        "slice_bits" [B,S+1] the totals of y_map[0 .. S-1] and of z_map (_plane_sum_cpu's order)
    A latent pixel is 16 x 16 image pixels.  Two launches (csrc/ratemap.hip); bit-identical across batch size,
    batch position and strides.  CPU tensors run the same sums on torch's fp32 log2 (the device's log2f may differ
    from it in the last bit of a term)."""
    y_lik, z_lik = _lik_batch(y_lik, "y_lik"), _lik_batch(z_lik, "z_lik")
    B, M, h, w = y_lik.shape
    S = int(slices)
    if S < 1 or M % S:
        raise ValueError(f"rate_maps: {M} channels do not split into {slices} slices")
    if h % 4 or w % 4 or tuple(z_lik.shape[::3]) != (B, w // 4) or z_lik.size(2) != h // 4 or z_lik.device != y_lik.device:
        raise ValueError(f"rate_maps: z_lik [B,N,h/4,w/4] on y_lik's device expected for y_lik {tuple(y_lik.shape)}, got "
                         f"{tuple(z_lik.shape)} on {z_lik.device}")
    N = z_lik.size(1)
    if not y_lik.is_cuda:
        ty, tz = -torch.log2(y_lik), -torch.log2(z_lik)
        y_map = torch.zeros(B, S, h, w, dtype=torch.float64)
        z_map = torch.zeros(B, h // 4, w // 4, dtype=torch.float64)
        for c in range(M // S):
            y_map = y_map + ty[:, c::M // S].double()
        for c in range(N):
            z_map = z_map + tz[:, c].double()
        return {"y_map": y_map, "z_map": z_map, "cell_bits": _cell_bits_cpu(y_map, z_map),
                "slice_bits": _slice_bits_cpu(y_map, z_map)}
    dev = y_lik.device
    with torch.cuda.device(dev):
        out = {"y_map": (B, S, h, w), "z_map": (B, h // 4, w // 4), "cell_bits": (B, h, w), "slice_bits": (B, S + 1)}
        out = {k: torch.empty(v, dtype=torch.float64, device=dev) for k, v in out.items()}
        if _lib.poison():
            for t in out.values():
                t.fill_(float("nan"))
        y_bs, z_bs = ((t.stride(0) if B > 1 else t[0].numel()) for t in (y_lik, z_lik))  # one image: no stride
        _lib.call("mlic_rate_map_run", _stream(), C.c_void_p(y_lik.data_ptr()), y_bs,
                  C.c_void_p(z_lik.data_ptr()), z_bs, B, M, S, h, w, N, C.c_void_p(out["y_map"].data_ptr()),
                  C.c_void_p(out["z_map"].data_ptr()), C.c_void_p(out["cell_bits"].data_ptr()),
                  C.c_void_p(out["slice_bits"].data_ptr()))
    return out


def _check_block(block, what: str) -> int:
    if isinstance(block, bool) or not isinstance(block, (int, np.integer)) or int(block) not in MAP_BLOCKS:
        raise ValueError(f"{what} must be one of {MAP_BLOCKS}, got {block!r}")
    return int(block)


def _sq_err_blocks_cpu(a: torch.Tensor, b: torch.Tensor, block: int, layout: str) -> torch.Tensor:
    """sq_err_blocks in torch integers: 4-dim uint8 batches of one shape -> int64 [B,ceil(H/block),ceil(W/block)]."""
    d = _nchw(a, layout).to(torch.int64) - _nchw(b, layout).to(torch.int64)
    sq = (d * d).sum(1)
    B, H, W = sq.shape
    nby, nbx = -(-H // block), -(-W // block)
    full = torch.zeros(B, nby * block, nbx * block, dtype=torch.int64, device=sq.device)
    full[:, :H, :W] = sq
    return full.reshape(B, nby, block, nbx, block).sum((2, 4))


def sq_err_blocks(a, b, block: int = 16, layout: Optional[str] = None) -> torch.Tensor:
    """Two uint8 image batches of one shape (any strides, read in place) -> int64 [B,ceil(H/block),ceil(W/block)] on
    their device: per block x block square (the last ones cropped to the image) the sum of squared byte differences
    over its pixels and three channels, in integers.  block: 8, 16, 32 or 64.  The grid's sum is egress_u8's sq_err
    and sq_err_roi's inside + outside.  One launch."""
    a, layout = _u8_batch(a, layout, "sq_err_blocks")
    b, _ = _u8_batch(b, layout, "sq_err_blocks")
    block = _check_block(block, "sq_err_blocks: block")
    if tuple(b.shape) != tuple(a.shape):
        raise ValueError(f"sq_err_blocks: images of one shape expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    b = b.to(a.device)
    if not a.is_cuda:
        return _sq_err_blocks_cpu(a, b, block, layout)
    a, b = _in_place(a, layout), _in_place(b, layout)
    B = a.size(0)
    H, W = _hw(a, layout)
    with torch.cuda.device(a.device):
        out = torch.full((B, -(-H // block), -(-W // block)), -1, dtype=torch.int32, device=a.device)  # < 2^30 each
        _lib.call("mlic_image_sq_err_blocks_u8", _stream(), C.c_void_p(a.data_ptr()),
                  (C.c_int64 * 4)(*_strides(a, layout)), C.c_void_p(b.data_ptr()), (C.c_int64 * 4)(*_strides(b, layout)),
                  B, H, W, block, C.c_void_p(out.data_ptr()))
        b.record_stream(torch.cuda.current_stream())
    return out.to(torch.int64)


def _check_heat(plane, H, W, cell, lo, hi, cmap, under, alpha, layout):
    """heat_u8's arguments, checked -> (plane float64 [B,ph,pw], cell, lo, hi, cmap index, under or None, alpha)."""
    if isinstance(plane, np.ndarray):
        plane = torch.from_numpy(np.ascontiguousarray(plane))
    if not torch.is_tensor(plane) or plane.dtype != torch.float64 or plane.dim() not in (2, 3) or 0 in plane.shape:
        raise ValueError("heat_u8: a float64 plane [B,ph,pw] (or one [ph,pw]) expected")
    if plane.dim() == 2:
        plane = plane.unsqueeze(0)
    cell = _check_block(cell, "heat_u8: cell")
    if layout not in ("hwc", "chw"):
        raise ValueError(f"heat_u8: layout must be 'hwc' or 'chw', got {layout!r}")
    B, ph, pw = plane.shape
    if not (1 <= H <= ph * cell and 1 <= W <= pw * cell):
        raise ValueError(f"heat_u8: a {ph} x {pw} plane of {cell}-pixel cells does not cover {H} x {W}")
    if cmap not in CMAPS:
        raise ValueError(f"heat_u8: cmap must be one of {CMAPS}, got {cmap!r}")
    lo = float(lo)
    if hi is None:  # the plane's largest finite value, or lo + 1 for a plane that has none above lo
        fin = plane[torch.isfinite(plane)]
        hi = float(fin.max()) if fin.numel() else lo
        if not hi > lo:
            hi = lo + 1.0
    hi = float(hi)
    if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo and math.isfinite(hi - lo)):
        raise ValueError(f"heat_u8: finite lo < hi expected, got ({lo!r}, {hi!r})")
    if isinstance(alpha, bool) or not isinstance(alpha, (int, np.integer)) or not 0 <= alpha <= 256:
        raise ValueError(f"heat_u8: alpha must be an integer in [0, 256], got {alpha!r}")
    if under is None:
        if alpha != 256:
            raise ValueError("heat_u8: alpha below 256 blends with an under-image: pass under=")
    else:
        under, _ = _u8_batch(under, layout, "heat_u8 under")
        shape = (B, H, W, 3) if layout == "hwc" else (B, 3, H, W)
        if tuple(under.shape) != shape:
            raise ValueError(f"heat_u8: under must have shape {shape}, got {tuple(under.shape)}")
    return plane, cell, lo, hi, CMAPS.index(cmap), under, int(alpha)


def _heat_colours(q: np.ndarray, cmap: int) -> np.ndarray:
    """q int64 [...] in [0, 255] -> int64 [..., 3], the library's integer colour maps."""
    if cmap == 0:
        return np.stack([q, q, q], -1)
    return np.stack([np.minimum(255, 3 * q), np.clip(3 * q - 255, 0, 255), np.clip(3 * q - 510, 0, 255)], -1)


def _heat_u8_cpu(plane, H: int, W: int, cell: int, lo: float, hi: float, cmap: int, under, alpha: int,
                 layout: str) -> torch.Tensor:
    """heat_u8 in NumPy (checked arguments, cmap as the index): the kernel's operations one by one."""
    p = plane.detach().cpu().numpy()
    v = p[:, np.arange(H) // cell][:, :, np.arange(W) // cell]  # [B,H,W]
    with np.errstate(all="ignore"):
        f = np.floor((v - lo) / (hi - lo) * 255.0 + 0.5)
    nan = np.isnan(v)
    q = np.where(nan, 0.0, np.clip(f, 0.0, 255.0)).astype(np.int64)
    col = _heat_colours(q, cmap)  # [B,H,W,3]
    if under is not None:
        u = _nchw(under.detach().cpu(), layout).permute(0, 2, 3, 1).numpy().astype(np.int64)
        col = (alpha * col + (256 - alpha) * u + 128) >> 8
    col = np.where(nan[..., None], np.array([255, 0, 255]), col).astype(np.uint8)
    out = torch.from_numpy(col)
    return out if layout == "hwc" else out.permute(0, 3, 1, 2).contiguous()


def heat_u8(plane, H: int, W: int, cell: int, lo: float = 0.0, hi: Optional[float] = None, cmap: str = "hot",
            under=None, alpha: int = 256, layout: str = "hwc") -> torch.Tensor:
    """A float64 plane [B,ph,pw] (or one [ph,pw]) drawn at H x W as a uint8 RGB heat map in `layout`: [B,H,W,3] or
    [B,3,H,W].  Pixel (y, x) shows cell (y // cell, x // cell); cell is 16 for cell_bits / y_map[s], 64 for z_map,
    the block for an error map (sq_err_blocks(...).double()).
        q = clamp(floor((v - lo) / (hi - lo) * 255 + 0.5), 0, 255)       (+-inf clamp; hi=None: the plane's maximum)
    cmap "gray" is (q, q, q); "hot" is (min(255, 3q), clamp(3q - 255, 0, 255), clamp(3q - 510, 0, 255)).  under: a
    uint8 image batch of the output's shape (any strides) to blend over, out = (alpha * colour + (256 - alpha) *
    under + 128) >> 8 with alpha in [0, 256]; a NaN cell is drawn (255, 0, 255) unblended.  One launch on the
    plane's device (csrc/ratemap.hip); a CPU plane runs the NumPy restatement."""
    plane, cell, lo, hi, cm, under, alpha = _check_heat(plane, H, W, cell, lo, hi, cmap, under, alpha, layout)
    if not plane.is_cuda:
        return _heat_u8_cpu(plane, H, W, cell, lo, hi, cm, under, alpha, layout)
    plane = plane.contiguous()
    B, ph, pw = plane.shape
    with torch.cuda.device(plane.device):
        out = torch.empty((B, H, W, 3) if layout == "hwc" else (B, 3, H, W), dtype=torch.uint8, device=plane.device)
        if under is not None:
            under = _in_place(under.to(plane.device), layout)
        _lib.call("mlic_image_heat_u8", _stream(), C.c_void_p(plane.data_ptr()), B, ph, pw, cell, lo, hi, cm, H, W,
                  C.c_void_p(out.data_ptr()), (C.c_int64 * 4)(*_strides(out, layout)),
                  None if under is None else C.c_void_p(under.data_ptr()),
                  None if under is None else (C.c_int64 * 4)(*_strides(under, layout)), alpha)
        if under is not None:
            under.record_stream(torch.cuda.current_stream())
    return out


_RATE_MAP_REFUSED = {"tile": "tiled coding", "overlap": "tiled coding", "scale": "scaled coding",
                     "coded_size": "scaled coding", "filter": "scaled coding", "depth": "samples deeper than 8 bits",
                     "msb": "samples deeper than 8 bits", "yuv": "Y'CbCr frames", "fmt": "Y'CbCr frames",
                     "max_bpp": "the rate loop", "max_passes": "the rate loop", "max_error": "residual coding"}


def _refuse_rate_map(what: str, names):
    """Rate maps exist for plain and ROI coding of 8-bit RGB: any other coding option is refused by its name."""
    for k in names:
        if k not in _RATE_MAP_REFUSED:
            raise TypeError(f"{what}: unexpected argument {k!r}")
        raise ValueError(f"{what}: rate maps together with {k}= ({_RATE_MAP_REFUSED[k]}) are not supported")


@torch.no_grad()
def rate_map(net, imgs_u8, level=None, layout: Optional[str] = None, roi=None, roi_levels=None, **refused) -> List[Dict]:
    """uint8 images (encode_images' forms) -> per image the rate maps of one net.rate_map over the batch (one ingest
    launch, one forward, the two map launches): {"y_map" [S,h,w], "z_map" [h/4,w/4], "cell_bits" [h,w],
    "slice_bits" [S+1]} (float64, on the model's device, on the padded image's grids: cells wholly in the padding
    included), "bits" (slice_bits added left to right, a float), "bpp" = bits / (H * W), "x_hat" (the padded fp32
    reconstruction [3,Hp,Wp]), "H", "W".  level / roi= with roi_levels= as encode_images takes them (roi not
    together with level).  tile=, scale= / coded_size=, depth=, yuv= and max_bpp= are refused by name."""
    _refuse_rate_map("rate_map", refused)
    img, layout = _u8_batch(imgs_u8, layout, "rate_map")
    B = img.size(0)
    H, W = _hw(img, layout)
    if (roi is None) != (roi_levels is None):
        raise ValueError("roi= and roi_levels=(lo, hi) go together")
    if roi is not None:
        if level is not None:
            raise ValueError("roi= together with level=: the levels of an ROI encode are roi_levels=(lo, hi)")
        lmap, _ = _roi_map(net, roi, roi_levels, (B, H, W), "rate_map")
        kw = {"gain_map": gain_plane(net, lmap)}
    else:
        _, kw = _levels(net, level, B)
    m = net.rate_map(ingest_u8(img.to(net.device), layout), **kw)
    out = []
    for b, sb in enumerate(m["slice_bits"].cpu().tolist()):
        bits = 0.0
        for v in sb:
            bits = bits + v
        out.append({"y_map": m["y_map"][b], "z_map": m["z_map"][b], "cell_bits": m["cell_bits"][b],
                    "slice_bits": m["slice_bits"][b], "bits": bits, "bpp": bits / (H * W), "x_hat": m["x_hat"][b],
                    "H": H, "W": W})
    return out


# -------------------------------------------------------------------------------------------- codec
def _levels(net, level, B: int):
    """-> (per-image level list or None, kwargs of net.compress / net.decompress)."""
    vbr = hasattr(net, "levels")
    if level is None:
        if vbr:
            raise ValueError("a variable-rate model needs level= (it is written into the file's header)")
        return None, {}
    if not vbr:
        raise ValueError("level= given for a fixed-rate model")
    lv = [int(v) for v in (level if isinstance(level, (list, tuple)) else np.asarray(level).reshape(-1).tolist())]
    if len(lv) == 1:
        lv = lv * B
    if len(lv) != B or any(not 0 <= v < net.levels for v in lv):
        raise ValueError(f"level: one value or {B}, each in [0, {net.levels})")
    return lv, {"s": lv}


def _check_budget(max_bpp, max_passes):
    if max_bpp is not None:
        if isinstance(max_bpp, bool) or not isinstance(max_bpp, (int, float, np.integer, np.floating)) \
                or not math.isfinite(max_bpp) or not max_bpp > 0:
            raise ValueError(f"max_bpp must be a positive finite number, got {max_bpp!r}")
    if isinstance(max_passes, bool) or not isinstance(max_passes, (int, np.integer)) or max_passes < 0:
        raise ValueError(f"max_passes must be a non-negative integer, got {max_passes!r}")


@torch.no_grad()
def rate_loop(net, x: torch.Tensor, H: int, W: int, level, max_bpp: float, max_passes: int = 8,
              pixels: Optional[int] = None, overhead: int = 0):
    """The reference's rate constraint (utils/testing.py:363-390, VBR :467-527) on the padded float images x
    [B,3,Hp,Wp] of H x W images: code the batch; the images whose whole file is above max_bpp bits per pixel
    (8 * len(file) / (H * W), header included) and that had fewer than max_passes filter passes are filtered and
    compacted by one blur3_pad launch and coded again as a smaller batch, until none is left.  The float image is
    what is filtered again; it is never re-quantised.  Per image the result is the file of the first pass count
    k <= max_passes that fits, else the file after max_passes passes (the reference loops forever there).
    level: None (fixed rate), one level or one per image, or "auto" (VBR): per image the highest level whose
    unfiltered file fits, found by scanning down from net.levels - 1 with the images that fit leaving the batch
    (no monotonicity assumed: the first fit from the top is the definition); an image over the budget at level
    0 goes on into the filter loop at level 0.  -> (files, passes, levels) in input order; levels is None for
    a fixed-rate model.
    pixels / overhead (scaled coding): the budget counts 8 * (len(file) + overhead) bits over `pixels` pixels --
    the display size and the scaled header -- while H x W, the coded size, is what is coded and filtered."""
    _check_budget(max_bpp, max_passes)
    if max_bpp is None:
        raise ValueError("rate_loop: max_bpp expected")
    pixels = H * W if pixels is None else int(pixels)
    B = x.size(0)
    auto = isinstance(level, str)
    if auto:
        if level != "auto":
            raise ValueError(f"level: an integer, one per image or 'auto' expected, got {level!r}")
        if not hasattr(net, "levels"):
            raise ValueError("level='auto' given for a fixed-rate model")
        lv = [net.levels - 1] * B
    else:
        lv, _ = _levels(net, level, B)
    files: List[Optional[bytes]] = [None] * B
    passes = [0] * B

    def code(cur, ids):
        kw = {} if lv is None else {"s": [lv[b] for b in ids]}
        out = net.compress(cur, **kw)
        ys, zs = out["strings"]
        for j, b in enumerate(ids):
            files[b] = write_container(H, W, out["shape"], ys[j], zs[j], None if lv is None else lv[b])

    def over(b):
        return 8.0 * (len(files[b]) + overhead) / pixels > max_bpp

    def keep(cur, ids, sub):
        """The images `sub` of the batch `cur` (which holds `ids`), compacted."""
        if len(sub) == len(ids):
            return cur
        return cur.index_select(0, torch.tensor([ids.index(b) for b in sub], dtype=torch.int64, device=cur.device))

    cur, ids = x, list(range(B))
    code(cur, ids)
    if auto:
        for l in range(net.levels - 2, -1, -1):
            sub = [b for b in ids if over(b)]
            if not sub:
                break
            cur, ids = keep(cur, ids, sub), sub
            for b in ids:
                lv[b] = l
            code(cur, ids)
    while True:
        sub = [b for b in ids if over(b) and passes[b] < max_passes]
        if not sub:
            break
        cur, ids = blur3_pad(cur, H, W, index=None if len(sub) == len(ids) else [ids.index(b) for b in sub]), sub
        for b in ids:
            passes[b] += 1
        code(cur, ids)
    return files, passes, lv


@torch.no_grad()
def encode_images(net, imgs_u8, level=None, layout: Optional[str] = None, max_bpp: Optional[float] = None,
                  max_passes: int = 8, return_info: bool = False, roi=None, roi_levels=None, depth: Optional[int] = None,
                  msb: bool = False, coded_size=None, scale=None, filter: str = "lanczos3", layered: bool = False,
                  max_error: Optional[int] = None, residual_segment: Optional[int] = None,
                  residual_coder: str = "device"):
    """uint8 images ([B,H,W,3] / [B,3,H,W] tensor or numpy array, or one image; layout=None tells them apart by
    the dimension of size 3) -> one file per image.  A host array crosses to the device as uint8; then one
    ingest launch, one net.compress over the batch, B containers.  level: the VBR level (one for the batch or
    one per image), required for *_VBR models.
    max_bpp: a budget in bits per pixel of the whole file; the images above it go through rate_loop (filter and
    code again, at most max_passes times each), and level="auto" (VBR, needs max_bpp) picks per image the highest
    level whose unfiltered file fits.  An image gets the file it gets when coded alone; files come back in input
    order.  return_info=True: (files, info) with info[b] = {"bytes", "bpp", "passes", "level", "met"}; met says
    whether the file is within the budget (True without one).
    roi=masks with roi_levels=(lo, hi) (a *_VBR model; not together with max_bpp or level): ROI coding.  masks:
    uint8 / bool [B,H,W] (or one [H,W]), nonzero = inside the ROI.  Each 64 x 64 block of the image is coded at
    level lo where it holds no ROI pixel and up to hi where it is all ROI (codec.roi_levels), and the file carries
    the level map as a third string (its header level is hi); info[b] gains "roi_levels", the map.
    depth=d (8..16) with msb: the images are uint16 (ingest_u16's sample format) and go through ingest_u16;
    everything after the ingest works on the float image, so level, max_bpp, level="auto" and roi= compose
    unchanged, and the file does not know its depth.  depth=None is the uint8 path.
    coded_size=(h, w) or scale=Fraction (one of the two; codec.coded_size states the rounding), with filter: scaled
    coding (DESIGN.md §5 "Scaled coding").  ingest_u8_scaled resamples the H x W image to h x w in the ingest
    launch, the model codes that image exactly as it codes any h x w image, and the file is the scaled file
    (write_container_scaled: the display size H x W and the filter around the coded image's file).  level and
    max_bpp act on the coded image; bpp, in the budget and in info, is the whole file over the display pixels;
    info[b] gains "coded" and "filter".  Refused together with roi= and depth=.
    layered=True: progressive coding (DESIGN.md §5 "Progressive coding").  The network pass is unchanged; the y
    symbols are coded as one rANS string per channel slice and the file is the layered file
    (write_container_layered), which decode_images decodes whole or cut after any layer.  info[b] gains
    "layer_bytes".  depth= composes (the file does not know its depth).  Refused, each by name, together with roi=,
    max_bpp=, level="auto", scale= and coded_size=.
    max_error=tau (0..127; None = off, 0 = lossless): residual coding (DESIGN.md §5 "Residual coding").  The image
    is coded as without it; then net.decompress runs on the strings just made (what a decoder will run),
    egress_u8 gives the base image, residual_front the quantised residual with its contexts and histograms, and the
    file is the residual file (write_container_residual) around the unchanged plain or VBR file: decode_images
    returns an image in which no sample is off by more than tau.  The bound is checked on the device before
    anything is written.  info[b] gains "max_error", "base_bytes" and "residual_bytes"; bytes and bpp are the
    whole file.  Refused, each by name, together with roi=, max_bpp=, level="auto", depth=, scale=, coded_size= and
    layered=.  Samples of 9..16 bits are coded with a bound by encode_residual16 (the "MLR3" file).
    residual_segment=L (256..65536; needs max_error=): the segmented residual file "MLR2" (DESIGN.md §5 "Residual
    coding", "Segments") instead of "MLR1": the residual string is cut into segments of L samples that code
    independently, so residual_coder="device" (the default; a CPU model takes the host entry) codes them with
    residual_encode_segments_kernel while sym and ctx stay on the device, and decode_images decodes them there.
    residual_coder="host" builds the same bytes on the host.  None: the "MLR1" file, unchanged.  info[b] gains
    "residual_segment" and "segments"."""
    residual_coder = _check_coder(residual_coder, "encode_images")
    if residual_segment is not None:
        if max_error is None:
            raise ValueError("encode_images: residual_segment= needs max_error= (it cuts the residual string of "
                             "residual coding into segments)")
        residual_segment = _check_segment(residual_segment, "encode_images")
    if max_error is not None:
        max_error = _check_tau(max_error, "encode_images")
        _refuse_residual("encode_images", **{"roi=": roi is not None or roi_levels is not None,
                                             "max_bpp=": max_bpp is not None, "level='auto'": isinstance(level, str),
                                             "depth=": depth is not None, "scale=": scale is not None,
                                             "coded_size=": coded_size is not None, "layered=": bool(layered)})
    if layered:
        _refuse_layered("encode_images", roi=roi is not None or roi_levels is not None, max_bpp=max_bpp is not None,
                        scale=scale is not None, coded_size=coded_size is not None,
                        **{"level='auto'": isinstance(level, str)})
    scaled = coded_size is not None or scale is not None
    if scaled:
        if coded_size is not None and scale is not None:
            raise ValueError("encode_images: coded_size= and scale= are two ways to say one thing: pass one")
        if roi is not None or roi_levels is not None:
            raise ValueError("encode_images: scaled coding together with roi= is not supported")
        if depth is not None:
            raise ValueError("encode_images: scaled coding together with depth= (uint16 samples) is not supported")
        _filter_id(filter, "encode_images")
    if depth is None:
        img, layout = _u8_batch(imgs_u8, layout, "encode_images")
        ingest = ingest_u8
    else:
        depth, msb = _check_depth(depth, "encode_images"), _check_msb(msb, "encode_images")
        img, layout = _u16_batch(imgs_u8, layout, "encode_images")

        def ingest(t, lay):
            return ingest_u16(t, depth, lay, msb)
    _check_budget(max_bpp, max_passes)
    if isinstance(level, str) and max_bpp is None:
        raise ValueError("level='auto' needs max_bpp (the level is chosen from the budget)")
    B = img.size(0)
    H, W = _hw(img, layout)
    if (roi is None) != (roi_levels is None):
        raise ValueError("roi= and roi_levels=(lo, hi) go together")
    if roi is not None:
        if max_bpp is not None:
            raise ValueError("roi= together with max_bpp is not supported (ROI coding inside the rate loop)")
        if level is not None:
            raise ValueError("roi= together with level=: the levels of an ROI encode are roi_levels=(lo, hi)")
        lmap, hi = _roi_map(net, roi, roi_levels, (B, H, W), "encode_images")
        out = net.compress(ingest(img.to(net.device), layout), gain_map=gain_plane(net, lmap))
        ys, zs = out["strings"]
        lmap = lmap.cpu().numpy()
        files = [write_container_roi(H, W, out["shape"], ys[b], zs[b], int(hi), lmap[b]) for b in range(B)]
        if not return_info:
            return files
        return files, [{"bytes": len(f), "bpp": 8.0 * len(f) / (H * W), "passes": 0, "level": int(hi), "met": True,
                        "roi_levels": lmap[b]} for b, f in enumerate(files)]
    img = img.to(net.device)
    h, w = H, W  # the size the model codes
    if scaled:
        h, w = _check_size(coded_size, "encode_images coded_size") if scale is None else _scaled_size(H, W, scale)
        _check_ratio(H, h, "encode_images")
        _check_ratio(W, w, "encode_images")
        x = ingest_u8_scaled(img, (h, w), filter, layout)
    else:
        x = ingest(img, layout)
    if layered:
        lv, kw = _levels(net, level, B)
        out = net.compress(x, layered=True, **kw)
        zs = out["strings"][1]
        files = [write_container_layered(h, w, out["shape"], zs[b], out["layers"][b], None if lv is None else lv[b])
                 for b in range(B)]
        passes = [0] * B
    elif max_bpp is None:
        lv, kw = _levels(net, level, B)
        out = net.compress(x, **kw)
        ys, zs = out["strings"]
        files = [write_container(h, w, out["shape"], ys[b], zs[b], None if lv is None else lv[b]) for b in range(B)]
        passes = [0] * B
    elif scaled:
        files, passes, lv = rate_loop(net, x, h, w, level, max_bpp, max_passes, pixels=H * W, overhead=16)
    else:
        files, passes, lv = rate_loop(net, x, H, W, level, max_bpp, max_passes)
    if scaled:
        files = [write_container_scaled(H, W, f, filter, vbr=lv is not None) for f in files]
    residual = None
    if max_error is not None:
        files, residual = _encode_residual(net, img, layout, files, out["strings"], out["shape"], lv, max_error,
                                           residual_segment, residual_coder)
    if not return_info:
        return files
    info = []
    for b, f in enumerate(files):
        bpp = 8.0 * len(f) / (H * W)
        info.append({"bytes": len(f), "bpp": bpp, "passes": passes[b], "level": None if lv is None else lv[b],
                     "met": max_bpp is None or bpp <= max_bpp})
        if residual is not None:
            info[-1].update(residual[b])
        if scaled:
            info[-1].update(coded=(h, w), filter=filter)
        if layered:
            info[-1]["layer_bytes"] = [len(l) for l in out["layers"][b]]
    return files, info


@torch.no_grad()
def decode_images(net, files: Sequence[bytes], ref=None, max_pixels: int = MAX_PIXELS, depth: Optional[int] = None,
                  msb: bool = False, out_size=None, filter: Optional[str] = None, slices: Optional[int] = None,
                  fill: str = "mean", enhance: bool = True, residual_coder: str = "device"):
    """Files of one padded size -> (uint8 [B,H,W,3] on the model's device, info).  info[b] holds H, W, level
    (None for a fixed-rate model), bytes, bpp and, with ref (uint8 [B,H,W,3]), the exact sq_err and psnr of
    image b.  Files whose H x W differ within the padded size come back in the top-left of a zeroed
    [B,max H,max W,3] tensor.  Every file goes through the validating parser first.  An ROI file (a *_VBR file
    with a level map, encode_images(roi=...)) is decoded through the gain plane of its own map, and info[b] then
    holds the map as "roi_levels".
    depth=d (8..16) with msb: the image comes back as uint16 words of that sample format (egress_u16), ref is
    uint16 likewise, and psnr is computed with peak 2^d - 1.  The file does not know its depth: any file decodes at
    any depth.
    A scaled file (encode_images(coded_size=...) / (scale=...)) decodes to its display size: the model decodes the
    coded image and egress_u8_scaled resamples it in the egress launch with the file's filter.  out_size=(H', W')
    overrides the output size of every file, plain, VBR or scaled (the thumbnail decode; a plain file is resampled
    with lanczos3); filter= overrides the filter.  ref, sq_err and psnr are at the output size; info[b] then holds
    the output size as H, W, and "display", "coded" and "filter"; bpp stays the file over its display pixels.
    Refused together with depth= and for ROI files.
    slices=K with fill= ("mean" / "zero"): the progressive decode (DESIGN.md §5 "Progressive coding") of plain, VBR
    and layered files -- the first K channel slices are entropy-decoded and the rest filled as
    net.decompress_layers says.  A layered file (encode_images(layered=True)) may be truncated (cut anywhere after
    its z string); for it slices=None means every layer present.  Files are decoded in groups of one (kind, K), and
    info[b] gains "slices" (and "layers_present" for a layered file).  Refused for ROI, tiled and scaled files and
    together with out_size=.
    Residual files (encode_images(max_error=tau)): the inner files are decoded as above; then residual_front gives
    the contexts and the digest of that base image, the digest is compared with the file's (on a mismatch the file
    is decoded alone and compared once more, then an error is raised: a picture whose bound cannot be vouched for is
    never returned), the residual string is rANS-decoded with the file's tables and residual_apply adds it back.
    info[b] gains "max_error" (the file's tau), "residual_bytes", "base_bytes" and, with ref, "max_abs_err".
    enhance=False returns the base picture, byte for byte decode_images(strip_residual(f)).  Refused, each by name:
    slices=, out_size=, filter= and depth= on residual files, and a call mixing residual files with others.
    Segmented residual files ("MLR2", encode_images(residual_segment=L)) are told apart by their magic: after the
    same digest and table checks residual_decode_segments decodes the segments (residual_coder="device": the kernel,
    its int16 output read in place by residual_apply; "host": the host entry) and checks per segment that exactly
    its words were consumed and the state is back at 2^31; an error names the file and the segment.  "MLR1" and
    "MLR2" files, sizes and tau may mix in one call: they decode in groups.  info[b] gains "residual_segment" and
    "segments".
    Deep residual files ("MLR3", encode_residual16; DESIGN.md §5 "Residual coding", "Deep samples") come back as
    uint16 [B,H,W,3] at the file's depth: the inner files are decoded at that depth, residual_front16 gives the
    contexts and the digest (the same decode-alone retry and the same error), residual_decode_segments the high parts,
    the low-bit plane's padding bits are checked and residual_apply16 puts the samples together.  depth=, if given,
    must be the file's; ref is uint16, psnr has peak 2^depth - 1; enhance=False returns the base picture at the file's
    depth; info[b] gains "depth", "shift" and "low_bytes".  Refused by name: slices=, out_size=, filter=, msb=True,
    and a call that mixes "MLR3" files with others.  Files that differ in tau, shift, depth, segment length or size
    decode in groups."""
    residual_coder = _check_coder(residual_coder, "decode_images")
    files = [bytes(f) for f in files]
    if not files:
        raise ValueError("decode_images: no files")
    if any(bytes(f[:4]) == b"MLR4" for f in files):
        raise ValueError("decode_images: a Y'CbCr residual file (MLR4) holds planes, not RGB: decode_yuv decodes it")
    if any(is_residual_deep_file(f) for f in files):
        for name, given in (("slices=", slices is not None), ("out_size=", out_size is not None),
                            ("filter=", filter is not None), ("msb=True", bool(msb))):
            if given:
                raise ValueError(f"decode_images: {name} on a residual file (MLR3) is not supported")
        if fill != "mean":
            raise ValueError("decode_images: fill= goes with slices= or layered files")
        if not all(is_residual_deep_file(f) for f in files):
            raise ValueError("decode_images: deep residual files (MLR3) and other files in one call are not supported: "
                             "decode them in separate calls")
        if depth is not None:
            depth = _check_depth(depth, "decode_images")
        return _decode_residual16(net, files, ref, max_pixels, bool(enhance), residual_coder, depth)
    if any(is_residual_file(f) for f in files):
        for name, given in (("slices=", slices is not None), ("out_size=", out_size is not None),
                            ("filter=", filter is not None), ("depth=", depth is not None)):
            if given:
                kind = "MLR2" if all(is_residual_seg_file(f) for f in files if is_residual_file(f)) else "MLR1"
                raise ValueError(f"decode_images: {name} on a residual file ({kind}) is not supported")
        if fill != "mean":
            raise ValueError("decode_images: fill= goes with slices= or layered files")
        if not all(is_residual_file(f) for f in files):
            raise ValueError("decode_images: residual files (MLR1) and other files in one call are not supported: "
                             "decode them in separate calls")
        return _decode_residual(net, files, ref, max_pixels, bool(enhance), residual_coder)
    if depth is not None:
        depth, msb = _check_depth(depth, "decode_images"), _check_msb(msb, "decode_images")
    slices = _check_prefix(net, slices, fill, "decode_images")
    if any(is_tiled_file(f) for f in files):
        if slices is not None:
            raise ValueError("decode_images: slices= on a tiled file is not supported (tiles have no layered form)")
        raise ValueError("decode_images: a tiled file (MLT1) is decoded by decode_tiled, whole or by region")
    vbr = hasattr(net, "levels")
    prefix = slices is not None or any(is_layered_file(f) for f in files)
    if prefix and out_size is not None:
        raise ValueError("decode_images: slices= / layered files together with out_size= are not supported")
    if prefix and any(is_scaled_file(f) for f in files):
        raise ValueError("decode_images: slices= on a scaled file is not supported (scaled coding has no layered form)")
    if prefix and filter is not None:
        raise ValueError("decode_images: filter= goes with scaled files and out_size=, not with slices= / layered files")
    if fill != "mean" and not prefix:
        raise ValueError("decode_images: fill= goes with slices= or layered files")
    if out_size is not None:
        out_size = _check_size(out_size, "decode_images out_size")
    if filter is not None:
        _filter_id(filter, "decode_images")
    if out_size is not None or any(is_scaled_file(f) for f in files):
        if depth is not None:
            raise ValueError("decode_images: scaled coding together with depth= (uint16 samples) is not supported")
        return _decode_scaled(net, files, ref, max_pixels, out_size, filter)
    if filter is not None:
        raise ValueError("decode_images: filter= given, but no file is scaled and there is no out_size=")
    maps = [None] * len(files)
    ks = None  # progressive decode: the slices to entropy-decode, per file
    if prefix:
        cs, ks = _parse_prefix(net, files, slices, max_pixels)
    elif vbr and any(is_roi_file(f) for f in files):
        # ROI files carry a level map; a plain VBR file beside them decodes through a constant map of its level
        cs = []
        for b, f in enumerate(files):
            c, maps[b] = parse_container_roi(f, min(int(net.levels), 16), max_pixels)
            cs.append(c)
    else:
        cs = [parse_container(f, vbr, net.levels if vbr else None, max_pixels) for f in files]
    if len({(c.hz, c.wz) for c in cs}) != 1:
        raise ValueError(f"decode_images: the files must share one padded size, got z grids "
                         f"{sorted({(c.hz, c.wz) for c in cs})}")
    B = len(files)
    if ks is not None:
        x_hat = _decompress_prefix(net, files, cs, ks, fill)
    else:
        pairs = [_strings(f, c) for f, c in zip(files, cs)]
        kw = {"s": [c.level for c in cs]} if vbr else {}
        if any(m is not None for m in maps):
            lmap = np.stack([np.full((c.hz, c.wz), c.level, np.uint8) if m is None else m for c, m in zip(cs, maps)])
            kw = {"gain_map": gain_plane(net, torch.from_numpy(lmap))}
        x_hat = net.decompress([[p[0] for p in pairs], [p[1] for p in pairs]], (cs[0].hz, cs[0].wz), **kw)["x_hat"]
    H, W = max(c.H for c in cs), max(c.W for c in cs)
    if ref is not None:
        ref, _ = (_u8_batch if depth is None else _u16_batch)(ref, "hwc", "decode_images ref")
        if tuple(ref.shape) != (B, H, W, 3):
            raise ValueError(f"decode_images: ref must be {'uint8' if depth is None else 'uint16'} {(B, H, W, 3)}, "
                             f"got {tuple(ref.shape)}")
        ref = ref.to(x_hat.device)

    def egress(x, h, w, **kw):
        if depth is None:
            return egress_u8(x, h, w, "hwc", **kw)
        return egress_u16(x.float(), h, w, depth, "hwc", msb, **kw)

    if all((c.H, c.W) == (H, W) for c in cs):
        r = egress(x_hat, H, W, ref=ref)
        img, sq = r if ref is not None else (r, None)
    else:
        img = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=x_hat.device) if depth is None else \
            torch.zeros(B, H, W, 3, dtype=torch.int16, device=x_hat.device).view(torch.uint16)
        sq = None if ref is None else torch.zeros(B, dtype=torch.int64, device=x_hat.device)
        for b, c in enumerate(cs):
            r = egress(x_hat[b:b + 1], c.H, c.W, out=img[b:b + 1, :c.H, :c.W],
                       ref=None if ref is None else ref[b:b + 1, :c.H, :c.W])
            if ref is not None:
                sq[b] = r[1][0]
    sq = None if sq is None else sq.cpu().tolist()
    info = []
    for b, c in enumerate(cs):
        d = {"H": c.H, "W": c.W, "level": c.level if vbr else None, "bytes": len(files[b]),
             "bpp": 8.0 * len(files[b]) / (c.H * c.W)}
        if maps[b] is not None:
            d["roi_levels"] = maps[b]
        if ks is not None:
            d["slices"] = ks[b]
            if isinstance(c, _lib.ContainerLayeredInfo):
                d["layers_present"] = int(c.layers_present)
        if sq is not None:
            d["sq_err"] = int(sq[b])
            d["psnr"] = psnr_from_sq_err(d["sq_err"], 3 * c.H * c.W, 255 if depth is None else (1 << depth) - 1)
        info.append(d)
    return img, info


def _parse_prefix(net, files, slices, max_pixels):
    """The progressive decode's files, each through its validating parser -> (infos, K per file).  A layered
    file may be truncated; slices=None then means every layer it still has."""
    vbr = hasattr(net, "levels")
    n_levels = net.levels if vbr else None
    S = int(net.slice_num)
    cs, ks = [], []
    for f in files:
        if is_layered_file(f):
            c = parse_container_layered(f, n_levels, max_pixels, allow_truncated=True)
            if (c.level >= 0) != vbr:
                raise ValueError(f"decode_images: the layered file {'carries a' if c.level >= 0 else 'has no'} level "
                                 f"word, the model is {'variable' if vbr else 'fixed'}-rate")
            if c.S != S:
                raise ValueError(f"decode_images: the layered file has {c.S} layers, the model has {S} slices")
            k = int(c.layers_present) if slices is None else slices
            if k > c.layers_present:
                raise ValueError(f"decode_images: slices={k}, but the file holds {c.layers_present} whole layers")
        else:
            if vbr and is_roi_file(f):
                raise ValueError("decode_images: slices= on an ROI file is not supported (ROI coding has no layered "
                                 "form)")
            c = parse_container(f, vbr, n_levels, max_pixels)
            k = slices
        cs.append(c)
        ks.append(k)
    return cs, ks


def _decompress_prefix(net, files, cs, ks, fill):
    """One net.decompress / net.decompress_layers per group of files of one (z grid, kind, K), in input order."""
    vbr = hasattr(net, "levels")
    groups: Dict = {}
    for b, (c, k) in enumerate(zip(cs, ks)):
        groups.setdefault(((c.hz, c.wz), isinstance(c, _lib.ContainerLayeredInfo), k), []).append(b)
    outs = [None] * len(files)
    for (shape, lay, k), ids in groups.items():
        kw = {"s": [cs[b].level for b in ids]} if vbr else {}
        if lay:
            out = net.decompress_layers([_layers(files[b], cs[b])[:k] for b in ids],
                                        [files[b][cs[b].z_off:cs[b].z_off + cs[b].z_len] for b in ids], shape,
                                        slices=k, fill=fill, **kw)["x_hat"]
        else:
            pairs = [_strings(files[b], cs[b]) for b in ids]
            out = net.decompress([[p[0] for p in pairs], [p[1] for p in pairs]], shape, slices=k, fill=fill,
                                 **kw)["x_hat"]
        if len(groups) == 1:
            return out
        for j, b in enumerate(ids):
            outs[b] = out[j:j + 1]
    return torch.cat(outs, 0)


@torch.no_grad()
def decode_progressive(net, data: bytes, steps=None, fill: str = "mean", ref=None, max_pixels: int = MAX_PIXELS):
    """One file (plain, VBR or layered, whole or truncated) decoded at a rising number of slices: steps, default
    (1, 2, 4, S), each in [0, S] and strictly increasing; for a truncated layered file the steps beyond its layers
    are left out.  -> a list of {"slices", "image" (uint8 [H,W,3] on the model's device), "bytes" (a layered
    file's length up to that layer; None for a plain file, whose single string does not say) and, with ref
    (uint8 [H,W,3]), "sq_err" and "psnr"}.  One independent decode per step: each is decode_images(slices=K)."""
    _check_prefix(net, None, fill, "decode_progressive")
    S = int(net.slice_num)
    steps = tuple(sorted({min(k, S) for k in (1, 2, 4, S)})) if steps is None else tuple(steps)
    if not steps or any(isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k <= S for k in steps) \
            or any(a >= b for a, b in zip(steps, steps[1:])):
        raise ValueError(f"decode_progressive: steps must be strictly increasing integers in [0, {S}], got {steps!r}")
    data = bytes(data)
    lay = is_layered_file(data)
    if lay:
        have = parse_container_layered(data, net.levels if hasattr(net, "levels") else None, max_pixels, True)
        steps = tuple(k for k in steps if k <= have.layers_present)
        if not steps:
            raise ValueError(f"decode_progressive: the file holds {have.layers_present} whole layers, below every step")
    if ref is not None:
        ref, _ = _u8_batch(ref, "hwc", "decode_progressive ref")
    out = []
    for k in steps:
        img, info = decode_images(net, [data], ref=ref, max_pixels=max_pixels, slices=int(k), fill=fill)
        d = {"slices": int(k), "image": img[0], "bytes": len(truncate_layered(data, int(k))) if lay else None}
        if ref is not None:
            d.update(sq_err=info[0]["sq_err"], psnr=info[0]["psnr"])
        out.append(d)
    return out


def _decode_scaled(net, files, ref, max_pixels, out_size, filter):
    """decode_images for scaled files and / or an out_size: every image leaves through egress_u8_scaled."""
    vbr = hasattr(net, "levels")
    n_levels = net.levels if vbr else None
    if vbr and any(not is_scaled_file(f) and is_roi_file(f) for f in files):
        raise ValueError("decode_images: scaled coding together with ROI files is not supported")
    cs, inner, disp, flt = [], [], [], []
    for f in files:
        if is_scaled_file(f):
            s = parse_container_scaled(f, n_levels, max_pixels)
            if bool(s.vbr) != vbr:
                raise ValueError(f"decode_images: the scaled file's inner file {'carries a' if s.vbr else 'has no'} "
                                 f"level word, the model is {'variable' if vbr else 'fixed'}-rate")
            cs.append(s.inner)
            inner.append(f[s.inner_off:s.inner_off + s.inner_len])
            disp.append((s.H, s.W))
            flt.append(FILTERS[s.filter] if filter is None else filter)
        else:
            c = parse_container(f, vbr, n_levels, max_pixels)
            cs.append(c)
            inner.append(f)
            disp.append((c.H, c.W))
            flt.append("lanczos3" if filter is None else filter)
    if len({(c.hz, c.wz) for c in cs}) != 1:
        raise ValueError(f"decode_images: the files must share one padded (coded) size, got z grids "
                         f"{sorted({(c.hz, c.wz) for c in cs})}")
    B = len(files)
    sizes = [disp[b] if out_size is None else out_size for b in range(B)]
    for c, (Ho, Wo) in zip(cs, sizes):
        _check_ratio(c.H, Ho, "decode_images")
        _check_ratio(c.W, Wo, "decode_images")
    pairs = [_strings(f, c) for f, c in zip(inner, cs)]
    kw = {"s": [c.level for c in cs]} if vbr else {}
    x_hat = net.decompress([[p[0] for p in pairs], [p[1] for p in pairs]], (cs[0].hz, cs[0].wz), **kw)["x_hat"]
    H, W = max(s[0] for s in sizes), max(s[1] for s in sizes)
    if ref is not None:
        ref, _ = _u8_batch(ref, "hwc", "decode_images ref")
        if tuple(ref.shape) != (B, H, W, 3):
            raise ValueError(f"decode_images: ref must be uint8 {(B, H, W, 3)} (the output size), got {tuple(ref.shape)}")
        ref = ref.to(x_hat.device)
    if len({(c.H, c.W, sz, fl) for c, sz, fl in zip(cs, sizes, flt)}) == 1:
        r = egress_u8_scaled(x_hat, cs[0].H, cs[0].W, (H, W), flt[0], "hwc", ref=ref)
        img, sq = r if ref is not None else (r, None)
    else:
        img = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=x_hat.device)
        sq = None if ref is None else torch.zeros(B, dtype=torch.int64, device=x_hat.device)
        for b, (c, (Ho, Wo)) in enumerate(zip(cs, sizes)):
            r = egress_u8_scaled(x_hat[b:b + 1], c.H, c.W, (Ho, Wo), flt[b], "hwc", out=img[b:b + 1, :Ho, :Wo],
                                 ref=None if ref is None else ref[b:b + 1, :Ho, :Wo])
            if ref is not None:
                sq[b] = r[1][0]
    sq = None if sq is None else sq.cpu().tolist()
    info = []
    for b, c in enumerate(cs):
        Ho, Wo = sizes[b]
        d = {"H": Ho, "W": Wo, "display": disp[b], "coded": (c.H, c.W), "filter": flt[b],
             "level": c.level if vbr else None, "bytes": len(files[b]),
             "bpp": 8.0 * len(files[b]) / (disp[b][0] * disp[b][1])}
        if sq is not None:
            d["sq_err"] = int(sq[b])
            d["psnr"] = psnr_from_sq_err(d["sq_err"], 3 * Ho * Wo)
        info.append(d)
    return img, info


# -------------------------------------------------------------------------------------------- tiles
def _check_tile_params(tile, overlap):
    ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (tile, overlap))
    if not ok or tile % 64 or not 128 <= tile <= 65472:
        raise ValueError(f"tile must be a multiple of 64 in [128, 65472], got {tile!r}")
    if overlap not in (0, 16, 32, 64) or overlap > tile // 2:
        raise ValueError(f"overlap must be 0, 16, 32 or 64 and at most tile / 2, got {overlap!r} (tile {tile})")


def _tile_axis(L: int, T: int, V: int):
    """[(start, extent)] of the tiles along an axis of length L."""
    S = T - V
    n = 1 if L <= T else -(-(L - V) // S)
    return [(k * S, min(T, L - k * S)) for k in range(n)]


def tile_grid(H: int, W: int, tile: int, overlap: int) -> Dict:
    """The tile grid of an H x W image (DESIGN.md §5 "Tiled coding"; the same definition as mlic_tile_grid): per
    axis of length L with S = tile - overlap, n = 1 if L <= tile else ceil((L - overlap) / S), tile k starts at k S
    and has extent min(tile, L - k S).  -> {"H", "W", "tile", "overlap", "ny", "nx", "ys", "xs": [(start, extent)]
    per axis, "rects": [(y0, x0, h, w)] row-major}."""
    _check_tile_params(tile, overlap)
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"tile_grid: a non-empty image expected, got {H} x {W}")
    ys, xs = _tile_axis(H, tile, overlap), _tile_axis(W, tile, overlap)
    return {"H": H, "W": W, "tile": int(tile), "overlap": int(overlap), "ny": len(ys), "nx": len(xs), "ys": ys, "xs": xs,
            "rects": [(y0, x0, h, w) for y0, h in ys for x0, w in xs]}


def tile_weights(L: int, tile: int, overlap: int, k: int) -> torch.Tensor:
    """Tile k's feather weights along an axis of length L, fp32 [extent]: in the strip it shares with tile k - 1
    (its first `overlap` positions j) (2 j + 1) / (2 overlap), in the strip it shares with tile k + 1 one minus that
    tile's weight, 1 elsewhere.  Dyadic rationals: the two weights of a strip position sum to exactly 1."""
    axis = _tile_axis(L, tile, overlap)
    ext, V, S = axis[k][1], overlap, tile - overlap
    w = torch.ones(ext, dtype=torch.float32)
    if V:
        ramp = (2 * torch.arange(V, dtype=torch.float32) + 1) / (2 * V)
        if k > 0:
            w[:V] = ramp
        if k + 1 < len(axis):
            w[S:] = 1 - ramp
    return w


def _region(region, H: int, W: int, what: str):
    if region is None:
        return 0, 0, H, W
    try:
        y0, x0, h, w = (int(v) for v in region)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: region must be (y0, x0, h, w), got {region!r}") from None
    if h < 1 or w < 1 or y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
        raise ValueError(f"{what}: region {(y0, x0, h, w)} is empty or outside the {H} x {W} image")
    return y0, x0, h, w


def _tiles_of_region(grid: Dict, region) -> List[int]:
    """Sorted indices of the tiles that intersect the region."""
    y0, x0, h, w = region
    return [ky * grid["nx"] + kx for ky, (ty, th) in enumerate(grid["ys"]) if ty < y0 + h and ty + th > y0
            for kx, (tx, tw) in enumerate(grid["xs"]) if tx < x0 + w and tx + tw > x0]


def blend_tiles(tiles, H: int, W: int, tile: int, overlap: int, region=None, layout: str = "hwc", ref=None,
                out: Optional[torch.Tensor] = None):
    """The region (y0, x0, h, w) (None: the whole image) of an H x W image as uint8 ([h,w,3] for layout "hwc",
    [3,h,w] for "chw"), blended from its tiles' x_hat.  tiles: ny * nx entries, row-major (or a dict index ->
    tensor); entry k is tile k's contiguous fp32 [3, pad64(h_k), pad64(w_k)] or None; every tile that intersects
    the region must be there, and all on one device.  Per pixel and channel acc (float64) = 0; acc += (wy * wx as
    float64) * x_hat over the covering tiles, tile row then tile column (tile_weights; each product exact, the
    sums rounded in that order); then floor(clamp(float32(acc), 0, 1) * 255), NaN -> 0.  A pixel one tile covers
    is egress_u8 of that tile.  out: optional uint8 tensor of the result's shape, any strides (only the region's
    bytes are written).  ref: the region's crop of the original, uint8 of the same shape and layout, any strides:
    returns (image, sq_err), sq_err int64 [1], the exact sum of squared differences.  CUDA tensors: one launch of
    the blend kernel on the current stream; CPU tensors: the torch restatement, bit for bit the same."""
    grid = tile_grid(H, W, tile, overlap)
    n = grid["ny"] * grid["nx"]
    if isinstance(tiles, dict):
        tiles = [tiles.get(k) for k in range(n)]
    tiles = list(tiles)
    if len(tiles) != n:
        raise ValueError(f"blend_tiles: {n} entries ({grid['ny']} x {grid['nx']} tiles) expected, got {len(tiles)}")
    if layout not in ("hwc", "chw"):
        raise ValueError(f"layout must be 'hwc' or 'chw', got {layout!r}")
    y0, x0, h, w = _region(region, H, W, "blend_tiles")
    need = _tiles_of_region(grid, (y0, x0, h, w))
    for k, t in enumerate(tiles):
        if t is None:
            if k in need:
                raise ValueError(f"blend_tiles: tile {k} covers the region and is missing")
            continue
        _, _, th, tw = grid["rects"][k]
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (3, _pad64(th), _pad64(tw)):
            raise ValueError(f"blend_tiles: tile {k} must be fp32 {(3, _pad64(th), _pad64(tw))}")
    dev = tiles[need[0]].device  # a region is never empty, so it has a covering tile, and that one is there
    if any(t is not None and t.device != dev for t in tiles):
        raise ValueError(f"blend_tiles: the tiles must be on one device ({dev})")
    shape = (h, w, 3) if layout == "hwc" else (3, h, w)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != dev:
        raise ValueError(f"blend_tiles: out must be uint8 {shape} on {dev}")
    if ref is not None:
        if isinstance(ref, np.ndarray):
            ref = torch.from_numpy(np.ascontiguousarray(ref))
        if not torch.is_tensor(ref) or ref.dtype != torch.uint8 or tuple(ref.shape) != shape:
            raise ValueError(f"blend_tiles: ref must be uint8 {shape}")
        ref = ref.to(dev)

    def rcc(t):  # element strides {row, column, channel}
        s = t.stride()
        return (s[0], s[1], s[2]) if layout == "hwc" else (s[1], s[2], s[0])

    if dev.type != "cuda":
        acc = torch.zeros(3, h, w, dtype=torch.float64)
        for k in need:
            ty, tx, th, tw = grid["rects"][k]
            ky, kx = divmod(k, grid["nx"])
            a, b = max(ty, y0), min(ty + th, y0 + h)
            c, d = max(tx, x0), min(tx + tw, x0 + w)
            wy = tile_weights(H, tile, overlap, ky)[a - ty:b - ty]
            wx = tile_weights(W, tile, overlap, kx)[c - tx:d - tx]
            wgt = (wy[:, None] * wx[None, :]).double()  # the fp32 product is exact (at most 14 bits)
            acc[:, a - y0:b - y0, c - x0:d - x0] += wgt * tiles[k][:, a - ty:b - ty, c - tx:d - tx].double()
        v = acc.float()
        v = torch.where(torch.isnan(v), torch.zeros_like(v), v)
        u = (v.clamp(0, 1) * 255).floor().to(torch.uint8)
        out.copy_(u.permute(1, 2, 0) if layout == "hwc" else u)
        if ref is None:
            return out
        dd = out.to(torch.int64) - ref.to(torch.int64)
        return out, (dd * dd).sum().reshape(1)
    if 0 in rcc(out)[1:]:
        raise ValueError("blend_tiles: out has a zero column or channel stride")
    with torch.cuda.device(dev):
        tiles = [None if t is None else t.contiguous() for t in tiles]
        ptrs = [0 if t is None else t.data_ptr() for t in tiles]
        table = torch.tensor(ptrs, dtype=torch.int64).to(dev)
        host = (C.c_void_p * n)(*[p or None for p in ptrs])
        sq = None
        if ref is not None:
            if 0 in rcc(ref)[1:]:
                ref = ref.contiguous()
            sq = torch.full((1,), -1, dtype=torch.int64, device=dev)
        _lib.call("mlic_image_tile_blend_u8", _stream(), C.c_void_p(table.data_ptr()), host, H, W, int(tile),
                  int(overlap), y0, x0, h, w, C.c_void_p(out.data_ptr()), (C.c_int64 * 3)(*rcc(out)),
                  None if ref is None else C.c_void_p(ref.data_ptr()),
                  None if ref is None else (C.c_int64 * 3)(*rcc(ref)),
                  None if sq is None else C.c_void_p(sq.data_ptr()))
        st = torch.cuda.current_stream()
        for t in [table, ref] + tiles:
            if t is not None:
                t.record_stream(st)
    return out if ref is None else (out, sq)


TILED_MAGIC = b"MLT1"
MAX_IMAGE_PIXELS = 1 << 32  # default bound on a tiled file's H * W (the tiles have MAX_PIXELS each)


def is_tiled_file(data: bytes) -> bool:
    """Whether the file starts with the tiled container's magic (read as a plain file's H it is about 1.3e9)."""
    return bytes(data[:4]) == TILED_MAGIC


def write_container_tiled(H: int, W: int, tile: int, overlap: int, files: Sequence[bytes], vbr: bool = False) -> bytes:
    """The tiled file of an H x W image (mlic_container_write_tiled): files = the tiles' per-image files, row-major."""
    files = [bytes(f) for f in files]
    payload = b"".join(files)
    lens = (C.c_uint64 * max(1, len(files)))(*[len(f) for f in files])
    n = C.c_size_t()
    args = (int(H), int(W), int(tile), int(overlap), int(vbr), payload, lens, len(files))
    _lib.call("mlic_container_write_tiled", *args, None, 0, C.byref(n))
    buf = C.create_string_buffer(max(1, n.value))
    _lib.call("mlic_container_write_tiled", *args, buf, len(buf), C.byref(n))
    return C.string_at(buf, n.value)


def parse_container_tiled(data: bytes, max_pixels: int = MAX_IMAGE_PIXELS) -> _lib.ContainerTiledInfo:
    """The validating parser of a tiled file (mlic_container_parse_tiled): raises _lib.MlicError on any malformed
    input.  max_pixels bounds H * W of the whole image."""
    data = bytes(data)
    info = _lib.ContainerTiledInfo()
    _lib.call("mlic_container_parse_tiled", data, len(data), int(max_pixels), C.byref(info))
    return info


def tiled_tile(data: bytes, info: _lib.ContainerTiledInfo, k: int):
    """(offset, length) of tile k's file inside a parsed tiled file (mlic_container_tiled_tile)."""
    off, ln = C.c_uint64(), C.c_uint64()
    _lib.call("mlic_container_tiled_tile", data, len(data), C.byref(info), int(k), C.byref(off), C.byref(ln))
    return off.value, ln.value


def _tile_file(data: bytes, t, grid: Dict, k: int, vbr: bool, n_levels):
    """Tile k's file out of a parsed tiled file, through the per-image parser: (bytes, ContainerInfo)."""
    off, ln = tiled_tile(data, t, k)
    f = data[off:off + ln]
    _, _, th, tw = grid["rects"][k]
    c = parse_container(f, vbr, n_levels, _pad64(th) * _pad64(tw))
    if (c.H, c.W) != (th, tw):
        raise _lib.MlicError(f"tiled file: tile {k} says {c.H} x {c.W}, the grid {th} x {tw}")
    return f, c


def _peek_tiled(data: bytes, n_levels, max_pixels) -> Dict:
    t = parse_container_tiled(data, max_pixels)
    grid = tile_grid(t.H, t.W, t.T, t.V)
    vbr = bool(t.vbr)
    tiles = []
    for k, (ty, tx, th, tw) in enumerate(grid["rects"]):
        f, c = _tile_file(data, t, grid, k, vbr, n_levels)
        tiles.append({"index": k, "y0": ty, "x0": tx, "H": th, "W": tw, "level": c.level if vbr else None,
                      "bytes": len(f), "bpp": 8.0 * len(f) / (th * tw)})
    return {"tiled": True, "H": t.H, "W": t.W, "tile": t.T, "overlap": t.V, "grid": (t.ny, t.nx), "vbr": vbr,
            "level": tiles[0]["level"], "tiles": tiles, "bytes": len(data), "bpp": 8.0 * len(data) / (t.H * t.W)}


def _refuse_with_tiles(what: str, max_bpp=None, level=None, roi=None, roi_levels=None):
    if max_bpp is not None:
        raise ValueError(f"{what}: max_bpp together with tiles is not supported (rate control per tiled image)")
    if isinstance(level, str):
        raise ValueError(f"{what}: level={level!r} together with tiles is not supported (it needs max_bpp)")
    if roi is not None or roi_levels is not None:
        raise ValueError(f"{what}: roi= together with tiles is not supported")
    if level is not None and (isinstance(level, (list, tuple)) or np.ndim(level) != 0):
        raise ValueError(f"{what}: per-tile levels are not supported: a VBR level is one level for the image")


def _refuse_scaled(what: str, other: str, *given):
    if any(g is not None for g in given):
        raise ValueError(f"{what}: scaled coding together with {other} is not supported")


def _refuse_deep_tiles(what: str, depth):
    """depth= exists on the tiled calls only to be refused by name: any depth means uint16 words (depth=8 too, as in
    encode_images(depth=8)), and tiles are uint8 images alone."""
    if depth is not None:
        raise ValueError(f"{what}: depth {_check_depth(depth, what)} together with tiles is not supported: the blend "
                         f"kernel (mlic_image_tile_blend_u8) writes bytes, there is no 16-bit blend egress (uint8 "
                         f"images take no depth=)")


@torch.no_grad()
def encode_tiled(net, img_u8, tile: int = 1024, overlap: int = 32, level=None, layout: Optional[str] = None,
                 tile_batch: int = 8, return_info: bool = False, max_bpp=None, roi=None, roi_levels=None, depth=None,
                 coded_size=None, scale=None, layered: bool = False, max_error=None):
    """One uint8 image ([H,W,3] / [3,H,W], tensor or numpy array) -> one tiled file (DESIGN.md §5 "Tiled coding"):
    the image is cut into the tiles of tile_grid(H, W, tile, overlap), each tile is coded by itself and its file
    is byte for byte encode_images of that crop, and the tiled container holds them row-major with an index.
    Tiles are ingested in place through strided views of the image (a run of equal tiles in a tile row is a batch
    whose image stride is tile - overlap columns) and coded per shape group (interior, right column, bottom row,
    corner) in chunks of at most tile_batch tiles, so device memory is the arena of tile_batch tiles plus the
    uint8 image itself, which crosses to the model's device whole (3 bytes per pixel).  level: the one VBR level of the image.  max_bpp, level="auto", roi= and per-tile levels are
    refused, and so is any depth= (uint16 words: the blend kernel writes bytes).  return_info=True: (file, info) with info =
    {"H", "W", "tile", "overlap", "grid", "bytes", "bpp", "level", "tile_bytes"}."""
    _refuse_with_tiles("encode_tiled", max_bpp, level, roi, roi_levels)
    _refuse_layered("encode_tiled", tiles=layered)
    _refuse_deep_tiles("encode_tiled", depth)
    _refuse_scaled("encode_tiled", "tiles", coded_size, scale)
    _refuse_residual("encode_tiled", tiles=max_error is not None)
    img, layout = _u8_batch(img_u8, layout, "encode_tiled")
    if img.size(0) != 1:
        raise ValueError(f"encode_tiled takes one image, got a batch of {img.size(0)}")
    if isinstance(tile_batch, bool) or not isinstance(tile_batch, (int, np.integer)) or tile_batch < 1:
        raise ValueError(f"tile_batch must be a positive integer, got {tile_batch!r}")
    H, W = _hw(img, layout)
    grid = tile_grid(H, W, tile, overlap)
    lv, _ = _levels(net, level, 1)
    img = _in_place(img.to(net.device), layout)
    _, sr, sc, sch = _strides(img, layout)
    S, nx = tile - overlap, grid["nx"]
    groups: Dict = {}
    for k, (_, _, th, tw) in enumerate(grid["rects"]):
        groups.setdefault((th, tw), []).append(k)
    files: List[Optional[bytes]] = [None] * len(grid["rects"])
    for (th, tw), ks in groups.items():
        for i in range(0, len(ks), tile_batch):
            chunk = ks[i:i + tile_batch]
            runs = [[chunk[0]]]  # consecutive tiles of one tile row
            for k in chunk[1:]:
                if k == runs[-1][-1] + 1 and k // nx == runs[-1][-1] // nx:
                    runs[-1].append(k)
                else:
                    runs.append([k])
            xs = []
            for run in runs:
                ty, tx = grid["rects"][run[0]][:2]
                size, stride = ((len(run), th, tw, 3), (S * sc, sr, sc, sch)) if layout == "hwc" else \
                               ((len(run), 3, th, tw), (S * sc, sch, sr, sc))
                xs.append(ingest_u8(torch.as_strided(img, size, stride, img.storage_offset() + ty * sr + tx * sc), layout))
            x = xs[0] if len(xs) == 1 else torch.cat(xs, 0)
            out = net.compress(x, **({} if lv is None else {"s": lv * len(chunk)}))
            ys, zs = out["strings"]
            for j, k in enumerate(chunk):
                files[k] = write_container(th, tw, out["shape"], ys[j], zs[j], None if lv is None else lv[0])
    data = write_container_tiled(H, W, tile, overlap, files, vbr=lv is not None)
    if not return_info:
        return data
    return data, {"H": H, "W": W, "tile": int(tile), "overlap": int(overlap), "grid": (grid["ny"], grid["nx"]),
                  "bytes": len(data), "bpp": 8.0 * len(data) / (H * W), "level": None if lv is None else lv[0],
                  "tile_bytes": [len(f) for f in files]}


@torch.no_grad()
def decode_tiled(net, data: bytes, region=None, ref=None, tile_batch: int = 8, max_pixels: int = MAX_IMAGE_PIXELS,
                 depth=None, out_size=None, slices=None):
    """A tiled file -> (uint8 [h,w,3] on the model's device, info): the region (y0, x0, h, w) of the image (None:
    all of it).  Only the tiles that intersect the region are entropy-decoded and synthesised (per shape group,
    in chunks of at most tile_batch tiles); their fp32 x_hat is kept (12 bytes per pixel of the decoded tiles, on top of the arena of
    tile_batch tiles) and one blend_tiles launch writes the region.  The file and every tile's file go through the validating parsers first.  info: H, W, tile, overlap,
    grid (ny, nx), region, tiles_decoded (sorted tile indices), level, bytes and bpp of the whole file and, with
    ref (uint8 [h,w,3], the region's crop of the original), the exact sq_err and psnr."""
    _refuse_deep_tiles("decode_tiled", depth)
    _refuse_scaled("decode_tiled", "tiles", out_size)
    if slices is not None:
        raise ValueError("decode_tiled: slices= on a tiled file is not supported (tiles have no layered form)")
    data = bytes(data)
    if is_residual_file(data):
        raise ValueError("decode_tiled: a residual file (MLR1): residual coding together with tiles is not supported; "
                         "decode_images decodes it")
    if is_scaled_file(data):
        raise ValueError("decode_tiled: a scaled file (MLS1): scaled coding together with tiles is not supported; "
                         "decode_images reads it")
    if isinstance(tile_batch, bool) or not isinstance(tile_batch, (int, np.integer)) or tile_batch < 1:
        raise ValueError(f"tile_batch must be a positive integer, got {tile_batch!r}")
    if not is_tiled_file(data):
        raise ValueError("decode_tiled: not a tiled file (no MLT1 magic): decode_images reads per-image files")
    t = parse_container_tiled(data, max_pixels)
    vbr = hasattr(net, "levels")
    if bool(t.vbr) != vbr:
        raise ValueError(f"decode_tiled: the file's tiles {'carry' if t.vbr else 'have no'} level word, the model is "
                         f"{'variable' if vbr else 'fixed'}-rate")
    H, W, T, V = t.H, t.W, t.T, t.V
    grid = tile_grid(H, W, T, V)
    reg = _region(region, H, W, "decode_tiled")
    if ref is not None:
        if isinstance(ref, np.ndarray):
            ref = torch.from_numpy(np.ascontiguousarray(ref))
        if not torch.is_tensor(ref) or ref.dtype != torch.uint8 or tuple(ref.shape) != (reg[2], reg[3], 3):
            raise ValueError(f"decode_tiled: ref must be uint8 {(reg[2], reg[3], 3)}, the region's crop of the original")
    need = _tiles_of_region(grid, reg)
    parsed = {k: _tile_file(data, t, grid, k, vbr, net.levels if vbr else None) for k in need}
    groups: Dict = {}
    for k in need:
        c = parsed[k][1]
        groups.setdefault((c.hz, c.wz), []).append(k)
    tiles: Dict = {}
    for shape, ks in groups.items():
        for i in range(0, len(ks), tile_batch):
            chunk = ks[i:i + tile_batch]
            pairs = [_strings(*parsed[k]) for k in chunk]
            kw = {"s": [parsed[k][1].level for k in chunk]} if vbr else {}
            x_hat = net.decompress([[p[0] for p in pairs], [p[1] for p in pairs]], shape, **kw)["x_hat"]
            x_hat = x_hat.float().contiguous()
            for j, k in enumerate(chunk):
                tiles[k] = x_hat[j]
    r = blend_tiles(tiles, H, W, T, V, reg, "hwc", ref=ref)
    img, sq = r if ref is not None else (r, None)
    info = {"H": H, "W": W, "tile": T, "overlap": V, "grid": (t.ny, t.nx), "region": reg, "tiles_decoded": need,
            "level": parsed[need[0]][1].level if vbr else None, "bytes": len(data), "bpp": 8.0 * len(data) / (H * W)}
    if sq is not None:
        info["sq_err"] = int(sq.cpu()[0])
        info["psnr"] = psnr_from_sq_err(info["sq_err"], 3 * reg[2] * reg[3])
    return img, info


# -------------------------------------------------------------------------------------------- YCbCr
_YUV_MATRIX = {"bt601": (0, 0.299, 0.114), "bt709": (1, 0.2126, 0.0722), "bt2020": (2, 0.2627, 0.0593)}
_YUV_SUB = {"i420": (2, 2), "yv12": (2, 2), "nv12": (2, 2), "nv21": (2, 2), "i422": (2, 1), "i444": (1, 1)}


class YuvFormat:
    """What a Y'CbCr frame means (mlic_yuv_desc; DESIGN.md §5 "YCbCr I/O" and "High-bit-depth I/O"): sub = (sub_x,
    sub_y), (1, 1) 4:4:4, (2, 1) 4:2:2 or (2, 2) 4:2:0; matrix "bt709" or "bt601" (and "bt2020", non-constant
    luminance, when depth > 8); full_range (False: Y in 16..235, C in 16..240, times 2^(depth-8));
    site_x, the horizontal chroma siting of a subsampled frame: "left" (co-sited with the even luma column: MPEG-2,
    H.264 / HEVC) or "centre" (JPEG, MPEG-1).  Vertical siting is always centre.  depth: bits per sample, 8 (uint8
    planes, the 8-bit kernels) or 9..16 (uint16 planes, csrc/image_io16.hip); msb: the samples of a uint16 word are
    MSB-aligned (P010 / P016) instead of LSB-aligned (y4m p10, I010).  None of this is in the file: it is the
    caller's knowledge on both sides."""

    def __init__(self, sub=(2, 2), matrix: str = "bt709", full_range: bool = False, site_x: str = "left",
                 depth: int = 8, msb: bool = False):
        try:
            sub = tuple(int(v) for v in sub)
        except (TypeError, ValueError):
            raise ValueError(f"YuvFormat: sub must be (sub_x, sub_y), got {sub!r}") from None
        if sub not in ((1, 1), (2, 1), (2, 2)):
            raise ValueError(f"YuvFormat: sub must be (1, 1), (2, 1) or (2, 2), got {sub!r}")
        depth, msb = _check_depth(depth, "YuvFormat"), _check_msb(msb, "YuvFormat")
        if msb and depth == 8:
            raise ValueError("YuvFormat: msb=True needs depth > 8 (8-bit samples are bytes)")
        if matrix not in _YUV_MATRIX:
            raise ValueError(f"YuvFormat: matrix must be 'bt601', 'bt709' or 'bt2020', got {matrix!r} (other matrices "
                             f"are out of scope)")
        if matrix == "bt2020" and depth == 8:
            raise ValueError("YuvFormat: matrix must be 'bt601' or 'bt709' at depth 8, got 'bt2020' (BT.2020 needs "
                             "depth > 8: the 8-bit kernels refuse it)")
        if not isinstance(full_range, (bool, np.bool_)):
            raise ValueError(f"YuvFormat: full_range must be a bool, got {full_range!r}")
        if site_x not in ("left", "centre"):
            raise ValueError(f"YuvFormat: site_x must be 'left' or 'centre', got {site_x!r}")
        self.sub, self.matrix, self.full_range, self.site_x = sub, matrix, bool(full_range), site_x
        self.depth, self.msb = depth, msb

    def __repr__(self):
        deep = f", depth={self.depth}, msb={self.msb}" if self.depth > 8 else ""
        return (f"YuvFormat(sub={self.sub}, matrix={self.matrix!r}, full_range={self.full_range}, "
                f"site_x={self.site_x!r}{deep})")

    def __eq__(self, other):
        return isinstance(other, YuvFormat) and \
            (self.sub, self.matrix, self.full_range, self.site_x, self.depth, self.msb) == \
            (other.sub, other.matrix, other.full_range, other.site_x, other.depth, other.msb)

    @property
    def maxv(self) -> int:
        return (1 << self.depth) - 1

    @property
    def dtype(self):
        return torch.uint8 if self.depth == 8 else torch.uint16

    @property
    def left(self) -> bool:
        return self.sub[0] == 2 and self.site_x == "left"

    def chroma_size(self, H: int, W: int):
        """(rows, columns) of the chroma planes of an H x W frame: the ceil rule."""
        return (H + self.sub[1] - 1) // self.sub[1], (W + self.sub[0] - 1) // self.sub[0]

    def desc(self) -> _lib.YuvDesc:
        return _lib.YuvDesc(self.sub[0], self.sub[1], _YUV_MATRIX[self.matrix][0], int(self.full_range),
                            int(self.site_x == "left"), (C.c_int32 * 3)(0, 0, 0))

    def constants(self, depth: Optional[int] = None) -> Dict[str, float]:
        """The kernels' fp32 constants, each folded in double and rounded to fp32 once (the library folds the same
        expressions): ingest yo, cy, crv, cgu, cgv, cbu; egress yr, yg, yb | br, bg, bb | rr, rg, rb.  depth: the
        sample depth they are folded for (default: the format's own): ys, cs, yo scale with 2^(depth-8) in limited
        range and are 2^depth - 1, 2^depth - 1, 0 in full range."""
        _, Kr, Kb = _YUV_MATRIX[self.matrix]
        Kg = 1.0 - Kr - Kb
        depth = self.depth if depth is None else depth
        if depth == 8:
            ys, cs, yo = (255.0, 255.0, 0.0) if self.full_range else (219.0, 224.0, 16.0)
        else:
            m, sc = float((1 << depth) - 1), float(1 << (depth - 8))
            ys, cs, yo = (m, m, 0.0) if self.full_range else (219.0 * sc, 224.0 * sc, 16.0 * sc)
        d = {"yo": yo, "cy": 1.0 / ys, "crv": 2.0 * (1.0 - Kr) / cs, "cgu": 2.0 * Kb * (1.0 - Kb) / (Kg * cs),
             "cgv": 2.0 * Kr * (1.0 - Kr) / (Kg * cs), "cbu": 2.0 * (1.0 - Kb) / cs,
             "yr": ys * Kr, "yg": ys * Kg, "yb": ys * Kb,
             "br": -(cs * Kr) / (2.0 * (1.0 - Kb)), "bg": -(cs * Kg) / (2.0 * (1.0 - Kb)), "bb": cs / 2.0,
             "rr": cs / 2.0, "rg": -(cs * Kg) / (2.0 * (1.0 - Kr)), "rb": -(cs * Kb) / (2.0 * (1.0 - Kr))}
        return {k: float(np.float32(v)) for k, v in d.items()}


def _check_fmt(fmt, what: str) -> YuvFormat:
    if not isinstance(fmt, YuvFormat):
        raise ValueError(f"{what}: fmt must be a YuvFormat, got {fmt!r}")
    return fmt


def yuv_frame_samples(H: int, W: int, layout: str) -> int:
    """Samples of one H x W frame in a raw layout (the ceil rule for the chroma planes)."""
    if layout not in _YUV_SUB:
        raise ValueError(f"yuv layout must be one of {sorted(_YUV_SUB)}, got {layout!r}")
    sx, sy = _YUV_SUB[layout]
    return H * W + 2 * ((H + sy - 1) // sy) * ((W + sx - 1) // sx)


def yuv_frame_bytes(H: int, W: int, layout: str, depth: int = 8) -> int:
    """Bytes of one H x W frame in a raw layout: one byte a sample at depth 8, two (a uint16 word) above."""
    return yuv_frame_samples(H, W, layout) * (1 if _check_depth(depth, "yuv_frame_bytes") == 8 else 2)


def split_yuv(buf, H: int, W: int, layout: str, depth: int = 8):
    """A raw frame buffer -> (y, cb, cr) as strided views of it, no copy.  buf: flat uint8 tensor or numpy array of
    yuv_frame_bytes(H, W, layout) bytes, or [B, that many]; or, for samples deeper than 8 bits, a uint16 buffer of
    yuv_frame_samples(H, W, layout) words together with depth= above 8 (P010 is layout "nv12" on a uint16 buffer
    with depth=10, and YuvFormat(depth=10, msb=True) says what the words mean).  Layouts: "i420" (Y, Cb, Cr planes), "yv12" (Y, Cr, Cb),
    "nv12" (Y, then interleaved Cb Cr rows: the chroma views have column stride 2), "nv21" (Cr Cb), "i422", "i444".
    y is [H, W] (or [B, H, W]), cb and cr are [ceil(H / sub_y), ceil(W / sub_x)]."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"split_yuv: a non-empty frame expected, got {H} x {W}")
    need = yuv_frame_samples(H, W, layout)
    is_np = isinstance(buf, np.ndarray)
    if not (is_np or torch.is_tensor(buf)) or buf.dtype not in (np.uint8, torch.uint8, np.uint16, torch.uint16) or \
            buf.ndim not in (1, 2):
        raise ValueError("split_yuv: a flat uint8 or uint16 tensor or array (or [B, samples]) expected")
    deep = _check_depth(depth, "split_yuv") > 8
    if deep != (buf.dtype in (np.uint16, torch.uint16)):
        raise ValueError(f"split_yuv: a frame of depth {depth} is a {'uint16' if deep else 'uint8'} buffer, got "
                         f"{buf.dtype} (uint8 bytes at depth 8, uint16 words with depth= above 8)")
    if buf.shape[-1] != need:
        unit = "bytes" if buf.dtype in (np.uint8, torch.uint8) else "uint16 words"
        raise ValueError(f"split_yuv: a {W}x{H} {layout} frame is {need} {unit}, the buffer has {buf.shape[-1]}")
    sx, sy = _YUV_SUB[layout]
    ch, cw = (H + sy - 1) // sy, (W + sx - 1) // sx
    lead = tuple(buf.shape[:-1])

    def view(a, shape):
        return a.reshape(lead + shape) if is_np else a.view(lead + shape)

    if not is_np and buf.stride(-1) != 1:
        raise ValueError("split_yuv: the buffer's bytes must be contiguous (views are returned, not copies)")
    y = view(buf[..., :H * W], (H, W))
    if layout in ("nv12", "nv21"):
        uv = view(buf[..., H * W:], (ch, cw, 2))
        a, b = uv[..., 0], uv[..., 1]
    else:
        a = view(buf[..., H * W:H * W + ch * cw], (ch, cw))
        b = view(buf[..., H * W + ch * cw:], (ch, cw))
    if is_np and not all(np.shares_memory(v, buf) for v in (y, a, b)):
        raise ValueError("split_yuv: the buffer cannot be viewed in place (make it contiguous)")
    return (y, b, a) if layout in ("yv12", "nv21") else (y, a, b)


def _yuv_planes(y, cb, cr, fmt: YuvFormat, what: str):
    """-> three 3-dim tensors [B,H,W], [B,ch,cw], [B,ch,cw] (one frame gains the batch dimension) of the format's
    sample type: uint8 at depth 8, uint16 above."""
    out = []
    for name, t in (("y", y), ("cb", cb), ("cr", cr)):
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(t if t.flags.writeable else t.copy())
        if not torch.is_tensor(t) or t.dtype != fmt.dtype or t.dim() not in (2, 3):
            kind = "uint8" if fmt.depth == 8 else "uint16"
            raise ValueError(f"{what}: {name} must be a {kind} tensor or array [B,h,w] (or one [h,w]) for a format of "
                             f"depth {fmt.depth}; bit depths above 8 are uint16 planes with YuvFormat(depth=)")
        out.append(t.unsqueeze(0) if t.dim() == 2 else t)
    y, cb, cr = out
    if 0 in y.shape:
        raise ValueError(f"{what}: empty frame {tuple(y.shape)}")
    B, H, W = y.shape
    want = (B,) + fmt.chroma_size(H, W)
    if tuple(cb.shape) != want or tuple(cr.shape) != want:
        raise ValueError(f"{what}: a {H} x {W} frame with sub={fmt.sub} has chroma planes {want}, got "
                         f"{tuple(cb.shape)} and {tuple(cr.shape)}")
    if len({t.device for t in out}) != 1:
        raise ValueError(f"{what}: the three planes must be on one device")
    return y, cb, cr


def _k32(fmt: YuvFormat, depth: Optional[int] = None):
    return {k: torch.tensor(v, dtype=torch.float32) for k, v in fmt.constants(depth).items()}


def yuv_upsample16(c: torch.Tensor, H: int, W: int, fmt: YuvFormat) -> torch.Tensor:
    """One chroma plane [B,ch,cw] (integers) on the luma grid, in sixteenths: int32 [B,H,W] in [0, 16 maxv].  Across
    columns of a subsampled axis with i = x >> 1 and indices clamped: centre siting 3 C[i] + C[i -+ 1] (- at even
    x), left siting 4 C[i] at even x and 2 C[i] + 2 C[i + 1] at odd x; down rows the centre rule; an unsubsampled
    axis contributes the factor 4.  The ingest kernel's integer step, restated."""
    c = c.to(torch.int32)
    ch, cw = c.shape[-2:]
    if fmt.sub[0] == 2:
        x = torch.arange(W)
        i, odd = x >> 1, (x & 1).bool()
        if fmt.left:
            nb = torch.where(odd, (i + 1).clamp(max=cw - 1), i)
            wa, wb = torch.where(odd, 2, 4).to(torch.int32), torch.where(odd, 2, 0).to(torch.int32)
        else:
            nb = (i + torch.where(odd, 1, -1)).clamp(0, cw - 1)
            wa, wb = torch.full((W,), 3, dtype=torch.int32), torch.ones(W, dtype=torch.int32)
        h = wa * c[..., i] + wb * c[..., nb]
    else:
        h = 4 * c
    if fmt.sub[1] == 2:
        yy = torch.arange(H)
        j, odd = yy >> 1, (yy & 1).bool()
        nb = (j + torch.where(odd, 1, -1)).clamp(0, ch - 1)
        return 3 * h[..., j, :] + h[..., nb, :]
    return 4 * h


def _ingest_yuv_cpu(y, cb, cr, fmt: YuvFormat) -> torch.Tensor:
    B, H, W = y.shape
    k = _k32(fmt)
    u = yuv_upsample16(cb, H, W, fmt).float() * 0.0625 - 128.0  # exact
    v = yuv_upsample16(cr, H, W, fmt).float() * 0.0625 - 128.0
    a = k["cy"] * (y.float() - k["yo"])
    r = a + k["crv"] * v
    g = (a - k["cgu"] * u) - k["cgv"] * v
    b = a + k["cbu"] * u
    out = torch.zeros(B, 3, _pad64(H), _pad64(W), dtype=torch.float32)
    out[:, :, :H, :W] = torch.stack([r, g, b], 1).clamp(0, 1)
    return out


def _ingest_yuv16_cpu(y, cb, cr, fmt: YuvFormat, depth: int, msb: bool) -> torch.Tensor:
    """The restatement of mlic_image_ingest_yuv16: _ingest_yuv_cpu on the samples of uint16 words, with half =
    2^(depth-1) in place of 128 and the constants of that depth.  Takes depth 8 too (the words are then bytes
    widened), where it gives _ingest_yuv_cpu's bits."""
    B, H, W = y.shape
    k = _k32(fmt, depth)
    half = float(1 << (depth - 1))
    ys, cbs, crs = (samples_of_words(t, depth, msb) for t in (y, cb, cr))
    u = yuv_upsample16(cbs, H, W, fmt).float() * 0.0625 - half  # exact: sixteenths below 2^20
    v = yuv_upsample16(crs, H, W, fmt).float() * 0.0625 - half
    a = k["cy"] * (ys.float() - k["yo"])
    r = a + k["crv"] * v
    g = (a - k["cgu"] * u) - k["cgv"] * v
    b = a + k["cbu"] * u
    out = torch.zeros(B, 3, _pad64(H), _pad64(W), dtype=torch.float32)
    out[:, :, :H, :W] = torch.stack([r, g, b], 1).clamp(0, 1)
    return out


def ingest_yuv(y, cb, cr, fmt: YuvFormat) -> torch.Tensor:
    """A Y'CbCr frame batch (uint8 planes at fmt.depth 8, uint16 words above: mlic_image_ingest_yuv16, with 128 ->
    2^(depth-1) and the constants of that depth) -> the model's input, contiguous fp32 [B,3,Hp,Wp], in one launch: y uint8
    [B,H,W], cb and cr uint8 [B,ceil(H / sub_y),ceil(W / sub_x)] (or one frame without B), each with any strides
    (split_yuv's views of an I420 / NV12 buffer, a row-padded pitch, a crop are read in place).  Chroma is
    upsampled in integers (yuv_upsample16), then a = cy (Y - yo); R = a + crv v; G = (a - cgu u) - cgv v;
    B = a + cbu u in fp32 with every operation rounded once, clamped to [0, 1]; +0 in the padding.  There is no
    intermediate 8-bit RGB.  CUDA tensors run the kernel on the current stream, CPU tensors the torch restatement
    (the same bits)."""
    fmt = _check_fmt(fmt, "ingest_yuv")
    y, cb, cr = _yuv_planes(y, cb, cr, fmt, "ingest_yuv")
    B, H, W = y.shape
    if not y.is_cuda:
        return _ingest_yuv_cpu(y, cb, cr, fmt) if fmt.depth == 8 else _ingest_yuv16_cpu(y, cb, cr, fmt, fmt.depth, fmt.msb)
    if fmt.depth == 8:
        y, cb, cr = (t.contiguous() if t.stride(2) == 0 else t for t in (y, cb, cr))
    else:
        y, cb, cr = (_dense_u16(t, (2,)) for t in (y, cb, cr))
    Hp, Wp = _pad64(H), _pad64(W)
    with torch.cuda.device(y.device):
        x = torch.empty(B, 3, Hp, Wp, dtype=torch.float32, device=y.device)
        if _lib.poison():
            x.fill_(float("nan"))
        d = fmt.desc()
        if fmt.depth == 8:
            _lib.call("mlic_image_ingest_yuv8", _stream(), *_plane_args(y, cb, cr), C.byref(d), B, H, W,
                      C.c_void_p(x.data_ptr()), Hp, Wp)
        else:
            _lib.call("mlic_image_ingest_yuv16", _stream(), *_plane_args(y, cb, cr), C.byref(d), fmt.depth, int(fmt.msb),
                      B, H, W, C.c_void_p(x.data_ptr()), Hp, Wp)
    return x


def _plane_args(*planes):
    out = []
    for t in planes:
        out += [C.c_void_p(t.data_ptr()), (C.c_int64 * 3)(*t.stride())]
    return out


def _yuv_of_rgb(x: torch.Tensor, fmt: YuvFormat, depth: Optional[int] = None):
    """fp32 [B,3,H,W] -> (t_Y, t_Cb, t_Cr) at full resolution, chroma without the 128: the egress kernel's order."""
    k = _k32(fmt, depth)
    x = torch.where(torch.isnan(x), torch.zeros_like(x), x).clamp(0, 1)
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    ty = (k["yo"] + (k["yr"] * r + k["yg"] * g)) + k["yb"] * b
    tb = (k["br"] * r + k["bg"] * g) + k["bb"] * b
    tr = (k["rr"] * r + k["rg"] * g) + k["rb"] * b
    return ty, tb, tr


def yuv_downsample(t: torch.Tensor, fmt: YuvFormat) -> torch.Tensor:
    """Full-resolution fp32 chroma [B,H,W] -> [B,ch,cw], the egress kernel's filter: centre siting the mean of the
    sub_x x sub_y block, left siting [1 2 1] / 4 across columns 2 i - 1, 2 i, 2 i + 1 and the mean down the rows;
    indices clamped into the image; the sum runs row-major from the first term, each sum rounded once."""
    sx, sy = fmt.sub
    if sx == 1:
        return t.clone()
    H, W = t.shape[-2:]
    ch, cw = fmt.chroma_size(H, W)
    i, j = torch.arange(cw), torch.arange(ch)
    cols = [((2 * i + e).clamp(0, W - 1), 2.0 if (fmt.left and e == 0) else 1.0) for e in ((-1, 0, 1) if fmt.left else (0, 1))]
    rows = [(sy * j + r).clamp(max=H - 1) for r in range(sy)]
    acc = None
    for rr in rows:
        line = t[..., rr, :]
        for cc, w in cols:
            term = w * line[..., cc]
            acc = term if acc is None else acc + term
    return acc * ((0.25 if fmt.left else 1.0 / sx) / sy)


def _yuv_byte(t: torch.Tensor) -> torch.Tensor:
    return (t + 0.5).clamp(0, 255).floor().to(torch.uint8)


def _egress_yuv16_cpu(x: torch.Tensor, fmt: YuvFormat, depth: int):
    """The restatement of mlic_image_egress_yuv16 up to the samples: fp32 [B,3,H,W] -> int32 (y, cb, cr) samples in
    [0, 2^depth - 1] (words_of_samples makes the words).  At depth 8 these are egress_yuv's bytes."""
    maxv, half = float((1 << depth) - 1), float(1 << (depth - 1))
    ty, tb, tr = _yuv_of_rgb(x, fmt, depth)

    def sample(t):
        return (t + 0.5).clamp(0, maxv).floor().to(torch.int32)

    return sample(ty), sample(yuv_downsample(tb, fmt) + half), sample(yuv_downsample(tr, fmt) + half)


def egress_yuv(x_hat: torch.Tensor, H: int, W: int, fmt: YuvFormat, ref=None, out=None):
    """The top-left H x W crop of fp32 [B,3,>=H,>=W] (a padded x_hat, read in place) -> (y, cb, cr): uint8 [B,H,W]
    and two [B,ceil(H / sub_y),ceil(W / sub_x)], in one launch.  Per pixel the clamped r, g, b (a NaN is 0) give
    t_Y and the full-resolution chroma; chroma is filtered at luma resolution before rounding (yuv_downsample), 128
    is added, and floor(clamp(t + 0.5, 0, 255)) is the byte.  out: optional (y, cb, cr) uint8 tensors of those
    shapes with any strides (split_yuv's views of an NV12 buffer, windows of larger canvases): only the planes'
    bytes are written.  ref: (y, cb, cr) of the original, any strides: returns (y, cb, cr, sq_err) with sq_err
    int64 [B,3], the exact per-plane sums of squared byte differences.  CUDA tensors run the kernel on the current
    stream, CPU tensors the torch restatement (the same bits).  A format of depth > 8 gives uint16 words
    (mlic_image_egress_yuv16: 2^(depth-1) in place of 128, 2^depth - 1 in place of 255, shifted up for msb) and takes
    uint16 out / ref planes; sq_err then sums squared sample differences."""
    fmt = _check_fmt(fmt, "egress_yuv")
    if not torch.is_tensor(x_hat) or x_hat.dim() != 4 or x_hat.size(1) != 3 or x_hat.dtype != torch.float32:
        raise ValueError("egress_yuv: fp32 [B,3,h,w] expected")
    B = x_hat.size(0)
    H, W = int(H), int(W)
    if not (1 <= H <= x_hat.size(2) and 1 <= W <= x_hat.size(3)) or B < 1:
        raise ValueError(f"egress_yuv: crop {H} x {W} of {tuple(x_hat.shape)}")
    ch, cw = fmt.chroma_size(H, W)
    shapes = ((B, H, W), (B, ch, cw), (B, ch, cw))
    dev = x_hat.device
    if out is None:
        if fmt.depth == 8:
            out = tuple(torch.empty(s, dtype=torch.uint8, device=dev) for s in shapes)
        else:  # uint16 is only moved and viewed on the device: allocate (and poison) as int16
            out = tuple(torch.empty(s, dtype=torch.int16, device=dev) for s in shapes)
        if x_hat.is_cuda and _lib.poison():
            for t in out:
                t.fill_(0xFF if fmt.depth == 8 else -1)
        if fmt.depth > 8:
            out = tuple(t.view(torch.uint16) for t in out)
    else:
        out = tuple(out)
        if len(out) != 3 or any(not torch.is_tensor(t) or t.dtype != fmt.dtype or tuple(t.shape) != s or t.device != dev
                                for t, s in zip(out, shapes)):
            raise ValueError(f"egress_yuv: out must be three {'uint8' if fmt.depth == 8 else 'uint16'} tensors "
                             f"{shapes} on {dev}")
    if ref is not None:
        ref = _yuv_planes(*ref, fmt, "egress_yuv ref")
        if tuple(ref[0].shape) != shapes[0]:
            raise ValueError(f"egress_yuv: ref must be a frame batch of {shapes[0]}, got {tuple(ref[0].shape)}")
        ref = tuple(t.to(dev) for t in ref)
    if not x_hat.is_cuda and fmt.depth > 8:
        smp = _egress_yuv16_cpu(x_hat[:, :, :H, :W], fmt, fmt.depth)
        for o, v in zip(out, smp):
            o.copy_(words_of_samples(v, fmt.depth, fmt.msb))
        if ref is None:
            return out
        sq = torch.stack([((v.to(torch.int64) - samples_of_words(r, fmt.depth, fmt.msb).to(torch.int64)) ** 2)
                          .flatten(1).sum(1) for v, r in zip(smp, ref)], 1)
        return out + (sq,)
    if not x_hat.is_cuda:
        ty, tb, tr = _yuv_of_rgb(x_hat[:, :, :H, :W], fmt)
        out[0].copy_(_yuv_byte(ty))
        out[1].copy_(_yuv_byte(yuv_downsample(tb, fmt) + 128.0))
        out[2].copy_(_yuv_byte(yuv_downsample(tr, fmt) + 128.0))
        if ref is None:
            return out
        sq = torch.stack([((o.to(torch.int64) - r.to(torch.int64)) ** 2).flatten(1).sum(1) for o, r in zip(out, ref)], 1)
        return out + (sq,)
    if x_hat.stride(3) != 1:
        x_hat = x_hat.contiguous()
    if any(t.stride(2) == 0 for t in out):
        raise ValueError("egress_yuv: an out plane has a zero column stride")
    with torch.cuda.device(dev):
        sq = None
        if ref is not None:
            ref = tuple(t.contiguous() if t.stride(2) == 0 else t for t in ref) if fmt.depth == 8 else \
                tuple(_dense_u16(t, (2,)) for t in ref)
            sq = torch.full((B, 3), -1, dtype=torch.int64, device=dev)
        d = fmt.desc()
        rargs = [None] * 6 if ref is None else _plane_args(*ref)
        if fmt.depth == 8:
            _lib.call("mlic_image_egress_yuv8", _stream(), C.c_void_p(x_hat.data_ptr()),
                      (C.c_int64 * 3)(*x_hat.stride()[:3]), B, H, W, C.byref(d), *_plane_args(*out), *rargs,
                      None if sq is None else C.c_void_p(sq.data_ptr()))
        else:
            _lib.call("mlic_image_egress_yuv16", _stream(), C.c_void_p(x_hat.data_ptr()),
                      (C.c_int64 * 3)(*x_hat.stride()[:3]), B, H, W, C.byref(d), fmt.depth, int(fmt.msb),
                      *_plane_args(*out), *rargs, None if sq is None else C.c_void_p(sq.data_ptr()))
        if ref is not None:
            for t in ref:
                t.record_stream(torch.cuda.current_stream())
    return out if ref is None else out + (sq,)


def psnr_yuv_from_sq_err(sq_err, H: int, W: int, fmt: YuvFormat) -> Dict:
    """{"sq_err", "psnr_y", "psnr_u", "psnr_v", "psnr_yuv"} from the three per-plane sums of squared sample
    differences of an H x W frame: PSNR per plane (peak 2^depth - 1: 255 at depth 8) and the 6 : 1 : 1 mean
    (6 Y + U + V) / 8."""
    ch, cw = fmt.chroma_size(H, W)
    sq = [int(v) for v in sq_err]
    py, pu, pv = (psnr_from_sq_err(s, n, fmt.maxv) for s, n in zip(sq, (H * W, ch * cw, ch * cw)))
    return {"sq_err": sq, "psnr_y": py, "psnr_u": pu, "psnr_v": pv, "psnr_yuv": (6.0 * py + pu + pv) / 8.0}


@torch.no_grad()
def encode_yuv(net, y, cb, cr, fmt: YuvFormat, level=None, max_bpp: Optional[float] = None, max_passes: int = 8,
               return_info: bool = False, roi=None, roi_levels=None, tile=None, coded_size=None, scale=None,
               layered: bool = False, max_error=None):
    """encode_images with the Y'CbCr ingest: a frame batch (ingest_yuv's planes; host arrays cross to the device as
    bytes) -> one file per frame.  The files are plain per-image files: nothing of fmt is written, decode_images
    decodes them to RGB and decode_yuv(fmt) to planes.  level, max_bpp, max_passes and return_info as in
    encode_images (the rate loop works on the float image, so a budget and level="auto" work unchanged).  roi= and
    tile= are refused: ROI and tiled coding together with Y'CbCr frames are out of scope, and so is layered=.  The planes follow the
    format's depth: uint8 at depth 8, uint16 words above (a P010 frame: YuvFormat(depth=10, msb=True))."""
    fmt = _check_fmt(fmt, "encode_yuv")
    if roi is not None or roi_levels is not None:
        raise ValueError("encode_yuv: roi= together with Y'CbCr frames is not supported")
    if tile is not None:
        raise ValueError("encode_yuv: tiles together with Y'CbCr frames are not supported")
    _refuse_scaled("encode_yuv", "Y'CbCr frames", coded_size, scale)
    _refuse_residual("encode_yuv", **{"Y'CbCr frames": max_error is not None})
    if layered:
        raise ValueError("encode_yuv: layered=True together with Y'CbCr frames is not supported (encode_images writes "
                         "layered files)")
    y, cb, cr = _yuv_planes(y, cb, cr, fmt, "encode_yuv")
    _check_budget(max_bpp, max_passes)
    if isinstance(level, str) and max_bpp is None:
        raise ValueError("level='auto' needs max_bpp (the level is chosen from the budget)")
    B, H, W = y.shape
    x = ingest_yuv(y.to(net.device), cb.to(net.device), cr.to(net.device), fmt)
    if max_bpp is None:
        lv, kw = _levels(net, level, B)
        out = net.compress(x, **kw)
        ys, zs = out["strings"]
        files = [write_container(H, W, out["shape"], ys[b], zs[b], None if lv is None else lv[b]) for b in range(B)]
        passes = [0] * B
    else:
        files, passes, lv = rate_loop(net, x, H, W, level, max_bpp, max_passes)
    if not return_info:
        return files
    info = []
    for b, f in enumerate(files):
        bpp = 8.0 * len(f) / (H * W)
        info.append({"bytes": len(f), "bpp": bpp, "passes": passes[b], "level": None if lv is None else lv[b],
                     "met": max_bpp is None or bpp <= max_bpp})
    return files, info


@torch.no_grad()
def decode_yuv(net, files: Sequence[bytes], fmt: YuvFormat, ref=None, max_pixels: int = MAX_PIXELS, out_size=None,
               slices=None, enhance: bool = True, residual_coder: str = "device"):
    """Files of one H x W -> ((y, cb, cr) on the model's device, info): decode_images with the Y'CbCr egress.
    info[b] holds H, W, level, bytes and bpp and, with ref=(y, cb, cr) of the originals, sq_err (three ints: Y, Cb,
    Cr), psnr_y, psnr_u, psnr_v and psnr_yuv = (6 Y + U + V) / 8 (peak 2^depth - 1).  The planes are uint8 for a
    format of depth 8 and uint16 words above; the file does not know its depth.  ROI, tiled and layered files and
    slices= are refused.  "MLR4" files (encode_residual_yuv's) decode through the residual layer: the planes are the
    input samples exactly at max_error 0 and within it otherwise, info gains encode_residual_yuv's fields and, with
    ref, "max_abs_err"; an fmt whose depth, sub, matrix, range or siting differ from the file's is refused by the
    field's name; enhance=False gives the base planes alone; a mix of residual and plain files is refused."""
    fmt = _check_fmt(fmt, "decode_yuv")
    files = [bytes(f) for f in files]
    if not files:
        raise ValueError("decode_yuv: no files")
    res = [is_residual_yuv_file(f) for f in files]
    if any(res):
        if not all(res):
            raise ValueError("decode_yuv: residual (MLR4) and plain files cannot be mixed in one call")
        if out_size is not None or slices is not None:
            raise ValueError("decode_yuv: out_size= / slices= together with residual (MLR4) files are not supported")
        if not isinstance(enhance, (bool, np.bool_)):
            raise ValueError(f"decode_yuv: enhance must be a bool, got {enhance!r}")
        return _decode_residual_yuv(net, files, fmt, ref, max_pixels, bool(enhance),
                                    _check_coder(residual_coder, "decode_yuv"))
    if any(is_tiled_file(f) for f in files):
        raise ValueError("decode_yuv: tiled files together with Y'CbCr frames are not supported")
    if slices is not None or any(is_layered_file(f) for f in files):
        raise ValueError("decode_yuv: slices= / layered files together with Y'CbCr frames are not supported "
                         "(decode_images decodes them)")
    _refuse_scaled("decode_yuv", "Y'CbCr frames", out_size, True if any(is_scaled_file(f) for f in files) else None)
    vbr = hasattr(net, "levels")
    if vbr and any(is_roi_file(f) for f in files):
        raise ValueError("decode_yuv: ROI files together with Y'CbCr frames are not supported")
    cs = [parse_container(f, vbr, net.levels if vbr else None, max_pixels) for f in files]
    if len({(c.H, c.W) for c in cs}) != 1:
        raise ValueError(f"decode_yuv: the files must share one size, got {sorted({(c.H, c.W) for c in cs})}")
    H, W = cs[0].H, cs[0].W
    pairs = [_strings(f, c) for f, c in zip(files, cs)]
    kw = {"s": [c.level for c in cs]} if vbr else {}
    x_hat = net.decompress([[p[0] for p in pairs], [p[1] for p in pairs]], (cs[0].hz, cs[0].wz), **kw)["x_hat"]
    r = egress_yuv(x_hat.float(), H, W, fmt, ref=ref)
    sq = None if ref is None else r[3].cpu().tolist()
    info = []
    for b, c in enumerate(cs):
        d = {"H": c.H, "W": c.W, "level": c.level if vbr else None, "bytes": len(files[b]),
             "bpp": 8.0 * len(files[b]) / (c.H * c.W)}
        if sq is not None:
            d.update(psnr_yuv_from_sq_err(sq[b], H, W, fmt))
        info.append(d)
    return tuple(r[:3]), info

# ---- residual coding of Y'CbCr frames (csrc/residual_yuv.h, csrc/residual_yuv.hip; DESIGN.md §5 "Y'CbCr frames")
RESIDUAL_YUV_MAGIC = b"MLR4"


def is_residual_yuv_file(data: bytes) -> bool:
    return bytes(data[:4]) == RESIDUAL_YUV_MAGIC


def _check_shift_yuv(shift, depth: int, what: str) -> int:
    top = 0 if depth == 8 else depth - 7
    if isinstance(shift, bool) or not isinstance(shift, (int, np.integer)) or not 0 <= shift <= top:
        raise ValueError(f"{what}: shift must be an integer in [0, {top}] at depth {depth} (0 at depth 8, depth - 7 "
                         f"above), got {shift!r}")
    return int(shift)


def residual_yuv_geom(H: int, W: int, sub) -> Dict:
    """The sizes of one frame in the canonical order (csrc/residual_yuv.h): per plane "h", "w", "off" (the index of
    its first sample), "G" (64-column groups of a row) and "rowbase" (groups before its first row); "N" samples and
    "groups" (the low-bit plane has groups * shift 64-bit words)."""
    sx, sy = sub
    h = [H, -(-H // sy), -(-H // sy)]
    w = [W, -(-W // sx), -(-W // sx)]
    G = [-(-v // 64) for v in w]
    off, rowbase, o, r = [], [], 0, 0
    for p in range(3):
        off.append(o)
        rowbase.append(r)
        o += h[p] * w[p]
        r += h[p] * G[p]
    return {"h": h, "w": w, "off": off, "G": G, "rowbase": rowbase, "N": o, "groups": r}


def residual_yuv_samples(H: int, W: int, sub) -> int:
    """N = H W + 2 hc wc, the samples of one frame (mlic_residual_yuv_samples)."""
    n = C.c_uint64()
    _lib.call("mlic_residual_yuv_samples", int(H), int(W), int(sub[0]), int(sub[1]), C.byref(n))
    return n.value


def residual_yuv_plane_words(H: int, W: int, sub, shift: int) -> int:
    """64-bit words of one frame's low-bit plane: shift (H G_0 + 2 hc G_1) (mlic_residual_yuv_plane_words)."""
    n = C.c_uint64()
    _lib.call("mlic_residual_yuv_plane_words", int(H), int(W), int(sub[0]), int(sub[1]), int(shift), C.byref(n))
    return n.value


def _yuv_samples_np(planes, fmt: YuvFormat):
    """Three planes (any device) -> three int64 sample arrays [B,h,w]."""
    if fmt.depth == 8:
        return [t.cpu().numpy().astype(np.int64) for t in planes]
    return [samples_of_words(t.cpu(), fmt.depth, fmt.msb).numpy().astype(np.int64) for t in planes]


def _pack_plane_yuv_np(lo, shift: int) -> np.ndarray:
    """Three lo arrays int64 [B,h_p,w_p] -> the low-bit planes uint64 [B, groups * shift]: rows in canonical order,
    word (rowbase_p + y G_p + g) shift + j holds bit j of lo at bit x mod 64, zero beyond the plane's width."""
    B = lo[0].shape[0]
    bit = np.uint64(1) << np.arange(64, dtype=np.uint64)
    parts = []
    for v in lo:
        _, h, w = v.shape
        G = -(-w // 64)
        pad = np.zeros((B, h, 64 * G), np.uint64)
        pad[..., :w] = v.astype(np.uint64)
        pad = pad.reshape(B, h, G, 64)
        out = np.zeros((B, h, G, shift), np.uint64)
        for j in range(shift):
            out[..., j] = (((pad >> np.uint64(j)) & np.uint64(1)) * bit).sum(-1, dtype=np.uint64)
        parts.append(out.reshape(B, -1))
    return np.concatenate(parts, 1)


def _unpack_plane_yuv_np(plane: np.ndarray, geom: Dict, shift: int):
    """The inverse of _pack_plane_yuv_np: uint64 [B, groups * shift] -> three lo arrays int64 [B,h_p,w_p]."""
    B = plane.shape[0]
    out = []
    for p in range(3):
        h, w, G = geom["h"][p], geom["w"][p], geom["G"][p]
        if shift == 0:
            out.append(np.zeros((B, h, w), np.int64))
            continue
        a = geom["rowbase"][p] * shift
        words = plane[:, a:a + h * G * shift].reshape(B, h, G, shift, 1)
        bits = ((words >> np.arange(64, dtype=np.uint64).reshape(1, 1, 1, 1, 64)) & np.uint64(1)).astype(np.int64)
        lo = (bits << np.arange(shift, dtype=np.int64).reshape(1, 1, 1, shift, 1)).sum(3)
        out.append(lo.reshape(B, h, 64 * G)[..., :w])
    return out


def _residual_front_yuv_cpu(base, x, fmt: YuvFormat, tau: int, shift: int, stats: bool = False) -> Dict:
    """residual_front_yuv / residual_stats_yuv in NumPy integers: the definitions of csrc/residual_yuv.h written out."""
    d = fmt.depth
    b = _yuv_samples_np(base, fmt)
    B = b[0].shape[0]
    out = {}
    ctx = None
    if not stats:
        ctx = []
        for p, v in enumerate(b):
            h, w = v.shape[1:]
            pad = np.pad(v, ((0, 0), (1, 1), (1, 1)), mode="edge")
            win = [pad[:, dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)]
            a = (np.maximum.reduce(win) - np.minimum.reduce(win)) >> (d - 8)
            ctx.append((_CLASS_OF[a] + 8 * p).astype(np.uint8).reshape(B, -1))
        ctx = np.concatenate(ctx, 1)
        flat = np.concatenate([v.reshape(B, -1) for v in b], 1)
        count = np.stack([np.bincount(ctx[i], minlength=RES_CTX) for i in range(B)])
        with np.errstate(over="ignore"):
            wgt = np.arange(1, flat.shape[1] + 1, dtype=np.uint64) * np.uint64(_DIGEST_K)
            digest = ((flat + 1).astype(np.uint64) * wgt).sum(1, dtype=np.uint64)
        out = {"ctx": torch.from_numpy(ctx), "ctx_count": torch.from_numpy(count.astype(np.int64)),
               "digest": torch.from_numpy(digest.view(np.int64).copy())}
    if x is None:
        return out
    xv = _yuv_samples_np(x, fmt)
    step, maxv = 2 * tau + 1, fmt.maxv
    q = [np.sign(a - c) * ((np.abs(a - c) + tau) // step) for a, c in zip(xv, b)]
    aq = np.concatenate([np.abs(v).reshape(B, -1) for v in q], 1)
    out.update(max_abs_q=torch.from_numpy(aq.max(1)), sum_abs_q=torch.from_numpy(aq.sum(1)))
    if stats:
        return out
    rec = [np.clip(c + v * step, 0, maxv) for c, v in zip(b, q)]
    hi = [v >> shift for v in q]
    lo = [v - (u << shift) for v, u in zip(q, hi)]
    hif = np.concatenate([v.reshape(B, -1) for v in hi], 1)
    bins = np.where(np.abs(hif) <= RES_MAX_M, hif + RES_MAX_M, RES_BINS - 1)
    key = ctx.astype(np.int64) * RES_BINS + bins
    hist = np.stack([np.bincount(key[i], minlength=RES_CTX * RES_BINS) for i in range(B)])
    err = np.concatenate([np.abs(a - r).reshape(B, -1) for a, r in zip(xv, rec)], 1)
    out.update(sym=torch.from_numpy(np.clip(hif, -32768, 32767).astype(np.int16)),
               plane=torch.from_numpy(_pack_plane_yuv_np(lo, shift).view(np.int64).copy()),
               hist=torch.from_numpy(hist.reshape(B, RES_CTX, RES_BINS).astype(np.int64)),
               max_err=torch.from_numpy(err.max(1).astype(np.int64)))
    return out


def _residual_planes(base, x, fmt: YuvFormat, what: str):
    base = _yuv_planes(*base, fmt, f"{what} base")
    if x is not None:
        x = _yuv_planes(*x, fmt, f"{what} x")
        if tuple(x[0].shape) != tuple(base[0].shape):
            raise ValueError(f"{what}: x {tuple(x[0].shape)} does not match base {tuple(base[0].shape)}")
        if x[0].device != base[0].device:
            raise ValueError(f"{what}: base and x are on different devices")
    return base, x


def _planes_in_place(planes, fmt: YuvFormat):
    if fmt.depth == 8:
        return tuple(t.contiguous() if t.stride(2) == 0 else t for t in planes)
    return tuple(_dense_u16(t, (2,)) for t in planes)


def _yuv_entry(kind: str, fmt: YuvFormat):
    """(the entry's name, the depth arguments the 16-bit entry takes)."""
    return (f"mlic_image_residual_{kind}_yuv8", ()) if fmt.depth == 8 else \
        (f"mlic_image_residual_{kind}_yuv16", (fmt.depth, int(fmt.msb)))


def residual_front_yuv(base, x=None, fmt: Optional[YuvFormat] = None, tau: int = 0, shift: int = 0) -> Dict:
    """residual_front16 for the planes of Y'CbCr frames (csrc/residual_yuv.hip, one launch over the three planes of
    all frames; DESIGN.md §5 "Residual coding", "Y'CbCr frames").  base, x: (y, cb, cr) in the forms ingest_yuv
    takes (uint8 planes at fmt.depth 8, uint16 words above, any strides: dense, semi-planar views, pitched rows).
    Returns {"ctx" uint8 [B,N], "ctx_count" int64 [B,24], "digest" int64 [B]} in the canonical order (plane, row,
    column; N = H W + 2 hc wc) and, with x, {"sym" int16 [B,N] (hi, saturated), "plane" int64 [B, shift (H G_0 +
    2 hc G_1)], "hist" int64 [B,24,128], "max_err", "max_abs_q", "sum_abs_q" int64 [B]}.  The shift is 0 at depth 8.
    CPU tensors take the NumPy restatement (the same bits)."""
    what = "residual_front_yuv"
    fmt, tau = _check_fmt(fmt, what), _check_tau(tau, what)
    shift = _check_shift_yuv(shift, fmt.depth, what)
    base, x = _residual_planes(base, x, fmt, what)
    if not base[0].is_cuda:
        return _residual_front_yuv_cpu(base, x, fmt, tau, shift)
    B, H, W = base[0].shape
    N = residual_yuv_samples(H, W, fmt.sub)
    base = _planes_in_place(base, fmt)
    dev = base[0].device
    with torch.cuda.device(dev):
        if x is not None:
            x = _planes_in_place(x, fmt)
        o = _front_buffers(dev, (B, N), x is not None, residual_yuv_plane_words(H, W, fmt.sub, shift))
        name, deep = _yuv_entry("front", fmt)
        d = fmt.desc()
        _lib.call(name, _stream(), *_plane_args(*base), *([None] * 6 if x is None else _plane_args(*x)), C.byref(d),
                  *deep, B, H, W, tau, shift, _ptr(o["ctx"]), _ptr(o["count"]), _ptr(o["digest"]), _ptr(o["sym"]),
                  _ptr(o["plane"]), _ptr(o["hist"]), _ptr(o["merr"]), _ptr(o["mq"]), _ptr(o["sq"]))
        return _front_result(o)


def residual_stats_yuv(base, x, fmt: YuvFormat, tau: int = 0) -> Dict:
    """{"max_abs_q" int64 [B], "sum_abs_q" int64 [B]} of the quantised residual of the planes x against base: what the
    shift is chosen from (residual_shift with the frame's N), by a statistics launch of the front kernel."""
    what = "residual_stats_yuv"
    fmt, tau = _check_fmt(fmt, what), _check_tau(tau, what)
    if x is None:
        raise ValueError(f"{what}: x is needed")
    base, x = _residual_planes(base, x, fmt, what)
    if not base[0].is_cuda:
        return _residual_front_yuv_cpu(base, x, fmt, tau, 0, stats=True)
    B, H, W = base[0].shape
    base, x = _planes_in_place(base, fmt), _planes_in_place(x, fmt)
    dev = base[0].device
    with torch.cuda.device(dev):
        mq = torch.full((B,), -1, dtype=torch.int32, device=dev)
        sq = torch.full((B,), -1, dtype=torch.int64, device=dev)
        name, deep = _yuv_entry("stats", fmt)
        d = fmt.desc()
        _lib.call(name, _stream(), *_plane_args(*base), *_plane_args(*x), C.byref(d), *deep, B, H, W, tau,
                  C.c_void_p(mq.data_ptr()), C.c_void_p(sq.data_ptr()))
    return {"max_abs_q": mq.to(torch.int64), "sum_abs_q": sq}


def _residual_apply_yuv_cpu(base, sym, plane, fmt: YuvFormat, tau, shift, ref, out):
    b = _yuv_samples_np(base, fmt)
    B, H, W = b[0].shape
    geom = residual_yuv_geom(H, W, fmt.sub)
    hi = np.asarray(sym.cpu()).astype(np.int64).reshape(B, -1)
    bad = np.flatnonzero((np.abs(hi) > RES16_MAX_HI).any(1))
    if bad.size:
        raise ValueError(f"residual_apply_yuv: frame {int(bad[0])} holds a symbol outside [-255, 255]")
    lo = _unpack_plane_yuv_np(np.ascontiguousarray(plane.cpu().numpy()).view(np.uint64).reshape(B, -1), geom, shift)
    rec = []
    for p in range(3):
        h, w, o = geom["h"][p], geom["w"][p], geom["off"][p]
        q = (hi[:, o:o + h * w].reshape(B, h, w) << shift) + lo[p]
        rec.append(np.clip(b[p] + q * (2 * tau + 1), 0, fmt.maxv))
    if fmt.depth == 8:
        planes = tuple(torch.from_numpy(v.astype(np.uint8)) for v in rec)
    else:
        planes = tuple(words_of_samples(torch.from_numpy(v), fmt.depth, fmt.msb) for v in rec)
    if out is not None:
        for o, v in zip(out, planes):
            o.copy_(v)
        planes = tuple(out)
    if ref is None:
        return planes
    r = _yuv_samples_np(ref, fmt)
    d = [a - c for a, c in zip(rec, r)]
    sq = np.stack([(v * v).reshape(B, -1).sum(1) for v in d], 1)
    me = np.stack([np.abs(v).reshape(B, -1).max(1) for v in d], 1).max(1)
    return planes + (torch.from_numpy(sq), torch.from_numpy(me))


def residual_apply_yuv(base, sym, plane, fmt: YuvFormat, tau: int, shift: int, ref=None, out=None):
    """The Y'CbCr decoder's last pass (csrc/residual_yuv.hip, one launch): the three planes clamp(base + ((sym <<
    shift) + lo) (2 tau + 1), 0, 2^depth - 1) in fmt's word type and alignment, lo read from `plane` (int64 [B, shift
    (H G_0 + 2 hc G_1)], residual_front_yuv's).  sym: int16 [B,N], dense, on base's device; a sym outside [-255, 255]
    is refused (ValueError naming the frame).  out: optional (y, cb, cr) of the planes' shapes with any strides:
    only the planes' samples are written.  ref (y, cb, cr): returns (y, cb, cr, sq_err int64 [B,3], max_abs_err
    int64 [B]), exact.  CPU tensors take the NumPy restatement."""
    what = "residual_apply_yuv"
    fmt, tau = _check_fmt(fmt, what), _check_tau(tau, what)
    shift = _check_shift_yuv(shift, fmt.depth, what)
    base = _yuv_planes(*base, fmt, f"{what} base")
    B, H, W = base[0].shape
    dev = base[0].device
    N = residual_yuv_geom(H, W, fmt.sub)["N"]
    if not torch.is_tensor(sym) or sym.dtype != torch.int16 or tuple(sym.shape) != (B, N):
        raise ValueError(f"{what}: sym must be an int16 tensor {(B, N)}")
    words = residual_yuv_geom(H, W, fmt.sub)["groups"] * shift
    if not torch.is_tensor(plane) or plane.dtype != torch.int64 or tuple(plane.shape) != (B, words):
        raise ValueError(f"{what}: plane must be an int64 tensor {(B, words)}")
    if sym.device != dev or plane.device != dev:
        raise ValueError(f"{what}: base, sym and plane must be on one device")
    shapes = tuple(tuple(t.shape) for t in base)
    if out is not None:
        out = tuple(out)
        if len(out) != 3 or any(not torch.is_tensor(t) or t.dtype != fmt.dtype or tuple(t.shape) != s or t.device != dev
                                for t, s in zip(out, shapes)):
            raise ValueError(f"{what}: out must be three {'uint8' if fmt.depth == 8 else 'uint16'} tensors {shapes} "
                             f"on {dev}")
    if ref is not None:
        ref = _yuv_planes(*ref, fmt, f"{what} ref")
        if tuple(ref[0].shape) != shapes[0]:
            raise ValueError(f"{what}: ref must be a frame batch of {shapes[0]}, got {tuple(ref[0].shape)}")
        ref = tuple(t.to(dev) for t in ref)
    if not base[0].is_cuda:
        return _residual_apply_yuv_cpu(base, sym, plane, fmt, tau, shift, ref, out)
    base = _planes_in_place(base, fmt)
    sym, plane = sym.contiguous(), plane.contiguous()
    with torch.cuda.device(dev):
        if out is None:
            out = tuple(_apply_out(s, fmt.depth > 8, dev) for s in shapes)
        elif any(t.stride(2) == 0 for t in out):
            raise ValueError(f"{what}: an out plane has a zero column stride")
        if ref is not None:
            ref = _planes_in_place(ref, fmt)
        sq, merr, status = _apply_buffers(dev, B, ref, (B, 3))
        name, deep = _yuv_entry("apply", fmt)
        d = fmt.desc()
        _lib.call(name, _stream(), *_plane_args(*base), _ptr(sym), _ptr(plane), C.byref(d), *deep, B, H, W, tau, shift,
                  *_plane_args(*out), *([None] * 6 if ref is None else _plane_args(*ref)), _ptr(sq), _ptr(merr),
                  _ptr(status))
        _apply_refusal(what, "frame", status, () if ref is None else ref)
    return out if ref is None else out + (sq, merr.to(torch.int64))


def write_container_residual_yuv(H: int, W: int, inner: bytes, segs: bytes, seg_bytes, segment: int, tau: int,
                                 fmt: YuvFormat, shift: int, low: bytes, digest: int, m, freq, vbr: bool = False) -> bytes:
    """The Y'CbCr residual file (mlic_container_write_residual_yuv): "MLR4", the header and the tables of the "MLR2"
    file (H, W the luma size), depth, shift, sub_x, sub_y, matrix and the flags of `fmt`, seg_len, n_seg, `inner`,
    the index and `segs`, and behind lo_len the low-bit plane `low` (little-endian 64-bit words).  Whether the
    words are MSB-aligned is not written: the file holds samples."""
    inner, segs, low = bytes(inner), bytes(segs), bytes(low)
    fmt = _check_fmt(fmt, "write_container_residual_yuv")
    own = (fmt.depth, shift, fmt.sub[0], fmt.sub[1], _YUV_MATRIX[fmt.matrix][0], fmt.full_range, fmt.site_x == "left")
    return _write_residual("_yuv", H, W, vbr, tau, own, digest, m, freq, (segment, seg_bytes), (inner, segs, low))


def parse_container_residual_yuv(data: bytes, n_levels: Optional[int] = None,
                                 max_pixels: int = MAX_PIXELS) -> _lib.ContainerResidualYuvInfo:
    """The validating parser of a Y'CbCr residual file (mlic_container_parse_residual_yuv): raises _lib.MlicError on
    any malformed input.  The fields of the "MLR3" parse, and sub_x, sub_y, matrix, full_range, site_x (1: left)."""
    return _parse_residual("mlic_container_parse_residual_yuv", _lib.ContainerResidualYuvInfo(), data, n_levels,
                           max_pixels)


_YUV_MATRIX_NAME = {v[0]: k for k, v in _YUV_MATRIX.items()}


def _fmt_fields(fmt: YuvFormat) -> Dict:
    return {"depth": fmt.depth, "sub": fmt.sub, "matrix": fmt.matrix, "full_range": fmt.full_range,
            "site_x": fmt.site_x}


def _file_fmt_fields(s) -> Dict:
    return {"depth": int(s.depth), "sub": (int(s.sub_x), int(s.sub_y)), "matrix": _YUV_MATRIX_NAME[int(s.matrix)],
            "full_range": bool(s.full_range), "site_x": "left" if s.site_x else "centre"}


def residual_yuv_format(data: bytes, msb: bool = False, n_levels: Optional[int] = None,
                        max_pixels: int = MAX_PIXELS) -> YuvFormat:
    """The YuvFormat an "MLR4" file was written with; msb (the alignment of uint16 words) is the caller's."""
    f = _file_fmt_fields(parse_container_residual_yuv(data, n_levels, max_pixels))
    return YuvFormat(f["sub"], f["matrix"], f["full_range"], f["site_x"], f["depth"], bool(msb) and f["depth"] > 8)


def _yuv_kind(fmt: YuvFormat) -> _ResidualKind:
    """The kind of Y'CbCr frames ("MLR4"): a batch is the three planes, all frames of one size."""
    def check_ref(ref, B, H, W, dev):
        ref = _yuv_planes(*ref, fmt, "decode_yuv ref")
        if tuple(ref[0].shape) != (B, H, W):
            raise ValueError(f"decode_yuv: ref must be a frame batch of {(B, H, W)}, got {tuple(ref[0].shape)}")
        return tuple(t.to(dev) for t in ref)

    geoms = {}  # a call's frames share one size: its geometry is worked out once

    def geom_of(h, w):
        if (h, w) not in geoms:
            geoms[h, w] = residual_yuv_geom(h, w, fmt.sub)
        return geoms[h, w]

    def check_low(b, pl, h, w, sh):
        geom = geom_of(h, w)
        for p in range(3):
            wp, G, a = geom["w"][p], geom["G"][p], geom["rowbase"][p] * sh
            if sh and wp % 64 and (pl[a:a + geom["h"][p] * G * sh].reshape(geom["h"][p], G, sh)[:, -1, :]
                                   >> np.uint64(wp % 64)).any():
                raise ValueError(f"decode_yuv: file {b}: the low-bit plane has bits set beyond column {wp} of plane "
                                 f"{p} (its padding bits must be zero)")

    def apply(base, sym, plane, tau, sh, ref, out):
        r = residual_apply_yuv(base, sym, plane, fmt, tau, sh, ref=ref, out=out)
        return None if ref is None else r[3:]

    def paste(dst, alone):
        for t, v in zip(dst, alone):
            _copy_words(t, v)

    return _ResidualKind(
        entry="decode_yuv", noun="frame", base_word="base planes", low=True,
        front=lambda base, x, tau, sh: residual_front_yuv(base, x, fmt, tau, sh),
        stats=lambda base, x, tau: residual_stats_yuv(base, x, fmt, tau), apply=apply,
        decode_inner=lambda net, inner, ref, max_pixels: decode_yuv(net, inner, fmt, ref=ref, max_pixels=max_pixels),
        size=lambda planes: (planes[0].size(1), planes[0].size(2), planes[0].device),
        crop=lambda planes, sl, h=None, w=None: tuple(t[sl] for t in planes),
        paste=paste, canvas=lambda base, zero: tuple(_like(t, zero) for t in base), check_ref=check_ref,
        samples=lambda h, w: geom_of(h, w)["N"],
        plane_words=lambda h, w, sh: geom_of(h, w)["groups"] * sh, check_low=check_low,
        score=lambda sq, h, w: psnr_yuv_from_sq_err(sq, h, w, fmt),
        extra=lambda sh: {"depth": fmt.depth, "shift": sh, "sub": fmt.sub},
        write=lambda H, W, inner, segs, sb, L, tau, sh, low, digest, m, freq, vbr: write_container_residual_yuv(
            H, W, inner, segs, sb, L, tau, fmt, sh, low, digest, m, freq, vbr=vbr))


@torch.no_grad()
def encode_residual_yuv(net, y, cb, cr, fmt: YuvFormat, max_error: int = 0, level=None,
                        residual_segment: int = DEFAULT_RESIDUAL_SEGMENT, residual_shift: Optional[int] = None,
                        residual_coder: str = "device", return_info: bool = False, **refused):
    """Lossless (max_error=0) and near-lossless coding of Y'CbCr frames (DESIGN.md §5 "Residual coding", "Y'CbCr
    frames") -> one "MLR4" file per frame.  The planes are ingested and compressed exactly as encode_yuv does (the
    inner file is that file, byte for byte); the base planes are the decode of that file alone through egress_yuv
    with the same format.  Above depth 8 residual_stats_yuv gives max|q| and sum|q| per frame and the shift rule
    (residual_shift with the frame's N) or residual_shift= the split; residual_front_yuv gives the high parts with
    their contexts and histograms and the low-bit plane; the bound is checked on the device, the high parts go
    through residual_tables and residual_encode_segments, the low bits are stored raw.  Every sample of every plane
    comes back within max_error, samples outside the legal range included.  max_bpp, level="auto", roi, tile,
    scale / coded_size and layered are refused by name.  return_info=True: (files, info), info[b] as
    encode_residual16 gives it, plus "sub" and "depth"."""
    what = "encode_residual_yuv"
    fmt, tau = _check_fmt(fmt, what), _check_tau(max_error, what)
    names = {"max_bpp": "max_bpp=", "max_passes": "max_bpp=", "roi": "roi=", "roi_levels": "roi=", "tile": "tiles",
             "coded_size": "scaled coding", "scale": "scaled coding", "layered": "layered="}
    for k, v in refused.items():
        if k not in names:
            raise TypeError(f"{what}() got an unexpected keyword argument {k!r}")
        if v is not None and v is not False:
            raise ValueError(f"{what}: residual coding of Y'CbCr frames together with {names[k]} is not supported")
    if isinstance(level, str):
        raise ValueError(f"{what}: residual coding of Y'CbCr frames together with level='auto' is not supported")
    L, coder = _check_segment(residual_segment, what), _check_coder(residual_coder, what)
    depth = fmt.depth
    shift = residual_shift
    if shift is not None:
        shift = _check_shift_yuv(shift, depth, what)
    y, cb, cr = _yuv_planes(y, cb, cr, fmt, what)
    inner, info = encode_yuv(net, y, cb, cr, fmt, level=level, return_info=True)
    B, H, W = y.shape
    x_hat, vbr = _inner_x_hat(net, inner)
    base = egress_yuv(x_hat.float(), H, W, fmt)
    x = tuple(t.to(base[0].device) for t in (y, cb, cr))
    kind = _yuv_kind(fmt)
    if depth == 8:
        shifts = [0] * B
    else:
        shifts = _residual_shifts(what, "residual_shift", kind, depth, kind.samples(H, W), kind.stats(base, x, tau),
                                  shift, B)
    files, extra = _encode_residual_layer(kind, what, base, x, H, W, tau, shifts, L, coder, inner, vbr)
    for d, f, e in zip(info, files, extra):
        d.update(e, bytes=len(f), bpp=8.0 * len(f) / (H * W))
    return (files, info) if return_info else files


def _decode_residual_yuv(net, files, fmt: YuvFormat, ref, max_pixels, enhance, coder):
    """decode_yuv for "MLR4" files: the inner files decoded to base planes, then the residual layer."""
    want = _fmt_fields(fmt)

    def check(b, s):
        got = _file_fmt_fields(s)
        for k in ("depth", "sub", "matrix", "full_range", "site_x"):
            if k == "site_x" and got["sub"][0] == 1:
                continue  # the siting of an unsubsampled frame means nothing
            if got[k] != want[k]:
                raise ValueError(f"decode_yuv: file {b} (MLR4) was written with {k}={got[k]!r}, fmt has "
                                 f"{k}={want[k]!r}: the residual applies to the encoder's base planes only")

    ss = _parse_residual_files("decode_yuv", net, files, max_pixels, check)
    if len({(s.H, s.W) for s in ss}) != 1:
        raise ValueError(f"decode_yuv: the files must share one size, got {sorted({(s.H, s.W) for s in ss})}")
    return _decode_residual_layer(_yuv_kind(fmt), net, files, ss, ref, max_pixels, enhance, coder)


def psnr_from_sq_err(sq_err: int, n: int, peak: int = 255) -> float:
    """PSNR (utils/metrics.py:32-33; peak 255, or 2^depth - 1 for deeper samples) from a sum of squared sample
    differences over n values."""
    return 10.0 * math.log10(float(peak) ** 2 * n / sq_err) if sq_err > 0 else float("inf")
