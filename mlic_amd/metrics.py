"""Image quality metrics of the evaluation harness (utils/metrics.py:13-53, utils/testing.py:397-421).

MS-SSIM follows pytorch_msssim's `ms_ssim(X, Y, data_range=255)` defaults, restated: 11-tap
Gaussian window (sigma 1.5) applied separably as a valid convolution, C1 = (0.01*255)^2, C2 = (0.03*255)^2,
five levels with weights 0.0448, 0.2856, 0.3001, 0.2363, 0.1333, relu(cs) from levels 0-3 and relu(ssim)
from level 4, avg_pool2d(2, 2, padding = side % 2) between levels, mean over channels of the weighted
product.  Images are the uint8 images the harness scores: floor(clamp(v, 0, 1) * 255).

CUDA tensors run the fused HIP kernels (csrc/metrics.hip) on the current stream; CPU tensors run a float32
torch restatement, so the harness also works on a machine without a GPU.
"""
from __future__ import annotations

import ctypes as C
import math

import torch
import torch.nn.functional as F

from . import _lib

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MIN_SIDE = 160  # min(H, W) must exceed it: (side - 1) // 2**4 >= 10 for the 11-tap window at level 4


def ms_ssim_db(v):
    """MS-SSIM in decibels, -10 log10(1 - v)."""
    if isinstance(v, torch.Tensor):
        return -10.0 * torch.log10(1.0 - v)
    return -10.0 * math.log10(1.0 - v)


def _check(a: torch.Tensor, b: torch.Tensor):
    if a.dim() != 4 or a.shape != b.shape:
        raise ValueError(f"ms_ssim_u8: two [B,C,H,W] tensors of one shape expected, got {tuple(a.shape)} and "
                         f"{tuple(b.shape)}")
    if a.device != b.device:
        raise ValueError("ms_ssim_u8: the two images are on different devices")
    if min(a.shape[-2:]) <= MIN_SIDE:
        raise ValueError(f"ms_ssim_u8: the smaller image side must exceed {MIN_SIDE} pixels, got "
                         f"{tuple(a.shape[-2:])}")
    if a.size(0) < 1 or a.size(1) < 1:
        raise ValueError("ms_ssim_u8: empty batch or no channels")


def _window() -> torch.Tensor:
    g = torch.exp(-(torch.arange(11, dtype=torch.float32) - 5) ** 2 / (2 * 1.5 ** 2))
    return g / g.sum()


def _blur(x: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    c = x.size(1)
    x = F.conv2d(x, g.view(1, 1, -1, 1).expand(c, 1, -1, 1), groups=c)
    return F.conv2d(x, g.view(1, 1, 1, -1).expand(c, 1, 1, -1), groups=c)


def _ms_ssim_cpu(a: torch.Tensor, b: torch.Tensor):
    x = torch.floor(a.float().clamp(0, 1) * 255)
    y = torch.floor(b.float().clamp(0, 1) * 255)
    g = _window()
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    terms = []
    for level in range(5):
        mu1, mu2 = _blur(x, g), _blur(y, g)
        s11 = _blur(x * x, g) - mu1 * mu1
        s22 = _blur(y * y, g) - mu2 * mu2
        s12 = _blur(x * y, g) - mu1 * mu2
        cs_map = (2 * s12 + c2) / (s11 + s22 + c2)
        if level < 4:
            terms.append(torch.relu(cs_map.flatten(2).mean(-1)))
            pad = (x.size(2) % 2, x.size(3) % 2)
            x, y = F.avg_pool2d(x, 2, 2, pad), F.avg_pool2d(y, 2, 2, pad)
        else:
            ssim_map = (2 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1) * cs_map
            terms.append(torch.relu(ssim_map.flatten(2).mean(-1)))
    t = torch.stack(terms, 1).double()  # [B, 5, C]
    w = torch.tensor(WEIGHTS, dtype=torch.float64).view(1, 5, 1)
    return torch.prod(t ** w, 1).mean(1), t


def _strided(t: torch.Tensor) -> torch.Tensor:
    t = t if t.dtype == torch.float32 else t.float()
    return t if t.stride(3) == 1 else t.contiguous()


def ms_ssim_u8(a: torch.Tensor, b: torch.Tensor, return_terms: bool = False):
    """Per-image MS-SSIM [B] (float64, on the inputs' device) of two [B,C,H,W] float images in [0,1],
    scored as uint8 images.  Views with unit column stride (a crop of a padded x_hat) are read in place.
    return_terms=True returns (value, terms): terms [B,5,C] float64 are the relu'd per-level per-channel
    means (cs of levels 0-3, ssim of level 4) the value is the weighted product of."""
    _check(a, b)
    if not a.is_cuda:
        v, t = _ms_ssim_cpu(a, b)
        return (v, t) if return_terms else v
    B, Cn, H, W = a.shape
    a, b = _strided(a), _strided(b)
    nbytes = C.c_size_t()
    _lib.call("mlic_ms_ssim_scratch_bytes", B, Cn, H, W, C.byref(nbytes))
    with torch.cuda.device(a.device):
        scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=a.device)
        out = torch.empty(B, dtype=torch.float64, device=a.device)
        terms = torch.empty(B, 5, Cn, dtype=torch.float64, device=a.device) if return_terms else None
        if _lib.poison():
            scratch.view(torch.float32).fill_(float("nan"))
            out.fill_(float("nan"))
            if terms is not None:
                terms.fill_(float("nan"))
        sa = (C.c_int64 * 3)(*a.stride()[:3])
        sb = (C.c_int64 * 3)(*b.stride()[:3])
        _lib.call("mlic_image_ms_ssim_u8", C.c_void_p(torch.cuda.current_stream().cuda_stream),
                  C.c_void_p(a.data_ptr()), sa, C.c_void_p(b.data_ptr()), sb, B, Cn, H, W,
                  C.c_void_p(scratch.data_ptr()), nbytes.value, C.c_void_p(out.data_ptr()),
                  None if terms is None else C.c_void_p(terms.data_ptr()))
    return (out, terms) if return_terms else out
