"""Float64 oracle of MS-SSIM for the metric tests, written from the definition (pytorch_msssim's defaults,
data_range 255) and independently of mlic_amd/metrics.py: the 2-D 11x11 window (outer product of the
Gaussian) through one F.conv2d per level over all five moment inputs, explicit zero-pad-in-front 2x2 mean
pooling.  Also the test images: one base image and eight distortions of it."""
import numpy as np
import torch
import torch.nn.functional as F

from mlic_amd import synthetic

WEIGHTS = [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]
DISTORTIONS = ("same", "n2", "n8", "n32", "blur", "off", "scale", "inv")


def to_u8_f64(x: torch.Tensor) -> torch.Tensor:
    """The uint8 image the library scores (float32 clamp, * 255, truncation), as float64."""
    return (x.float().clamp(0, 1) * 255).to(torch.uint8).double()


def _pool(x: torch.Tensor) -> torch.Tensor:
    h, w = x.shape[-2:]
    x = F.pad(x, (w % 2, 0, h % 2, 0))  # an odd side gets one zero row / column in front
    h, w = x.shape[-2:]
    return x.reshape(*x.shape[:-2], h // 2, 2, w // 2, 2).sum((-3, -1)) / 4.0


def ms_ssim(a: torch.Tensor, b: torch.Tensor):
    """(value [B], terms [B, 5, C]) in float64 of two [B, C, H, W] images in [0, 1]."""
    assert a.shape == b.shape and a.dim() == 4 and min(a.shape[-2:]) > 160
    x, y = to_u8_f64(a.cpu()), to_u8_f64(b.cpu())
    B, C = x.shape[:2]
    k = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-k * k / (2 * 1.5 ** 2))
    g = g / g.sum()
    win = torch.outer(g, g).view(1, 1, 11, 11)
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    terms = []
    for level in range(5):
        h, w = x.shape[-2:]
        stack = torch.stack([x, y, x * x, y * y, x * y], 0).reshape(5 * B * C, 1, h, w)
        m = F.conv2d(stack, win).reshape(5, B, C, h - 10, w - 10)
        mu1, mu2 = m[0], m[1]
        s11, s22, s12 = m[2] - mu1 * mu1, m[3] - mu2 * mu2, m[4] - mu1 * mu2
        cs_map = (2 * s12 + c2) / (s11 + s22 + c2)
        if level < 4:
            terms.append(cs_map.mean((-2, -1)).clamp(min=0))
            x, y = _pool(x), _pool(y)
        else:
            ssim_map = (2 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1) * cs_map
            terms.append(ssim_map.mean((-2, -1)).clamp(min=0))
    t = torch.stack(terms, 1)  # [B, 5, C]
    wts = torch.tensor(WEIGHTS, dtype=torch.float64).view(1, 5, 1)
    return torch.prod(t ** wts, 1).mean(1), t


def distort(a: torch.Tensor, kind: str) -> torch.Tensor:
    gen = torch.Generator().manual_seed(20 + DISTORTIONS.index(kind))
    if kind == "same":
        return a
    if kind in ("n2", "n8", "n32"):
        return a + torch.randn(a.shape, generator=gen) * (int(kind[1:]) / 255.0)  # unclamped on purpose
    if kind == "blur":
        c = a.size(1)
        return F.conv2d(F.pad(a, (2, 2, 2, 2), mode="replicate"), torch.full((c, 1, 5, 5), 1 / 25.0), groups=c)
    if kind == "off":
        return a + 10 / 255.0
    if kind == "scale":
        return 0.7 * a
    if kind == "inv":
        return 1 - a
    raise KeyError(kind)


# name -> (H, W, C, storage H, storage W): a case whose storage is larger is taken as the view
# [:, :, :H, :W] of tensors of the storage size
SHAPES = {
    "161x161": (161, 161, 3, 161, 161),   # every level odd, padded pooling four times, 1x1 final map
    "176x208": (176, 208, 3, 176, 208),   # all-even chain ending at 11x13
    "180x250v": (180, 250, 3, 192, 256),  # 250 -> 125 -> 63 -> 32 -> 16, strided view
    "333x517": (333, 517, 3, 333, 517),   # several tiles per side, ragged edges
    "176x208c1": (176, 208, 1, 176, 208),  # single channel
}

_cache = {}
_storage = {}


def case(shape: str, kind: str):
    """(a, b, value [1], terms [1, 5, C]) of one parity case; computed once, shared, never modified."""
    key = (shape, kind)
    if key not in _cache:
        H, W, C, SH, SW = SHAPES[shape]
        fa = synthetic.synth_image(SH, SW, 3)[:, :C].contiguous()
        fb = distort(fa, kind).contiguous()
        a, b = fa[:, :, :H, :W], fb[:, :, :H, :W]
        v, t = ms_ssim(a, b)
        _cache[key] = (a, b, v, t)
        _storage[key] = (fa, fb)
    return _cache[key]


def on_device(shape: str, kind: str, dev):
    """The case's (a, b) on `dev` with the same strides: the storage-sized tensors are uploaded and the
    same view is taken there."""
    case(shape, kind)
    H, W = SHAPES[shape][:2]
    fa, fb = _storage[(shape, kind)]
    return fa.to(dev)[:, :, :H, :W], fb.to(dev)[:, :, :H, :W]
