"""Image quality metrics of the evaluation harness (utils/metrics.py:13-53, utils/testing.py:397-421).

MS-SSIM follows pytorch_msssim's `ms_ssim(X, Y, data_range=255)` defaults, restated: 11-tap
Gaussian window (sigma 1.5) applied separably as a valid convolution, C1 = (0.01*255)^2, C2 = (0.03*255)^2,
five levels with weights 0.0448, 0.2856, 0.3001, 0.2363, 0.1333, relu(cs) from levels 0-3 and relu(ssim)
from level 4, avg_pool2d(2, 2, padding = side % 2) between levels, mean over channels of the weighted
product.  Images are the uint8 images the harness scores: floor(clamp(v, 0, 1) * 255).

LPIPS follows `lpips.LPIPS(net="vgg", version="0.1")(a/255, b/255, normalize=True)` in eval mode, restated
(DESIGN.md §3): the uint8 images as v/255, t = 2v - 1, the ScalingLayer, VGG16's thirteen 3x3 convs with five taps
after the ReLUs of conv1_2, 2_2, 3_3, 4_3 and 5_3, unit-normalised over channels (eps 1e-10), the squared
difference weighted by the 1x1 `lin` layers, averaged over pixels and summed over the taps.

CUDA tensors run the fused HIP kernels (csrc/metrics.hip, csrc/lpips.hip) on the current stream; CPU tensors run
a float32 torch restatement, so the harness also works on a machine without a GPU.
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


# ---------------------------------------------------------------------------------------------------------
# LPIPS-VGG

LPIPS_MIN_SIDE = 16  # min(H, W) must reach it: four floor poolings leave tap 4 at least one pixel
LPIPS_FEATURES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)  # the convs' indices in vgg16().features
LPIPS_CIN = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512)
LPIPS_COUT = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
LPIPS_TAP_LAST = (1, 3, 6, 9, 12)  # tap k is the ReLU'd output of this conv; a 2x2 floor max-pool follows taps 0-3
LPIPS_TAP_C = (64, 128, 256, 512, 512)
LPIPS_SHIFT = (-0.030, -0.088, -0.188)
LPIPS_SCALE = (0.458, 0.448, 0.450)
_LPIPS_SLICE = (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)  # the package's net.slice{n} of each conv


def lpips_synthetic_weights(seed: int = 0):
    """Deterministic LPIPS-VGG weights in the `lpips` package's state_dict layout, for tests and benchmarks
    (not the trained ones): conv w ~ N(0, 2 / (9 Cin)), bias uniform in +-0.05, lin_k = U(0, 1) * 2 / C, the
    package's shift and scale."""
    gen = torch.Generator().manual_seed(int(seed))
    sd = {"scaling_layer.shift": torch.tensor(LPIPS_SHIFT).view(1, 3, 1, 1),
          "scaling_layer.scale": torch.tensor(LPIPS_SCALE).view(1, 3, 1, 1)}
    for idx, sl, cin, cout in zip(LPIPS_FEATURES, _LPIPS_SLICE, LPIPS_CIN, LPIPS_COUT):
        sd[f"net.slice{sl}.{idx}.weight"] = torch.randn(cout, cin, 3, 3, generator=gen) * math.sqrt(2.0 / (9 * cin))
        sd[f"net.slice{sl}.{idx}.bias"] = (torch.rand(cout, generator=gen) - 0.5) * 0.1
    for k, c in enumerate(LPIPS_TAP_C):
        sd[f"lin{k}.model.1.weight"] = torch.rand(1, c, 1, 1, generator=gen) * (2.0 / c)
    return sd


def _lpips_parse(weights):
    """The two accepted spellings -> {"convs": [(w, b)] * 13, "lins": [w] * 5, "shift", "scale"} of float32 CPU
    tensors.  One rule for both: a conv tensor is "<prefix.>IDX.weight|bias" with IDX its features index."""
    if isinstance(weights, (tuple, list)):
        if len(weights) != 2 or not isinstance(weights[0], dict):
            raise ValueError("LPIPS: weights must be a state_dict or (features_state_dict, [five lin tensors])")
        feats, lins = weights
        if len(lins) != 5:
            raise ValueError(f"LPIPS: five lin tensors expected, got {len(lins)}")
        weights = dict(feats)
        for k, t in enumerate(lins):
            weights[f"lin{k}.model.1.weight"] = t
    elif not isinstance(weights, dict):
        raise ValueError("LPIPS: weights must be a state_dict or (features_state_dict, [five lin tensors])")
    cw, cb, lw = [None] * 13, [None] * 13, [None] * 5
    shift = scale = None

    def shaped(name, t, want):
        if tuple(t.shape) != tuple(want):
            raise ValueError(f"LPIPS: tensor {name} has shape {tuple(t.shape)}, expected {tuple(want)}")
        return t.detach().to("cpu", torch.float32).contiguous().clone()

    for name, t in weights.items():
        if name.startswith("lins."):
            continue  # the package's duplicate of lin{k}
        if name in ("scaling_layer.shift", "scaling_layer.scale"):
            v = shaped(name, t, (1, 3, 1, 1))
            if name.endswith("shift"):
                shift = v
            else:
                scale = v
            continue
        if len(name) == 19 and name.startswith("lin") and name.endswith(".model.1.weight") and name[3] in "01234":
            k = int(name[3])
            lw[k] = shaped(name, t, (1, LPIPS_TAP_C[k], 1, 1))
            continue
        stem, _, kind = name.rpartition(".")
        idx = stem.rpartition(".")[2]
        if kind not in ("weight", "bias") or not idx.isdigit():
            raise ValueError(f"LPIPS: unexpected tensor {name}")
        if int(idx) not in LPIPS_FEATURES:
            raise ValueError(f"LPIPS: extra conv tensor {name} (VGG16 has no conv at features index {idx})")
        l = LPIPS_FEATURES.index(int(idx))
        slot = cw if kind == "weight" else cb
        if slot[l] is not None:
            raise ValueError(f"LPIPS: extra conv tensor {name} (features index {idx} given twice)")
        slot[l] = shaped(name, t, (LPIPS_COUT[l], LPIPS_CIN[l], 3, 3) if kind == "weight" else (LPIPS_COUT[l],))
    for l, idx in enumerate(LPIPS_FEATURES):
        if cw[l] is None:
            raise ValueError(f"LPIPS: missing tensor {idx}.weight")
        if cb[l] is None:
            raise ValueError(f"LPIPS: missing tensor {idx}.bias")
    for k in range(5):
        if lw[k] is None:
            raise ValueError(f"LPIPS: missing tensor lin{k}.model.1.weight")
    if (shift is None) != (scale is None):
        raise ValueError("LPIPS: missing tensor scaling_layer." + ("shift" if shift is None else "scale"))
    if shift is None:
        shift, scale = torch.tensor(LPIPS_SHIFT).view(1, 3, 1, 1), torch.tensor(LPIPS_SCALE).view(1, 3, 1, 1)
    return {"convs": list(zip(cw, cb)), "lins": lw, "shift": shift, "scale": scale}


def _lpips_cpu(a: torch.Tensor, b: torch.Tensor, w):
    def features(x):
        x = torch.floor(torch.nan_to_num(x.float(), nan=0.0).clamp(0, 1) * 255) / 255
        x = (2 * x - 1 - w["shift"]) / w["scale"]
        taps = []
        for l, (cw, cb) in enumerate(w["convs"]):
            if l and l - 1 in LPIPS_TAP_LAST:
                x = F.max_pool2d(x, 2, 2)
            x = torch.relu(F.conv2d(x, cw, cb, padding=1))
            if l in LPIPS_TAP_LAST:
                taps.append(x)
        return taps

    terms = []
    for fa, fb, lin in zip(features(a), features(b), w["lins"]):
        na = fa.square().sum(1, keepdim=True).sqrt()
        nb = fb.square().sum(1, keepdim=True).sqrt()
        d = (fa / (na + 1e-10) - fb / (nb + 1e-10)).square()
        terms.append((d * lin).sum(1).mean((1, 2)))
    t = torch.stack(terms, 1).double()  # [B, 5]
    return t.sum(1), t


class LPIPS:
    """LPIPS-VGG of uint8-valued images.  `weights`: a state_dict in the `lpips` package's layout
    (net.slice{n}.{idx}.weight|bias, lin{k}.model.1.weight, scaling_layer.shift|scale), or the pair
    (torchvision vgg16().features state_dict, [five lin tensors [1,C,1,1]]).  metric(a, b) -> [B] float64 on
    the inputs' device; CUDA tensors run the HIP library on the current stream (one handle per device, made at
    the first call), CPU tensors a float32 torch restatement."""

    def __init__(self, weights):
        self._w = _lpips_parse(weights)
        self._handles = {}
        self._precision = 2

    def _tensors(self):
        names, tensors = [], []
        for idx, (cw, cb) in zip(LPIPS_FEATURES, self._w["convs"]):
            names += [f"{idx}.weight", f"{idx}.bias"]
            tensors += [cw, cb]
        for k, t in enumerate(self._w["lins"]):
            names.append(f"lin{k}.model.1.weight")
            tensors.append(t)
        names += ["scaling_layer.shift", "scaling_layer.scale"]
        tensors += [self._w["shift"], self._w["scale"]]
        return names, tensors

    def _handle(self, dev: torch.device):
        key = str(dev)
        if key not in self._handles:
            names, tensors = self._tensors()
            h = lpips_create_handle(names, [t.to(dev) for t in tensors], dev)
            _lib.call("mlic_lpips_set_precision", h, self._precision)
            self._handles[key] = h
        return self._handles[key]

    def set_precision(self, precision: int):
        """2 = split-fp16 conv_x4 (default), 0 = the fp32 MFMA conv, for the twelve dense convs."""
        if precision not in (0, 2):
            raise ValueError("LPIPS: precision must be 2 (split-fp16) or 0 (fp32 MFMA)")
        self._precision = precision
        for h in self._handles.values():
            _lib.call("mlic_lpips_set_precision", h, precision)

    def range_fallbacks(self, reset: bool = False) -> int:
        """Calls the fp16 range guard re-ran with the fp32 convs, over this object's handles."""
        total = 0
        for h in self._handles.values():
            n = C.c_int64()
            _lib.call("mlic_lpips_range_fallbacks", h, C.byref(n), 1 if reset else 0)
            total += n.value
        return total

    def __call__(self, a: torch.Tensor, b: torch.Tensor, return_terms: bool = False):
        """Per-pair LPIPS [B] (float64) of two [B,3,H,W] float images in [0,1], scored as uint8 images; views
        with unit column stride are read in place.  return_terms=True returns (value, terms [B,5]): the five
        taps' terms the value is the sum of."""
        if a.dim() != 4 or a.shape != b.shape or a.size(1) != 3:
            raise ValueError(f"LPIPS: two [B,3,H,W] tensors of one shape expected, got {tuple(a.shape)} and "
                             f"{tuple(b.shape)}")
        if a.device != b.device:
            raise ValueError("LPIPS: the two images are on different devices")
        if min(a.shape[-2:]) < LPIPS_MIN_SIDE:
            raise ValueError(f"LPIPS: both image sides must be at least {LPIPS_MIN_SIDE} pixels, got "
                             f"{tuple(a.shape[-2:])}")
        if a.size(0) < 1:
            raise ValueError("LPIPS: empty batch")
        if not a.is_cuda:
            v, t = _lpips_cpu(a, b, self._w)
            return (v, t) if return_terms else v
        B, _, H, W = a.shape
        a, b = _strided(a), _strided(b)
        h = self._handle(a.device)
        nbytes = C.c_size_t()
        _lib.call("mlic_lpips_scratch_bytes", B, H, W, C.byref(nbytes))
        with torch.cuda.device(a.device):
            scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=a.device)
            out = torch.empty(B, dtype=torch.float64, device=a.device)
            terms = torch.empty(B, 5, dtype=torch.float64, device=a.device) if return_terms else None
            if _lib.poison():
                scratch.fill_(0xFF)
                out.fill_(float("nan"))
                if terms is not None:
                    terms.fill_(float("nan"))
            sa = (C.c_int64 * 3)(*a.stride()[:3])
            sb = (C.c_int64 * 3)(*b.stride()[:3])
            _lib.call("mlic_image_lpips_u8", h, C.c_void_p(torch.cuda.current_stream().cuda_stream),
                      C.c_void_p(a.data_ptr()), sa, C.c_void_p(b.data_ptr()), sb, B, H, W,
                      C.c_void_p(scratch.data_ptr()), nbytes.value, C.c_void_p(out.data_ptr()),
                      None if terms is None else C.c_void_p(terms.data_ptr()))
        return (out, terms) if return_terms else out

    def close(self):
        handles, self._handles = getattr(self, "_handles", {}), {}
        for h in handles.values():
            _lib.call("mlic_lpips_destroy", h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lpips_create_handle(names, tensors, dev: torch.device) -> C.c_void_p:
    """mlic_lpips_create on float32 tensors that live on `dev` (the raw ABI, for LPIPS and the tests)."""
    n = len(names)
    tensors = [t.contiguous() for t in tensors]
    arr_names = (C.c_char_p * n)(*[s.encode() for s in names])
    arr_ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in tensors])
    shapes = (C.c_int64 * sum(t.dim() for t in tensors))(*[d for t in tensors for d in t.shape])
    ndims = (C.c_int * n)(*[t.dim() for t in tensors])
    h = C.c_void_p()
    with torch.cuda.device(dev):
        _lib.call("mlic_lpips_create", n, arr_names, arr_ptrs, shapes, ndims,
                  C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(h))
    return h
