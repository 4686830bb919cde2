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

DISTS follows `DISTS_pytorch.DISTS()(a/255, b/255)` in eval mode, restated: the uint8 images as
v/255, (v - mean) / std, the same thirteen convs with the four max-pools replaced by L2 pooling (3x3 Hanning
window, stride 2, ceil grids), and per channel of six feature sets (the image and the five taps) the structure
term from the means and the texture term from the variances and the covariance, weighted by alpha and beta.

CUDA tensors run the fused HIP kernels (csrc/metrics.hip, csrc/lpips.hip, csrc/dists.hip) on the current stream;
CPU tensors run a float32 torch restatement, so the harness also works on a machine without a GPU.
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


class _VggMetric:
    """What LPIPS and DISTS share: one library handle per device (made at the first call), the call on the
    current stream with poison handling, the CPU restatement for CPU tensors.  A subclass sets NAME (the prefix
    of its messages), ABI (mlic_{ABI}_* entry points), TERMS (terms per pair), MIN_SIDE, and provides
    _parse(weights), _tensors() and _cpu(a, b)."""
    NAME = ABI = ""
    TERMS = MIN_SIDE = 0

    def __init__(self, weights):
        self._w = self._parse(weights)
        self._handles = {}
        self._precision = 2

    def _handle(self, dev: torch.device):
        key = str(dev)
        if key not in self._handles:
            names, tensors = self._tensors()
            h = _create_handle(self.ABI, names, [t.to(dev) for t in tensors], dev)
            _lib.call(f"mlic_{self.ABI}_set_precision", h, self._precision)
            self._handles[key] = h
        return self._handles[key]

    def set_precision(self, precision: int):
        """2 = split-fp16 conv_x4 (default), 0 = the fp32 MFMA conv, for the twelve dense convs."""
        if precision not in (0, 2):
            raise ValueError(f"{self.NAME}: precision must be 2 (split-fp16) or 0 (fp32 MFMA)")
        self._precision = precision
        for h in self._handles.values():
            _lib.call(f"mlic_{self.ABI}_set_precision", h, precision)

    def range_fallbacks(self, reset: bool = False) -> int:
        """Calls the fp16 range guard re-ran with the fp32 convs, over this object's handles."""
        total = 0
        for h in self._handles.values():
            n = C.c_int64()
            _lib.call(f"mlic_{self.ABI}_range_fallbacks", h, C.byref(n), 1 if reset else 0)
            total += n.value
        return total

    def __call__(self, a: torch.Tensor, b: torch.Tensor, return_terms: bool = False):
        """Per-pair value [B] (float64) of two [B,3,H,W] float images in [0,1], scored as uint8 images; views
        with unit column stride are read in place.  return_terms=True returns (value, terms [B,TERMS]): the
        terms the value is the sum of."""
        if a.dim() != 4 or a.shape != b.shape or a.size(1) != 3:
            raise ValueError(f"{self.NAME}: two [B,3,H,W] tensors of one shape expected, got {tuple(a.shape)} and "
                             f"{tuple(b.shape)}")
        if a.device != b.device:
            raise ValueError(f"{self.NAME}: the two images are on different devices")
        if min(a.shape[-2:]) < self.MIN_SIDE:
            raise ValueError(f"{self.NAME}: both image sides must be at least {self.MIN_SIDE} pixels, got "
                             f"{tuple(a.shape[-2:])}")
        if a.size(0) < 1:
            raise ValueError(f"{self.NAME}: empty batch")
        if not a.is_cuda:
            v, t = self._cpu(a, b)
            return (v, t) if return_terms else v
        B, _, H, W = a.shape
        a, b = _strided(a), _strided(b)
        h = self._handle(a.device)
        nbytes = C.c_size_t()
        _lib.call(f"mlic_{self.ABI}_scratch_bytes", B, H, W, C.byref(nbytes))
        with torch.cuda.device(a.device):
            scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=a.device)
            out = torch.empty(B, dtype=torch.float64, device=a.device)
            terms = torch.empty(B, self.TERMS, dtype=torch.float64, device=a.device) if return_terms else None
            if _lib.poison():
                scratch.fill_(0xFF)
                out.fill_(float("nan"))
                if terms is not None:
                    terms.fill_(float("nan"))
            sa = (C.c_int64 * 3)(*a.stride()[:3])
            sb = (C.c_int64 * 3)(*b.stride()[:3])
            _lib.call(f"mlic_image_{self.ABI}_u8", h, C.c_void_p(torch.cuda.current_stream().cuda_stream),
                      C.c_void_p(a.data_ptr()), sa, C.c_void_p(b.data_ptr()), sb, B, H, W,
                      C.c_void_p(scratch.data_ptr()), nbytes.value, C.c_void_p(out.data_ptr()),
                      None if terms is None else C.c_void_p(terms.data_ptr()))
        return (out, terms) if return_terms else out

    def close(self):
        handles, self._handles = getattr(self, "_handles", {}), {}
        for h in handles.values():
            _lib.call(f"mlic_{self.ABI}_destroy", h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LPIPS(_VggMetric):
    """LPIPS-VGG of uint8-valued images.  `weights`: a state_dict in the `lpips` package's layout
    (net.slice{n}.{idx}.weight|bias, lin{k}.model.1.weight, scaling_layer.shift|scale), or the pair
    (torchvision vgg16().features state_dict, [five lin tensors [1,C,1,1]]).  metric(a, b) -> [B] float64 on
    the inputs' device; CUDA tensors run the HIP library on the current stream (one handle per device, made at
    the first call), CPU tensors a float32 torch restatement.  terms [B,5]: the five taps' terms."""
    NAME, ABI, TERMS, MIN_SIDE = "LPIPS", "lpips", 5, LPIPS_MIN_SIDE
    _parse = staticmethod(_lpips_parse)

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

    def _cpu(self, a, b):
        return _lpips_cpu(a, b, self._w)


def _create_handle(abi: str, names, tensors, dev: torch.device) -> C.c_void_p:
    n = len(names)
    tensors = [t.contiguous() for t in tensors]
    arr_names = (C.c_char_p * n)(*[s.encode() for s in names])
    arr_ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in tensors])
    shapes = (C.c_int64 * sum(t.dim() for t in tensors))(*[d for t in tensors for d in t.shape])
    ndims = (C.c_int * n)(*[t.dim() for t in tensors])
    h = C.c_void_p()
    with torch.cuda.device(dev):
        _lib.call(f"mlic_{abi}_create", n, arr_names, arr_ptrs, shapes, ndims,
                  C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(h))
    return h


def lpips_create_handle(names, tensors, dev: torch.device) -> C.c_void_p:
    """mlic_lpips_create on float32 tensors that live on `dev` (the raw ABI, for LPIPS and the tests)."""
    return _create_handle("lpips", names, tensors, dev)


def dists_create_handle(names, tensors, dev: torch.device) -> C.c_void_p:
    """mlic_dists_create on float32 tensors that live on `dev` (the raw ABI, for DISTS and the tests)."""
    return _create_handle("dists", names, tensors, dev)


# ---------------------------------------------------------------------------------------------------------
# DISTS

DISTS_MIN_SIDE = 16  # one rule for the harness; the grids the dense convs are exercised at
DISTS_SET_C = (3, 64, 128, 256, 512, 512)  # the image, then the five taps
DISTS_CHANNELS = 1475
DISTS_MEAN = (0.485, 0.456, 0.406)
DISTS_STD = (0.229, 0.224, 0.225)
DISTS_C1 = DISTS_C2 = 1e-6
_DISTS_POOLS = (4, 9, 16, 23)  # the features indices of the package's L2pooling layers (stage 2 - 5)


def dists_synthetic_weights(seed: int = 0):
    """Deterministic DISTS weights in the DISTS_pytorch state_dict layout, for tests and benchmarks (not the
    trained ones): the thirteen convs drawn exactly as lpips_synthetic_weights(seed) draws them (same generator,
    same order: the same trunk), then alpha and beta = |N(0.1, 0.01)|, the package's init, its mean and std and
    its L2-pooling filter buffers."""
    gen = torch.Generator().manual_seed(int(seed))
    sd = {}
    for idx, st, cin, cout in zip(LPIPS_FEATURES, _LPIPS_SLICE, LPIPS_CIN, LPIPS_COUT):
        sd[f"stage{st}.{idx}.weight"] = torch.randn(cout, cin, 3, 3, generator=gen) * math.sqrt(2.0 / (9 * cin))
        sd[f"stage{st}.{idx}.bias"] = (torch.rand(cout, generator=gen) - 0.5) * 0.1
    for name in ("alpha", "beta"):
        sd[name] = (torch.randn(1, DISTS_CHANNELS, 1, 1, generator=gen) * 0.01 + 0.1).abs()
    sd["mean"] = torch.tensor(DISTS_MEAN).view(1, 3, 1, 1)
    sd["std"] = torch.tensor(DISTS_STD).view(1, 3, 1, 1)
    g = torch.tensor([1.0, 2.0, 1.0])
    g = torch.outer(g, g) / 16.0
    for st, (idx, c) in enumerate(zip(_DISTS_POOLS, LPIPS_TAP_C[:4]), start=2):
        sd[f"stage{st}.{idx}.filter"] = g.expand(c, 1, 3, 3).contiguous()
    return sd


def _dists_parse(weights):
    """The two accepted spellings -> {"convs": [(w, b)] * 13, "alpha", "beta", "mean", "std"} of float32 CPU
    tensors.  Conv tensors are matched by their trailing features index, the rule of _lpips_parse."""
    how = "DISTS: weights must be a state_dict or (features_state_dict, {'alpha': ..., 'beta': ...})"
    if isinstance(weights, (tuple, list)):
        if len(weights) != 2 or not isinstance(weights[0], dict) or not isinstance(weights[1], dict):
            raise ValueError(how)
        merged = dict(weights[0])
        merged.update(weights[1])
        weights = merged
    elif not isinstance(weights, dict):
        raise ValueError(how)
    cw, cb = [None] * 13, [None] * 13
    head = {"alpha": None, "beta": None, "mean": None, "std": None}

    def shaped(name, t, want):
        if tuple(t.shape) != tuple(want):
            raise ValueError(f"DISTS: tensor {name} has shape {tuple(t.shape)}, expected {tuple(want)}")
        return t.detach().to("cpu", torch.float32).contiguous().clone()

    for name, t in weights.items():
        if name.endswith(".filter"):
            continue  # the package's L2-pooling buffers: the window is fixed by the definition
        if name in head:
            head[name] = shaped(name, t, (1, DISTS_CHANNELS, 1, 1) if name in ("alpha", "beta") else (1, 3, 1, 1))
            continue
        stem, _, kind = name.rpartition(".")
        idx = stem.rpartition(".")[2]
        if kind not in ("weight", "bias") or not idx.isdigit():
            raise ValueError(f"DISTS: unexpected tensor {name}")
        if int(idx) not in LPIPS_FEATURES:
            raise ValueError(f"DISTS: extra conv tensor {name} (VGG16 has no conv at features index {idx})")
        l = LPIPS_FEATURES.index(int(idx))
        slot = cw if kind == "weight" else cb
        if slot[l] is not None:
            raise ValueError(f"DISTS: extra conv tensor {name} (features index {idx} given twice)")
        slot[l] = shaped(name, t, (LPIPS_COUT[l], LPIPS_CIN[l], 3, 3) if kind == "weight" else (LPIPS_COUT[l],))
    for l, idx in enumerate(LPIPS_FEATURES):
        if cw[l] is None:
            raise ValueError(f"DISTS: missing tensor {idx}.weight")
        if cb[l] is None:
            raise ValueError(f"DISTS: missing tensor {idx}.bias")
    for name in ("alpha", "beta"):
        if head[name] is None:
            raise ValueError(f"DISTS: missing tensor {name}")
    if (head["mean"] is None) != (head["std"] is None):
        raise ValueError("DISTS: missing tensor " + ("mean" if head["mean"] is None else "std"))
    if head["mean"] is None:
        head["mean"], head["std"] = torch.tensor(DISTS_MEAN).view(1, 3, 1, 1), torch.tensor(DISTS_STD).view(1, 3, 1, 1)
    w = head["alpha"].double().sum().item() + head["beta"].double().sum().item()
    if not math.isfinite(w) or w == 0.0:
        raise ValueError(f"DISTS: the sum of tensors alpha and beta must be finite and nonzero, got {w}")
    return {"convs": list(zip(cw, cb)), **head}


def _l2pool(x: torch.Tensor) -> torch.Tensor:
    c = x.size(1)
    g = torch.tensor([1.0, 2.0, 1.0], dtype=x.dtype)
    g = (torch.outer(g, g) / 16.0).expand(c, 1, 3, 3)
    return (F.conv2d(x * x, g, stride=2, padding=1, groups=c) + 1e-12).sqrt()


def _dists_cpu(a: torch.Tensor, b: torch.Tensor, w):
    """float32 features, float64 statistics, the difference form (identical images give exactly 0)."""
    def features(x):
        x = torch.floor(torch.nan_to_num(x.float(), nan=0.0).clamp(0, 1) * 255) / 255
        sets = [x]
        x = (x - w["mean"]) / w["std"]
        for l, (cw, cb) in enumerate(w["convs"]):
            if l and l - 1 in LPIPS_TAP_LAST:
                x = _l2pool(x)
            x = torch.relu(F.conv2d(x, cw, cb, padding=1))
            if l in LPIPS_TAP_LAST:
                sets.append(x)
        return sets

    total = w["alpha"].double().sum() + w["beta"].double().sum()
    al = (w["alpha"].double() / total).flatten().split(DISTS_SET_C)
    be = (w["beta"].double() / total).flatten().split(DISTS_SET_C)
    terms = []
    for fa, fb, ak, bk in zip(features(a), features(b), al, be):
        fa, fb = fa.double().flatten(2), fb.double().flatten(2)  # [B, C, pixels]
        mua, mub = fa.mean(2), fb.mean(2)
        d = fa - fb
        mud = d.mean(2)
        va = (fa - mua.unsqueeze(2)).square().mean(2)
        vb = (fb - mub.unsqueeze(2)).square().mean(2)
        vd = (d - mud.unsqueeze(2)).square().mean(2)  # = va + vb - 2 cov, subtracted before it is squared
        terms.append((ak * (mud.square() / (mua.square() + mub.square() + DISTS_C1))).sum(1))
        terms.append((bk * (vd / (va + vb + DISTS_C2))).sum(1))
    t = torch.stack(terms, 1)  # [B, 12]
    return t.sum(1), t


class DISTS(_VggMetric):
    """DISTS of uint8-valued images (DISTS_pytorch 0.1 in eval mode, restated: DESIGN.md §3).  `weights`: a
    state_dict in the package's layout (stage{n}.{idx}.weight|bias, alpha, beta [1,1475,1,1], optional mean and
    std [1,3,1,1]; the stage{n}.{idx}.filter buffers are ignored), or the pair (torchvision vgg16().features
    state_dict, {"alpha": ..., "beta": ...}).  metric(a, b) -> [B] float64 on the inputs' device, as LPIPS;
    terms [B,12] = [T1_0, T2_0, .., T1_5, T2_5], the structure and texture terms of the image and the five taps,
    in the difference form: identical images give exactly 0."""
    NAME, ABI, TERMS, MIN_SIDE = "DISTS", "dists", 12, DISTS_MIN_SIDE
    _parse = staticmethod(_dists_parse)

    def _tensors(self):
        names, tensors = [], []
        for idx, (cw, cb) in zip(LPIPS_FEATURES, self._w["convs"]):
            names += [f"{idx}.weight", f"{idx}.bias"]
            tensors += [cw, cb]
        for name in ("alpha", "beta", "mean", "std"):
            names.append(name)
            tensors.append(self._w[name])
        return names, tensors

    def _cpu(self, a, b):
        return _dists_cpu(a, b, self._w)
