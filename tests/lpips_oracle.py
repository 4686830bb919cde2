"""Float64 oracle of LPIPS-VGG for the metric tests, written from the definition (lpips.LPIPS(net="vgg",
version="0.1") in eval mode with normalize=True) and independently of mlic_amd/metrics.py: the
backbone as one flat op list run by F.conv2d / F.max_pool2d in float64, the head as a 1x1 F.conv2d.  Also the
test images (one base image and six distortions of it) and the synthetic weights (seed 7) all LPIPS tests share.
Every case is computed once, cached and never modified."""
import torch
import torch.nn.functional as F

from mlic_amd import metrics, synthetic

SEED = 7
DISTORTIONS = ("same", "n1", "n8", "blur", "inv", "off")
# vgg16().features up to relu5_3: conv index, "T" = tap (after the ReLU of the conv before it), "M" = MaxPool2d(2, 2)
OPS = (0, 2, "T", "M", 5, 7, "T", "M", 10, 12, 14, "T", "M", 17, 19, 21, "T", "M", 24, 26, 28, "T")
SLICE = {0: 1, 2: 1, 5: 2, 7: 2, 10: 3, 12: 3, 14: 3, 17: 4, 19: 4, 21: 4, 24: 5, 26: 5, 28: 5}

# name -> (H, W, storage H, storage W): a case whose storage is larger is the view [:, :, :H, :W] of it
SHAPES = {
    "16x16": (16, 16, 16, 16),       # tap 4 is 1 x 1
    "37x53": (37, 53, 37, 53),       # every pool drops a row or a column; no 8 x 32 conv tile is full
    "72x136": (72, 136, 72, 136),    # several conv tiles in both directions
    "72x136v": (72, 136, 80, 160),   # the same size inside a larger buffer: unit column stride, not contiguous
}

_weights = {}
_cache = {}
_storage = {}
_feat_a = {}


def weights(scale_conv0: float = 1.0):
    """The shared synthetic weights (`lpips` layout); scale_conv0 multiplies conv1_1's weight and bias."""
    if scale_conv0 not in _weights:
        sd = metrics.lpips_synthetic_weights(SEED)
        if scale_conv0 != 1.0:
            sd = dict(sd)
            for k in ("net.slice1.0.weight", "net.slice1.0.bias"):
                sd[k] = sd[k] * scale_conv0
        _weights[scale_conv0] = sd
    return _weights[scale_conv0]


def to_unit_f64(x: torch.Tensor) -> torch.Tensor:
    """u / 255 of the uint8 image the library scores (float32 clamp, * 255, truncation), as float64."""
    x = torch.where(torch.isnan(x), torch.zeros_like(x), x.float())
    return (x.clamp(0, 1) * 255).to(torch.uint8).double() / 255.0


def features(x: torch.Tensor, sd):
    """The five ReLU'd taps (float64) of images x [B, 3, H, W] given in [0, 1]."""
    t = 2.0 * to_unit_f64(x.cpu()) - 1.0
    t = (t - sd["scaling_layer.shift"].double()) / sd["scaling_layer.scale"].double()
    taps = []
    for op in OPS:
        if op == "T":
            taps.append(t)
        elif op == "M":
            t = F.max_pool2d(t, kernel_size=2, stride=2)
        else:
            p = f"net.slice{SLICE[op]}.{op}."
            t = F.conv2d(t, sd[p + "weight"].double(), sd[p + "bias"].double(), stride=1, padding=1).clamp(min=0)
    return taps


def head(fa, fb, sd):
    """(value [B], terms [B, 5]) from the two images' taps."""
    terms = []
    for k, (xa, xb) in enumerate(zip(fa, fb)):
        ua = xa / (xa.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        ub = xb / (xb.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        m = F.conv2d((ua - ub) ** 2, sd[f"lin{k}.model.1.weight"].double())  # [B, 1, h, w]
        terms.append(m.mean((1, 2, 3)))
    t = torch.stack(terms, 1)
    return t.sum(1), t


def lpips(a: torch.Tensor, b: torch.Tensor, sd=None):
    sd = weights() if sd is None else sd
    return head(features(a, sd), features(b, sd), sd)


def distort(a: torch.Tensor, kind: str) -> torch.Tensor:
    gen = torch.Generator().manual_seed(40 + DISTORTIONS.index(kind))
    if kind == "same":
        return a.clone()
    if kind in ("n1", "n8"):
        return a + torch.randn(a.shape, generator=gen) * (int(kind[1:]) / 255.0)  # unclamped on purpose
    if kind == "blur":
        return F.conv2d(F.pad(a, (2, 2, 2, 2), mode="replicate"), torch.full((3, 1, 5, 5), 1 / 25.0), groups=3)
    if kind == "inv":
        return 1 - a
    if kind == "off":
        return 1.6 * a - 0.3  # leaves [0, 1] on both sides: the clamp matters
    raise KeyError(kind)


def case(shape: str, kind: str):
    """(a, b, value [1], terms [1, 5]) of one parity case; computed once, shared, never modified."""
    key = (shape, kind)
    if key not in _cache:
        H, W, SH, SW = SHAPES[shape]
        if shape not in _storage:
            _storage[shape] = synthetic.synth_image(SH, SW, 5).contiguous()
            _feat_a[shape] = features(_storage[shape][:, :, :H, :W], weights())
        fa = _storage[shape]
        fb = distort(fa, kind).contiguous()
        a, b = fa[:, :, :H, :W], fb[:, :, :H, :W]
        v, t = head(_feat_a[shape], features(b, weights()), weights())
        _cache[key] = (a, b, v, t)
        _storage[key] = (fa, fb)
    return _cache[key]


def on_device(shape: str, kind: str, dev):
    """The case's (a, b) on `dev` with the same strides: the storage-sized tensors are uploaded and the same
    view is taken there."""
    case(shape, kind)
    H, W = SHAPES[shape][:2]
    fa, fb = _storage[(shape, kind)]
    return fa.to(dev)[:, :, :H, :W], fb.to(dev)[:, :, :H, :W]


def rel_err(got: torch.Tensor, want: torch.Tensor) -> float:
    """max |got - want| / |want| over the elements (want nonzero)."""
    return ((got.double() - want).abs() / want.abs()).max().item()
