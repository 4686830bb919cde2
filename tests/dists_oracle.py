"""Float64 oracle of DISTS for the metric tests, written from the definition (DISTS_pytorch 0.1's DISTS() in eval
mode) and independently of mlic_amd/metrics.py: the backbone as one flat op list run by F.conv2d in
float64 (the L2 pooling as a depthwise F.conv2d of x^2 with the normalised Hanning window), the head in the
package's LITERAL form 1 - sum(alpha S1 + beta S2) / w with the covariance as E[xy] - mu_x mu_y.  The product
computes the algebraically equal difference form, so the two differ in algebra as well as in precision.

Images, distortions, shapes and storage come from tests/lpips_oracle.py; the synthetic weights are
metrics.dists_synthetic_weights(7) (the same trunk as the LPIPS tests).  Every case is computed once, cached and
never modified."""
import torch
import torch.nn.functional as F

import lpips_oracle as lo
from mlic_amd import metrics

SEED = lo.SEED
DISTORTIONS = lo.DISTORTIONS
SHAPES = lo.SHAPES
C1 = C2 = 1e-6
SET_C = (3, 64, 128, 256, 512, 512)
# vgg16().features up to relu5_3 as the package cuts it: conv index, "T" = a feature set (after the ReLU of the
# conv before it), "P" = L2pooling in place of the MaxPool2d
OPS = (0, 2, "T", "P", 5, 7, "T", "P", 10, 12, 14, "T", "P", 17, 19, 21, "T", "P", 24, 26, 28, "T")
STAGE = {0: 1, 2: 1, 5: 2, 7: 2, 10: 3, 12: 3, 14: 3, 17: 4, 19: 4, 21: 4, 24: 5, 26: 5, 28: 5}

_weights = {}
_cache = {}
_feat_a = {}


def weights(scale_conv0: float = 1.0):
    """The shared synthetic weights (package layout); scale_conv0 multiplies conv1_1's weight and bias."""
    if scale_conv0 not in _weights:
        sd = metrics.dists_synthetic_weights(SEED)
        if scale_conv0 != 1.0:
            sd = dict(sd)
            for k in ("stage1.0.weight", "stage1.0.bias"):
                sd[k] = sd[k] * scale_conv0
        _weights[scale_conv0] = sd
    return _weights[scale_conv0]


def l2pool(t: torch.Tensor) -> torch.Tensor:
    a = torch.hann_window(5, periodic=False, dtype=torch.float64)[1:-1]  # np.hanning(5)[1:-1] = 0.5 1 0.5
    g = a[:, None] * a[None, :]
    g = g / g.sum()
    c = t.size(1)
    out = F.conv2d(t ** 2, g[None, None].repeat(c, 1, 1, 1), stride=2, padding=1, groups=c)
    return (out + 1e-12).sqrt()


def features(x: torch.Tensor, sd):
    """The six feature sets (float64) of images x [B, 3, H, W] given in [0, 1]: the image, then the five taps."""
    v = lo.to_unit_f64(x.cpu())
    sets = [v]
    t = (v - sd["mean"].double()) / sd["std"].double()
    for op in OPS:
        if op == "T":
            sets.append(t)
        elif op == "P":
            t = l2pool(t)
        else:
            p = f"stage{STAGE[op]}.{op}."
            t = F.conv2d(t, sd[p + "weight"].double(), sd[p + "bias"].double(), stride=1, padding=1).clamp(min=0)
    return sets


def head(fa, fb, sd):
    """(value [B], terms [B, 12]) in the package's literal form; term 2k = sum_c alpha_c (1 - S1_c) / w over set k,
    term 2k + 1 = sum_c beta_c (1 - S2_c) / w (alpha / w and beta / w sum to 1 together)."""
    w_sum = sd["alpha"].double().sum() + sd["beta"].double().sum()
    alpha = torch.split(sd["alpha"].double() / w_sum, SET_C, dim=1)
    beta = torch.split(sd["beta"].double() / w_sum, SET_C, dim=1)
    dist1 = dist2 = 0
    terms = []
    for k, (x, y) in enumerate(zip(fa, fb)):
        x_mean, y_mean = x.mean([2, 3], keepdim=True), y.mean([2, 3], keepdim=True)
        s1 = (2 * x_mean * y_mean + C1) / (x_mean ** 2 + y_mean ** 2 + C1)
        x_var = ((x - x_mean) ** 2).mean([2, 3], keepdim=True)
        y_var = ((y - y_mean) ** 2).mean([2, 3], keepdim=True)
        xy_cov = (x * y).mean([2, 3], keepdim=True) - x_mean * y_mean
        s2 = (2 * xy_cov + C2) / (x_var + y_var + C2)
        d1, d2 = (alpha[k] * s1).sum(1, keepdim=True), (beta[k] * s2).sum(1, keepdim=True)
        dist1, dist2 = dist1 + d1, dist2 + d2
        terms += [(alpha[k].sum() - d1).flatten(), (beta[k].sum() - d2).flatten()]
    return (1 - (dist1 + dist2)).flatten(), torch.stack(terms, 1)


def dists(a: torch.Tensor, b: torch.Tensor, sd=None):
    sd = weights() if sd is None else sd
    return head(features(a, sd), features(b, sd), sd)


def case(shape: str, kind: str):
    """(a, b, value [1], terms [1, 12]) of one parity case on lpips_oracle's images; computed once, shared."""
    key = (shape, kind)
    if key not in _cache:
        a, b = lo.case(shape, kind)[:2]
        if shape not in _feat_a:
            _feat_a[shape] = features(a, weights())
        v, t = head(_feat_a[shape], features(b, weights()), weights())
        _cache[key] = (a, b, v, t)
    return _cache[key]


def on_device(shape: str, kind: str, dev):
    return lo.on_device(shape, kind, dev)


def abs_err(got: torch.Tensor, want: torch.Tensor) -> float:
    """max |got - want| over the elements: the terms can be exactly 0 or about 1e-8, so errors are absolute."""
    return (got.double() - want).abs().max().item()
