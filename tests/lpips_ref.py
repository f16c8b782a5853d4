"""Spec mirror of LPIPS (piq 0.5.4 `piq.LPIPS(reduction='mean')`, restated; ccvs_amd/tools/pytorch_metrics/lpips.py states the six
steps) in float64 torch on the host, and a generator of random weights at VGG16's true widths.

The weights are NOT the pretrained ones (those are never in the repository): convolutions with He initialisation,
std = sqrt(2 / (9 Cin)), keep the activations O(1) through all 13 layers; biases 0.05 randn; linear heads uniform in [0, 1).  With
y = clamp(x + 0.1 randn) the scores come out near 0.1 per image (tests/test_lpips_host.py checks both on the CPU).
"""
import math

import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
# torchvision's configuration D without the last pool
CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512)
TAPS = (3, 8, 15, 22, 29)   # module indices of relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
TAP_CHANNELS = (64, 128, 256, 512, 512)


def modules():
    """[(module index, "conv" | "relu" | "pool", cin, cout)] in torchvision's numbering of vgg16().features (last pool left out)."""
    out, i, cin = [], 0, 3
    for v in CFG:
        if v == "M":
            out.append((i, "pool", cin, cin))
            i += 1
        else:
            out.append((i, "conv", cin, v))
            out.append((i + 1, "relu", v, v))
            i += 2
            cin = v
    return out


def random_weights(seed):
    """{"vgg": {"features.N.weight" / ".bias"}, "lin": [five [1, C, 1, 1]]} in fp32 from a seed."""
    g = torch.Generator().manual_seed(seed)
    vgg = {}
    for i, kind, cin, cout in modules():
        if kind == "conv":
            vgg[f"features.{i}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
            vgg[f"features.{i}.bias"] = 0.05 * torch.randn(cout, generator=g)
    lin = [torch.rand(1, c, 1, 1, generator=g) for c in TAP_CHANNELS]
    return {"vgg": vgg, "lin": lin}


def features(x, weights, dtype=torch.float64):
    """Steps 1-3: the five tapped maps (behind their ReLU) of x [N, 3, H, W], computed in `dtype`."""
    x = x.to(dtype)
    mean = torch.tensor(MEAN, dtype=dtype).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=dtype).view(1, 3, 1, 1)
    h = (x - mean) / std
    taps = []
    for i, kind, _, _ in modules():
        if kind == "conv":
            h = F.conv2d(h, weights["vgg"][f"features.{i}.weight"].to(dtype), weights["vgg"][f"features.{i}.bias"].to(dtype), padding=1)
        elif kind == "relu":
            h = F.relu(h)
            if i in TAPS:
                taps.append(h)
        else:
            h = F.max_pool2d(h, 2, 2)
    return taps


def layer_distance(fx, fy, w):
    """Steps 4-5 for one layer: fx, fy [N, C, H, W] float64, w [1, C, 1, 1] -> [N]."""
    w = w.to(fx.dtype).reshape(1, -1, 1, 1)
    nx = fx / (torch.sqrt((fx ** 2).sum(dim=1, keepdim=True)) + 1e-10)
    ny = fy / (torch.sqrt((fy ** 2).sum(dim=1, keepdim=True)) + 1e-10)
    return (w * (nx - ny) ** 2).sum(dim=1).mean(dim=(1, 2))


def per_image(x, y, weights, dtype=torch.float64):
    """Steps 1-6 without the last mean: [N]."""
    fx, fy = features(x, weights, dtype), features(y, weights, dtype)
    total = torch.zeros(x.shape[0], dtype=dtype)
    for a, b, w in zip(fx, fy, weights["lin"]):
        total = total + layer_distance(a, b, w)
    return total


def lpips(x, y, weights, dtype=torch.float64):
    """piq.LPIPS(reduction='mean')(x, y)."""
    return per_image(x, y, weights, dtype).mean()


def pair(shape, seed, noise=0.1):
    """x uniform in [0, 1), y = clamp(x + noise randn), fp32."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(*shape, generator=g)
    y = (x + noise * torch.randn(*shape, generator=g)).clamp(0, 1)
    return x, y
