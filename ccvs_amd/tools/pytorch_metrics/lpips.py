"""LPIPS from a weight file the user names: piq.LPIPS(reduction='mean') (piq 0.5.4, the reference's tools/pytorch_metrics/metrics.py:12-13)
on the GPU.  The weights -- torchvision's VGG16 and the five linear heads of the LPIPS release -- are not in this repository and are
never downloaded; `load_lpips_weights` reads them from the one file the converter at the bottom writes.

The distance, for x, y [N, 3, H, W] fp32 in [0, 1] (a restatement of piq's code; parity with piq itself is not pinned -- piq is not
installed where the tests run -- the float64 mirror tests/lpips_ref.py of this text is what the kernels are held to):
  1. (x - mean) / std with ImageNet's mean (0.485, 0.456, 0.406) and std (0.229, 0.224, 0.225)                 ops.lpips_prep
  2. torchvision's vgg16().features without its last pool: 3 x 3 convolutions, padding 1, with bias             ops.conv2d
     (modules 0 2 | 5 7 | 10 12 14 | 17 19 21 | 24 26 28; widths 64 64 | 128 128 | 256 x 3 | 512 x 3 | 512 x 3),
     each followed by ReLU                                                                                      ops.relu_
     and the blocks separated by MaxPool2d(2, 2) in floor mode                                                  ops.relu_maxpool2
  3. five taps behind the ReLU of modules 3, 8, 15, 22, 29 (the last convolution of each block)
  4. each tapped map normalised over its channels, f / (sqrt(sum_c f^2) + 1e-10)
  5. per layer the squared difference weighted by the layer's head w_l [1, C, 1, 1] and averaged over H_l, W_l  ops.lpips_layer
  6. per image the sum over the five layers; reduction='mean' is the mean over the images.
Every tapped layer is the last convolution in front of a pool (or the network's end), so its pre-activation map is read by
`ops.lpips_layer` (ReLU on read) and by `ops.relu_maxpool2`, and never needs a ReLU pass of its own.

No CPU fallback: the kernels live in libccvs_hip.so.  The converter is host code:
  python -m ccvs_amd.tools.pytorch_metrics.lpips --vgg vgg16.pth --lin lpips_weights.pt --out lpips_vgg16.pt
"""
import argparse
import os
import re

import torch

from ccvs_amd import ops

# (module index in vgg16().features, input channels, output channels) of the 13 convolutions, block by block; a block's last
# convolution is tapped (behind its ReLU: modules 3, 8, 15, 22, 29)
VGG16_BLOCKS = (
    ((0, 3, 64), (2, 64, 64)),
    ((5, 64, 128), (7, 128, 128)),
    ((10, 128, 256), (12, 256, 256), (14, 256, 256)),
    ((17, 256, 512), (19, 512, 512), (21, 512, 512)),
    ((24, 512, 512), (26, 512, 512), (28, 512, 512)),
)
VGG16_CONVS = tuple(conv for block in VGG16_BLOCKS for conv in block)
LIN_CHANNELS = tuple(block[-1][2] for block in VGG16_BLOCKS)   # 64, 128, 256, 512, 512
MIN_SIDE = 32   # four pools: block 5 then runs on 2 x 2 maps


def _tensor(v, key):
    if not isinstance(v, torch.Tensor):
        raise ValueError(f"load_lpips_weights: {key} is a {type(v).__name__}, not a tensor")
    return v.detach().to(device="cpu", dtype=torch.float32)


def load_lpips_weights(path_or_dict):
    """Read and validate LPIPS weights: a file written with torch.save (read with weights_only=True) or the dict itself, holding
      "vgg"  a VGG16 state dict keyed `features.N.weight / .bias` (torchvision's) or `N.weight / .bias` (its `.features` alone);
             entries that are not one of the 13 convolutions (the classifier) are ignored;
      "lin"  the five heads, each [1, C, 1, 1] or [C]: a sequence, or a dict whose values are taken in sorted-key order (the LPIPS
             release keys them lin0.model.1.weight ... lin4.model.1.weight).
    Returns {"vgg": {"features.N.weight": [Cout, Cin, 3, 3], "features.N.bias": [Cout], ...}, "lin": [five [1, C, 1, 1]]}, fp32 on the
    host.  A missing layer or a wrong shape raises ValueError naming the key."""
    src = path_or_dict
    if not isinstance(src, dict):
        src = torch.load(os.fspath(src), map_location="cpu", weights_only=True)
    if not isinstance(src, dict) or "vgg" not in src or "lin" not in src:
        raise ValueError('load_lpips_weights: the weights are a dict with the entries "vgg" and "lin" (write one with '
                         "python -m ccvs_amd.tools.pytorch_metrics.lpips)")
    vgg_in = src["vgg"]
    if not isinstance(vgg_in, dict):
        raise ValueError('load_lpips_weights: "vgg" is not a state dict')
    vgg = {}
    for n, cin, cout in VGG16_CONVS:
        for kind, shape in (("weight", (cout, cin, 3, 3)), ("bias", (cout,))):
            key = f"features.{n}.{kind}"
            found = key if key in vgg_in else (f"{n}.{kind}" if f"{n}.{kind}" in vgg_in else None)
            if found is None:
                raise ValueError(f"load_lpips_weights: vgg has no {key} (nor {n}.{kind})")
            t = _tensor(vgg_in[found], found)
            if tuple(t.shape) != shape:
                raise ValueError(f"load_lpips_weights: vgg {found} is {tuple(t.shape)}, not {shape}")
            vgg[key] = t.contiguous()
    lin_in = src["lin"]
    if isinstance(lin_in, dict):
        names = sorted(lin_in)
        heads = [lin_in[k] for k in names]
    elif isinstance(lin_in, (list, tuple)):
        names = [f"lin[{i}]" for i in range(len(lin_in))]
        heads = list(lin_in)
    else:
        raise ValueError('load_lpips_weights: "lin" is neither a sequence nor a dict of the five heads')
    if len(heads) != len(LIN_CHANNELS):
        raise ValueError(f'load_lpips_weights: "lin" holds {len(heads)} heads ({", ".join(map(str, names))}), not {len(LIN_CHANNELS)}')
    lin = []
    for name, head, c in zip(names, heads, LIN_CHANNELS):
        t = _tensor(head, name)
        if tuple(t.shape) not in ((1, c, 1, 1), (c,)):
            raise ValueError(f"load_lpips_weights: lin {name} is {tuple(t.shape)}, not (1, {c}, 1, 1) or ({c},)")
        lin.append(t.reshape(1, c, 1, 1).contiguous())
    return {"vgg": vgg, "lin": lin}


class LPIPS:
    """piq.LPIPS(reduction='mean') on the GPU from user-supplied weights (a path or dict `load_lpips_weights` takes).

    precision: None follows `ops.CONV_PRECISION` (split-bf16 by default), "f32" is the exact-fp32 convolution.  The 13 convolutions
    are packed once, here.  `per_image(x, y)` returns float64 [N] on the device, `__call__` their mean as a 0-dim fp32 device tensor;
    nothing synchronises with the host.  The image pairs are processed in chunks of `chunk_pairs(H, W)`, chosen so that the two largest
    feature maps alive at a time (64 channels at full resolution, both images of every pair) stay under `max_workspace_bytes`; the
    real and the fake half of a chunk go through the same convolution launches, so equal images give equal features, bit for bit."""

    def __init__(self, weights, precision=None, max_workspace_bytes=2 << 30):
        if precision not in (None, "f32"):
            raise ValueError(f"LPIPS: precision is None (ops.CONV_PRECISION) or 'f32', not {precision!r}")
        if not torch.cuda.is_available():
            raise ops._lib.CcvsError("LPIPS needs a GPU: the HIP path has no CPU fallback")
        w = load_lpips_weights(weights)
        self.precision = precision
        self.max_workspace_bytes = int(max_workspace_bytes)
        self.blocks = []
        for block in VGG16_BLOCKS:
            convs = []
            for n, cin, cout in block:
                packed = ops.pack_conv_weight(w["vgg"][f"features.{n}.weight"].cuda(), precision, scale=1.0)
                convs.append((packed, w["vgg"][f"features.{n}.bias"].cuda(), cout))
            self.blocks.append(convs)
        self.lin = [t.reshape(-1).cuda() for t in w["lin"]]

    def chunk_pairs(self, h, w):
        """Image pairs per chunk: the largest count whose two full-resolution 64-channel maps (x and y halves) fit max_workspace_bytes."""
        per_pair = 2 * 2 * 64 * h * w * 4   # two maps x two images x 64 channels x fp32
        return max(1, self.max_workspace_bytes // per_pair)

    def per_image(self, x, y):
        ops._need_gpu(x, y)
        if x.shape != y.shape or x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32 or y.dtype != torch.float32:
            raise ValueError(f"LPIPS: x and y are fp32 [N, 3, H, W] of one shape, got {tuple(x.shape)} {x.dtype} and {tuple(y.shape)} {y.dtype}")
        n, _, h, w = x.shape
        if min(h, w) < MIN_SIDE:
            raise ValueError(f"LPIPS: the shorter side is {min(h, w)}, under {MIN_SIDE} (the network pools four times)")
        x, y = x.contiguous(), y.contiguous()
        out = torch.empty(n, dtype=torch.float64, device=x.device)
        step = self.chunk_pairs(h, w)
        for i0 in range(0, n, step):
            m = min(step, n - i0)
            f = torch.empty(2 * m, 3, h, w, dtype=torch.float32, device=x.device)
            ops.lpips_prep(x[i0:i0 + m], out=f[:m])
            ops.lpips_prep(y[i0:i0 + m], out=f[m:])
            acc = out[i0:i0 + m]
            for l, convs in enumerate(self.blocks):
                for j, (packed, bias, cout) in enumerate(convs):
                    f = ops.conv2d(f, packed, bias, cout, 3, pad=1)
                    if j + 1 < len(convs):
                        ops.relu_(f)
                ops.lpips_layer(f, self.lin[l], relu=True, out=acc, accumulate=l > 0)   # f: the block's last pre-activation map
                if l + 1 < len(self.blocks):
                    f = ops.relu_maxpool2(f)
        return out

    def __call__(self, x, y):
        return self.per_image(x, y).mean().float()


def convert(vgg_path, lin_path, out_path):
    """The one file `load_lpips_weights` reads, from torchvision's VGG16 checkpoint (vgg16-397923af.pth) and a file with the five
    linear heads (the LPIPS release's vgg.pth, or piq's copy of it).  Host only."""
    vgg = torch.load(vgg_path, map_location="cpu", weights_only=True)
    lin = torch.load(lin_path, map_location="cpu", weights_only=True)
    if isinstance(lin, dict):
        lin = {k: v for k, v in lin.items() if re.search(r"lin\d", str(k))} or lin   # (a release file may hold other entries)
    w = load_lpips_weights({"vgg": vgg, "lin": lin})
    torch.save(w, out_path)
    return w


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="write the LPIPS weight file the metrics command reads (--lpips_weights)")
    parser.add_argument("--vgg", type=str, required=True, help="torchvision's VGG16 state dict")
    parser.add_argument("--lin", type=str, required=True, help="the five linear heads (a dict or a list of tensors)")
    parser.add_argument("--out", type=str, required=True)
    return parser.parse_args(argv)


if __name__ == "__main__":
    _args = parse_args()
    convert(_args.vgg, _args.lin, _args.out)
    print(f"wrote {_args.out}")
