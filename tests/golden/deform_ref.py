"""A plain-torch CPU restatement of torchvision.ops.DeformConv2d (no modulation mask), for the fixtures and tests of the
--q_use_deformed_conv variant: torchvision is not a dependency of this project, and the reference harness stubs it.

Semantics (torchvision's deform_conv2d kernel): tap t = i * kw + j of output (y, x) samples the input at
(y * stride - pad + i * dil + offset[2t], x * stride - pad + j * dil + offset[2t + 1]) -- channel 2t is the ROW offset --
bilinearly in pixel units: 0 when the point lies outside (-1, H) x (-1, W), and a corner outside the image adds 0."""
import math

import torch
from torch import nn


def bilinear_zero(x, hy, wx):
    """x [B,C,H,W], hy / wx [B,Ho,Wo] sample positions -> [B,C,Ho,Wo] (torchvision's bilinear_interpolate)."""
    b, c, h, w = x.shape
    inside = ~((hy <= -1) | (hy >= h) | (wx <= -1) | (wx >= w))
    h0, w0 = torch.floor(hy), torch.floor(wx)
    lh, lw = hy - h0, wx - w0
    hh, hw = 1 - lh, 1 - lw
    h0, w0 = h0.long(), w0.long()
    h1, w1 = h0 + 1, w0 + 1
    flat = x.reshape(b, c, h * w)

    def corner(yy, xx):
        ok = (yy >= 0) & (yy <= h - 1) & (xx >= 0) & (xx <= w - 1) & inside
        idx = (yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)).view(b, 1, -1).expand(b, c, -1)
        return flat.gather(2, idx).view(b, c, *yy.shape[1:]) * ok.unsqueeze(1).to(x.dtype)

    w1_, w2_, w3_, w4_ = (t.unsqueeze(1) for t in (hh * hw, hh * lw, lh * hw, lh * lw))
    return w1_ * corner(h0, w0) + w2_ * corner(h0, w1) + w3_ * corner(h1, w0) + w4_ * corner(h1, w1)


def deform_conv2d(x, offset, weight, bias=None, stride=1, padding=0, dilation=1):
    b, c, h, w = x.shape
    o, ci, kh, kw = weight.shape
    assert ci == c
    ho = (h + 2 * padding - dilation * (kh - 1) - 1) // stride + 1
    wo = (w + 2 * padding - dilation * (kw - 1) - 1) // stride + 1
    assert offset.shape == (b, 2 * kh * kw, ho, wo), offset.shape
    ys = (torch.arange(ho, dtype=x.dtype) * stride - padding).view(1, ho, 1)
    xs = (torch.arange(wo, dtype=x.dtype) * stride - padding).view(1, 1, wo)
    cols = []
    for t in range(kh * kw):
        i, j = divmod(t, kw)
        cols.append(bilinear_zero(x, ys + i * dilation + offset[:, 2 * t], xs + j * dilation + offset[:, 2 * t + 1]))
    col = torch.stack(cols, dim=2)                                   # [B, C, taps, Ho, Wo]
    out = torch.einsum("bcthw,oct->bohw", col, weight.reshape(o, c, kh * kw).to(x.dtype))
    if bias is not None:
        out = out + bias.to(x.dtype).view(1, -1, 1, 1)
    return out


class DeformConv2d(nn.Module):
    """torchvision.ops.DeformConv2d(in, out, k, stride, padding, dilation, groups=1, bias) with its initialiser."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True):
        super().__init__()
        assert groups == 1
        self.stride, self.padding, self.dilation = stride, padding, dilation
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, kernel_size, kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1 / math.sqrt(in_channels * kernel_size * kernel_size)
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, input, offset, mask=None):
        assert mask is None
        return deform_conv2d(input, offset, self.weight, self.bias, self.stride, self.padding, self.dilation)
