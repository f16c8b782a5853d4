"""Plain-torch restatement of the skip_rgb head's ToRGB (skip_autoencoder.py:268-306), the stand-in the fixtures and the GPU tests
compare `ops.to_rgb` with: the 1 x 1 EqualConv2d to 3 channels (weight * 1/sqrt(C), its bias), ToRGB's own [1, 3, 1, 1] bias, then
Upsample([1,3,3,1]) of the coarser level's RGB -- upfirdn2d(skip, outer([1,3,3,1]) / 64 * 4, up=2, down=1, pad=(2, 1)), i.e. zero
insertion, padding 2 before and 1 after, and the 4 x 4 filter (symmetric: correlation and convolution agree)."""
import math

import torch
import torch.nn.functional as F


def upsample2(skip):
    """[N, C, h, w] -> [N, C, 2h, 2w], in the dtype of `skip`."""
    n, c, h, w = skip.shape
    k = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=skip.dtype)
    k = torch.outer(k, k)
    k = k / k.sum() * 4
    z = skip.new_zeros(n * c, 1, 2 * h, 2 * w)
    z[:, :, ::2, ::2] = skip.reshape(n * c, 1, h, w)
    z = F.pad(z, (2, 1, 2, 1))
    return F.conv2d(z, k.view(1, 1, 4, 4)).view(n, c, 2 * h, 2 * w)


def to_rgb(x, weight, b_conv, bias, skip=None):
    """x [N, C, H, W]; weight [3, C, 1, 1] (unscaled, as the state dict holds it); b_conv [3]; bias [1, 3, 1, 1]; skip [N, 3, H/2, W/2]."""
    scale = 1 / math.sqrt(x.shape[1])
    out = F.conv2d(x, weight * scale, bias=b_conv)
    out = out + bias.view(1, 3, 1, 1)
    if skip is not None:
        out = out + upsample2(skip)
    return out
