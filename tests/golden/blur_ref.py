"""A plain-torch CPU restatement of torchvision 0.8.1's `transforms.GaussianBlur` on tensors, for the fixtures and tests of the
deblurring mode (helpers/generator.py:381-390 `blur`): torchvision is not a dependency of this project, and the reference harness
stubs it.  tests/test_deblur_host.py pins what this file states.

Semantics (torchvision/transforms/functional_tensor.py `gaussian_blur`, transforms.py `GaussianBlur`):
  * 1-D weights: x = linspace(-(k-1)/2, (k-1)/2, k), pdf = exp(-0.5 (x / sigma)^2), normalised by their sum -- float32;
  * the 2-D kernel is their outer product (`kernel1d[:, None] @ kernel1d[None, :]`), in the input's dtype;
  * padding k // 2 on each side, mode "reflect", then a depthwise conv2d (groups = C);
  * `forward` draws sigma with `torch.empty(1).uniform_(sigma_min, sigma_max).item()`: one draw from the CPU default generator per
    call, whose value is exactly sigma when a single number is given."""
import torch
import torch.nn.functional as F


def kernel_size(blur_sigma):
    """helpers/generator.py:386-387: the odd size int(3 s) (+ 1 if even), clamped to 3 .. 13."""
    k = int(3 * blur_sigma) + 1 if int(3 * blur_sigma) % 2 == 0 else int(3 * blur_sigma)
    return max(3, min(k, 13))


def gaussian_kernel1d(k, sigma):
    half = (k - 1) * 0.5
    x = torch.linspace(-half, half, steps=k)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


def gaussian_blur(img, k, sigma, dtype=None):
    """img [N, C, H, W] -> the blurred planes; `dtype` (e.g. float64): run the padding and convolution in it, with the float32 weights
    cast exactly (an accuracy reference for the HIP kernel)."""
    dtype = dtype or img.dtype
    w1 = gaussian_kernel1d(k, sigma).to(dtype)
    w2 = torch.mm(w1[:, None], w1[None, :])
    c = img.shape[-3]
    x = F.pad(img.to(dtype), [k // 2] * 4, mode="reflect")
    return F.conv2d(x, w2.expand(c, 1, k, k), groups=c)


class GaussianBlur:
    """transforms.GaussianBlur(kernel_size, sigma) with a single number for both: the stand-in the fixture script installs."""

    def __init__(self, kernel_size, sigma):
        self.kernel_size = int(kernel_size)
        self.sigma = (float(sigma), float(sigma))

    def __call__(self, img):
        sigma = torch.empty(1).uniform_(self.sigma[0], self.sigma[1]).item()
        return gaussian_blur(img, self.kernel_size, sigma)


def blur(vid, blur_sigma):
    """helpers/generator.py:381-390 on [B, T, C, H, W]."""
    bs, t = vid.shape[:2]
    out = GaussianBlur(kernel_size(blur_sigma), blur_sigma)(vid.reshape(-1, *vid.shape[2:]))
    return out.view(bs, t, *vid.shape[2:])
