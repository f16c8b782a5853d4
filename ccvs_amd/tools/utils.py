"""The three tensor helpers of the reference's tools/utils.py that sit on the hot path
(tools/utils.py:40-62), plus the small host helpers helpers/generator.py imports."""
import os

import numpy as np
import torch


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("ccvs_amd needs a GPU: the synthesis path runs on HIP kernels only (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def to_cuda(tensor_dic, key, flatten_empty=True):
    """tools/utils.py:40-48: move `tensor_dic[key]` (tensor or list of tensors) to the GPU;
    a missing key yields an empty tensor."""
    dev = _device()
    if key in tensor_dic:
        if isinstance(tensor_dic[key], list):
            return [t.to(dev) for t in tensor_dic[key]]
        if 0 in tensor_dic[key].size() and flatten_empty:
            tensor_dic[key] = torch.Tensor([])
        return tensor_dic[key].to(dev)
    return torch.Tensor([]).to(dev)


def flatten_vid(x, vid_ndim=5):
    """tools/utils.py:50-55."""
    vid_size = None
    if x.ndim == vid_ndim:
        vid_size = x.shape[:2]
        x = x.reshape(-1, *x.shape[2:])
    return x, vid_size


def unflatten_vid(x, vid_size):
    """tools/utils.py:57-62."""
    if vid_size is not None and x.size(0) != 0:
        b, t = vid_size
        return x.view(b, t, *x.shape[1:])
    return x


def mkdir(path):
    """tools/utils.py:19-21."""
    os.makedirs(path, exist_ok=True)


def mkdirs(paths):
    """tools/utils.py:12-17."""
    for path in ([paths] if isinstance(paths, str) else list(paths)):
        mkdir(path)


def _psd_sqrt(sigma):
    """The symmetric square root of a covariance matrix by `eigh`.  Negative eigenvalues are clipped to 0, and so are the positive
    ones under the solver's own error, n eps max|lam|: an exact zero comes back as +-that much, and the square root of such noise
    (~1e-8 sqrt(max)) would put rank into directions that have none."""
    lam, vec = np.linalg.eigh((sigma + sigma.T) / 2)
    floor = len(lam) * np.finfo(np.float64).eps * np.abs(lam).max(initial=0.0)
    return (vec * np.sqrt(np.where(lam > floor, lam, 0.0))) @ vec.T


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2):
    """tools/utils.py:65-116: the Frechet distance |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2) between two Gaussians, float64, with
    numpy alone (the reference calls scipy.linalg.sqrtm on the unsymmetric product S1 S2 and drops the imaginary part of the result).
    With R1 = sqrt(S1), R2 = sqrt(S2) (`_psd_sqrt`), S1 S2 has the eigenvalues of the symmetric positive semi-definite
    R1 S2 R1 = (R1 R2)(R1 R2)^T, so tr sqrt(S1 S2) is the sum of the square roots of that matrix's eigenvalues -- the sum of the singular
    values of R1 R2, which is how it is computed: `eigvalsh(R1 S2 R1)` returns an exact zero as +-eps |S1||S2| and its square root as
    ~1e-8, several hundred times over when there are fewer samples than dimensions, whereas a singular value comes back within eps
    |R1 R2| of itself.  Nothing complex arises, rank-deficient covariances included, so the reference's `eps` retry has no counterpart."""
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, dtype=np.float64)), np.atleast_1d(np.asarray(mu2, dtype=np.float64))
    sigma1, sigma2 = np.atleast_2d(np.asarray(sigma1, dtype=np.float64)), np.atleast_2d(np.asarray(sigma2, dtype=np.float64))
    assert mu1.shape == mu2.shape, "Training and test mean vectors have different lengths"
    assert sigma1.shape == sigma2.shape, "Training and test covariances have different dimensions"
    diff = mu1 - mu2
    tr_covmean = np.linalg.svd(_psd_sqrt(sigma1) @ _psd_sqrt(sigma2), compute_uv=False).sum()
    return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * tr_covmean


class DummyOpt:
    """tools/utils.py:128-136: a no-op optimiser stand-in."""

    def zero_grad(self):
        pass

    def step(self):
        pass


def color_transfer(im, colormap):
    """tools/utils.py:138-147 colours a semantic layout: layouts are outside the hot path."""
    raise NotImplementedError("layout colour maps are outside the MI355X hot path")

