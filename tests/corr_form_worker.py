"""Worker of tests/test_correlation_ref_gpu.py::test_pair_form_bits_equal_single_pixel_form: runs `ops.correlation7x7` over FORM_CASES
under whatever CCVS_CORR_PAIR the parent set (the library reads the switch once per process) and writes the results to the .npz
named on the command line.  The parent imports FORM_CASES and form_inputs from here, so both processes see the same inputs."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (C, H, W, first_div): every case runs at stride 1 and 2, lrelu off and on.  Output widths Wo = ceil(W / s) of 63, 64, 65, 66,
# 126 and 128 reach both tile widths and, where Wo is even and >= 64, the two-pixel form (at stride 2: W = 127, 128, 131, 256);
# Ho % 8 takes 0, 1 and 7 at both strides; C % 8 takes 0, 1 and 7 around the 8-channel chunk, C < 8 included; H or W < 7.
FORM_CASES = (
    (1, 8, 63, 1), (3, 9, 64, 2), (7, 15, 65, 3), (8, 16, 66, 15), (9, 17, 128, 1), (17, 23, 127, 2), (24, 16, 256, 3),
    (15, 9, 129, 15), (33, 14, 131, 1), (16, 33, 130, 2), (12, 17, 126, 3), (40, 7, 64, 15), (5, 3, 5, 1), (2, 6, 70, 2),
    (31, 1, 1, 3),
)
STRIDES = (1, 2)


def form_inputs(i, case):
    """first [N / div, C, H, W] (distinct images), second [N, C, H, W]; N = 2 div, or div when div = 15."""
    c, h, w, div = case
    n = div if div == 15 else 2 * div
    g = torch.Generator().manual_seed(1000 + i)
    first = torch.randn(n // div, c, h, w, generator=g) * 0.8 + 0.1
    second = torch.randn(n, c, h, w, generator=g) * 1.3 - 0.2
    return first, second


def run_forms(device="cuda"):
    from ccvs_amd import ops
    out = {}
    for i, case in enumerate(FORM_CASES):
        first, second = (t.to(device) for t in form_inputs(i, case))
        for s in STRIDES:
            for lrelu in (False, True):
                out[f"{i}_s{s}_l{int(lrelu)}"] = ops.correlation7x7(first, second, s, first_div=case[3], lrelu=lrelu)
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    got = run_forms()
    np.savez(sys.argv[1], **{k: v.cpu().numpy() for k, v in got.items()})
