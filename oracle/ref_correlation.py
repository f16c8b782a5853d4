"""ctypes binding of `oracle/_ref/libccvs_ref_correlation.so`: the reference's own 7x7 correlation kernel, compiled by
`oracle/build_ref_correlation.py` (see there).  TEST INFRASTRUCTURE: only tests import this module."""
import ctypes
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_ref", "libccvs_ref_correlation.so")

_LIB = []


def load():
    if not _LIB:
        if not os.path.isfile(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not found: the reference correlation oracle is not built. Run "
                               "`python -c \"import __graft_entry__ as g; g.build()\"` with the reference checkout named by "
                               "CCVS_REFERENCE_ROOT (or `python oracle/build_ref_correlation.py`)")
        lib = ctypes.CDLL(LIB_PATH)
        vp, i32 = ctypes.c_void_p, ctypes.c_int32
        lib.ref_correlation7x7.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp]
        lib.ref_correlation7x7.restype = ctypes.c_int
        _LIB.append(lib)
    return _LIB[0]


def ref_correlation(first, second, stride):
    """The reference's `FunctionCorrelation(first, second, stride)` forward on the current stream: first, second [N, C, H, W]
    float32 on the GPU -> [N, 49, ceil(H/s), ceil(W/s)]."""
    assert first.is_cuda and second.is_cuda and first.dtype == second.dtype == torch.float32
    assert first.shape == second.shape and first.dim() == 4, (first.shape, second.shape)
    first, second = first.contiguous(), second.contiguous()
    n, c, h, w = first.shape
    s = int(stride)
    out = torch.empty(n, 49, -(-h // s), -(-w // s), dtype=torch.float32, device=first.device)
    err = load().ref_correlation7x7(ctypes.c_void_p(first.data_ptr()), ctypes.c_void_p(second.data_ptr()),
                                    ctypes.c_void_p(out.data_ptr()), n, c, h, w, s,
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if err != 0:
        raise RuntimeError(f"ref_correlation7x7 failed with hipError_t {err}")
    return out
