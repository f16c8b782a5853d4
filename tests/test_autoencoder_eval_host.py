"""not gpu: the yardstick and the host side of the frame autoencoder's validation figures.

  1. tests/golden/tiny_aeval.npz meets the conditions its maker asserts (`aeval_ref.conditions`): on both launch lines the nearest two
     codewords are at least 1e-4 apart in squared distance at every position, at least 4 codes are used, 2 <= perplexity <= n_e - 1,
     and the reference's L1 is at least ten times the pixel bar;
  2. the float64 restatements of tests/aeval_ref.py reproduce the reference's own values from the reference's z, indices and decoded
     frames, within the bounds the GPU tests use -- so those bounds are checked here against the reference alone;
  3. include/ccvs_hip_eval.h, which include/ccvs_hip.h includes, declares the five new symbols and nothing else, the built library
     exports them, `lib.py` lists them in `EVAL_EXPORTS`, the ABI version stays 6, a C program that includes ccvs_hip.h alone sees
     the prototypes, CPU tensors raise.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import aeval_ref as A  # noqa: E402
import ref_harness as rh  # noqa: E402

N_E = 32   # --q_z_num of the tiny launch lines

SYMBOLS = ("ccvs_l1_workspace_bytes", "ccvs_l1_mean", "ccvs_vq_stats_workspace_bytes", "ccvs_vq_stats", "ccvs_code_perplexity")


def test_fixture_meets_its_conditions(golden_dir):
    gold, lines = A.load_gold(golden_dir)
    assert lines == {"plain": list(rh.TINY_ARGV), "norm": list(rh.TINY_ARGV) + ["--q_normalize_out"]}
    assert gold["img"].shape == (8, 3, 32, 32)
    assert np.array_equal(gold["img"], A.frames(int(gold["clip"][0]), float(gold["clip"][1])).numpy())
    for line in A.LINES:
        A.conditions(gold, line, N_E)
        assert gold[f"{line}/code"].shape == (8 * 64,) and gold[f"{line}/z"].shape == (8, 16, 8, 8)
        assert gold[f"{line}/fake_img"].shape == (8, 3, 32, 32)
    assert os.path.getsize(os.path.join(golden_dir, "tiny_aeval.npz")) < 1 << 20


@pytest.mark.parametrize("line", A.LINES)
def test_float64_restatements_reproduce_the_reference(golden_dir, line):
    gold, _ = A.load_gold(golden_dir)
    cb = A.weights(golden_dir, gold, line, "q")["embedding.weight"].numpy()
    z, code = gold[f"{line}/z"], gold[f"{line}/code"].astype(np.int64)
    scale = A.row_scale64(cb) if line == "norm" else None
    m, counts = A.vq_stats64(z, code, cb, scale)
    used = int((counts > 0).sum())
    # the codes are the nearest rows of this codebook, by the fixture's margin
    zf = np.moveaxis(z.reshape(8, 16, 64), 1, 2).reshape(-1, 16).astype(np.float64)
    assert np.array_equal(((zf[:, None, :] - cb[None].astype(np.float64)) ** 2).sum(axis=2).argmin(axis=1), code)
    assert abs(A.top2_gap64(z, cb) - float(gold[f"{line}/min_gap"])) <= 1e-12
    # quantiser loss: float64 against the reference's fp32 value -- within the GPU bound with delta = 0 (its 1e-6 relative part)
    loss = (1.0 + A.BETA) * m
    ref_loss = float(gold[f"{line}/q_loss"])
    print(f"{line}: q_loss f64 {loss:.9f} / reference {ref_loss:.9f}; bound at delta 1e-4: {A.quant_loss_bound(float(gold[f'{line}/max_dz']), ref_loss):.3e}")
    assert abs(loss - float(gold[f"{line}/q_loss64"])) <= 1e-12
    assert abs(loss - ref_loss) <= A.quant_loss_bound(float(gold[f"{line}/max_dz"]), ref_loss, delta=0.0)
    assert A.quant_loss_bound(float(gold[f"{line}/max_dz"]), ref_loss) < 0.01 * ref_loss   # the bound says something
    # perplexity: float64 against the reference's fp32 value
    ppl = A.perplexity64(counts, code.size)
    ref_ppl = float(gold[f"{line}/perplexity"])
    print(f"{line}: perplexity f64 {ppl:.9f} / reference {ref_ppl:.9f}; bound {A.perplexity_bound(used, ref_ppl):.3e}")
    assert abs(ppl - float(gold[f"{line}/perplexity64"])) <= 1e-12
    assert abs(ppl - ref_ppl) <= A.perplexity_bound(used, ref_ppl)
    # L1: float64 of the reference's frames against its fp32 mean
    l1 = A.l1_mean64(gold["img"], gold[f"{line}/fake_img"])
    assert abs(l1 - float(gold[f"{line}/l1"])) <= 1e-6 * l1
    # max|z_q - z| as recorded
    rows = cb.astype(np.float64)[code] * (1.0 if scale is None else scale[code][:, None])
    zq = rows.reshape(8, 64, 16).transpose(0, 2, 1).reshape(z.shape)
    assert abs(np.abs(zq - z).max() - float(gold[f"{line}/max_dz"])) <= 1e-12


def test_restatements_on_known_answers():
    assert A.perplexity64([5, 5, 5, 5], 20) == pytest.approx(4.0, rel=1e-8)
    assert A.perplexity64([7, 0, 0], 7) == pytest.approx(1.0, rel=1e-8)
    z = np.zeros((1, 2, 1, 3))
    z[0, :, 0, 1] = [1.0, 2.0]
    m, counts = A.vq_stats64(z, [0, 1, 0], np.array([[0.0, 0.0], [1.0, 0.0]]))
    assert m == pytest.approx(4.0 / 6.0) and counts.tolist() == [2, 1]
    m, counts = A.vq_stats64(z, [0, 2, -1], np.array([[0.0, 0.0], [1.0, 0.0]]))
    assert np.isnan(m) and counts.tolist() == [1, 0]
    assert A.l1_mean64([1.0, -1.0, 0.0], [0.0, 1.0, 0.0]) == pytest.approx(1.0)


def test_new_symbols_declared_and_exported(tmp_path):
    from ccvs_amd import lib, ops
    header = open(os.path.join(ROOT, "include", "ccvs_hip_eval.h")).read()
    assert re.search(r'^#include "ccvs_hip_eval.h"', open(os.path.join(ROOT, "include", "ccvs_hip.h")).read(), re.M)
    assert sorted(set(re.findall(r"\b(ccvs_[a-zA-Z0-9_]+)\s*\(", header))) == sorted(SYMBOLS) == sorted(lib.EVAL_EXPORTS)
    assert not set(lib.EVAL_EXPORTS) & set(lib.EXPORTS)
    handle = ctypes.CDLL(lib.LIB_PATH)
    for sym in SYMBOLS:
        assert hasattr(handle, sym), sym
    # a C program that includes ccvs_hip.h alone gets the prototypes (taking a function's address needs its declaration)
    c = tmp_path / "p.c"
    c.write_text('#include "ccvs_hip.h"\nvoid* p[] = {' + ", ".join("(void*)" + s for s in SYMBOLS) + "};\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "p.o")], check=True)
    handle.ccvs_abi_version.restype = ctypes.c_int
    assert handle.ccvs_abi_version() == 6
    L = lib.load()
    # the workspace sizes are host functions of the shape alone: one float64 per stage-1 workgroup
    assert L.ccvs_l1_workspace_bytes(1) == 8 and L.ccvs_l1_workspace_bytes(0) == 0
    assert L.ccvs_l1_workspace_bytes(16 * 16 * 3 * 256 * 256) == L.ccvs_l1_workspace_bytes(1 << 40) == 8 * 1024
    assert L.ccvs_vq_stats_workspace_bytes(256, 512, 64) == 8 * 256 * 8 and L.ccvs_vq_stats_workspace_bytes(1, 1, 1) == 8
    with pytest.raises(lib.CcvsError):
        ops.l1_mean(torch.zeros(4), torch.zeros(4))
    with pytest.raises(lib.CcvsError):
        ops.vq_stats(torch.zeros(1, 2, 1, 1), torch.zeros(1, dtype=torch.int64), torch.zeros(4, 2))
    with pytest.raises(lib.CcvsError):
        ops.code_perplexity(torch.ones(4, dtype=torch.int32), 4)
