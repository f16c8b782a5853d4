"""not gpu: the host side and the yardstick of the transformer's teacher-forced loss.

  1. `loss_rows` against the reference's list comprehensions (transformer_model.py:215-220, restated in tests/tloss_ref.py): both
     layouts, `state_size` 1 and 3, one to three frames, logits that end mid-frame;
  2. the fixture tests/golden/tiny_tloss.npz is conditioned (its per-token NLLs spread), and `oracle.gpt_forward` + `F.cross_entropy`
     reproduces every `t_loss` and per-token value of it within 1e-6: the composition the GPU tests compare against;
  3. the header declares and the library exports `ccvs_token_nll` / `ccvs_mean_f32`, the ABI version stays 6, CPU tensors raise;
  4. `ccvs_amd` never imports the oracle.
"""
import ctypes
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import tloss_ref as R  # noqa: E402


@pytest.mark.parametrize("state_front", [False, True])
@pytest.mark.parametrize("state_size", [1, 3])
def test_loss_rows_equal_the_reference_lists(state_size, state_front):
    from ccvs_amd.models.skip_vid_generator.models.transformer_model import loss_rows
    size, num_blocks = 4, 3
    tot = size + state_size
    lengths = [f * tot - 1 for f in (1, 2, 3)] + [tot + 2, 2 * tot + state_size, 1, 0]   # whole frames; mid-frame; degenerate
    for n in lengths:
        got = loss_rows(n, state_size, tot, num_blocks, state_front)
        want = R.reference_rows(n, state_size, tot, num_blocks, state_front)
        assert got == want, (n, state_size, state_front)
        assert sorted(got[0] + got[1]) == list(range(n))
    if not state_front:   # a known answer: 2 frames of 1 state + 4 frame tokens, 9 logits -> position 5 is the second frame's state slot
        assert loss_rows(2 * (4 + 1) - 1, 1, 5, 3, False) == ([4], [0, 1, 2, 3, 5, 6, 7, 8])


def test_fixture_is_conditioned_and_the_oracle_composition_reproduces_it(golden_dir):
    gold, cases = R.load_gold(golden_dir)
    assert float(gold["head_factor"]) > 1.0
    assert set(cases) == {"plain", "crop", "p2p", "start", "label", "state2", "state3", "state_front", "deblur"}
    for name, case in cases.items():
        xopt = R.transformer_options(case["argv"])
        nll, state_nll, want = gold[f"{name}/nll"], gold[f"{name}/state_nll"], float(gold[f"{name}/t_loss"])
        assert R.well_conditioned(nll, xopt.z_num), f"{name}: the fixture's NLLs say nothing (all ~ log V)"
        d = R.inputs_of(gold, name)
        t_loss, f, s = R.oracle_loss(R.weights_of(gold, case["net"]), xopt, d)
        print(f"{name}: t_loss {t_loss.item():.7f} / {want:.7f}  per-token max|diff| {(f - torch.from_numpy(nll)).abs().max().item():.2e}")
        assert abs(t_loss.item() - want) <= 1e-6 * max(1.0, abs(want)), name
        assert tuple(f.shape) == nll.shape and tuple(s.shape) == state_nll.shape, name
        assert (f - torch.from_numpy(nll)).abs().max().item() <= 1e-5
        if s.numel():
            assert (s - torch.from_numpy(state_nll)).abs().max().item() <= 1e-5
        assert (s.numel() > 0) == (d["state_code"].numel() > 0)
    assert gold["crop/code"].shape[1] > R.transformer_options(cases["crop"]["argv"]).z_len
    assert gold["crop/nll"].shape[1] == R.transformer_options(cases["crop"]["argv"]).z_len - 1


def test_new_symbols_declared_and_exported():
    from ccvs_amd import lib, ops
    header = open(os.path.join(ROOT, "include", "ccvs_hip.h")).read()
    handle = ctypes.CDLL(lib.LIB_PATH)
    for sym in ("ccvs_token_nll", "ccvs_mean_f32"):
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in lib.EXPORTS and hasattr(handle, sym), sym
    handle.ccvs_abi_version.restype = ctypes.c_int
    assert handle.ccvs_abi_version() == 6
    with pytest.raises(lib.CcvsError):
        ops.token_nll(torch.zeros(3, 8), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(lib.CcvsError):
        ops.mean_f32(torch.zeros(4))


def test_product_does_not_import_the_oracle():
    for base, _, files in os.walk(os.path.join(ROOT, "ccvs_amd")):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(base, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", text, re.M), f"{f} imports the oracle"
