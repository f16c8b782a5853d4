"""not gpu: the STFT decoder's yardstick and host side.

  1. the CPU composition of tests/stft_decoder_ref.py (oracle `conv_layer` x 5, tanh, embedding lookup, `F.mse_loss`) against the
     reference's own outputs stored in tests/golden/tiny_stft_decoder.npz (tests/golden/make_stft_decoder_golden.py);
  2. the same against the live reference on fresh seeds, where a reference checkout is present;
  3. `StftDecoder`'s state-dict layout and seeded initial values against the reference's (the seeded `StftModel`: GPU file);
  4. the header declares and the library exports `ccvs_channel_head` / `ccvs_mse`, the ABI version stays 6;
  5. `--decode_stft` parses, is off by default, needs `--x_stft`, and moves no other option of the reference's launch lines.
"""
import argparse
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402
import stft_decoder_ref as R  # noqa: E402

T = torch.from_numpy
ONE_ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "tiny_stft_decoder.npz"))


def nets_of(gold, prefixes=("ae", "ad", "aq")):
    return {p: {k[len(p) + 1:]: T(gold[k]) for k in gold.files if k.startswith(p + "/")} for p in prefixes}


def tiny_aopt():
    from ccvs_amd.tools.options import Options
    return Options().parse(True, True, load_state_estimator=True, load_stft_ae=True, argv=rh.TINY_STATE_ARGV)["stft_ae"]


def test_composition_equals_the_reference_outputs(gold, golden_dir):
    """The yardstick of the GPU tests: same arithmetic on the same kind of CPU, 1e-5 abs (the fp32 op bar); the losses within one
    fp32 rounding.  The stored reference output must be large enough for a 1e-3 comparison against it to mean something."""
    nets = nets_of(gold)
    vid, img = T(gold["vid_decoder"]), T(gold["img_decoder"])
    assert R.well_conditioned(vid), "the fixture's reference output is too small to test against"
    assert vid.shape == (2, 5, 1, 16, 8) and img.shape == (2, 1, 16, 8)
    codes = T(gold["state_code"])
    with torch.no_grad():
        d_vid = (R.stft_decode(nets, [2, 1], codes, "vid") - vid).abs().max().item()
        d_img = (R.stft_decode(nets, [2, 1], codes[:, :2], "img") - img).abs().max().item()
        loss, pred, _ = R.eval_stft_reconstruction(nets, T(gold["stft"]))
    print(f"composition vs stored reference: vid {d_vid:.3e} img {d_img:.3e} loss {loss.item():.8f} / {float(gold['eval_stft_reconstruction']):.8f}")
    assert d_vid <= 1e-5 and d_img <= 1e-5
    assert (pred - T(gold["eval_stft_pred"])).abs().max().item() <= 1e-5
    want = float(gold["eval_stft_reconstruction"])
    assert abs(loss.item() - want) <= ONE_ULP * abs(want)
    # eval_state_estimator on the networks and inputs of tiny_statemodel.npz
    base = np.load(os.path.join(golden_dir, "tiny_statemodel.npz"))
    snets = {"s": {k[2:]: T(base[k]) for k in base.files if k.startswith("s/")},
             "sq": {k[3:]: T(base[k]) for k in base.files if k.startswith("sq/")}}
    from ccvs_amd.tools.options import Options
    sopt = Options().parse(True, True, load_state_estimator=True, argv=rh.TINY_STATEMODEL_ARGV)["state_estimator"]
    with torch.no_grad():
        s_loss, s_q, _ = R.eval_state_estimator(snets, sopt, T(base["z"]), T(base["given"]))
    want = float(gold["eval_state_estimator"])
    assert abs(s_loss.item() - want) <= ONE_ULP * abs(want)
    assert (s_q - T(gold["eval_state_q"])).abs().max().item() <= 1e-7


@pytest.mark.skipif(not rh.reference_available(), reason="no reference checkout (CCVS_REFERENCE_ROOT)")
def test_composition_equals_the_live_reference_on_fresh_seeds():
    ns = rh.load_reference()
    aopt = rh.parse_reference_options(rh.TINY_STATE_ARGV)["stft_ae"]
    for seed in (101, 202):
        torch.manual_seed(seed)
        sm = ns.stft_model.StftModel(aopt, is_train=False, is_main=False).eval()
        sds = {"ae": sm.net_e.state_dict(), "ad": sm.net_d.state_dict(), "aq": sm.net_q.state_dict()}
        with torch.no_grad():
            R.condition_weights(sds["ae"], sds["ad"], sds["aq"], 4.0, seed, last_factor=16.0)
            stft = torch.rand(2, 3, 1, 16, 8) * 2 - 1
            codes = torch.randint(0, aopt.stft_num, (2, 3 * 2))
            vid = sm({"state_code": codes.clone()}, mode="vid_decoder")["stft"]
            img = sm({"state_code": codes[:, :2].clone()}, mode="img_decoder")["stft"]
            loss = sm({"stft": stft.clone()}, mode="eval_stft_reconstruction")
            assert (R.stft_decode(sds, aopt.stft_shape, codes, "vid") - vid).abs().max().item() <= 1e-5
            assert (R.stft_decode(sds, aopt.stft_shape, codes[:, :2], "img") - img).abs().max().item() <= 1e-5
            got = R.eval_stft_reconstruction(sds, stft)[0]
            assert abs(got.item() - loss.item()) <= ONE_ULP * abs(loss.item())


def test_stft_decoder_layout_and_seeded_values(gold):
    from ccvs_amd.models.skip_vid_generator.models import skip_autoencoder as sae
    torch.manual_seed(0)
    net = sae.StftDecoder(tiny_aopt())
    own = {k: v for k, v in net.state_dict().items() if not k.endswith(".kernel")}
    ref = {k[3:]: gold[k] for k in gold.files if k.startswith("ad/")}
    assert set(own) == set(ref), set(own) ^ set(ref)
    assert "convs.0.0.weight" in own and "convs.4.0.bias" in own
    for k, v in own.items():
        assert tuple(v.shape) == ref[k].shape, k
    kernels = [k for k in net.state_dict() if k.endswith(".kernel")]
    assert kernels == ["convs.1.1.kernel", "convs.2.1.kernel", "convs.3.1.kernel"]
    for k in ("convs.0.0.weight", "convs.4.0.weight"):
        assert np.array_equal(own[k].numpy(), gold["seed0/" + k]), f"{k}: initialiser stream differs from the reference"
    # a reference checkpoint (its state dict, blur buffers included) loads unchanged
    full = dict(ref)
    full.update({k: net.state_dict()[k].numpy() for k in kernels})
    net.load_state_dict({k: T(np.asarray(v)) for k, v in full.items()}, strict=True)


def test_new_symbols_declared_and_exported():
    from ccvs_amd import lib
    header = open(os.path.join(ROOT, "include", "ccvs_hip.h")).read()
    handle = ctypes.CDLL(lib.LIB_PATH)
    for sym in ("ccvs_channel_head", "ccvs_mse"):
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in lib.EXPORTS and hasattr(handle, sym), sym
    handle.ccvs_abi_version.restype = ctypes.c_int
    assert handle.ccvs_abi_version() == 6
    from ccvs_amd import ops
    with pytest.raises(lib.CcvsError):
        ops.channel_head(torch.zeros(1, 4, 2, 2), torch.zeros(4), 0.5)
    with pytest.raises(lib.CcvsError):
        ops.mse(torch.zeros(4), torch.zeros(4))


def _plain(v):
    return list(v) if isinstance(v, (list, tuple)) else v


def test_decode_stft_option(golden_dir):
    from ccvs_amd.tools.options import Options
    from ccvs_amd.helpers.generator import Generator
    parse = lambda argv: Options().parse(True, True, load_state_estimator=True, load_stft_ae=True, argv=argv)
    off, on = parse(rh.TINY_STATE_ARGV), parse(rh.TINY_STATE_ARGV + ["--decode_stft"])
    assert off["transformer"].decode_stft is False and on["transformer"].decode_stft is True
    action = [a for a in Options().initialize(argparse.ArgumentParser())._actions if "--decode_stft" in a.option_strings]
    assert len(action) == 1 and action[0].help.startswith("(ccvs_amd)") and action[0].default is False
    assert Generator(on).decode_stft and not Generator(off).decode_stft
    with pytest.raises(ValueError, match="x_stft"):
        Generator(parse(rh.TINY_ARGV + ["--decode_stft"]))
    with pytest.raises(NotImplementedError):
        Generator(parse(rh.TINY_STATE_ARGV + ["--decode_stft", "--step_by_step"]))
    # every launch line of the reference still parses to the values the reference's own parser gives; the flag moves nothing else
    with open(os.path.join(golden_dir, "reference_launch_lines.json")) as f:
        lines = json.load(f)
    with open(os.path.join(golden_dir, "reference_checks.json")) as f:
        parsed = json.load(f)["launch_lines"]
    for script, argv in sorted(lines.items()):
        got, got_on = parse(argv), parse(argv + ["--decode_stft"])
        assert got["transformer"].decode_stft is False
        for key in ("transformer", "qvid_generator", "stft_ae"):
            fields = rh.LAUNCH_LINE_FIELDS[key]
            if key == "stft_ae" and not ("stft_ae" in parsed[script] and "--x_stft" in argv):
                continue
            for f in fields:
                if f in parsed[script][key]:
                    assert _plain(getattr(got[key], f)) == parsed[script][key][f], (script, key, f)
            a, b = vars(got[key]), vars(got_on[key])
            assert {k: v for k, v in a.items() if k not in ("decode_stft", "signature") and not k.endswith("_path")} == \
                   {k: v for k, v in b.items() if k not in ("decode_stft", "signature") and not k.endswith("_path")}, (script, key)
