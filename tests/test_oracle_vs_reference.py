"""not gpu: the oracle against outputs of the REAL reference, stored under tests/golden/ (reference_checks.npz / .json:
`make_golden.py refchecks`, which imports the reference through tests/golden/ref_harness.py; the weights are re-drawn
from their stored spec by `ref_harness.seeded_weights`, the uint8 outputs are compared by SHA-256):
freshly initialised encoder / decoder, the GPT's position modes, the bytes of `save_video_batch`, and the reference's own
parser on every `scripts/*/save_videos*.sh` launch line."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import ref_harness as rh  # noqa: E402
from oracle import ccvs_oracle as O  # noqa: E402

T = torch.from_numpy


@pytest.fixture(scope="module")
def ref(golden_dir):
    return np.load(os.path.join(golden_dir, "reference_checks.npz"))


@pytest.fixture(scope="module")
def ref_meta(golden_dir):
    with open(os.path.join(golden_dir, "reference_checks.json")) as f:
        return json.load(f)


def _weights(ref_meta, key):
    return rh.seeded_weights(ref_meta[key]["spec"], ref_meta[key]["seed"])


def _same_bytes(u8, want):
    assert list(u8.shape) == want["shape"] and str(u8.dtype) == want["dtype"]
    assert hashlib.sha256(u8.contiguous().numpy().tobytes()).hexdigest() == want["sha256"]


def test_encoder_decoder_fresh_weights(ref, ref_meta):
    """New seed, new input: reference modules vs the oracle driven by their state dicts."""
    from ccvs_amd.tools.options import Options
    opt = Options().parse(load_qvid_generator=True, load_transformer=True, argv=rh.TINY_ARGV)["qvid_generator"]
    enc, dec = _weights(ref_meta, "fresh/enc"), _weights(ref_meta, "fresh/dec")
    vid, z = T(ref["fresh/vid"]), T(ref["fresh/z"])
    inter = [T(ref[f"fresh/inter{i}"]) for i in range(int(ref["fresh/n_inter"]))]
    with torch.no_grad():
        oz, ointer = O.encoder_forward(enc, opt, vid)
        assert len(ointer) == len(inter)
        assert torch.equal(z, oz) and all(torch.equal(a, b) for a, b in zip(inter, ointer))
        ctx = [[f[:, :1] for f in inter], [f[:, 1:] for f in inter]]
        orgb, oflows, ooccs = O.decoder_forward(dec, opt, z[:, :1].contiguous(), ctx, return_all=True)
        assert (T(ref["fresh/rgb"]) - orgb).abs().max() < 1e-6
        flows_occs = [T(ref[f"fresh/flow_occ{i}"]) for i in range(2 * int(ref["fresh/n_flows"]))]
        assert len(flows_occs) == len(oflows) + len(ooccs)
        for a, b in zip(flows_occs, oflows + ooccs):
            assert (a - b).abs().max() < 1e-6


def test_gpt_spatio_temporal_and_flat_positions(ref, ref_meta):
    for mode in ("spatio-temporal", None):
        tag = f"gpt_{mode or 'flat'}"
        cfg = O.namespace(z_shape=[4, 4], emb_mode=mode, n_layer=1, n_head=2, z_len=48)
        with torch.no_grad():
            got = O.gpt_forward(_weights(ref_meta, tag), cfg, T(ref[f"{tag}/idx"]))
        assert (T(ref[f"{tag}/logits"]) - got).abs().max() < 1e-6


def test_output_stage_vs_reference_save_video_batch(ref_meta):
    """The oracle's output stage (clamp / rescale / x255 / uint8, the imagenet de-normalisation branch, the 3x3 state marker)
    against the reference's own `save_video_batch` (helpers/generator.py:285-333) with `torchvision.io.write_video` replaced
    by a recorder: byte for byte, including a marker clipped at the frame border."""
    vid = torch.rand(2, 3, 3, 64, 64, generator=torch.Generator().manual_seed(1)) * 2.4 - 1.2
    state = torch.tensor([[[0.5, 0.25]] * 3, [[0.999, 0.0]] * 3])      # the second marker sits in a corner: clipped cross
    want = ref_meta["save_video_batch"]
    assert want["bair_state"]["names"] == ["vid_00006.mp4", "vid_00007.mp4"]
    _same_bytes(O.mark_state(O.pack_u8(vid), state, "bair"), want["bair_state"])
    _same_bytes(O.pack_u8(vid), want["bairhd"])
    _same_bytes(O.pack_u8_imagenet(vid), want["kinetics600"])


def _plain(v):
    """The stored values went through JSON: tuples are lists there."""
    return json.loads(json.dumps(v))


def test_every_reference_save_script_parses_like_the_reference(ref_meta, golden_dir):
    """The flags of all nine `scripts/*/save_videos*.sh` launch lines: the product's `Options` must accept them (training-only
    flags ignored) and give the fields the synthesis path reads the values the reference's own parser gives."""
    from ccvs_amd.tools.options import Options
    with open(os.path.join(golden_dir, "reference_launch_lines.json")) as f:
        lines = json.load(f)
    parsed = ref_meta["launch_lines"]
    assert len(lines) >= 9 and sorted(parsed) == sorted(lines)
    x_fields, q_fields = rh.LAUNCH_LINE_FIELDS["transformer"], rh.LAUNCH_LINE_FIELDS["qvid_generator"]
    for script, argv in sorted(lines.items()):
        want = parsed[script]
        got = Options().parse(load_qvid_generator=True, load_transformer=True, load_state_estimator=True, load_stft_ae=True, argv=argv)
        for key, fields in (("transformer", x_fields), ("qvid_generator", q_fields)):
            for f in fields:
                if f in want[key]:
                    assert _plain(getattr(got[key], f)) == want[key][f], (script, key, f, getattr(got[key], f), want[key][f])
        if "stft_ae" in want and "--x_stft" in argv:
            for f in rh.LAUNCH_LINE_FIELDS["stft_ae"]:
                assert _plain(getattr(got["stft_ae"], f)) == want["stft_ae"][f], (script, f)
