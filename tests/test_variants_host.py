"""not gpu: the flow-decoder variants of Matching (--q_use_masked_flow, --q_use_deformed_conv, --q_use_tradeoff, --q_no_corr):
every variant's decoder constructs with the reference's parameter names, shapes and order, and loads a reference-layout state
dict strictly (tests/golden/tiny_variants.json, made by make_golden_variants.py); and the CPU DeformConv2d restatement the
fixtures and the GPU tests rely on is pinned against plain convolutions and a hand-computed case."""
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import deform_ref  # noqa: E402
import ref_harness as rh  # noqa: E402

META = json.load(open(os.path.join(HERE, "golden", "tiny_variants.json")))
CONFIGS = sorted(META["configs"])


def _decoder(name):
    from ccvs_amd.tools.options import Options
    from ccvs_amd.models.skip_vid_generator.models.skip_autoencoder import SkipGANDecoder
    opt = Options().parse(load_qvid_generator=True, load_transformer=True, argv=META["argv"] + META["configs"][name]["flags"])
    return SkipGANDecoder(opt["qvid_generator"])


@pytest.mark.parametrize("name", CONFIGS)
def test_variant_state_dict_layout(name):
    dec = _decoder(name)
    own = [[k, list(v.shape)] for k, v in dec.state_dict().items() if not k.endswith(".kernel")]
    assert own == META["configs"][name]["state_dict"]   # names, shapes and order


@pytest.mark.parametrize("name", CONFIGS)
def test_variant_loads_reference_layout_strictly(name):
    dec = _decoder(name)
    sd = rh.seeded_weights(META["configs"][name]["weight_spec"], META["weight_seed"])
    sd.update({k: v for k, v in dec.state_dict().items() if k.endswith(".kernel")})
    dec.load_state_dict(sd, strict=True)
    if "--q_use_deformed_conv" in META["configs"][name]["flags"]:
        m = dec.inter_blocks[1].matching
        assert torch.equal(m.deform.weight.detach(), sd["inter_blocks.1.matching.deform.weight"])


def test_variant_modules():
    dec = _decoder("all")
    for i, blk in enumerate(dec.inter_blocks):
        m = blk.matching
        assert m.upsample_corr is None and m.convs[0].conv.weight.shape[1] == 2 * blk.feat_size
        assert (m.upsample_toff is None) == (i == 0) and m.deform is not None
    with pytest.raises(Exception):   # a trade-off level needs feat_size % 32 == 0 (torch rejects the grouped up-sampling)
        _ = torch.nn.ConvTranspose2d(32, 48, 4, stride=2, padding=1, groups=32, bias=False)


def test_deform_ref_zero_offset_is_conv():
    g = torch.Generator().manual_seed(0)
    x, w, b = torch.randn(2, 5, 7, 9, generator=g, dtype=torch.float64), torch.randn(4, 5, 3, 3, generator=g, dtype=torch.float64), torch.randn(4, generator=g, dtype=torch.float64)
    off = torch.zeros(2, 18, 7, 9, dtype=torch.float64)
    assert torch.allclose(deform_ref.deform_conv2d(x, off, w, b, padding=1), F.conv2d(x, w, b, padding=1), atol=1e-12)


def test_deform_ref_integer_offset_is_shifted_conv():
    """Offset (dy, dx) = (2, -1) for every tap: the conv of the input shifted by that much, zero-padded."""
    g = torch.Generator().manual_seed(1)
    x, w = torch.randn(1, 3, 8, 6, generator=g, dtype=torch.float64), torch.randn(2, 3, 3, 3, generator=g, dtype=torch.float64)
    off = torch.zeros(1, 9, 2, 8, 6, dtype=torch.float64)
    off[:, :, 0], off[:, :, 1] = 2.0, -1.0
    got = deform_ref.deform_conv2d(x, off.view(1, 18, 8, 6), w, None, padding=1)
    # out[y, x] = sum_ij w[i, j] x[y + 1 + i, x - 2 + j], zero outside: an unpadded conv of the input zero-padded by 4, cropped
    full = F.conv2d(F.pad(x, (4, 4, 4, 4)), w)
    assert torch.allclose(got, full[:, :, 5:5 + 8, 2:2 + 6], atol=1e-12)


def test_deform_ref_fractional_border_by_hand():
    """One channel, weight = the centre tap only: the output is the bilinear sample at (y + dy, x + dx).  At (0, 0) with
    (dy, dx) = (-0.25, 0.5): rows -1 (outside, 0) and 0 with weights 0.25 / 0.75, columns 0 and 1 with 0.5 / 0.5."""
    x = torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], dtype=torch.float64).view(1, 1, 2, 3)
    w = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
    w[0, 0, 1, 1] = 1.0
    off = torch.zeros(1, 9, 2, 2, 3, dtype=torch.float64)
    off[:, :, 0], off[:, :, 1] = -0.25, 0.5
    out = deform_ref.deform_conv2d(x, off.view(1, 18, 2, 3), w, None, padding=1)[0, 0]
    assert out[0, 0].item() == 0.75 * (0.5 * 1.0 + 0.5 * 2.0)
    # (0, 2): column 2.5 -> corners 2 (inside) and 3 (outside): 0.75 * 0.5 * 3
    assert out[0, 2].item() == 0.75 * 0.5 * 3.0
    # (1, 0): row 0.75 -> rows 0 / 1 with 0.25 / 0.75
    assert out[1, 0].item() == 0.25 * (0.5 * 1.0 + 0.5 * 2.0) + 0.75 * (0.5 * 4.0 + 0.5 * 5.0)
    # a point at or beyond -1 / H is 0: dy = -1 at row 0
    off[:, :, 0] = -1.0
    assert deform_ref.deform_conv2d(x, off.view(1, 18, 2, 3), w, None, padding=1)[0, 0, 0].abs().max().item() == 0.0
