"""not gpu: the yardstick of tests/test_attention_forms_gpu.py can tell right from wrong.

`attention_ref` (tests/attention_ref.py) returns a float64 attention and a per-element error bound `tol` derived from float64
magnitudes.  For the smallest prefill case of the GPU grid that spans two 32-key tiles with a ragged query block, (Tq, pos0) =
(33, 31), and the decode case L = BATCH + 1 (one register batch of the decode form plus one row), one per head dimension:

  a. torch's own fp32 attention on the CPU stays within `tol` on every element (and uses little of it);
  b. each wrong reference, computed in float64, exceeds `tol` on at least one element of EVERY (b, h):
       the mask one key longer, the extra key and value zero (what an uninitialised but finite cache row would give),
       the mask one key shorter,
       one interior key dropped,
       scale 1 / sqrt(D + 1),
       the running-max rescale of the online softmax omitted between 32-key tiles.
     These are the host-side images of the kernel's `j < L` select, of the `written` zero-fill and the clamp of the prefill
     form's fetch, and of its `alpha` rescale.

The score patterns of the GPU test (q scaled by 8, key 0 dominant, scores rising with the key index) go through (a) as well, and
through (b) for the scale on the prefill case (the single query of a decode case may be one-hot); they are exempt from (b) for the three mask mutations: a near-one-hot softmax puts a weight
below fp32 resolution on almost every key, so adding, removing or dropping one really does not change the result, and no bound
could or should see it.  The rescale mutation is asserted on the prefill cases, whose form has the running max (the
decode form is two-pass, and a single query whose maximum falls in tile 0 is immune to it), where the pattern makes the maximum
move between tiles (unit, q8, rising); it must be exactly harmless where the maximum stands still from tile 0 on (key0)."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_ref as R  # noqa: E402

B, H = 2, 3
DS = (16, 32, 64)


def decode_batch(d):
    return 16 * (64 // (d // 4))


def fp32_attention(q, k, v, pos0):
    """Plain fp32 torch on the CPU."""
    return R.masked_attention(q, k, v, R.visible(q.shape[-2], k.shape[-2], pos0))


def cases(d):
    return [("prefill", 33, 31), ("decode", 1, decode_batch(d))]


def exceeds_everywhere(wrong, out, tol):
    """The wrong result is outside tol on at least one element of every (b, h); returns the smallest per-(b, h) max ratio."""
    ratio = ((wrong - out).abs() / tol).amax((-2, -1))
    return ratio.min().item()


@pytest.mark.parametrize("d", DS)
def test_fp32_is_inside_and_every_wrong_reference_is_outside(d):
    for form, tq, pos0 in cases(d):
        length = pos0 + tq
        q, k, v = R.make_inputs("unit", B, H, tq, length, d, seed=100 + d)
        q64, k64, v64 = q.double(), k.double(), v.double()
        out, tol = R.attention_ref(q64, k64, v64, pos0)
        used = ((fp32_attention(q, k, v, pos0).double() - out).abs() / tol).max().item()
        print(f"{form} D={d} Tq={tq} pos0={pos0}: fp32 torch uses {used:.3f} of tol")
        assert used <= 1.0
        # the float64 online softmax is the same function (so its rescale-free variant below differs by the rescale alone)
        assert ((R.online_softmax(q64, k64, v64, pos0) - out).abs() / tol).max().item() < 1e-6
        wrong = {
            "mask one key longer": R.wrong_mask_longer(q64, k64, v64, pos0),
            "mask one key shorter": R.wrong_mask_shorter(q64, k64, v64, pos0),
            "interior key dropped": R.wrong_dropped_key(q64, k64, v64, pos0, length // 2),
            "scale 1/sqrt(D+1)": R.wrong_scale(q64, k64, v64, pos0),
        }
        if form == "prefill":   # the decode form is two-pass and has no running max; one query whose max is in tile 0 is immune
            wrong["no rescale between tiles"] = R.online_softmax(q64, k64, v64, pos0, rescale=False)
        for name, w in wrong.items():
            least = exceeds_everywhere(w, out, tol)
            print(f"  {name}: smallest per-(b,h) max err/tol = {least:.3g}")
            assert least > 1.0, (form, d, name, least)


@pytest.mark.parametrize("pattern", [p for p in R.PATTERNS if p != "unit"])
@pytest.mark.parametrize("d", DS)
def test_score_patterns(d, pattern):
    for form, tq, pos0 in [("prefill", 129, 127), ("decode", 1, decode_batch(d))]:
        length = pos0 + tq
        q, k, v = R.make_inputs(pattern, B, H, tq, length, d, seed=200 + d)
        R.pattern_property(pattern, q, k, pos0)
        q64, k64, v64 = q.double(), k.double(), v.double()
        out, tol = R.attention_ref(q64, k64, v64, pos0)
        used = ((fp32_attention(q, k, v, pos0).double() - out).abs() / tol).max().item()
        print(f"{form} D={d} {pattern}: fp32 torch uses {used:.3f} of tol")
        assert used <= 1.0
        if form == "prefill":     # 129 queries per (b, h): some of them are not one-hot
            assert exceeds_everywhere(R.wrong_scale(q64, k64, v64, pos0), out, tol) > 1.0
        norescale = R.online_softmax(q64, k64, v64, pos0, rescale=False)
        if pattern == "key0":     # the max never moves: alpha == 1 everywhere, the factor is the identity
            assert torch.equal(norescale, R.online_softmax(q64, k64, v64, pos0))
        elif form == "prefill":
            assert exceeds_everywhere(norescale, out, tol) > 1.0


def test_reference_definition():
    """attention_ref is the plain definition: a loop over queries with torch.softmax on the visible slice."""
    d, tq, pos0 = 16, 5, 3
    q, k, v = (t.double() for t in R.make_inputs("unit", 1, 2, tq, pos0 + tq, d, seed=1))
    out, tol = R.attention_ref(q, k, v, pos0)
    for t in range(tq):
        n = pos0 + t + 1
        p = torch.softmax((q[:, :, t:t + 1] @ k[:, :, :n].transpose(-2, -1)) / math.sqrt(d), -1)
        assert torch.allclose(out[:, :, t:t + 1], p @ v[:, :, :n], rtol=1e-13, atol=1e-15)
    assert tol.shape == out.shape and (tol > 0).all()
