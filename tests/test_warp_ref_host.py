"""No GPU: what the bound of tests/warp_ref.py can and cannot tell apart, on the very tensors that tests/test_warp_forms_gpu.py
sends to the kernels.

  * the float64 mirror is the reference's operation: it equals `grid_sample` in float64 on the reference's grid;
  * the reference's own fp32 arithmetic (torch on the CPU, through the oracle) lies within the bound on every element of every
    case -- were it not, the derivation would be wrong;
  * each wrong reading of the reference (`warp_ref.MUTATIONS`) leaves the bound on at least one case, the two readings of `conf`
    on a saturated one;
  * where the mirror says an exact 0 is due, the fp32 reference gives one, and such pixels are a real share of the lattice and
    far-flow cases;
  * the case table launches all 15 instantiations."""
import os
import sys

import pytest
import torch

from oracle import ccvs_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_ref as R  # noqa: E402

F = torch.nn.functional
CASES = R.cases()


def by_op(*ops):
    return [c for c in CASES if c.op in ops]


def grid64(height, width):
    """`O.backwarp_grid` with the linspace itself in float64 (the oracle's is fp32, as the reference's: 6e-8 of a grid unit)."""
    hor = torch.linspace(-1.0 + (1.0 / width), 1.0 - (1.0 / width), width, dtype=torch.float64).view(1, 1, 1, -1).expand(-1, -1, height, -1)
    ver = torch.linspace(-1.0 + (1.0 / height), 1.0 - (1.0 / height), height, dtype=torch.float64).view(1, 1, -1, 1).expand(-1, -1, -1, width)
    return torch.cat([hor, ver], dim=1)


def ref_backwarp32(inp):
    x = R.stack(inp["ctxs"])
    return O.backwarp(x, inp["flow"] * inp["mult"], O.backwarp_grid(inp["H"], inp["W"]))


def ref_fp32(case):
    """The reference's fp32 path on the CPU."""
    inp = R.reference(case)["inp"]
    warped = ref_backwarp32(inp)
    if case.op in ("backwarp", "backwarp_p8"):
        return warped
    if case.op == "warp_proj":
        return F.leaky_relu(O.equal_conv2d(warped, inp["weight"], inp["bias"]), 0.1)
    k, occs, dec = inp["k"], inp["occ"], inp["dec"]
    n, c, h, w = dec.shape
    if k > 1:                                         # the expression of test_ops_gpu.py::test_warp_fuse_blend
        confs = (1 - torch.sigmoid(occs)).view(-1, k, 1, h, w) + 1e-6
        wi = (warped.view(-1, k, c, h, w) * confs).sum(1) / confs.sum(1)
        occ = (occs.view(-1, k, 1, h, w) * confs).sum(1) / confs.sum(1)
    else:
        wi, occ = warped, occs
    m = torch.sigmoid(occ)
    return m * dec + (1 - m) * wi


def test_case_table_launches_every_instantiation():
    got = {R.launched(c.op, *R.FORMS[c.form], cout=c.var) for c in CASES}
    assert got == R.ALL_INSTANTIATIONS, sorted(R.ALL_INSTANTIATIONS ^ got)
    assert R.k_values() == (1, 2, 16)
    for form in R.FORMS:                              # every regime in every form, k = 1, 2, CCVS_MAX_CTX in every form
        assert {c.regime for c in CASES if c.form == form and c.op == "fuse_blend"} == set(R.REGIMES) | {"saturated"}
        assert {c.var for c in CASES if c.form == form and c.op == "fuse_blend"} == set(R.k_values())
        assert {c.regime for c in CASES if c.form == form and c.op == "backwarp"} == set(R.REGIMES)


def test_mirror_is_grid_sample_in_float64():
    worst = 0.0
    for case in CASES:
        inp = R.reference(case)["inp"]
        x = R.stack(inp["ctxs"]).double()
        got = R.backwarp(x, inp["flow"], inp["mult"])[0]
        want = O.backwarp(x, inp["flow"].double() * inp["mult"], grid64(inp["H"], inp["W"]))
        d = float((got - want).abs().max())
        worst = max(worst, d)
        assert d <= 1e-12, (case, d)
    print(f"mirror against float64 grid_sample: largest difference {worst:.3e}")


@pytest.mark.parametrize("op", ["backwarp", "backwarp_p8", "warp_proj", "fuse_blend"])
def test_fp32_reference_is_within_the_bound(op):
    for case in by_op(op):
        ref = R.reference(case)
        got = ref_fp32(case)
        assert torch.isfinite(got).all(), case
        ratio = R.worst_ratio(got, ref["want"], ref["tol"])
        print(f"{case.op} {case.form} {case.regime} {case.var}: fp32 reference, largest err / bound {ratio:.4f}")
        assert ratio <= 1.0, (case, ratio)


def test_every_mutation_leaves_the_bound():
    rows = []
    for name, (fn, ops) in R.MUTATIONS.items():
        best = (0.0, None)
        best_sat = (0.0, None)
        for case in by_op(*ops):
            ref = R.reference(case)
            ratio = R.worst_ratio(fn(case.op, ref["inp"]), ref["want"], ref["tol"])
            if ratio > best[0]:
                best = (ratio, case)
            if case.regime == "saturated" and ratio > best_sat[0]:
                best_sat = (ratio, case)
        if name in R.CONF_MUTATIONS:
            best = best_sat
        rows.append((name, best[1], best[0]))
    for name, case, ratio in rows:
        print(f"{name:20s} {case and tuple(case)!s:48s} largest err / bound {ratio:.3e}")
    for name, case, ratio in rows:
        assert ratio > 1.0, f"{name} stays within the bound on every case"


def test_every_mutation_leaves_the_bound_in_every_form():
    """Stronger than asked: each launch form alone would catch each mutation (a kernel is wrong in one form at a time)."""
    for name, (fn, ops) in R.MUTATIONS.items():
        for form in R.FORMS:
            sel = [c for c in by_op(*ops) if c.form == form and (name not in R.CONF_MUTATIONS or c.regime == "saturated")]
            worst = 0.0
            for case in sel:
                ref = R.reference(case)
                worst = max(worst, R.worst_ratio(fn(case.op, ref["inp"]), ref["want"], ref["tol"]))
                if worst > 1.0:
                    break
            assert worst > 1.0, (name, form, worst)


def test_k1_through_the_k_formula_is_the_same_function():
    """`mut_k1_through_formula`: conf v / conf and occ conf / conf with conf >= 1e-6 are v and occ; the reading changes float64
    roundings only and stays far inside the bound -- the one listed mutation that no test can or should catch."""
    fn = R.EQUIVALENT_MUTATIONS["k1_through_formula"][0]
    for case in by_op("fuse_blend"):
        if case.var != 1:
            continue
        ref = R.reference(case)
        got = fn(case.op, ref["inp"])
        assert torch.isfinite(got).all()
        rel = float(((got - ref["want"]).abs() / (ref["want"].abs() + ref["inp"]["dec"].double().abs() + 1e-300)).max())
        assert rel <= 1e-9, (case, rel)               # 1e-6 carries 1e-16 / 1e-6 relative in float64
        assert R.worst_ratio(got, ref["want"], ref["tol"]) <= 1e-2, case


def test_exact_zeros_where_the_position_is_far_outside():
    for case in CASES:
        if case.regime not in R.ZERO_REGIMES or case.op == "fuse_blend":
            continue
        ref = R.reference(case)
        far = ref["far"]
        share = float(far.double().mean())
        assert 0.05 <= share <= 0.60, (case, share)
        got = ref_fp32(case)
        if case.op == "warp_proj":
            due = F.leaky_relu(ref["inp"]["bias"], 0.1).view(1, -1, 1, 1).expand_as(got)
        else:
            due = torch.zeros_like(got)
        sel = far.unsqueeze(1).expand_as(got)
        assert torch.equal(got[sel], due[sel]), case
        if case.op != "warp_proj":
            assert bool((ref["tol"][sel] == 0).all()) and bool((ref["want"][sel] == 0).all()), case
    shares = {c.form: float(R.reference(c)["far"].double().mean()) for c in by_op("backwarp") if c.regime == "far"}
    print("share of exact-zero pixels, far regime:", shares)


def test_saturated_fp32_reference_is_finite_and_keeps_dec():
    for case in by_op("fuse_blend"):
        if case.regime != "saturated":
            continue
        ref = R.reference(case)
        inp = ref["inp"]
        got = ref_fp32(case)
        assert torch.isfinite(got).all() and torch.isfinite(ref["want"]).all() and torch.isfinite(ref["tol"]).all(), case
        k = inp["k"]
        occ = inp["occ"].view(R.NF, k, 1, inp["H"], inp["W"])
        classes = [(occ == 100).all(1), (occ == 30).all(1), ((occ == -30).sum(1) == 1) & ((occ == 30).sum(1) == k - 1), (occ == -100).all(1)]
        for cls in classes:
            assert cls.any(), case
        keep = (occ >= 30).all(1).expand_as(got)
        assert keep.any()
        d = inp["dec"].double()
        assert bool(((ref["want"] - d).abs()[keep] <= ref["tol"][keep]).all()), case     # the mirror itself: dec to within the bound
        assert bool(((got.double() - d).abs()[keep] <= ref["tol"][keep]).all()), case
