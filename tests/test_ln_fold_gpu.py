"""-m gpu: the LayerNorm that the transformer actually runs -- folded into the GEMM (gpt.hip: `ln_shift` / `ln_accum` / `ln_finish` /
`gemm_epilogue` in `gemm16_kernel<1,1,4>`, `<2,2,1>`, their tiled-weight variants, `gemm16_rb_kernel`, `gemm_seq_kernel` and the
persistent `gpt_step_kernel`) -- held to LayerNorm's own accuracy on rows of large mean, small spread and a leading outlier.

Reference, bound and row patterns: tests/ln_fold_ref.py -- `want = Linear(LayerNorm(x))` in float64 from the UNFOLDED W, b, gamma,
beta, and |got - want| <= 1e-5 A with A = ((|xhat| + 1) |gamma| + |beta|) @ |W|^T + |b|, which does not grow with a row's mean
(GELU: 1.2 A + 1e-3).  The patterns P0..P6 cycle over the rows, so every 16-row block holds several of them.  The other GEMM
suites draw rows of mean 0.3 and std 0.7 and bound the fold by the size of its own intermediates; on these rows the fold as it
was -- one-pass statistics and `x @ W'^T - mean s` on the raw activations -- exceeded this bound 3 to 1400 times on P1..P4
(tests/test_ln_fold_host.py emulates it).

Every output buffer starts as NaN, x is a column slice of a wider NaN-margined tensor (ldx = K + 32), epilogues none and GELU,
and every shape asserts the form it reaches with `plan()` of tests/test_gemm_forms_gpu.py.  Each case prints its largest
|err| / (REL A) per pattern before it asserts (run with -s)."""
import functools
import os
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ln_fold_ref as R  # noqa: E402
from test_gemm_forms_gpu import DECODE_LN, DECODE_QKV, nan_out, plan  # noqa: E402
from test_gemm_forms_gpu import untouched as view_untouched  # noqa: E402
from test_gemm_tiled_gpu import MS as TILED_MS, NK as TILED_NK  # noqa: E402
from test_gemm_tiled_gpu import out_buf, tile_nan_padded  # noqa: E402
from test_gemm_tiled_gpu import untouched as rows_untouched  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ccvs_amd import ops as _ops
    return _ops


def x_slice(x_cpu):
    """x on the GPU as columns [16, 16 + K) of a [M, K + 32] tensor whose margins are NaN."""
    m, k = x_cpu.shape
    wide = torch.full((m, k + 32), NAN)
    wide[:, 16:16 + k] = x_cpu
    x = wide.cuda()[:, 16:16 + k]
    assert x.stride(0) == k + 32
    return x


@functools.lru_cache(maxsize=None)
def ln_case(m, n, k):
    """Pattern rows, operands and the float64 reference of one shape: built once, shared, read-only."""
    from ccvs_amd import ops as _ops
    x_cpu = R.pattern_rows(m, k, seed=m * 7 + n * 3 + k)
    w, b, gamma, beta = R.linear_operands(n, k, seed=m + 11 * n + k)
    want, a = R.ln_linear_ref(x_cpu, w, b, gamma, beta)
    packed = tuple(t.cuda() for t in _ops.pack_ln_linear(w, b, gamma, beta))
    return SimpleNamespace(x=x_slice(x_cpu), packed=packed, want=want, a=a)


# (M, N, K, form): the smallest shapes that run the K loop several times, and one deep K
#   tile1 (32, 130, 1040) from DECODE_LN: one K slice of 16 full batches + 1 remainder step, ragged N;  (16, 64, 4096): 4 slices of 16 batches
#   tile2 (48, 96, 1024): 4 slices of 16 one-step batches, three row blocks (the fourth of the second tile wholly outside)
#   rb    (260, 40, 1152): 8 slices of one full batch + one remainder step, five 64-row groups, ragged N
DECODE = [(32, 130, 1040, "tile1"), (16, 64, 4096, "tile1"), (48, 96, 1024, "tile2"), (260, 40, 1152, "rb")]
assert (32, 130, 1040) in [s[:3] for s in DECODE_LN]
#   seq   (129, 96, 1040): 65 K stages (odd: the `break` out of the two-stage loop), one row in the second row tile;  (300, 130, 48): 3 stages, ragged third tile
SEQ = [(129, 96, 1040), (300, 130, 48)]


@pytest.mark.parametrize("m,n,k,form", DECODE)
def test_gemm_ln_decode_forms_as_layernorm(ops, m, n, k, form):
    """ops.gemm_ln, single-position calls: the weight-stream forms and the row-blocked one."""
    assert plan(m, n, k, True)[0] == form and plan(m, n, k, True)[2] == 1
    c = ln_case(m, n, k)
    _, out = nan_out(m, n, False)
    got = ops.gemm_ln(c.x, *c.packed, epilogue=ops.EPI_NONE, out=out)
    R.check(got, c.want, c.a, f"gemm_ln {form} {m}x{n}x{k}")
    big, out = nan_out(m, n, True)
    got = ops.gemm_ln(c.x, *c.packed, epilogue=ops.EPI_GELU, out=out)
    R.check(got, *R.gelu_ref(c.want, c.a), f"gemm_ln {form} {m}x{n}x{k} gelu")
    view_untouched(big, n)


@pytest.mark.parametrize("m,n,k", SEQ)
def test_gemm_ln_sequence_form_as_layernorm(ops, m, n, k):
    """ops.gemm_ln(..., GEMM_SEQ): the shifts are read from global memory, the statistics summed from the fragments out of LDS."""
    assert plan(m, n, k, True, seq=True)[0] == "seq"
    c = ln_case(m, n, k)
    _, out = nan_out(m, n, False)
    got = ops.gemm_ln(c.x, *c.packed, epilogue=ops.EPI_NONE | ops.GEMM_SEQ, out=out)
    R.check(got, c.want, c.a, f"gemm_ln seq {m}x{n}x{k}")
    big, out = nan_out(m, n, True)
    got = ops.gemm_ln(c.x, *c.packed, epilogue=ops.EPI_GELU | ops.GEMM_SEQ, out=out)
    R.check(got, *R.gelu_ref(c.want, c.a), f"gemm_ln seq {m}x{n}x{k} gelu")
    view_untouched(big, n)


# one one-block and one 2 x 2 shape of test_gemm_tiled_folded_layernorm's table (MS x NK[:4]) with K >= 1024: ragged rows, a ragged column tile
TILED = [(23, 40, 1024, "tile1"), (37, 48, 1024, "tile2")]
assert all(m in TILED_MS and (n, k) in TILED_NK[:4] for m, n, k, _ in TILED)


@pytest.mark.parametrize("m,n,k,form", TILED)
def test_gemm_tiled_folded_layernorm_as_layernorm(ops, m, n, k, form):
    """ops.gemm_tiled(..., ln_s=...): the tiled-weight instantiations, bit for bit the row-major ones."""
    assert plan(m, n, k, True)[0] == form
    c = ln_case(m, n, k)
    wg, bb, s = c.packed
    wt = tile_nan_padded(ops, wg)
    for name, epi, want, a in (("none", ops.EPI_NONE, c.want, c.a), ("gelu", ops.EPI_GELU) + R.gelu_ref(c.want, c.a)):
        _, ref = out_buf(m, n)
        ops.gemm_ln(c.x, wg, bb, s, epilogue=epi, out=ref)
        big, out = out_buf(m, n)
        ops.gemm_tiled(c.x, wt, n, bb, epi, out=out, ln_s=s)
        R.check(out, want, a, f"gemm_tiled ln {form} {m}x{n}x{k} {name}")
        assert torch.equal(out, ref), "tiled and row-major weights differ"
        rows_untouched(big, m, n)


def qkv_case(ops, rows, C, seed):
    x_cpu = R.pattern_rows(rows, C, seed=seed)
    w, b, gamma, beta = R.linear_operands(3 * C, C, seed=seed + 1)
    want, a = R.ln_linear_ref(x_cpu, w, b, gamma, beta)
    return x_slice(x_cpu), tuple(t.cuda() for t in ops.pack_ln_linear(w, b, gamma, beta)), want, a


def check_qkv(q, kc, vc, want, a, B, Tq, C, H, pos, what):
    """q and the slots [pos, pos + Tq) of both caches against the reference's three column blocks; every other slot still NaN.
    (Rows are (b, t) pairs, b-major: row r of the [B * Tq, ...] views has pattern r % 7.)"""
    D = C // H
    slots = lambda cache: cache[:, :, pos:pos + Tq].transpose(1, 2).reshape(B * Tq, C)   # [B,H,Tq,D] -> [B*Tq, C]
    R.check(q, want[:, :C], a[:, :C], what + " q")
    R.check(slots(kc), want[:, C:2 * C], a[:, C:2 * C], what + " k cache")
    R.check(slots(vc), want[:, 2 * C:], a[:, 2 * C:], what + " v cache")
    for cache in (kc, vc):
        assert torch.isnan(cache[:, :, :pos]).all() and torch.isnan(cache[:, :, pos + Tq:]).all(), "a slot outside [pos, pos + Tq) was written"
    assert D * H == C


@pytest.mark.parametrize("B,C,H,tmax,pos0,pos_dev,want_plan", DECODE_QKV)
def test_gemm_ln_qkv_decode_as_layernorm(ops, B, C, H, tmax, pos0, pos_dev, want_plan):
    """ops.gemm_ln_qkv with Tq = 1, what every decode step runs, on the four DECODE_QKV shapes."""
    assert plan(B, 3 * C, C, True) == want_plan
    x, packed, want, a = qkv_case(ops, B, C, seed=B + C + pos0)
    kc = torch.full((B, H, tmax, C // H), NAN, device="cuda")
    vc = torch.full((B, H, tmax, C // H), NAN, device="cuda")
    q = torch.full((B, C), NAN, device="cuda")
    pd = torch.tensor([pos_dev], dtype=torch.int32, device="cuda") if pos_dev is not None else None
    ops.gemm_ln_qkv(x, *packed, kc, vc, B, 1, pos0, pd, out=q)
    check_qkv(q, kc, vc, want, a, B, 1, C, H, pos0 + (pos_dev or 0), f"qkv {want_plan[0]} B={B} C={C}")


def test_gemm_ln_qkv_prefill_as_layernorm(ops):
    """ops.gemm_ln_qkv with B * Tq = 300 rows and C = 256 (as test_gemm_ln_qkv_multi_tile): the whole-sequence form's scatter."""
    B, Tq, C, H, tmax, pos0, pos_dev = 3, 100, 256, 4, 128, 5, 7
    assert plan(B * Tq, 3 * C, C, True, seq=True)[0] == "seq"
    x, packed, want, a = qkv_case(ops, B * Tq, C, seed=300)
    kc = torch.full((B, H, tmax, C // H), NAN, device="cuda")
    vc = torch.full((B, H, tmax, C // H), NAN, device="cuda")
    pd = torch.tensor([pos_dev], dtype=torch.int32, device="cuda")
    q = ops.gemm_ln_qkv(x, *packed, kc, vc, B, Tq, pos0, pd)
    check_qkv(q, kc, vc, want, a, B, Tq, C, H, pos0 + pos_dev, "qkv seq 300x768x256")


def test_gemm_tiled_qkv_scatter_as_layernorm(ops):
    """The tiled-weights scatter, once: 37 rows (2 x 2 tile, ragged), C = 64."""
    m, C, H, tmax, pos0, pos_dev = 37, 64, 4, 7, 2, 3
    assert plan(m, 3 * C, C, True)[0] == "tile2"
    x, (wg, bb, s), want, a = qkv_case(ops, m, C, seed=37 + 64)
    kc = torch.full((m, H, tmax, C // H), NAN, device="cuda")
    vc = torch.full((m, H, tmax, C // H), NAN, device="cuda")
    q = torch.full((m, C), NAN, device="cuda")
    pd = torch.tensor([pos_dev], dtype=torch.int32, device="cuda")
    ops.gemm_tiled(x, ops.tile_weight(wg), 3 * C, bb, out=q, ln_s=s, kcache=kc, vcache=vc, pos0=pos0, pos_dev=pd)
    check_qkv(q, kc, vc, want, a, m, 1, C, H, pos0 + pos_dev, "qkv tiled tile2 37x192x64")


# ---------------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------------
def test_gpt_with_a_large_shared_offset_in_the_residual_stream(ops):
    """A tiny GPT (n_embd 64, 2 layers, vocab 200) whose token embedding carries a constant: the residual rows entering ln1 have
    |mean| / std of about 100 (asserted on the float64 side).  Prefill logits and 8 greedy decode steps of the three step paths --
    per-op, launch chain, persistent -- against the oracle's forward on .double() weights, elementwise within the bound of
    tests/ln_fold_ref.py evaluated at the head (ln_f + head, on the float64 residual rows); and the three paths equal one another
    bit for bit."""
    from ccvs_amd.models.skip_vid_generator.models import mingpt
    from oracle import ccvs_oracle as O
    torch.manual_seed(3)
    B, T0, NEW, V, C, H, L = 16, 8, 9, 200, 64, 4, 2
    net = mingpt.GPT(vocab_size=V, block_size=64, num_blocks=4, n_layer=L, n_head=H, n_embd=C, emb_mode="temporal", shape=(4, 4)).cuda()
    for p in net.parameters():   # non-trivial LayerNorm / bias values
        p.data.add_(0.05 * torch.randn_like(p))
    code = torch.randint(0, V, (B, T0), generator=torch.Generator().manual_seed(5)).cuda()
    sd = {k: v.detach().double().cpu() for k, v in net.state_dict().items()}
    cfg = SimpleNamespace(z_shape=(4, 4), emb_mode="temporal")
    x0 = sd["tok_emb.weight"][code.cpu()] + O.gpt_pos_emb(sd, cfg, T0)
    offset = 100.0 * x0.std(dim=-1, unbiased=False).median().item()
    with torch.no_grad():
        net.tok_emb.weight.add_(offset)
    sd["tok_emb.weight"] = net.tok_emb.weight.detach().double().cpu()

    def run(persistent):
        net.drop_engine_state()
        net.persistent_step = persistent
        trace = []
        toks = net.generate(code, NEW, sample=False, trace=trace)
        net.check_steps()
        net.persistent_step = False
        return toks.cpu(), torch.stack(trace, dim=1).cpu()   # [B, T0 + NEW], [B, NEW, V]: logits at positions T0 - 1 .. T0 + NEW - 2

    net.drop_engine_state()
    net.begin(B, T0 + NEW)
    logits = net.prefill(code)
    seq, per_op = [code], []
    for i in range(NEW):
        per_op.append(logits.clone())
        tok = logits.argmax(dim=-1, keepdim=True)
        seq.append(tok)
        if i < NEW - 1:
            logits = net.step(tok)
    toks, per_op = torch.cat(seq, dim=1).cpu(), torch.stack(per_op, dim=1).cpu()
    paths = {"per-op": (toks, per_op), "launch chain": run(False), "persistent": run(True)}

    # float64: the oracle's blocks on the greedy sequence (teacher-forced: position t sees tokens 0..t, as the cached steps do)
    x = sd["tok_emb.weight"][toks[:, :-1]] + O.gpt_pos_emb(sd, cfg, T0 + NEW - 1)
    ratios = []
    for i in range(L):
        ratios.append((x.mean(-1).abs() / x.std(-1, unbiased=False)).median().item())
        x = O.gpt_block(sd, f"blocks.{i}", x, H)
    print(f"|mean| / std of the rows entering ln1, median per layer: {[round(r, 1) for r in ratios]}")
    assert 50 <= ratios[0] <= 200 and all(r >= 25 for r in ratios), ratios
    rows = x[:, T0 - 1:].reshape(B * NEW, C)
    want, a = R.ln_linear_ref(rows, sd["head.weight"], torch.zeros(V, dtype=torch.float64), sd["ln_f.weight"], sd["ln_f.bias"], eps=net.ln_f.eps)
    direct = F.linear(F.layer_norm(x, (C,), sd["ln_f.weight"], sd["ln_f.bias"], net.ln_f.eps), sd["head.weight"])[:, T0 - 1:].reshape(B * NEW, V)
    assert ((want - direct).abs() / a).max().item() < 1e-12
    worst = {}
    for name, (tk, lg) in paths.items():
        assert torch.equal(tk, toks), f"{name}: other tokens than the per-op path"
        got = lg.double().reshape(B * NEW, V)
        assert torch.isfinite(got).all(), name
        frac = ((got - want).abs() / (R.REL * a)).view(B, NEW, V)
        worst[name] = (frac[:, 0].max().item(), frac[:, 1:].max().item())
        print(f"{name}: max |err| / (REL A): prefill {worst[name][0]:.3g}, decode steps {worst[name][1]:.3g}")
    for name, (tk, lg) in paths.items():
        assert torch.equal(lg, per_op), f"{name}: logits differ from the per-op path's"
    assert max(max(v) for v in worst.values()) <= 1.0, worst
