"""The decode GEMM on TILED weights (`ccvs_gpt_decode.w_tiled`, `ccvs_gemm_tiled`; gpt.hip: gemm16_tile<.., WT = true>): W cut into
1-KB blocks of 16 rows x 16 columns, block (ct, kb) at float offset (ct K / 16 + kb) 256, so that one wave load is eight whole
128-byte lines.  Only WHERE a float lives changes: the same floats reach the same lanes, the K slicing, MFMA order and reduction
are the row-major kernel's, so every result must equal the row-major kernel's bit for bit -- any difference is an addressing bug.

Op level (-m gpu): `ops.gemm_tiled` against `ops.gemm_nt` / `gemm_ln` / `gemm_ln_qkv` with torch.equal, and against float64 on the CPU
with the bound of tests/test_gemm_forms_gpu.py (|err| <= 1e-5 A, A = |x| @ |w|^T: see that module's docstring).  The shapes reach
every address path of the tile body:
    M 16, 23          one 16 x 16 block per workgroup (U = 4), ragged rows
    M 37, 48, 64      2 x 2 blocks, ragged second row block (37: five rows in the third 16-row block, the fourth wholly outside)
    N 48, 40          under the 2 x 2 tile the second column block of workgroup 1 lies wholly outside (48: three column tiles);
                      40: a ragged column tile, whose padding rows in the tiled W are NaN here
    N 3 C             the QKV scatter into NaN-filled caches: every slot but the written one stays NaN
    K 64              one 16-deep batch per wave: the remainder loop only (one-block form) / one full batch (2 x 2)
    K 1024            full batches, four K slices of 256
    K 4096, N 64      split-K over workgroups (kz = 4) and the slab reduction
The rows of x behind M (up to the next multiple of 16), the padding rows of W and every output are NaN beforehand: every kept
output must be finite, rows >= M and columns >= N untouched.

Step level (-m gpu): a 2-layer GPT (C 64, H 4, V 96, Tmax 32), 20 tokens from a 5-token prefix, with the tiled weights off and on:
tokens, logits, the residual stream, q / att / h, the appended KV rows and the counters are the same bits -- at 16, 48 and 64 rows,
15 rows in 3 groups of 5, graph-replayed and eager, sampled in the kernel, greedy and from a host noise stream, launch chain and
persistent step; and the full-size GPT (24 x 1024, V 1024, 64 rows) picks the same tokens for a fixed seed.

Host (no GPU): `ops.tile_weight` against the index formula, N = 40, K = 64."""
import functools

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
REL = 1e-5
NAN = float("nan")


def tiled_offset(r, c, K):
    """Float offset of W[r][c] in the tiled layout."""
    return ((((r // 16) * (K // 16) + c // 16) * 4 + (c % 16) // 4) * 16 + r % 16) * 4 + c % 4


def test_tile_weight_matches_the_index_formula():
    from ccvs_amd import ops
    N, K = 40, 64
    w = torch.arange(N * K, dtype=torch.float32).view(N, K)
    t = ops.tile_weight(w)
    assert t.shape == (48 * K,) and t.is_contiguous()
    seen = torch.zeros(48 * K, dtype=torch.bool)
    for r in range(48):
        src = min(r, N - 1)   # padding rows repeat the last row
        for c in range(K):
            o = tiled_offset(r, c, K)
            assert t[o].item() == w[src, c].item(), (r, c, o)
            seen[o] = True
    assert seen.all()
    # block (ct, kb) is 256 contiguous floats; lane li + 16 g owns floats 4 lane .. 4 lane + 3 = W[16 ct + li][16 kb + 4 g ..]
    ct, kb, li, g = 1, 2, 5, 3
    base = (ct * (K // 16) + kb) * 256 + 4 * (li + 16 * g)
    assert torch.equal(t[base:base + 4], w[16 * ct + li, 16 * kb + 4 * g:16 * kb + 4 * g + 4])


def test_gemm_header_and_exports_agree():
    """include/ccvs_hip_gemm.h, which include/ccvs_hip.h includes, declares `lib.GEMM_EXPORTS` and nothing else; the built library exports
    them; the descriptor's new field is its last and the ABI version stays 6."""
    import ctypes
    import os
    import re
    from ccvs_amd import lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ccvs_hip_gemm.h")).read()
    assert re.search(r'^#include "ccvs_hip_gemm.h"', open(os.path.join(root, "include", "ccvs_hip.h")).read(), re.M)
    assert sorted(set(re.findall(r"\b(ccvs_[a-zA-Z0-9_]+)\s*\(", header))) == sorted(lib.GEMM_EXPORTS) == ["ccvs_gemm_tiled", "ccvs_gemm_tiled_max_rows"]
    assert not set(lib.GEMM_EXPORTS) & (set(lib.EXPORTS) | set(lib.EVAL_EXPORTS) | set(lib.INPUT_EXPORTS))
    assert lib.GptDecode._fields_[-1][0] == "w_tiled"
    if os.path.exists(lib.LIB_PATH):
        handle = ctypes.CDLL(lib.LIB_PATH)
        assert all(hasattr(handle, sym) for sym in lib.GEMM_EXPORTS)
        handle.ccvs_abi_version.restype = ctypes.c_int
        assert handle.ccvs_abi_version() == 6


# ---------------------------------------------------------------------------------------------------------------------------
# op level
# ---------------------------------------------------------------------------------------------------------------------------
def plan(M, N, K, ln):
    """gpt.hip's gemm_kz + gemm16_plan for a decode call (as tests/test_gemm_forms_gpu.py transcribes them): (form, ks, kz, full batches,
    remainder steps per slice)."""
    cdiv = lambda a, b: -(-a // b)
    kz = 1
    if not ln and cdiv(N, 16) * 16 <= 1024:
        while K >= 2048 and kz < 4 and cdiv(N, 16) * kz * 2 <= 256 and K % (64 * kz * 2) == 0:
            kz *= 2
    ks = 4
    while ks > 1 and K % (16 * ks * kz) != 0:
        ks >>= 1
    form = "tile2" if M > 32 and N >= 32 else "tile1"
    step = 64 if form == "tile1" else 16
    kper = K // (ks * kz)
    return form, ks, kz, kper // step, (kper % step) // 16


MS = [16, 23, 37, 48, 64]
NK = [(48, 64), (40, 64), (48, 1024), (40, 1024), (64, 4096)]
assert [plan(m, 40, 64, False)[0] for m in MS] == ["tile1", "tile1", "tile2", "tile2", "tile2"]
assert plan(16, 40, 64, False) == ("tile1", 4, 1, 0, 1) and plan(48, 40, 64, True) == ("tile2", 4, 1, 1, 0)
assert plan(23, 48, 1024, False) == ("tile1", 4, 1, 4, 0) and plan(37, 48, 1024, True) == ("tile2", 4, 1, 16, 0)
assert plan(16, 64, 4096, False) == ("tile1", 4, 4, 4, 0) and plan(64, 64, 4096, False) == ("tile2", 4, 4, 16, 0)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ccvs_amd import ops as _ops
    return _ops


def check(got, want, scale, what):
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), what
    ratio = ((got - want).abs() / scale).max().item()
    assert ratio <= REL, f"{what}: max |err| / A = {ratio:.3e} > {REL:.0e}"


def pad16(n):
    return -(-n // 16) * 16


def x_rows(x_cpu):
    """x on the GPU as the first M rows of a buffer of pad16(M) rows whose other rows are NaN."""
    m, k = x_cpu.shape
    big = torch.full((pad16(m), k), NAN, device="cuda")
    big[:m] = x_cpu.cuda()
    return big[:m]


def tile_nan_padded(ops, w):
    """tile_weight(w) with the padding rows (N up to a multiple of 16) NaN instead of copies of the last row."""
    n, k = w.shape
    full = torch.cat([w, torch.full((pad16(n) - n, k), NAN, device=w.device)], dim=0)
    t = ops.tile_weight(full)
    assert t.numel() == pad16(n) * k and int(torch.isnan(t).sum()) == (pad16(n) - n) * k
    return t


def out_buf(m, n):
    """A NaN buffer [pad16(m), n + 24]; the output is its rows [0, m), columns [8, 8 + n)."""
    big = torch.full((pad16(m), n + 24), NAN, device="cuda")
    return big, big[:m, 8:8 + n]


def untouched(big, m, n):
    assert torch.isnan(big[m:]).all(), "a row >= M was written"
    assert torch.isnan(big[:, :8]).all() and torch.isnan(big[:, 8 + n:]).all(), "a column outside [0, N) was written"


@functools.lru_cache(maxsize=None)
def nt_case(ops, m, n, k):
    g = torch.Generator().manual_seed(1000 * m + 10 * n + k)
    x_cpu = torch.randn(m, k, generator=g)
    w = torch.randn(n, k, generator=g) / k ** 0.5
    b = torch.randn(n, generator=g)
    res = torch.randn(m, n, generator=g)
    x64, w64 = x_cpu.double(), w.double()
    wc = w.cuda()
    return dict(x=x_rows(x_cpu), w=wc, wt=tile_nan_padded(ops, wc), b=b.cuda(), res=res.cuda(), xw=x64 @ w64.t(), a=x64.abs() @ w64.abs().t(),
                b64=b.double(), res64=res.double())


@gpu
@pytest.mark.parametrize("n,k", NK)
@pytest.mark.parametrize("m", MS)
def test_gemm_tiled_equals_row_major_and_float64(ops, m, n, k):
    """ccvs_gemm_tiled as ccvs_gemm_nt: epilogues none, GELU and residual (the residual in a strided buffer of its own)."""
    c = nt_case(ops, m, n, k)
    z = c["xw"] + c["b64"]
    for name, epi, bias, want, scale in (("none", ops.EPI_NONE, c["b"], z, c["a"]),
                                         ("gelu", ops.EPI_GELU, c["b"], F.gelu(z), 1.2 * c["a"] + 1e-3),
                                         ("residual", ops.EPI_RESIDUAL, None, c["xw"] + c["res64"], c["a"])):
        r = None
        if epi == ops.EPI_RESIDUAL:
            rbig, r = out_buf(m, n)
            r.copy_(c["res"])
        _, ref = out_buf(m, n)
        ops.gemm_nt(c["x"], c["w"], bias, epi, residual=r, out=ref)
        big, out = out_buf(m, n)
        got = ops.gemm_tiled(c["x"], c["wt"], n, bias, epi, residual=r, out=out)
        assert got is out
        what = f"{name} {m}x{n}x{k}"
        assert torch.isfinite(out).all(), what
        assert torch.equal(out, ref), f"{what}: tiled and row-major weights differ in {int((out != ref).sum())} elements"
        check(out, want, scale, what)
        untouched(big, m, n)
        if r is not None:
            assert torch.equal(r, c["res"]), "the residual was written"


def ln_reference(x_cpu, packed, eps=1e-5):
    wg, bb, s = (t.double().cpu() for t in packed)
    x64 = x_cpu.double()
    mean = x64.mean(dim=1, keepdim=True)
    rstd = 1 / torch.sqrt(x64.var(dim=1, unbiased=False, keepdim=True) + eps)
    want = rstd * (x64 @ wg.t() - mean * s) + bb
    a = rstd * (x64.abs() @ wg.abs().t() + mean.abs() * s.abs()) + bb.abs()
    return want, a


@gpu
@pytest.mark.parametrize("n,k", NK[:4])
@pytest.mark.parametrize("m", MS)
def test_gemm_tiled_folded_layernorm(ops, m, n, k):
    """ccvs_gemm_tiled as ccvs_gemm_ln: rows of non-zero mean, epilogues none and GELU."""
    g = torch.Generator().manual_seed(m + 11 * n + k)
    x_cpu = torch.randn(m, k, generator=g) * 0.7 + 0.3
    w, b = torch.randn(n, k, generator=g) / k ** 0.5, torch.randn(n, generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(k, generator=g), 0.2 * torch.randn(k, generator=g)
    packed = ops.pack_ln_linear(w, b, gamma, beta)
    want, a = ln_reference(x_cpu, packed)
    wg, bb, s = (t.cuda() for t in packed)
    wt = tile_nan_padded(ops, wg)
    x = x_rows(x_cpu)
    for name, epi, wnt, scale in (("none", ops.EPI_NONE, want, a), ("gelu", ops.EPI_GELU, F.gelu(want), 1.2 * a + 1e-3)):
        _, ref = out_buf(m, n)
        ops.gemm_ln(x, wg, bb, s, epilogue=epi, out=ref)
        big, out = out_buf(m, n)
        ops.gemm_tiled(x, wt, n, bb, epi, out=out, ln_s=s)
        what = f"ln {name} {m}x{n}x{k}"
        assert torch.isfinite(out).all(), what
        assert torch.equal(out, ref), f"{what}: tiled and row-major weights differ in {int((out != ref).sum())} elements"
        check(out, wnt, scale, what)
        untouched(big, m, n)


@gpu
@pytest.mark.parametrize("C,H", [(64, 4), (256, 4)])
@pytest.mark.parametrize("m", MS)
def test_gemm_tiled_qkv_scatter(ops, m, C, H):
    """ccvs_gemm_tiled as ccvs_gemm_ln_qkv with one position per row (N = 3 C: 12 / 48 column tiles): q, and the one written slot of
    both caches (device-resident position), equal the row-major kernel's and meet the float64 bound; every other slot stays NaN."""
    D, tmax, pos0, pos_dev = C // H, 7, 2, 3
    g = torch.Generator().manual_seed(m + C)
    x_cpu = torch.randn(m, C, generator=g) * 0.7 + 0.3
    w, b = torch.randn(3 * C, C, generator=g) / C ** 0.5, torch.randn(3 * C, generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    packed = ops.pack_ln_linear(w, b, gamma, beta)
    want, a = ln_reference(x_cpu, packed)
    wg, bb, s = (t.cuda() for t in packed)
    wt = ops.tile_weight(wg)
    x = x_rows(x_cpu)
    pd = torch.tensor([pos_dev], dtype=torch.int32, device="cuda")
    pos = pos0 + pos_dev
    runs = []
    for tiled in (False, True):
        kc = torch.full((m, H, tmax, D), NAN, device="cuda")
        vc = torch.full((m, H, tmax, D), NAN, device="cuda")
        q = torch.full((m, C), NAN, device="cuda")
        if tiled:
            ops.gemm_tiled(x, wt, 3 * C, bb, out=q, ln_s=s, kcache=kc, vcache=vc, pos0=pos0, pos_dev=pd)
        else:
            ops.gemm_ln_qkv(x, wg, bb, s, kc, vc, m, 1, pos0, pd, out=q)
        runs.append((q, kc, vc))
    (q0, k0, v0), (q, kc, vc) = runs
    assert torch.equal(q, q0) and torch.equal(kc[:, :, pos], k0[:, :, pos]) and torch.equal(vc[:, :, pos], v0[:, :, pos])
    check(q, want[:, :C], a[:, :C], "q")
    check(kc[:, :, pos], want[:, C:2 * C].view(m, H, D), a[:, C:2 * C].view(m, H, D), "k cache")
    check(vc[:, :, pos], want[:, 2 * C:].view(m, H, D), a[:, 2 * C:].view(m, H, D), "v cache")
    for cache in (kc, vc):
        assert torch.isnan(cache[:, :, :pos]).all() and torch.isnan(cache[:, :, pos + 1:]).all(), "a slot other than pos was written"


@gpu
def test_gemm_tiled_refuses_what_it_does_not_cover(ops):
    """Tiled weights are read by the decode forms only: more rows than they take is an error, never another kernel on the wrong layout."""
    from ccvs_amd.lib import CcvsError
    x = torch.randn(257, 64, device="cuda")
    wt = ops.tile_weight(torch.randn(48, 64, device="cuda"))
    with pytest.raises(CcvsError):
        ops.gemm_tiled(x, wt, 48)


# ---------------------------------------------------------------------------------------------------------------------------
# step level
# ---------------------------------------------------------------------------------------------------------------------------
def _net(seed=3, n_layer=2, n_embd=64, n_head=4, vocab=96, block=32, shape=(4, 4), num_blocks=2):
    from ccvs_amd.models.skip_vid_generator.models import mingpt
    torch.manual_seed(seed)
    net = mingpt.GPT(vocab_size=vocab, block_size=block, num_blocks=num_blocks, n_layer=n_layer, n_head=n_head, n_embd=n_embd, emb_mode="temporal",
                     shape=shape).cuda()
    for p in net.parameters():
        p.data.add_(0.05 * torch.randn_like(p))
    return net


def _run(net, tiled, codes, n_new, groups, use_graph, sample, noise="device", host_streams=None, persistent=False):
    net.drop_engine_state()
    net.tiled_weights, net.persistent_step = tiled, persistent
    keys = [(0x1234567 + 977 * g, 0xabcdef01 ^ (g << 7)) for g in range(groups)]
    if groups > 1:
        net.noise_key, net.row_offset, net.noise_call = list(keys), [32] * groups, 0
    else:
        net.noise_key, net.row_offset, net.noise_call = keys[0], 32, 0
    if host_streams is not None:
        net.noise_streams = [s.clone() for s in host_streams]
    out = net.generate(codes, n_new, sample=sample, top_k=20, noise=noise, use_graph=use_graph)
    net.check_steps()
    torch.cuda.synchronize()
    c = net._cache
    assert c["desc"][1].desc.w_tiled == (1 if tiled and codes.shape[0] <= 256 else 0) and c["desc"][1].persistent == persistent
    state = {"tokens": out.clone(), "logits": c["logits"].clone(), "x": c["x"].clone(), "q": c["q"].clone(), "att": c["att"].clone(), "h": c["h"].clone(),
             "k": [k.clone() for k in c["k"]], "v": [v.clone() for v in c["v"]], "len": c["len_dev"].clone(), "widx": c["widx"].clone(),
             "state": c["state"].clone()}
    net.noise_key, net.row_offset, net.noise_streams, net.persistent_step = None, 0, None, False
    return state


def _assert_same(a, b, what):
    for key in ("tokens", "logits", "x", "q", "att", "h", "len", "widx", "state"):
        assert torch.equal(a[key], b[key]), f"{what}: `{key}` differs between row-major and tiled weights"
    L = int(a["len"].max())     # (the caches are torch.empty: only the appended rows are defined)
    for l, (ka, kb, va, vb) in enumerate(zip(a["k"], b["k"], a["v"], b["v"])):
        assert torch.equal(ka[:, :, :L], kb[:, :, :L]) and torch.equal(va[:, :, :L], vb[:, :, :L]), f"{what}: KV cache of layer {l} differs"


N_NEW, PREFIX = 20, 5


@pytest.fixture(scope="module")
def small():
    return _net()


@gpu
@pytest.mark.parametrize("batch,groups", [(16, 1), (16, 3), (16, 4), (5, 3)])
@pytest.mark.parametrize("use_graph", [True, False])
def test_step_tiled_weights_equal_row_major(small, batch, groups, use_graph):
    """16, 48, 64 rows and 15 rows in 3 groups of 5; sampled in the kernel (Philox); graph-replayed and eager."""
    g = torch.Generator().manual_seed(batch * 10 + groups)
    codes = torch.randint(0, 96, (batch * groups, PREFIX), generator=g).cuda()
    base = _run(small, False, codes, N_NEW, groups, use_graph, sample=True)
    tiled = _run(small, True, codes, N_NEW, groups, use_graph, sample=True)
    assert not torch.equal(base["tokens"][:, PREFIX:], base["tokens"][:, PREFIX:PREFIX + 1].expand(-1, N_NEW)), "degenerate sample"
    _assert_same(base, tiled, f"{batch} x {groups} rows, graph={use_graph}")


@gpu
def test_step_of_more_rows_than_the_tiled_forms_take_keeps_row_major_weights(small, ops):
    """257 rows: the step runs the row-blocked GEMM, which reads row-major weights -- `GPT.tiled_weights` then leaves the descriptor
    row-major (`_run` checks w_tiled == 0) instead of handing tiled pointers to a kernel that cannot read them; 256 rows still run tiled."""
    assert ops.gemm_tiled_max_rows() == 256
    for rows in (256, 257):
        codes = torch.randint(0, 96, (rows, PREFIX), generator=torch.Generator().manual_seed(rows)).cuda()
        _assert_same(_run(small, False, codes, 6, 1, True, sample=False), _run(small, True, codes, 6, 1, True, sample=False), f"{rows} rows")


@gpu
def test_step_tiled_weights_greedy_and_host_noise(small):
    batch, groups = 16, 3
    codes = torch.randint(0, 96, (batch * groups, PREFIX), generator=torch.Generator().manual_seed(7)).cuda()
    _assert_same(_run(small, False, codes, N_NEW, groups, True, sample=False), _run(small, True, codes, N_NEW, groups, True, sample=False), "greedy")
    g = torch.Generator().manual_seed(9)
    streams = [torch.empty(N_NEW, batch, 96).exponential_(1, generator=g).cuda() for _ in range(groups)]
    base = _run(small, False, codes, N_NEW, groups, True, sample=True, noise="host", host_streams=streams)
    tiled = _run(small, True, codes, N_NEW, groups, True, sample=True, noise="host", host_streams=streams)
    _assert_same(base, tiled, "host noise streams")


@gpu
@pytest.mark.parametrize("batch,groups", [(16, 1), (16, 3), (5, 3)])
def test_step_tiled_weights_persistent_form(small, batch, groups):
    """The persistent step (one block per workgroup at 16 and 15 rows, 2 x 2 blocks at 48) on tiled weights against the launch chain on
    row-major ones."""
    codes = torch.randint(0, 96, (batch * groups, PREFIX), generator=torch.Generator().manual_seed(groups)).cuda()
    base = _run(small, False, codes, N_NEW, groups, True, sample=True)
    tiled = _run(small, True, codes, N_NEW, groups, True, sample=True, persistent=True)
    _assert_same(base, tiled, f"persistent, {batch} x {groups} rows")


@gpu
def test_step_tiled_weights_follow_an_update_of_proj(small):
    """The tiled copies are cached on (data_ptr, _version) of their sources -- the projection and mlp[3] weights included, which the
    row-major step reads in place: after an in-place update the next sequence runs on new copies."""
    codes = torch.randint(0, 96, (16, PREFIX), generator=torch.Generator().manual_seed(1)).cuda()
    first = _run(small, True, codes, N_NEW, 1, True, sample=False)
    saved = small.blocks[1].attn.proj.weight.detach().clone()
    try:
        with torch.no_grad():
            small.blocks[1].attn.proj.weight.copy_(saved.flip(0))
        _assert_same(_run(small, False, codes, N_NEW, 1, True, sample=False), _run(small, True, codes, N_NEW, 1, True, sample=False), "updated proj")
        assert not torch.equal(small._cache["logits"], first["logits"])
    finally:
        with torch.no_grad():
            small.blocks[1].attn.proj.weight.copy_(saved)


@gpu
def test_step_tiled_weights_full_size_gpt_same_tokens():
    """BAIR geometry (24 x 1024, 16 heads, V 1024), 64 stacked rows, fixed seed: the tokens and logits of 40 steps are the row-major step's."""
    net = _net(seed=0, n_layer=24, n_embd=1024, n_head=16, vocab=1024, block=1024, shape=(8, 8), num_blocks=16)
    codes = torch.randint(0, 1024, (64, 64), generator=torch.Generator().manual_seed(0)).cuda()
    base = _run(net, False, codes, 40, 4, True, sample=True)
    tiled = _run(net, True, codes, 40, 4, True, sample=True)
    _assert_same(base, tiled, "full size")
