"""-m gpu: the token loop on a bf16 KV cache (`GPT.kv_dtype = "bf16"`, `--x_kv_dtype bf16`) above the kernels that
tests/test_kv_bf16_gpu.py checks: `ccvs_gpt_decode_step_bf16kv` (the launch chain, eager and as a replayed hipGraph), `GPT._layers`'
bf16 route, the descriptor / capture keys, and `Transformer` / `Generator` with the flag.  The tiny model of the fixtures (2 layers,
2 heads, C = 32: head dim 16, z_len 256) and a second small model with head dim 64.

  layer-0 cache   after a teacher-forced run on the same tokens in both modes, layer 0's bf16 cache is the reference rounding of layer
                  0's fp32 cache bit for bit (layer 0's K / V depend on the embeddings only): prefill rows, rows appended by per-op
                  decode steps, and rows appended by the launch chain of a graph-replayed generate().
  the chain       the logits of every bf16-mode decode step of the launch chain equal, bit for bit (what the fp32 tests ask of the
                  fp32 chain against its per-op path, tests/test_ln_fold_gpu.py), (a) the per-op engine's (`GPT.step`) and (b) a
                  composition written out here from the ops on the SAME stored cache: gpt_embed, gemm_ln, attention_bf16 in the
                  pre-appended form, gemm_nt, gemm_ln, gemm_nt, ..., the head.
  forms agree     eager step launches and graph replay give the same tokens and the same cache bits: one and three row groups; greedy,
                  host noise (three groups: one pre-drawn stream per group) and Philox; with and without top_p = 0.9; two runs give the same bits; rows 2..3 alone equal
                  rows 2..3 inside a batch.
  capture key     a step captured in one dtype is never replayed for the other: switching dtype on the same GPT object re-allocates
                  (new cache dict, no graphs carried over) and fp32 gives the fp32 mode's golden tokens again.
  Transformer     with --x_kv_dtype bf16: the plain path, the sliding-window path and beam search (beam 3) generate; run_pipelined
                  equals the serial schedule token for token and pixel for pixel; the persistent-step combination raises.
Without the flag the tiny model's golden streams are tests/test_e2e_gpu.py's (unchanged, and run on this tree).

NOT BUILT: the issue's check of the deeper layers' caches against a float64 recomputation with a band around rounding midpoints.  The
tolerance it names (the tiny golden test's 1e-4) puts 5 to 13 % of unit-scale values inside the band -- 2 tol / 2^(e-7) of the values in
[2^e, 2^(e+1)) -- against its own cap of 1 %, so the check as specified cannot hold and no other tolerance was to be invented."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_bf16_ref as K  # noqa: E402
from tests.test_e2e_gpu import tiny, TINY_ARGV, _load, _sd  # noqa: F401,E402  (fixture)

pytestmark = pytest.mark.gpu

KEYS = [(0x1234567 + 977 * g, 0xabcdef01 ^ (g << 7)) for g in range(3)]
ROW_OFFSETS = [32, 1000, 0xffffffff]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ccvs_amd import ops as _ops
    return _ops


def _gpt64():
    """2 layers, 2 heads of 64 dims, vocabulary 200 (no multiple of 16)."""
    from ccvs_amd.models.skip_vid_generator.models import mingpt
    torch.manual_seed(5)
    net = mingpt.GPT(vocab_size=200, block_size=512, num_blocks=32, n_layer=2, n_head=2, n_embd=128, emb_mode="temporal", shape=(4, 4)).cuda()
    for p in net.parameters():
        p.data.add_(0.1 * torch.randn_like(p))
    return net


@pytest.fixture(scope="module")
def nets(tiny):
    return {"tiny": (tiny["tr"].net_t, 32), "d64": (_gpt64(), 200)}


class mode:
    """`with mode(net, "bf16"):` -- the dtype for the block, fp32 and a dropped engine state afterwards."""

    def __init__(self, net, kv_dtype):
        self.net, self.kv_dtype = net, kv_dtype

    def __enter__(self):
        self.net.drop_engine_state()
        self.net.kv_dtype = self.kv_dtype
        return self.net

    def __exit__(self, *exc):
        self.net.kv_dtype = "fp32"
        self.net.noise_key, self.net.row_offset, self.net.noise_call, self.net.noise_streams = None, 0, 0, None
        self.net.drop_engine_state()


def cache_bits(net, n):
    """The first n positions of every layer's K and V as int32 bit patterns (bf16) or fp32 values, on the host."""
    c = net._cache
    out = []
    for t in c["k"] + c["v"]:
        t = t[:, :, :n].cpu()
        out.append(K.bits_of(t) if t.dtype == torch.bfloat16 else t.clone())
    return out


def teacher_forced(net, tokens, t0):
    """prefill of tokens[:, :t0], then one per-op step per further token (the last token is not fed).  -> logits [n, B, V]."""
    b, t = tokens.shape
    net.begin(b, t)
    logits = [net.prefill(tokens[:, :t0].contiguous())]
    for i in range(t0, t - 1):
        logits.append(net.step(tokens[:, i:i + 1]))
    torch.cuda.synchronize()
    return torch.stack(logits)


# ------------------------------------------------------------------ layer-0 cache
@pytest.mark.parametrize("which", ["tiny", "d64"])
def test_layer0_cache_is_the_rounding_of_the_fp32_cache(nets, which):
    net, vocab = nets[which]
    b, t0, n_new = 3, 70, 9
    codes = torch.randint(0, vocab, (b, t0), generator=torch.Generator().manual_seed(3)).cuda()
    with mode(net, "bf16"):
        tokens = net.generate(codes, n_new, sample=False)          # graph replay: rows t0 .. appended by the launch chain
        torch.cuda.synchronize()
        n = t0 + n_new - 1
        assert net._cache["k"][0].dtype == torch.bfloat16 and net._cache["len"] == n
        chain = cache_bits(net, n)
        net.drop_engine_state()
        teacher_forced(net, tokens, t0)                            # per-op: prefill rows, then the appending decode form
        per_op = cache_bits(net, n)
    with mode(net, "fp32"):
        teacher_forced(net, tokens, t0)
        assert net._cache["k"][0].dtype == torch.float32
        full = cache_bits(net, n)
    n_layer = len(full) // 2
    for name, got in (("launch chain", chain), ("per-op", per_op)):
        for kv, off in (("K", 0), ("V", n_layer)):
            want = K.bf16_bits(full[off])
            assert torch.equal(got[off][:, :, :t0], want[:, :, :t0]), f"{name}: layer 0 {kv}, prefill rows"
            assert torch.equal(got[off][:, :, t0:], want[:, :, t0:]), f"{name}: layer 0 {kv}, rows appended by decode steps"
    for a, b_ in zip(chain, per_op):                               # and every layer: the two bf16 paths store the same bits
        assert torch.equal(a, b_), "launch chain and per-op path store different cache bits"
    # the deeper layer sees rounded keys and values: its cache is NOT the rounding of the fp32 mode's (the mode is not a no-op)
    assert not torch.equal(chain[1], K.bf16_bits(full[1]))


# ------------------------------------------------------------------ the chain
@pytest.mark.parametrize("which", ["tiny", "d64"])
def test_chain_logits_equal_the_per_op_composition(ops, nets, which):
    net, vocab = nets[which]
    b, t0, n_new = 3, 37, 7
    C, H = net.config.n_embd, net.config.n_head
    codes = torch.randint(0, vocab, (b, t0), generator=torch.Generator().manual_seed(4)).cuda()
    with mode(net, "bf16"):
        trace = []
        tokens = net.generate(codes, n_new, sample=False, trace=trace)       # eager launches of ccvs_gpt_decode_step_bf16kv
        chain = torch.stack(trace)                                           # [n_new, B, V]: logits in front of every pick
        c = net._cache
        kc, vc, table = [t.clone() for t in c["k"]], [t.clone() for t in c["v"]], c["pos_table"].clone()
        net.drop_engine_state()
        per_op = teacher_forced(net, tokens, t0)
        assert torch.equal(chain, per_op), "launch chain and per-op engine give different logits"
        # (b) written out, on the cache the chain left behind: step i feeds token t0 + i - 1 at that position
        for i in range(1, n_new):
            pos = t0 + i - 1
            x = ops.gpt_embed(tokens[:, pos:pos + 1], net._token_table(), table, pos)
            for li, blk in enumerate(net.blocks):
                qkv_w, fc_w = blk.folded()
                qkv = ops.gemm_ln(x, *qkv_w, eps=blk.ln1.eps).view(b, 1, 3 * C)
                att = ops.attention_bf16(qkv[..., :C], kc[li], vc[li], pos)                       # pre-appended: the stored row
                stored = K.bits_of(kc[li][:, :, pos].cpu()).view(b, C)
                assert torch.equal(stored, K.bf16_bits(qkv[:, 0, C:2 * C].cpu().contiguous())), "stored K row is not the rounded GEMM row"
                stored_v = K.bits_of(vc[li][:, :, pos].cpu()).view(b, C)
                assert torch.equal(stored_v, K.bf16_bits(qkv[:, 0, 2 * C:].cpu().contiguous())), "stored V row is not the rounded GEMM row"
                x = ops.gemm_nt(att.view(b, C), blk.attn.proj.weight, blk.attn.proj.bias, ops.EPI_RESIDUAL, residual=x)
                h = ops.gemm_ln(x, *fc_w, eps=blk.ln2.eps, epilogue=ops.EPI_GELU)
                x = ops.gemm_nt(h, blk.mlp[3].weight, blk.mlp[3].bias, ops.EPI_RESIDUAL, residual=x)
            logits = net._head(x)
            assert torch.equal(logits, chain[i]), f"step {i}: the composition of the ops differs from the chain's logits"
        assert H * (C // H) == C


# ------------------------------------------------------------------ forms agree
def _generate(net, codes, groups, sampler, top_p, form, n_new, offsets=None, keys=None):
    """-> (tokens on the host, cache bits).  sampler: "greedy" | "philox" | "host"."""
    net.drop_engine_state()
    keys = KEYS[:groups] if keys is None else keys
    offsets = ROW_OFFSETS[:groups] if offsets is None else offsets
    if groups > 1:
        net.noise_key, net.row_offset = list(keys), list(offsets)
    else:
        net.noise_key, net.row_offset = keys[0], offsets[0]
    net.noise_call = 0
    kw = dict(sample=sampler != "greedy", top_k=20, top_p=top_p, use_graph=form == "graph")
    if sampler == "host":
        g = torch.Generator().manual_seed(77)
        kw.update(noise="host", host_noise=lambda nb, nv: torch.empty(nb, nv).exponential_(generator=g))
        if groups > 1:   # stacked batches: every group's stream is pre-drawn, [n_new, rows of the group, V] (GPT.noise_streams)
            v, per = net.head.weight.shape[0], codes.shape[0] // groups
            net.noise_streams = [torch.empty(n_new, per, v).exponential_(generator=g).cuda() for _ in range(groups)]
    out = net.generate(codes, n_new, **kw)
    torch.cuda.synchronize()
    return out.cpu(), cache_bits(net, codes.shape[1] + n_new - 1)


@pytest.mark.parametrize("which", ["tiny", "d64"])
def test_eager_and_graph_agree_exactly(nets, which):
    net, vocab = nets[which]
    b, t0, n_new = 6, 5, 21      # 20 decode steps: two replays of the 8-step graph and four of the 1-step graph
    codes = torch.randint(0, vocab, (b, t0), generator=torch.Generator().manual_seed(1)).cuda()
    with mode(net, "bf16"):
        seen = {}
        for groups, sampler, top_p in [(1, "greedy", None), (3, "greedy", None), (1, "philox", None), (3, "philox", None), (1, "philox", 0.9),
                                       (3, "philox", 0.9), (1, "host", None), (1, "host", 0.9), (3, "host", None), (3, "host", 0.9), (1, "greedy", 0.9)]:
            eager = _generate(net, codes, groups, sampler, top_p, "eager", n_new)
            graph = _generate(net, codes, groups, sampler, top_p, "graph", n_new)
            again = _generate(net, codes, groups, sampler, top_p, "graph", n_new)
            what = (groups, sampler, top_p)
            assert ((eager[0] >= 0) & (eager[0] < vocab)).all() and torch.equal(eager[0][:, :t0], codes.cpu()), what
            assert torch.equal(eager[0], graph[0]) and torch.equal(graph[0], again[0]), f"{what}: tokens differ between the forms / runs"
            for x, y, z in zip(eager[1], graph[1], again[1]):
                assert torch.equal(x, y) and torch.equal(y, z), f"{what}: cache bits differ between the forms / runs"
            seen[what] = graph[0]
        assert torch.equal(seen[(1, "greedy", None)], seen[(3, "greedy", None)]), "greedy tokens depend on the grouping"
        assert torch.equal(seen[(1, "greedy", None)], seen[(1, "greedy", 0.9)]), "the greedy pick depends on top_p"
        assert not torch.equal(seen[(1, "philox", None)][:, t0:], seen[(1, "greedy", None)][:, t0:])
        # batch-slot independence: rows 2..3 alone, under the words they have inside the batch
        whole, whole_bits = _generate(net, codes, 1, "philox", None, "graph", n_new, offsets=[32])
        alone, alone_bits = _generate(net, codes[2:4].contiguous(), 1, "philox", None, "graph", n_new, offsets=[34])
        assert torch.equal(whole[2:4], alone), "rows 2..3 alone draw other tokens"
        for x, y in zip(whole_bits, alone_bits):
            assert torch.equal(x[2:4], y), "rows 2..3 alone store other cache bits"
        stacked, _ = _generate(net, codes, 3, "philox", 0.9, "graph", n_new)
        for g in range(3):
            alone, _ = _generate(net, codes[2 * g:2 * g + 2].contiguous(), 1, "philox", 0.9, "eager", n_new, offsets=ROW_OFFSETS[g:g + 1], keys=KEYS[g:g + 1])
            assert torch.equal(stacked[2 * g:2 * g + 2], alone), f"group {g} alone draws other tokens"


# ------------------------------------------------------------------ capture key
def test_switching_dtype_reallocates_and_fp32_keeps_its_golden_tokens(tiny):
    g, tr, xopt = tiny["gold"], tiny["tr"], tiny["xopt"]
    net = tr.net_t
    xopt.sample, xopt.top_k = False, 10
    want = torch.from_numpy(g["gen_code_greedy"])
    with mode(net, "fp32"):
        base = tr({"code": want[:, :64].clone()}, mode="inference", total_len=256)["code"].cpu()
        c32 = net._cache
        assert c32["kv_dtype"] == torch.float32 and len(c32["graphs"]) > 0 and c32["q"].shape == (2, 32)
        key32 = set(c32["graphs"])
        net.kv_dtype = "bf16"                                  # same object, same batch size, same lengths
        out16 = tr({"code": want[:, :64].clone()}, mode="inference", total_len=256)["code"].cpu()
        c16 = net._cache
        assert c16 is not c32 and c16["kv_dtype"] == torch.bfloat16 and c16["k"][0].dtype == torch.bfloat16 and c16["q"].shape == (2, 96)
        assert len(c16["graphs"]) > 0 and not (set(c16["graphs"]) & key32), "a capture key does not carry the dtype"
        assert all(k[-1] == torch.bfloat16 or torch.bfloat16 in k for k in c16["graphs"])
        assert c16["desc"][1].kv_dtype == torch.bfloat16 and c32["desc"][1].kv_dtype == torch.float32
        assert net._caches[2] is c16
        assert out16.shape == base.shape and ((out16 >= 0) & (out16 < 32)).all() and torch.equal(out16[:, :64], want[:, :64])
        net.kv_dtype = "fp32"
        back = tr({"code": want[:, :64].clone()}, mode="inference", total_len=256)["code"].cpu()
        assert net._cache is not c16 and net._cache["kv_dtype"] == torch.float32
        assert torch.equal(back, base), "fp32 tokens changed after a bf16 run on the same object"
    if not torch.equal(base, want):     # (the golden audit of tests/test_e2e_gpu.py: a divergence only at a logit near-tie)
        bb, t = (base != want).nonzero()[0].tolist()
        lg = torch.from_numpy(g["gpt_logits"])[bb, t - 1]
        assert (lg[base[bb, t]] - lg[want[bb, t]]).abs().item() < 1e-4


# ------------------------------------------------------------------ Transformer / Generator with the flag
@pytest.fixture(scope="module")
def tiny16(tiny):
    from ccvs_amd.tools.options import Options
    from ccvs_amd.models.skip_vid_generator.models.transformer_model import Transformer
    opt = Options().parse(load_qvid_generator=True, load_transformer=True, argv=TINY_ARGV + ["--x_kv_dtype", "bf16"])
    tr = Transformer(opt["transformer"], is_train=False, is_main=True).eval()
    _load(tr.net_t, _sd(tiny["gold"], "t"))
    assert tr.net_t.kv_dtype == "bf16"
    return dict(opt=opt, xopt=opt["transformer"], tr=tr)


def test_transformer_generates_on_a_bf16_cache(tiny, tiny16, golden_dir):
    tr, xopt = tiny16["tr"], tiny16["xopt"]
    want = torch.from_numpy(tiny["gold"]["gen_code_greedy"])
    xopt.sample, xopt.top_k = False, 10
    # plain path, and the sliding window (total_len > z_len: two slides, each a re-prefill of the window on the bf16 cache)
    for total in (256, 256 + 2 * 64):
        out = tr({"code": want[:, :64].clone()}, mode="inference", total_len=total)["code"].cpu()
        assert tr.net_t._cache["k"][0].dtype == torch.bfloat16
        again = tr({"code": want[:, :64].clone()}, mode="inference", total_len=total)["code"].cpu()
        assert out.shape == (2, total) and ((out >= 0) & (out < 32)).all() and torch.equal(out[:, :64], want[:, :64])
        assert torch.equal(out, again), f"total_len {total}: two runs differ"
        if total == 256:
            # the greedy stream is the argmax of the mode's own teacher-forced logits (whole-sequence forward on a bf16 cache), up to near-ties
            logits = tr.net_t(out[:, :-1].cuda()).cpu()
            pick = logits[:, 63:].argmax(-1)
            diff = (pick != out[:, 64:]).nonzero()
            for bb, t in diff.tolist():
                lg = logits[bb, 63 + t]
                assert (lg[pick[bb, t]] - lg[out[bb, 64 + t]]).abs().item() < 1e-4, (bb, t)
            share = (out[:, 64:] != want[:, 64:]).float().mean().item()
            print(f"tiny model, greedy: {share:.3f} of the tokens differ from the fp32 mode's golden stream")
    # beam search (beam 3, as tests/golden/tiny_beam.npz's case): hypotheses are cache rows, pruning gathers bf16 rows
    g = np.load(os.path.join(golden_dir, "tiny_beam.npz"))
    code = torch.from_numpy(g["code"])
    empty = torch.tensor([])
    old = (xopt.sample, xopt.top_k, getattr(xopt, "beam_size", None), getattr(xopt, "no_sample", False), tr.sample_noise)
    try:
        xopt.beam_size, xopt.top_k = 3, 10
        tr.sample_noise, tr.generator = "host", None
        for name, sample, no_sample, add_len in (("greedy", False, False, 12), ("prune", False, True, 12), ("sampled_prune", True, True, 8)):
            xopt.sample, xopt.no_sample = sample, no_sample
            torch.manual_seed(5)
            got = tr.fill_code(code.clone().cuda(), empty.cuda(), empty.cuda(), None, empty, add_len=add_len)[0].cpu()
            torch.manual_seed(5)
            again = tr.fill_code(code.clone().cuda(), empty.cuda(), empty.cuda(), None, empty, add_len=add_len)[0].cpu()
            ref = torch.from_numpy(g["beam_" + name])
            assert got.shape == ref.shape and ((got >= 0) & (got < 32)).all() and torch.equal(got[:, :code.shape[1]], code), name
            assert torch.equal(got, again), name
            assert tr.net_t._cache["k"][0].dtype == torch.bfloat16
    finally:
        xopt.sample, xopt.top_k, xopt.beam_size, xopt.no_sample, tr.sample_noise = old
    tr.net_t.drop_engine_state()


def test_pipelined_equals_serial_on_a_bf16_cache(tiny, tiny16):
    from ccvs_amd.helpers.generator import Generator
    xopt, tr = tiny16["xopt"], tiny16["tr"]
    xopt.sample, xopt.top_k, xopt.rec_pass = True, 10, False
    old_noise = tr.sample_noise
    tr.sample_noise = "device"
    try:
        gen = Generator(tiny16["opt"])
        gen.vid_model, gen.transformer_model = tiny["qv"], tr
        batches = [gen.synthetic_batch(2, seed=80 + i)["vid"] for i in range(4)]
        serial = [gen.generate_vid({"vid": b.clone()}, global_iter=10 + i, schedule="serial") for i, b in enumerate(batches)]
        stream = [gen.generate_vid({"vid": b.clone()}, global_iter=10 + i, schedule="stream") for i, b in enumerate(batches[:2])]
        res = gen.run_pipelined(({"vid": b.clone()} for b in batches), first_iter=10, lanes=2, chains=2)
        torch.cuda.synchronize()
        assert [r["index"] for r in res] == [10, 11, 12, 13]
        for want, got in zip(serial, res):
            assert torch.equal(got["fake"]["code"], want["fake"]["code"]), "pipelined tokens differ from the serial schedule"
            assert torch.equal(got["fake"]["vid"], want["fake"]["vid"])
        for want, got in zip(serial, stream):
            assert torch.equal(got["fake"]["code"], want["fake"]["code"]), "stream schedule differs from the serial one"
        assert all(c["kv_dtype"] == torch.bfloat16 for chain in gen._chains for c in chain[0].net_t._caches.values())
        assert not torch.equal(res[0]["fake"]["code"], res[1]["fake"]["code"])
    finally:
        xopt.sample, xopt.rec_pass = False, True
        tr.sample_noise = old_noise
        tr.net_t.drop_engine_state()


def test_persistent_step_and_state_front_are_refused(tiny, tiny16, monkeypatch):
    from ccvs_amd.tools.options import Options
    from ccvs_amd.models.skip_vid_generator.models.transformer_model import Transformer
    net = tiny16["tr"].net_t
    net.drop_engine_state()
    net.persistent_step = True
    try:
        with pytest.raises(ValueError, match="CCVS_DECODE_PERSISTENT=1 together with a bf16 KV cache.*fp32 caches only"):
            net.generate(torch.zeros(2, 8, dtype=torch.int64, device="cuda"), 6)
        assert net._cache is None and not net._caches
    finally:
        net.persistent_step = False
    monkeypatch.setenv("CCVS_DECODE_PERSISTENT", "1")
    with pytest.raises(ValueError, match="CCVS_DECODE_PERSISTENT=1 together with --x_kv_dtype bf16"):
        Transformer(tiny16["xopt"], is_train=False, is_main=True)
    monkeypatch.delenv("CCVS_DECODE_PERSISTENT")
    sf = Options().parse(load_qvid_generator=True, load_transformer=True, argv=TINY_ARGV + ["--x_kv_dtype", "bf16", "--x_state_front"])
    with pytest.raises(NotImplementedError, match="--x_state_front together with --x_kv_dtype bf16"):
        Transformer(sf["transformer"], is_train=False, is_main=True)
    # the descriptor itself refuses too (ops.GptDecodeStep), whatever built it
    from ccvs_amd import ops
    with pytest.raises(ValueError, match="fp32 KV caches only"):
        ops.GptDecodeStep([], B=1, C=32, H=2, Tmax=8, ln_eps=1e-5, tok_emb=None, pos_table=None, pos_off=0, head=(None, None, None), tok=None,
                          codes=None, widx=None, length=None, x=None, q=None, att=None, h=None, logits=None, noise=None, top_k=None,
                          temperature=1.0, state=None, persistent=True, kv_dtype="bf16")
