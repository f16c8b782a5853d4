"""-m gpu: nucleus (top-p) sampling in the token pick (gpt.hip: sample_topk_row's TOPP form through `ops.sample_topk(top_p=...)` and the
pick of the decode step) against the float64 reference of tests/nucleus_ref.py -- every single pick.  What the reference is, how its
margin m_p is derived and how a pick is judged (right for SOME nucleus inside the uncertain band) is in that module;
tests/test_nucleus_host.py checks the reference and runs an fp32 emulation of the kernel over the same table (`nucleus_ref.CASES`).
The helpers shared with the top-k pick's tests (strided views, the small GPT, the teacher-forced pass) are tests/test_pick_gpu.py's.

1  every pick of the table: greedy, host noise, Philox with immediate words; V in {1, 5, 255, 256, 257, 1000, 16384, 40164}, top_k in
   {None, 7, V - 1}, p in {0.1, 0.5, 0.9, 0.999}; logits random, quantised (exact ties), tied at the k-th value, constant, with -inf,
   two-level; a row-strided logits view on a NaN-poisoned buffer and a strided `out` whose gaps keep their poison.
2  exact properties, no margin: a row whose pick without top_p lies in the certain nucleus picks the same token with it (same noise);
   constant rows keep everything at any p; two-level rows with p below the high level's mass never pick a low entry under Philox noise
   while top_p=None on the same noise does; top_p = 1.0 and None give the bits of the existing entry points.
3  non-finite rows give token 0, the finite rows beside them keep their bits.
4  the form's own vocabulary cap (40164) is picked right (part of 1); one more raises and writes nothing.
5  in the decode step (graph replay, eager launches and the persistent step, one and three row groups): every token accepted for the
   logits of a teacher-forced per-op pass and the mirror's draw; the device-resident counters; batch-slot independence; the three
   forms draw the same tokens; two runs, same tokens; a step captured with one top_p is not replayed for another (two-level logits:
   other cache key, other tokens).
6  `Transformer` with --x_top_p 0.9 generates; with --x_beam_size as well it raises.

Every case prints its number of rows with an uncertain entry and of picks that needed the band (run with -s).

Observed on an MI355X: 201 case lines (tests 1-5), every pick accepted on the CERTAIN nucleus -- no pick needed the band; rows with an
uncertain entry: 1 of 64 in the three lines of V = 257, top_k = None, T = 1.0, p = 0.9, none elsewhere in the table, all 64 in
`test_boundary_exactly_at_p_is_out` (by construction: G == p).  There this build's expf gave exactly 0.5 for two of the three floats
around -ln 2, so the exact assertion ran.  Graph replay, eager launches and the persistent step drew the same tokens.

Mutations of gpt.hip, each built once by hand and run against this file:
  G < P -> G <= P (`P + 1`): fails `test_boundary_exactly_at_p_is_out` and nothing else -- a boundary that is exact in the kernel's
  integers is the only place where the two differ;
  the nucleus taken over all of V (`key >= thr` dropped from the mass passes, the total over every entry): fails test 1 at every V
  from 255 on and at the cap, `test_nucleus_is_taken_on_the_top_k_set`, `test_pick_inside_the_certain_nucleus_is_unchanged` at
  V = 16384, the boundary test, the top_k = 7 case of test 3, all six cases of test 5 and test 6 (17 of 37);
  the boundary tie split (entries AT the boundary key kept at even indices only): fails `test_boundary_tie_is_kept_whole`, the
  constant rows, the two-level rows, test 1 from V = 5 on, the certain-nucleus test, the boundary test and test 5 (28 of 37; the
  mutation also splits a tie that is the whole nucleus, which is why so much notices)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nucleus_ref as N  # noqa: E402
import pick_ref as R  # noqa: E402
import test_pick_gpu as TP  # noqa: E402  (helpers only)

pytestmark = pytest.mark.gpu

POISON = TP.POISON


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ccvs_amd import ops as _ops
    return _ops


def _judge(what, pick, xs, mask, p, noise64, c, cap_rows=None):
    pick = pick.cpu().numpy()
    sure_in, _, unc = N.nucleus(xs, mask, p)
    ok = N.accept(pick, xs, mask, p, noise64, c)
    s, d = R.scores64(xs, sure_in, noise64)
    band = ~R.accept(pick, s, d, c, sure_in) & ok               # right only for a nucleus larger than the certain one
    print(f"nucleus {what}: rows with an uncertain entry {int(unc.any(1).sum())} of {len(pick)}, picks that needed the band {int(band.sum())}")
    bad = np.nonzero(~ok)[0]
    assert ok.all(), (f"{what}: rows {bad[:8].tolist()} picked {pick[bad[:8]].tolist()}, float64 argmax on the certain nucleus "
                      f"{s.argmax(1)[bad[:8]].tolist()}, in the certain nucleus {sure_in[bad[:8], np.clip(pick[bad[:8]], 0, xs.shape[1] - 1)].tolist()}")
    assert band.sum() <= R.MARGIN_ONLY_CAP * (len(pick) if cap_rows is None else cap_rows), f"{what}: {int(band.sum())} picks needed the band"


def _case(ops, V, top_k, T, p):
    lg = N.case_logits(V, top_k)
    B = lg.shape[0]
    xs, mask = R.kept(lg, T, top_k)
    ndev, n64, p64 = TP._noise(B, V)
    view, out, out_buf = TP._strided(lg)
    for name, kw, noise64, c in (("greedy", {}, None, R.C_HOST), ("host noise", dict(noise=ndev), n64, R.C_HOST),
                                 ("philox", dict(philox=R.PHILOX_WORDS), p64, R.C_PHILOX)):
        out_buf.fill_(POISON)
        got = ops.sample_topk(view, top_k, T, out=out, top_p=p, **kw)
        assert got.data_ptr() == out.data_ptr() and TP._gaps_poisoned(out_buf), "the pick wrote between the elements of a strided `out`"
        _judge(f"V={V} top_k={top_k} T={T} p={p} {name}", got, xs, mask, p, noise64, c)
        if name == "greedy":
            assert torch.equal(got, ops.sample_topk(lg.cuda(), top_k, T, top_p=p)), "dense and row-strided logits give different picks"


# ------------------------------------------------------------------ 1, 4
@pytest.mark.parametrize("V", [v for v in N.VOCABS if v != N.V_TOPP_MAX])
def test_nucleus_pick_vs_float64(ops, V):
    for v, top_k, T, p in N.CASES:
        if v == V:
            _case(ops, V, top_k, T, p)


def test_nucleus_pick_at_its_vocabulary_cap(ops):
    """The largest vocabulary of the form -- ((V + 273) & ~1) + 524 words, 160 KB of LDS -- is picked right; one more raises with the
    launcher's message and writes nothing, while the top-k form still takes it."""
    from ccvs_amd.lib import CcvsError
    assert ops.sample_topp_max_vocab() == N.V_TOPP_MAX
    for v, top_k, T, p in N.CASES:
        if v == N.V_TOPP_MAX:
            _case(ops, v, top_k, T, p)
    out = torch.full((2,), POISON, dtype=torch.int64, device="cuda")
    lg = torch.zeros(2, N.V_TOPP_MAX + 1, device="cuda")
    with pytest.raises(CcvsError, match=f"ccvs_sample_topp: vocabulary {N.V_TOPP_MAX + 1} too large for the top_p form"):
        ops.sample_topk(lg, 7, 1.0, out=out, top_p=0.9)
    with pytest.raises(CcvsError, match=f"ccvs_sample_topp_philox: vocabulary {N.V_TOPP_MAX + 1} too large for the top_p form"):
        ops.sample_topk(lg, 7, 1.0, out=out, philox=R.PHILOX_WORDS, top_p=0.9)
    torch.cuda.synchronize()
    assert (out == POISON).all()
    assert ops.sample_topk(lg, 7, 1.0, out=out, top_p=1.0).tolist() == [0, 0]


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("V,top_k,T,p", [(1000, None, 1.0, 0.9), (1000, 50, 0.7, 0.5), (257, None, 1.3, 0.999), (16384, 100, 1.0, 0.9), (5, None, 1.0, 0.5)])
def test_pick_inside_the_certain_nucleus_is_unchanged(ops, V, top_k, T, p):
    """Same noise: where the pick without top_p lies in the certain nucleus, the pick with top_p is that token -- the scores are the
    same bits (e / the top-k set's fp32 total / noise), the argmax is over a subset that holds the winner."""
    lg = N.case_logits(V, top_k)
    xs, mask = R.kept(lg, T, top_k)
    sure_in = N.nucleus(xs, mask, p)[0]
    ndev, _, _ = TP._noise(lg.shape[0], V)
    dev = lg.cuda()
    n_in = 0
    for kw in ({}, dict(noise=ndev), dict(philox=R.PHILOX_WORDS)):
        base = ops.sample_topk(dev, top_k, T, **kw).cpu().numpy()
        got = ops.sample_topk(dev, top_k, T, top_p=p, **kw).cpu().numpy()
        rows = sure_in[np.arange(len(base)), base]
        n_in += int(rows.sum())
        assert np.array_equal(got[rows], base[rows]), f"rows {np.nonzero(rows & (got != base))[0][:8].tolist()}"
    assert n_in >= lg.shape[0]


@pytest.mark.parametrize("p", N.TOP_PS)
def test_constant_rows_keep_everything(ops, p):
    V, B = 1000, 64
    lg = torch.full((B, V), -1.75, device="cuda")
    for top_k in (None, 7):
        base = ops.sample_topk(lg, top_k, 0.7, philox=R.PHILOX_WORDS)
        assert torch.equal(ops.sample_topk(lg, top_k, 0.7, philox=R.PHILOX_WORDS, top_p=p), base)
        assert len(set(base.tolist())) > B // 2
    assert ops.sample_topk(lg, None, 0.7, top_p=p).tolist() == [0] * B        # greedy: the lowest index among equals


def _two_level(V, n, B, seed=3):
    row = N.two_level_row(V, n, 0.0, torch.Generator().manual_seed(seed))
    return row.expand(B, V).contiguous(), (row == 0.0).numpy()


@pytest.mark.parametrize("V,n,top_k", [(1000, 300, None), (1000, 300, 999), (257, 100, None), (16384, 5000, None)])
def test_two_level_rows_never_pick_below_the_boundary(ops, V, n, top_k):
    """n entries at 0, the rest at -1; the high level holds n / (n + (V - n) / e) > 0.5 of the mass, so at p = 0.5 the boundary lies
    between the levels: G_high = 0, G_low = that mass, more than 0.03 above p (m_p is below 10^-5).  Under Philox noise no row picks a
    low entry; with top_p=None on the same noise many do -- the case discriminates.  This is the assertion that fails when the
    nucleus is computed but not applied."""
    B = 256
    lg, high = _two_level(V, n, B)
    mass = n / (n + (V - n) / np.e)
    xs, mask = R.kept(lg[:1], 1.0, top_k)
    sure_in, sure_out, unc = N.nucleus(xs, mask, 0.5)
    assert mass > 0.53 and np.array_equal(sure_in[0], high) and np.array_equal(sure_out[0], ~high) and not unc.any()
    dev = lg.cuda()
    got = ops.sample_topk(dev, top_k, 1.0, philox=R.PHILOX_WORDS, top_p=0.5).cpu().numpy()
    assert high[got].all(), f"rows {np.nonzero(~high[got])[0][:8].tolist()} picked a low entry"
    base = ops.sample_topk(dev, top_k, 1.0, philox=R.PHILOX_WORDS).cpu().numpy()
    assert (~high[base]).sum() > B // 4, "top_p=None never picks a low entry either: the case shows nothing"
    assert np.array_equal(got[high[base]], base[high[base]])
    assert len(set(got.tolist())) > 32
    # p above the high level's mass: the low level is in, whole -- the picks are those without top_p
    assert np.array_equal(ops.sample_topk(dev, top_k, 1.0, philox=R.PHILOX_WORDS, top_p=0.999).cpu().numpy(), base)


def _expf_is_half(ops, d):
    """Whether the pick's own expf(d) is exactly 0.5, read off the top-k kernel: entry a at 0 with noise 1 scores (1 / T) / 1, entry b
    at d with noise 0.5 scores (e_d / T) / 0.5 -- equal bits iff e_d == 0.5 (both divisions by 0.5 and 1 are exact), and among equal
    scores the lowest index wins: b in front of a wins iff e_d >= 0.5, b behind a wins iff e_d > 0.5."""
    lg = torch.full((2, 8), -80.0)
    noise = torch.ones(2, 8)
    lg[0, 5], lg[0, 2], noise[0, 2] = 0.0, d, 0.5               # b = 2 in front of a = 5
    lg[1, 2], lg[1, 5], noise[1, 5] = 0.0, d, 0.5               # b = 5 behind a = 2
    return ops.sample_topk(lg.cuda(), 2, 1.0, noise=noise.cuda()).tolist() == [2, 2]


def test_boundary_exactly_at_p_is_out(ops):
    """G < p, not G <= p.  An exactly representable boundary needs exact masses: entry 7 at 0 (e = 1) and a tie of two entries at d with
    expf(d) == 0.5 exactly, top_k = 3: T = 2, the tie's G = 1 / 2 = float32(0.5) in the kernel's integers too, so at p = 0.5 it is out
    and every row picks 7; one ulp above 0.5 it is in.  Whether this build's expf gives 0.5 for one of the three floats around -ln 2 is
    read off the top-k kernel first (`_expf_is_half`); where it does not, only the reference's verdict is asserted."""
    V, B = 64, 64
    ln2 = np.float32(-np.log(2.0))
    exact = [float(d) for d in (ln2, np.nextafter(ln2, np.float32(-1)), np.nextafter(ln2, np.float32(0))) if _expf_is_half(ops, float(d))]
    print(f"nucleus boundary at p: expf(d) == 0.5 exactly for d in {exact}")
    lg = torch.full((B, V), -30.0)
    lg[:, 7] = 0.0
    lg[:, 20] = lg[:, 41] = exact[0] if exact else float(ln2)
    xs, mask = R.kept(lg, 1.0, 3)
    got = ops.sample_topk(lg.cuda(), 3, 1.0, philox=R.PHILOX_WORDS, top_p=0.5)
    _judge("boundary at p", got, xs, mask, 0.5, R.philox_noise(B, V, R.PHILOX_WORDS), R.C_PHILOX, cap_rows=B * 64)
    if exact:
        assert (got == 7).all(), f"G == p was kept: {sorted(set(got.tolist()))}"
        above = float(np.nextafter(np.float32(0.5), np.float32(1)))
        assert set(ops.sample_topk(lg.cuda(), 3, 1.0, philox=R.PHILOX_WORDS, top_p=above).tolist()) == {7, 20, 41}


def test_boundary_tie_is_kept_whole(ops):
    """A tie group that straddles p is kept whole: 1 entry at 1.0 and 40 at 0.0 (the rest far below); p = 0.5 falls inside the group
    (G = e / (e + 40) = 0.064 < 0.5 for each of its members).  All 40 are drawn under Philox noise, and nothing below them."""
    V, B = 300, 1024
    row = torch.full((V,), -9.0)
    order = torch.randperm(V, generator=torch.Generator().manual_seed(11))
    row[order[0]] = 1.0
    row[order[1:41]] = 0.0
    lg = row.expand(B, V).contiguous().cuda()
    want = (row >= 0.0).numpy()
    seen = np.zeros(V, dtype=bool)
    for step in range(4):
        seen[ops.sample_topk(lg, None, 1.0, philox=(5, 6, 0, step, 1), top_p=0.5).cpu().numpy()] = True
    assert np.array_equal(seen, want), f"drawn outside the nucleus {np.nonzero(seen & ~want)[0][:8].tolist()}, never drawn {np.nonzero(want & ~seen)[0][:8].tolist()}"


def test_nucleus_is_taken_on_the_top_k_set(ops):
    """top_k = 4 of a row whose top 4 hold little of the whole mass: on the renormalised top-k set p = 0.6 keeps the two largest (masses
    0.4, 0.3, 0.2, 0.1 of the set); over all of V all four would have G < 0.6."""
    V, B = 2000, 512
    row = torch.zeros(V)                                           # 1996 entries of mass 1 each
    row[[3, 500, 901, 1777]] = torch.log(torch.tensor([4.0, 3.0, 2.0, 1.0])) + 1.0
    lg = row.expand(B, V).contiguous().cuda()
    xs, mask = R.kept(row[None], 1.0, 4)
    sure_in, _, unc = N.nucleus(xs, mask, 0.6)
    assert np.nonzero(sure_in[0])[0].tolist() == [3, 500] and not unc.any()
    got = set(ops.sample_topk(lg, 4, 1.0, philox=R.PHILOX_WORDS, top_p=0.6).tolist())
    assert got == {3, 500}, sorted(got)


def test_top_p_off_is_the_existing_entry_point(ops):
    from ccvs_amd import lib
    L = lib.load()
    V, top_k, T = 1000, 50, 0.7
    lg = N.case_logits(V, top_k)
    ndev, _, _ = TP._noise(lg.shape[0], V)
    view, out, out_buf = TP._strided(lg)
    for kw in ({}, dict(noise=ndev), dict(philox=R.PHILOX_WORDS)):
        base = ops.sample_topk(view, top_k, T, **kw).clone()
        for off in (None, 1.0, 1):
            out_buf.fill_(POISON)
            assert torch.equal(ops.sample_topk(view, top_k, T, out=out, top_p=off, **kw), base) and TP._gaps_poisoned(out_buf)
        assert not torch.equal(ops.sample_topk(view, top_k, T, top_p=0.1, **kw), base) or not kw
    # the new C entry points with top_p = 1: the top-k kernel, the same bits
    got = torch.full_like(base, POISON)
    lib.check(L.ccvs_sample_topp(ops._p(view), view.stride(0), ops._p(ndev), ops._p(got), 1, lg.shape[0], V, top_k, T, 1.0, ops._stream()), "ccvs_sample_topp")
    assert torch.equal(got, ops.sample_topk(view, top_k, T, noise=ndev))
    k0, k1, row0, step, call = R.PHILOX_WORDS
    lib.check(L.ccvs_sample_topp_philox(ops._p(view), view.stride(0), ops._p(got), 1, lg.shape[0], V, top_k, T, 1.0, k0, k1, row0, step, call, ops._stream()),
              "ccvs_sample_topp_philox")
    assert torch.equal(got, ops.sample_topk(view, top_k, T, philox=R.PHILOX_WORDS))


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("top_k", [None, 7])
def test_non_finite_rows_return_token_0(ops, top_k):
    V, T, p = 300, 0.9, 0.9
    lg, bad, fine = TP._bad_rows(V, torch.Generator().manual_seed(9))
    dev = lg.cuda()
    noise = R.case_noise(V, rows=10).cuda()
    k0, k1, row0, step, call = R.PHILOX_WORDS
    for name, kw in (("greedy", {}), ("host noise", dict(noise=noise)), ("philox", dict(philox=R.PHILOX_WORDS))):
        got = ops.sample_topk(dev, top_k, T, top_p=p, **kw).cpu()
        assert ((got >= 0) & (got < V)).all(), f"{name}: index outside [0, {V}): {got.tolist()}"
        assert (got[bad] == 0).all(), f"{name}: {got.tolist()}"
        for b in fine:
            alone = dict(kw)
            if "noise" in kw:
                alone["noise"] = noise[b:b + 1].contiguous()
            if "philox" in kw:
                alone["philox"] = (k0, k1, row0 + b, step, call)
            assert torch.equal(ops.sample_topk(dev[b:b + 1], top_k, T, top_p=p, **alone).cpu(), got[b:b + 1]), f"{name}: finite row {b} changed"
    xs, mask = R.kept(lg[fine], T, top_k)
    got = ops.sample_topk(dev, top_k, T, top_p=p, noise=noise).cpu()
    _judge(f"finite rows beside non-finite ones top_k={top_k}", got[fine], xs, mask, p, noise[fine].double().cpu().numpy(), R.C_HOST, cap_rows=64)


# ------------------------------------------------------------------ 5
T0, N_NEW, VOCAB, TOP_K, TOP_P = TP.T0, TP.N_NEW, TP.VOCAB, TP.TOP_K, 0.9


def _generate(net, codes, keys, offsets, call, form, top_p=TOP_P, top_k=TOP_K, drop=True):
    """TP._generate with top_p.  -> (tokens on the host, {widx, len, state} after the call, the descriptor's cache key)."""
    if drop:
        net.drop_engine_state()
    net.persistent_step = form == "persistent"
    if len(keys) > 1:
        net.noise_key, net.row_offset = list(keys), list(offsets)
    else:
        net.noise_key, net.row_offset = keys[0], offsets[0]
    net.noise_call = call
    try:
        out = net.generate(codes, N_NEW, sample=True, top_k=top_k, noise="device", use_graph=form != "eager", top_p=top_p)
        net.check_steps()
        torch.cuda.synchronize()
        c = net._cache
        after = {"widx": c["widx"].cpu(), "len": c["len_dev"].cpu(), "state": c["state"].cpu().view(-1, 8)}
        return out.cpu(), after, (c["desc"][0], tuple(c["graphs"]), c["desc"][1].desc.top_p)
    finally:
        net.noise_key, net.row_offset, net.persistent_step = None, 0, False


@pytest.mark.parametrize("form", ["graph", "eager", "persistent"])
@pytest.mark.parametrize("groups,call", [(1, 0), (3, 5)])
def test_decode_step_picks_against_the_reference(ops, groups, call, form):
    net = TP._gpt()
    B, per = 6, 6 // groups
    codes = torch.randint(0, VOCAB, (B, T0), generator=torch.Generator().manual_seed(1)).cuda()
    keys, offsets = TP.KEYS[:groups], TP.ROW_OFFSETS[:groups]
    tokens, after, key = _generate(net, codes, keys, offsets, call, form)
    assert key[2] == float(np.float32(TOP_P)) and (form == "eager" or key[1])
    assert torch.equal(tokens[:, :T0], codes.cpu()) and ((tokens >= 0) & (tokens < VOCAB)).all()
    again, _, _ = _generate(net, codes, keys, offsets, call, form)
    assert torch.equal(again, tokens), "two runs, other tokens"
    plain, _, _ = _generate(net, codes, keys, offsets, call, form, top_p=None)
    assert not torch.equal(plain, tokens), "top_p = 0.9 changes nothing on 72 picks of the top 20"
    logits = TP._teacher_forced_logits(net, tokens)
    for i in range(N_NEW):
        step = 0xffffffff if i == 0 else i - 1
        xs, mask = R.kept(logits[i], 1.0, TOP_K)
        noise = np.stack([R.exp1_noise(VOCAB, offsets[b // per] + b % per, step, call, *keys[b // per]) for b in range(B)])
        _judge(f"decode {form} groups={groups} call={call} token {i}", tokens[:, T0 + i], xs, mask, TOP_P, noise, R.C_PHILOX, cap_rows=B * N_NEW)
    assert after["widx"].tolist() == [T0 + N_NEW] * groups and after["len"].tolist() == [T0 + N_NEW - 1] * groups
    st = after["state"].to(torch.int64) & 0xffffffff
    for g in range(groups):
        assert st[g, [0, 2, 3, 4, 5, 6]].tolist() == [N_NEW - 1, 0, call, keys[g][0], keys[g][1], offsets[g]], (g, st[g].tolist())


def test_decode_step_tokens_do_not_depend_on_the_batch_slot_or_the_form(ops):
    net = TP._gpt()
    codes = torch.randint(0, VOCAB, (6, T0), generator=torch.Generator().manual_seed(1)).cuda()
    whole, _, _ = _generate(net, codes, TP.KEYS[:1], [32], 0, "graph")
    alone, _, _ = _generate(net, codes[2:4].contiguous(), TP.KEYS[:1], [34], 0, "graph")
    assert torch.equal(whole[2:4], alone), "one group: rows 2..3 alone draw other tokens"
    for form in ("eager", "persistent"):
        other, _, _ = _generate(net, codes, TP.KEYS[:1], [32], 0, form)
        assert torch.equal(whole, other), f"graph replay and the {form} step draw different tokens"
    stacked, _, _ = _generate(net, codes, TP.KEYS, TP.ROW_OFFSETS, 0, "graph")
    for g in range(3):
        alone, _, _ = _generate(net, codes[2 * g:2 * g + 2].contiguous(), TP.KEYS[g:g + 1], TP.ROW_OFFSETS[g:g + 1], 0, "eager")
        assert torch.equal(stacked[2 * g:2 * g + 2], alone), f"three groups: group {g} alone draws other tokens"


@pytest.mark.parametrize("form", ["graph", "persistent"])
def test_captured_step_is_not_replayed_for_another_top_p(ops, form):
    """Two-level logits whatever the input: ln_f's gain 0 and shift e_0 make the logits column 0 of the head -- 60 entries at 0, 140
    at -1 (the high level holds 0.538).  top_p = 0.5 draws high entries only; 0.9 on the SAME engine state (no drop between the calls)
    draws low ones too: its step was captured anew under another key.  Back at 0.5 the tokens are the first call's."""
    net = TP._gpt()
    row = N.two_level_row(VOCAB, 60, 0.0, torch.Generator().manual_seed(2))
    high = (row == 0.0).numpy()
    with torch.no_grad():
        net.ln_f.weight.zero_()
        net.ln_f.bias.zero_()
        net.ln_f.bias[0] = 1.0
        net.head.weight.zero_()
        net.head.weight[:, 0] = row.cuda()
    codes = torch.randint(0, VOCAB, (6, T0), generator=torch.Generator().manual_seed(1)).cuda()
    a, _, key_a = _generate(net, codes, TP.KEYS[:1], [32], 0, form, top_p=0.5, top_k=None)
    b, _, key_b = _generate(net, codes, TP.KEYS[:1], [32], 0, form, top_p=0.9, top_k=None, drop=False)
    c, _, key_c = _generate(net, codes, TP.KEYS[:1], [32], 0, form, top_p=0.5, top_k=None, drop=False)
    assert high[a[:, T0:].numpy()].all(), "top_p = 0.5 drew a low entry"
    assert (~high[b[:, T0:].numpy()]).sum() >= 10, "top_p = 0.9 replayed the step captured for 0.5"
    assert torch.equal(a, c)
    assert key_a[0] != key_b[0] and key_a[1] != key_b[1] and key_a[0] == key_c[0] and (key_a[2], key_b[2]) == (0.5, float(np.float32(0.9)))
    assert all(0.5 in k for k in key_a[1]) and all(0.9 in k for k in key_b[1])


# ------------------------------------------------------------------ 6
def test_transformer_generates_with_x_top_p():
    from tests.test_e2e_gpu import TINY_ARGV
    from ccvs_amd.tools.options import Options
    from ccvs_amd.models.skip_vid_generator.models.transformer_model import Transformer
    torch.manual_seed(3)
    argv = TINY_ARGV + ["--x_top_k", "10", "--x_sample", "--x_sample_noise", "device"]
    empty = torch.tensor([])
    code = torch.randint(0, 32, (2, 64), generator=torch.Generator().manual_seed(4)).cuda()
    outs = {}
    for name, extra in (("off", []), ("on", ["--x_top_p", "0.9"])):
        xopt = Options().parse(load_qvid_generator=True, load_transformer=True, argv=argv + extra)["transformer"]
        torch.manual_seed(3)
        tr = Transformer(xopt, is_train=False, is_main=True).eval()
        with torch.no_grad():
            for prm in tr.net_t.parameters():
                prm.add_(0.3 * torch.randn_like(prm))
        tr.net_t.noise_key, tr.net_t.row_offset, tr.net_t.noise_call = (11, 12), 0, 0
        out = tr.fill_code(code.clone(), empty.cuda(), empty.cuda(), None, empty, add_len=16)[0]
        torch.cuda.synchronize()
        assert out.shape == (2, 80) and torch.equal(out[:, :64], code) and ((out >= 0) & (out < 32)).all()
        assert tr.net_t._cache["desc"][1].desc.top_p == (float(np.float32(0.9)) if extra else 0.0)
        outs[name] = out.cpu()
    assert not torch.equal(outs["on"], outs["off"])
    xopt.beam_size = 3
    with pytest.raises(NotImplementedError, match="--x_top_p"):
        tr.fill_code(code.clone(), empty.cuda(), empty.cuda(), None, empty, add_len=4)
