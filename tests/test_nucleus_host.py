"""Not gpu: the host reference of nucleus sampling (tests/nucleus_ref.py) checked on its own, an fp32 emulation of the kernel over the
case table of tests/test_nucleus_gpu.py, and the layers around the kernel that need no GPU.

  1. `nucleus_ref.nucleus` against a sort-and-cumsum restatement of the `transformers` TopPLogitsWarper on inputs without ties;
  2. the emulation (`nucleus_ref.emulate_fp32`: fp32 expf, integer masses, the integer comparison) over `nucleus_ref.CASES`: its set
     holds every certain member and no certain non-member, and its picks -- greedy and with host noise -- pass `nucleus_ref.accept`;
  3. per case at most `pick_ref.MARGIN_ONLY_CAP` of the rows have an uncertain entry at all (the reference alone);
  4. the ABI: include/ccvs_hip_sampling.h declares what the library exports = `lib.SAMPLING_EXPORTS`, disjoint from every other list;
     51 / ABI 6 unmoved; `top_p` is the C descriptor's last field and `lib.GptDecode.top_p` sits at its offset; the cap the library
     reports is the reference's;
  5. refusals by name, before any launch (the calls run here without a GPU): `ops.sample_topk(top_p=...)` outside (0, 1], the C entry
     points, the cap, the decode step and the step program with a bad top_p;
  6. `--x_top_p` / `--x_top_p_state` parse, default None, and leave the reference's launch line as it parses."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nucleus_ref as N  # noqa: E402
import pick_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ 1
def _untied_logits(rows, V, seed):
    """randn * 2 rows of V DIFFERENT fp32 values each (the first V distinct ones of 2 V draws, in drawing order)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(rows):
        r = (torch.randn(2 * V + 8, generator=g) * 2).numpy()
        _, first = np.unique(r, return_index=True)
        out.append(r[np.sort(first)[:V]])
    return torch.from_numpy(np.stack(out))


@pytest.mark.parametrize("V,top_k,p", [(200, None, 0.9), (200, 50, 0.5), (1000, None, 0.999), (1000, 7, 0.1), (5, None, 0.5), (16384, 100, 0.9)])
def test_reference_is_the_transformers_rule(V, top_k, p):
    T = 1.0                                                            # xs = the logits themselves: no tie comes back through the division
    lg = _untied_logits(96, V, 31 * V + 7)
    xs, mask = R.kept(lg, T, top_k)
    assert all(len(np.unique(r)) == V for r in xs), "an input with ties"
    sure_in, sure_out, unc = N.nucleus(xs, mask, p)
    want = N.transformers_rule(xs, mask, p)
    rows = ~unc.any(axis=1)
    assert rows.mean() >= 0.75      # (p = 0.999 on 1000 entries: single entries at the boundary carry about 10^-5, the band is hit in a tenth of the rows)
    assert np.array_equal(sure_in[rows], want[rows]) and np.array_equal(sure_out[rows], ~want[rows])
    assert not (sure_in & ~want).any() and not (sure_out & want).any()       # rows with a band: outside it the two agree as well
    assert sure_in[np.arange(96), xs.argmax(1)].all(), "the most likely token is always kept"
    sizes = sure_in.sum(1)
    assert (sizes >= 1).all() and (sizes <= mask.sum(1)).all()
    if p >= 0.9 and top_k is None:
        assert sizes.max() > 1


def test_reference_ties_share_one_fate():
    """Quantised rows: entries of equal xs are all in, all out or all uncertain; a two-level row keeps the high level whole."""
    lg = N.case_logits(257, None)
    xs, mask = R.kept(lg, 1.0, None)
    for p in N.TOP_PS:
        sure_in, sure_out, unc = N.nucleus(xs, mask, p)
        for b in range(lg.shape[0]):
            for state in (sure_in[b], sure_out[b], unc[b]):
                vals = np.unique(xs[b][state])
                assert not np.isin(xs[b][~state], vals).any(), (p, b)
        assert sure_in[4].all() and sure_in[5].all(), "constant rows keep everything"
    # row 2: 85 entries at 0.5 (mass 85 e / (85 e + 172)), the rest at -0.5: p = 0.5 lies inside the high level
    sure_in, _, unc = N.nucleus(xs, mask, 0.5)
    assert np.array_equal(sure_in[2], xs[2] == 0.5) and not unc[2].any()


# ------------------------------------------------------------------ 2, 3
@pytest.mark.parametrize("V", N.VOCABS)
def test_emulated_kernel_passes_and_the_band_is_rare(V):
    cases = [c for c in N.CASES if c[0] == V]
    assert cases
    for _, top_k, T, p in cases:
        lg = N.case_logits(V, top_k)
        xs, mask = R.kept(lg, T, top_k)
        sure_in, sure_out, unc = N.nucleus(xs, mask, p)
        share = unc.any(axis=1).mean()
        print(f"nucleus V={V} top_k={top_k} T={T} p={p}: rows with an uncertain entry {int(unc.any(axis=1).sum())} of {len(xs)}, "
              f"median nucleus {int(np.median(sure_in.sum(1)))}")
        assert share <= R.MARGIN_ONLY_CAP, f"V={V} top_k={top_k} p={p}: {share:.3f} of the rows have an uncertain entry"
        n32 = R.case_noise(V, rows=lg.shape[0])
        for name, noise32, noise64 in (("greedy", None, None), ("host noise", n32, n32.double().numpy())):
            pick, keep = N.emulate_fp32(xs, mask, p, noise32)
            assert not (sure_in & ~keep).any() and not (sure_out & keep).any(), f"V={V} top_k={top_k} p={p}: the emulated set leaves the band"
            ok = N.accept(pick, xs, mask, p, noise64, R.C_HOST)
            assert ok.all(), f"V={V} top_k={top_k} T={T} p={p} {name}: rows {np.nonzero(~ok)[0][:8].tolist()}"


def test_case_table_covers_what_it_should():
    assert N.VOCABS == (1, 5, 255, 256, 257, 1000, 16384, N.V_TOPP_MAX) and N.V_TOPP_MAX == 40164 < R.V_PICK_MAX
    assert {c[3] for c in N.CASES} == set(N.TOP_PS)
    for V in N.VOCABS:
        ks = {c[1] for c in N.CASES if c[0] == V}
        assert ks == ({None, 7, V - 1} if V > 1 else {None, 7})
    lg = N.case_logits(1000, 7)
    assert all(sorted(set(lg[r].tolist())) == [-0.5, 0.5] for r in range(3)) and len(set(lg[4].tolist())) == 1 == len(set(lg[5].tolist()))


# ------------------------------------------------------------------ 4
def test_sampling_symbols_declared_and_exported(tmp_path):
    from ccvs_amd import lib
    header = open(os.path.join(ROOT, "include", "ccvs_hip_sampling.h")).read()
    main = open(os.path.join(ROOT, "include", "ccvs_hip.h")).read()
    assert re.search(r'^#include "ccvs_hip_sampling.h"', main, re.M) and not re.search(r"ccvs_sample_topp", main)
    declared = sorted(set(re.findall(r"^\w[\w \*]*?\b(ccvs_\w+)\(", header, re.M)))
    assert declared == sorted(lib.SAMPLING_EXPORTS) == ["ccvs_sample_topp", "ccvs_sample_topp_max_vocab", "ccvs_sample_topp_philox"]
    others = [getattr(lib, n) for n in dir(lib) if n.endswith("EXPORTS") and n != "SAMPLING_EXPORTS"]
    assert len(others) == 14 and not any(set(lib.SAMPLING_EXPORTS) & set(o) for o in others) and len(lib.EXPORTS) == 51
    handle = ctypes.CDLL(lib.LIB_PATH)
    for sym in lib.SAMPLING_EXPORTS:
        assert hasattr(handle, sym), sym
    assert lib.load().ccvs_abi_version() == 6
    assert open(os.path.join(ROOT, "ccvs_amd", "csrc", "Makefile")).read().count("ccvs_hip_sampling.h") == 1
    # the descriptor: top_p is the C struct's last field, the mirror's property sits on it, and the sizes agree
    c = tmp_path / "p.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ccvs_hip.h"\nvoid* p[] = {' + ", ".join("(void*)" + s for s in lib.SAMPLING_EXPORTS)
                 + '};\nint main(){ccvs_gpt_decode d; printf("%zu %zu %zu %zu", sizeof(d), offsetof(ccvs_gpt_decode, top_p), sizeof(d.top_p), '
                 'offsetof(ccvs_gpt_decode, w_tiled)); return 0;}\n')
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "p.o")], check=True)
    exe = tmp_path / "q"
    (tmp_path / "q.c").write_text(c.read_text().replace("void* p[] = {" + ", ".join("(void*)" + s for s in lib.SAMPLING_EXPORTS) + "};\n", ""))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "q.c"), "-o", str(exe)], check=True)
    size, off, width, off_tiled = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert (size, off, width) == (ctypes.sizeof(lib.GptDecode), lib.GptDecode.TOP_P_OFFSET, 4) and off + width == size and off > off_tiled
    struct = main[main.index("typedef struct ccvs_gpt_decode"):main.index("} ccvs_gpt_decode;")]
    assert re.findall(r"^\s*(?:const\s+)?\w+\**\s+\**(\w+);", struct, re.M)[-1] == "top_p"
    d = lib.GptDecode()
    assert d.top_p == 0.0
    d.top_p = 0.9
    assert d.top_p == float(np.float32(0.9)) and d.w_tiled == 0
    assert bytes(d)[off:off + 4] == np.float32(0.9).tobytes()
    from ccvs_amd import ops
    assert ops.sample_topp_max_vocab() == N.V_TOPP_MAX


# ------------------------------------------------------------------ 5
def test_refusals_by_name_before_any_launch():
    from ccvs_amd import lib, ops
    L = lib.load()
    lg = torch.zeros(2, 40)
    for bad in (0.0, -0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="top_p"):
            ops.sample_topk(lg, 7, 1.0, top_p=bad)            # before the tensors are looked at: no GPU needed
        with pytest.raises(ValueError, match="top_p"):
            ops.check_top_p(bad)
    assert ops.check_top_p(None) is None and ops.check_top_p(1.0) is None and ops.check_top_p(1) is None and ops.check_top_p(0.25) == 0.25
    with pytest.raises(TypeError):
        ops.sample_topk(lg, 7, 1.0, None, None, None, 0.9)    # keyword-only
    # the C entry points refuse in front of their launch: the pointers below are never read
    fake = ctypes.c_void_p(64)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(lib.CcvsError, match="ccvs_sample_topp: top_p"):
            lib.check(L.ccvs_sample_topp(fake, 40, None, fake, 1, 2, 40, 7, 1.0, bad, None), "ccvs_sample_topp")
        with pytest.raises(lib.CcvsError, match="ccvs_sample_topp_philox: top_p"):
            lib.check(L.ccvs_sample_topp_philox(fake, 40, fake, 1, 2, 40, 7, 1.0, bad, 1, 2, 3, 4, 5, None), "ccvs_sample_topp_philox")
    with pytest.raises(lib.CcvsError, match="ccvs_sample_topp: null pointer"):
        lib.check(L.ccvs_sample_topp(fake, 40, None, None, 1, 2, 40, 7, 1.0, 0.9, None), "ccvs_sample_topp")
    with pytest.raises(lib.CcvsError, match="ccvs_sample_topp: bad arguments"):
        lib.check(L.ccvs_sample_topp(fake, 40, None, fake, 1, 2, 40, 7, 0.0, 0.9, None), "ccvs_sample_topp")
    V = N.V_TOPP_MAX + 1
    with pytest.raises(lib.CcvsError, match=f"ccvs_sample_topp: vocabulary {V} too large for the top_p form \\(at most {N.V_TOPP_MAX}\\)"):
        lib.check(L.ccvs_sample_topp(fake, V, None, fake, 1, 2, V, 7, 1.0, 0.9, None), "ccvs_sample_topp")
    with pytest.raises(lib.CcvsError, match=f"ccvs_sample_topp_philox: vocabulary {V} too large for the top_p form"):
        lib.check(L.ccvs_sample_topp_philox(fake, V, fake, 1, 2, V, 7, 1.0, 0.9, 1, 2, 3, 4, 5, None), "ccvs_sample_topp_philox")
    # the decode step: a descriptor whose pointers are never read
    layers = (lib.GptLayer * 1)()
    d = lib.GptDecode()
    d.B, d.C, d.H, d.F, d.n_layer, d.Tmax, d.vocab, d.V = 2, 32, 2, 128, 1, 16, 40, 40
    d.layers = layers
    for name, ctype in lib.GptDecode._fields_:
        if ctype is ctypes.c_void_p and name not in ("noise", "noise_stream", "program"):
            setattr(d, name, 64)
    d.temperature, d.groups = 1.0, 1
    for bad in (-0.5, 1.5, float("nan")):
        d.top_p = bad
        with pytest.raises(lib.CcvsError, match="ccvs_gpt_decode_step: top_p"):
            lib.check(L.ccvs_gpt_decode_step(ctypes.byref(d), None), "ccvs_gpt_decode_step")
    d.persistent, d.program = 1, 64
    for bad in (-0.5, 1.5, float("nan")):
        d.top_p = bad
        with pytest.raises(lib.CcvsError, match="ccvs_gpt_decode_prepare: top_p"):
            lib.check(L.ccvs_gpt_decode_prepare(ctypes.byref(d), None), "ccvs_gpt_decode_prepare")
    d.top_p, d.persistent, d.V = 0.9, 0, N.V_TOPP_MAX + 1
    with pytest.raises(lib.CcvsError, match=f"ccvs_gpt_decode_step: vocabulary {N.V_TOPP_MAX + 1} too large for the top_p form"):
        lib.check(L.ccvs_gpt_decode_step(ctypes.byref(d), None), "ccvs_gpt_decode_step")


# ------------------------------------------------------------------ 6
def test_options_parse():
    from ccvs_amd.tools.options import Options, BAIR_ARGV
    base = Options().parse(True, True, argv=BAIR_ARGV)
    assert base["transformer"].top_p is None and base["transformer"].top_p_state is None
    opt = Options().parse(True, True, argv=BAIR_ARGV + ["--x_top_p", "0.9", "--x_top_p_state", "0.5"])
    assert opt["transformer"].top_p == 0.9 and opt["transformer"].top_p_state == 0.5 and opt["transformer"].top_k == base["transformer"].top_k
    a, b = vars(base["transformer"]), vars(opt["transformer"])
    assert {k for k in a if a[k] != b[k]} == {"top_p", "top_p_state"}
    assert vars(base["qvid_generator"]) == vars(opt["qvid_generator"])
