"""CPU: the reference of the bf16 KV-cache mode (tests/kv_bf16_ref.py) and the host side of `--x_kv_dtype`.

  1. the integer round-to-nearest-even equals `torch.Tensor.to(torch.bfloat16)` bit for bit: ties both ways, denormals, +-0, +-inf, the
     largest finite fp32 (rounds to inf), 2^20 random bit patterns; NaN stays NaN; truncation (the wrong rounding) differs.
  2. the op-level cost of the mode, in float64 on the inputs the GPU tests use, is inside the stated bound; the figures are printed.
  3. `lib.KV16_SYMBOLS` is what include/ccvs_hip_kv16.h declares, the header compiles as C, the library exports the symbols, and the
     new step entry refuses `persistent = 1` with the reason, before any launch.
  4. `--x_kv_dtype` parses (default fp32), a bad value is rejected, nothing else of the launch line moves.
  5. the KV bytes per batch that the Generator logs: the BAIR arithmetic of DESIGN.md 4.28 (192 MiB per sequence row in fp32)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_ref as R  # noqa: E402
import kv_bf16_ref as K  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32(bits):
    return torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32) if max(bits) < 2 ** 31 else \
        torch.tensor([b - 2 ** 32 if b >= 2 ** 31 else b for b in bits], dtype=torch.int64).to(torch.int32).view(torch.float32)


# ------------------------------------------------------------------ 1
def test_rounding_equals_torch():
    special = [
        0x00000000, 0x80000000,                          # +-0
        0x7f800000, 0xff800000,                          # +-inf
        0x7f7fffff, 0xff7fffff,                          # the largest finite fp32: rounds to inf
        0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000,  # ties: down to the even 0x3f80, up to the even 0x3f82
        0x3f807fff, 0x3f808001,                          # just below / above a tie
        0x00000001, 0x00007fff, 0x00008000, 0x00008001, 0x00018000, 0x007fffff, 0x80008000,   # denormals (a tie among them)
        0x00800000, 0x7f7f7fff, 0x7f7f8000,              # the smallest normal; the last bf16 below inf; the tie above it (to inf)
    ]
    x = f32(special)
    got, want = K.bf16_bits(x), K.bits_of(x.to(torch.bfloat16))
    assert torch.equal(got, want), [(hex(s), hex(g), hex(w)) for s, g, w in zip(special, got.tolist(), want.tolist()) if g != w]
    assert got[:6].tolist() == [0x0000, 0x8000, 0x7f80, 0xff80, 0x7f80, 0xff80]
    assert got[6:10].tolist() == [0x3f80, 0x3f82, 0xbf80, 0xbf82]
    g = torch.Generator().manual_seed(11)
    rnd = torch.randint(0, 2 ** 32, (1 << 20,), generator=g, dtype=torch.int64)
    rnd = torch.where(rnd >= 2 ** 31, rnd - 2 ** 32, rnd).to(torch.int32).view(torch.float32)
    finite = ~torch.isnan(rnd)
    assert torch.equal(K.bf16_bits(rnd)[finite], K.bits_of(rnd.to(torch.bfloat16))[finite])
    # NaN stays NaN, whatever its payload (torch's own cast may keep payload bits; the mode stores the canonical 0x7fc0)
    nans = f32([0x7fc00000, 0x7f800001, 0xffc00001, 0x7fffffff])
    assert torch.isnan(K.bf16_round(nans)).all() and torch.isnan(nans.to(torch.bfloat16).float()).all()
    assert torch.equal(K.bf16_round(rnd[finite]), rnd[finite].to(torch.bfloat16).float())
    # the wrong rounding is told apart: about half of all values round up
    assert (K.truncate(rnd[finite]) != K.bf16_round(rnd[finite])).float().mean().item() > 0.4


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("d", (16, 32, 64))
def test_mode_cost_is_inside_its_bound(d):
    worst = 0.0
    for pattern in R.PATTERNS:
        for tq, pos0 in ((129, 127), (1, 8192 // d)):
            q, k, v = R.make_inputs(pattern, 2, 3, tq, pos0 + tq, d, seed=200 + d)
            err, bound = K.mode_cost(q, k, v, pos0)
            ratio = (err / bound).max().item()
            print(f"D={d} {pattern} Tq={tq}: max |exact - stored| = {err.max().item():.3e}, largest err / bound = {ratio:.4f}")
            worst = max(worst, ratio)
            # and the kernels' own bound is far smaller than what the mode costs: the two do not blur into each other
            _, tol = K.attention_rounded_ref(q, k, v, pos0)
            assert tol.max().item() < bound.min().item()
    assert worst <= 1.0, worst


# ------------------------------------------------------------------ 3
def test_kv16_symbols_declared_and_exported(tmp_path):
    from ccvs_amd import lib
    header = open(os.path.join(ROOT, "include", "ccvs_hip_kv16.h")).read()
    assert re.search(r'^#include "ccvs_hip_kv16.h"', open(os.path.join(ROOT, "include", "ccvs_hip.h")).read(), re.M)
    declared = sorted(set(re.findall(r"^\w[\w \*]*?\b(ccvs_\w+)\(", header, re.M)))
    assert declared == sorted(lib.KV16_SYMBOLS) == ["ccvs_attention_bf16", "ccvs_gpt_decode_step_bf16kv", "ccvs_kv_append_bf16"]
    others = [getattr(lib, n) for n in dir(lib) if n.endswith("EXPORTS") or (n.endswith("SYMBOLS") and n != "KV16_SYMBOLS")]
    assert not any(set(lib.KV16_SYMBOLS) & set(o) for o in others)
    handle = ctypes.CDLL(lib.LIB_PATH)
    for sym in lib.KV16_SYMBOLS:
        assert hasattr(handle, sym), sym
    c = tmp_path / "p.c"
    c.write_text('#include "ccvs_hip.h"\nvoid* p[] = {' + ", ".join("(void*)" + s for s in lib.KV16_SYMBOLS) + "};\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "p.o")], check=True)
    L = lib.load()
    assert L.ccvs_abi_version() == 6
    for sym in lib.KV16_SYMBOLS:
        assert getattr(L, sym).argtypes is not None and getattr(L, sym).restype is ctypes.c_int


def test_step_entry_refuses_the_persistent_form_before_any_launch():
    """A descriptor of plausible (never dereferenced) addresses: the refusal comes from the argument checks."""
    from ccvs_amd import lib
    L = lib.load()
    layer = lib.GptLayer(*([64] * 12))
    d = lib.GptDecode()
    d.B, d.C, d.H, d.F, d.n_layer, d.Tmax, d.vocab, d.V, d.ln_eps = 2, 32, 2, 128, 1, 64, 32, 32, 1e-5
    d.layers = ctypes.pointer(layer)
    for name in ("tok_emb", "pos_table", "head_w", "head_b", "head_s", "tok", "codes", "widx", "len", "x", "q", "att", "h", "logits", "state",
                 "workspace", "program"):
        setattr(d, name, 64)
    d.temperature, d.persistent = 1.0, 1
    with pytest.raises(lib.CcvsError, match="ccvs_gpt_decode_step_bf16kv: persistent = 1 is refused.*fp32 KV caches only"):
        lib.check(L.ccvs_gpt_decode_step_bf16kv(ctypes.byref(d), None), "ccvs_gpt_decode_step_bf16kv")
    # every other refusal of the chain names the entry the caller came through
    d.persistent, d.top_p = 0, 1.5
    with pytest.raises(lib.CcvsError, match="ccvs_gpt_decode_step_bf16kv: top_p"):
        lib.check(L.ccvs_gpt_decode_step_bf16kv(ctypes.byref(d), None), "ccvs_gpt_decode_step_bf16kv")
    with pytest.raises(lib.CcvsError, match="ccvs_gpt_decode_step: top_p"):
        lib.check(L.ccvs_gpt_decode_step(ctypes.byref(d), None), "ccvs_gpt_decode_step")
    # (and the argument checks of the attention entry: the appending form is the decode form; one new row needs the other)
    vp = ctypes.c_void_p
    with pytest.raises(lib.CcvsError, match="appending form is the decode form"):
        lib.check(L.ccvs_attention_bf16(vp(64), 96, 96, vp(64), vp(64), 96, vp(64), vp(64), vp(64), 1, 2, 2, 0, None, 0, 8, 16, None), "a")
    with pytest.raises(lib.CcvsError, match="row groups"):
        lib.check(L.ccvs_attention_bf16(vp(64), 96, 96, None, None, 96, vp(64), vp(64), vp(64), 3, 2, 1, 0, vp(64), 2, 8, 16, None), "a")
    with pytest.raises(lib.CcvsError, match="one new row without the other"):
        lib.check(L.ccvs_attention_bf16(vp(64), 96, 96, vp(64), None, 96, vp(64), vp(64), vp(64), 1, 2, 1, 0, None, 0, 8, 16, None), "a")
    with pytest.raises(lib.CcvsError, match="ccvs_kv_append_bf16: k, v and the caches must be 16-byte aligned"):   # the rows are read 16 bytes at a time
        lib.check(L.ccvs_kv_append_bf16(vp(68), vp(64), 96, 96, vp(64), vp(64), 1, 2, 2, 0, None, 8, 16, None), "a")
    with pytest.raises(lib.CcvsError, match="positions 7..9 exceed cache 8"):
        lib.check(L.ccvs_kv_append_bf16(vp(64), vp(64), 96, 96, vp(64), vp(64), 1, 2, 2, 7, None, 8, 16, None), "a")


# ------------------------------------------------------------------ 4
def test_option_parses_and_rejects():
    from ccvs_amd.tools.options import Options, BAIR_ARGV
    base = Options().parse(True, True, argv=BAIR_ARGV)
    assert base["transformer"].kv_dtype == "fp32"
    opt = Options().parse(True, True, argv=BAIR_ARGV + ["--x_kv_dtype", "bf16"])
    assert opt["transformer"].kv_dtype == "bf16"
    a, b = vars(base["transformer"]), vars(opt["transformer"])
    assert {k for k in a if a[k] != b[k]} == {"kv_dtype"}
    assert vars(base["qvid_generator"]) == vars(opt["qvid_generator"])
    with pytest.raises(SystemExit):
        Options().parse(True, True, argv=BAIR_ARGV + ["--x_kv_dtype", "fp16"])
    src = open(os.path.join(ROOT, "ccvs_amd", "tools", "options.py")).read()
    assert re.search(r'"--x_kv_dtype".*?help="\(ccvs_amd\)', src, re.S)
    from ccvs_amd import ops
    assert ops.check_kv_dtype("bf16") is torch.bfloat16 and ops.check_kv_dtype("fp32") is torch.float32
    assert ops.check_kv_dtype(torch.bfloat16) is torch.bfloat16
    for bad in ("fp16", None, torch.float16, 16):
        with pytest.raises(ValueError, match="kv_dtype"):
            ops.check_kv_dtype(bad)


# ------------------------------------------------------------------ 5
def test_kv_cache_bytes_is_the_shape_arithmetic():
    from ccvs_amd.models.skip_vid_generator.models import mingpt
    net = mingpt.GPT(vocab_size=8, block_size=1024, num_blocks=16, n_layer=24, n_head=16, n_embd=1024, emb_mode="temporal", shape=(8, 8))
    assert net.kv_dtype == "fp32"
    assert net.kv_cache_bytes(1, 1024) == 24 * 16 * 1024 * 64 * 2 * 4 == 192 * 2 ** 20
    assert net.kv_cache_bytes(16, 1024) == 3 * 2 ** 30
    net.kv_dtype = "bf16"
    assert net.kv_cache_bytes(16, 1024) == 3 * 2 ** 29
    net.kv_dtype = "fp16"
    with pytest.raises(ValueError, match="kv_dtype"):
        net.kv_cache_bytes(1, 1)
