"""not gpu: the C-ABI library loads and exports every symbol include/ccvs_hip.h declares
(no compute calls), the ctypes mirror of ccvs_conv_desc matches the C struct, the product
refuses to run without a GPU instead of falling back, and the host-side logic (flags, Namespace
split, sharding, state-dict layout, initialiser parity with the reference) is right."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    from ccvs_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.dirname(lib.LIB_PATH), "-j4"], check=True)
    return lib


def header_symbols():
    src = open(os.path.join(ROOT, "include", "ccvs_hip.h")).read()
    return sorted(set(re.findall(r"\b(ccvs_[a-zA-Z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol(built_lib):
    handle = ctypes.CDLL(built_lib.LIB_PATH)
    declared = header_symbols()
    assert len(declared) >= 18
    for sym in declared:
        assert hasattr(handle, sym), f"{sym} declared in include/ccvs_hip.h but not exported"
    assert sorted(built_lib.EXPORTS) == declared, "ccvs_amd/lib.py EXPORTS out of sync with the header"
    built_lib.load()
    handle.ccvs_abi_version.restype = ctypes.c_int
    assert handle.ccvs_abi_version() == 6


def test_conv_last_launch_is_declared_exported_and_empty_without_a_launch(built_lib):
    """`ccvs_conv_last_launch` (include/ccvs_hip.h): additive to ABI 6, host code -- callable with no GPU, "" on a thread that has launched
    no convolution; a refused call (CPU tensors never reach the library, a bad descriptor does) leaves it alone."""
    import threading
    from ccvs_amd import ops
    assert "ccvs_conv_last_launch" in header_symbols() and "ccvs_conv_last_launch" in built_lib.EXPORTS and len(built_lib.EXPORTS) == 51
    L = built_lib.load()
    seen = []
    t = threading.Thread(target=lambda: seen.append(ops.conv_last_launch()))   # a fresh thread: its own (empty) record
    t.start()
    t.join()
    assert seen == [""]
    before = ops.conv_last_launch()
    d = built_lib.ConvDesc()
    d.N = d.Cin = d.Cout = d.Hin = d.Win = 1
    d.kh, d.kw, d.CoutPad = 2, 3, 32   # unsupported kernel shape: refused before any GPU call
    one = ctypes.c_void_p(16)
    for fn in (L.ccvs_conv2d, L.ccvs_conv2d_bf16x3):
        assert fn(one, one, None, None, one, ctypes.byref(d), None) != 0
    assert ops.conv_last_launch() == before
    assert L.ccvs_abi_version() == 6


def test_conv_desc_layout_matches_c(built_lib, tmp_path):
    fields = [f[0] for f in built_lib.ConvDesc._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "ccvs_hip.h"\nint main(){printf("%zu", sizeof(ccvs_conv_desc));\n'
    prog += "".join(f'printf(" %zu", offsetof(ccvs_conv_desc, {f}));\n' for f in fields) + "return 0;}\n"
    c = tmp_path / "d.c"
    c.write_text(prog)
    exe = tmp_path / "d"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(built_lib.ConvDesc)
    assert out[1:] == [getattr(built_lib.ConvDesc, f).offset for f in fields]


def test_gpt_decode_layout_matches_c(built_lib, tmp_path):
    """The ctypes mirrors of ccvs_gpt_decode (incl. the row-group field) and ccvs_gpt_layer match the C structs."""
    progs = []
    for cname, cls in (("ccvs_gpt_decode", built_lib.GptDecode), ("ccvs_gpt_layer", built_lib.GptLayer), ("ccvs_ctx_list", built_lib.CtxList)):
        fields = [f[0] for f in cls._fields_]
        prog = f'printf("%zu", sizeof({cname}));\n' + "".join(f'printf(" %zu", offsetof({cname}, {f}));\n' for f in fields) + 'printf("\\n");\n'
        progs.append((cls, fields, prog))
    c = tmp_path / "g.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ccvs_hip.h"\nint main(){' + "".join(p for _, _, p in progs) + "return 0;}\n")
    exe = tmp_path / "g"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    for (cls, fields, _), line in zip(progs, lines):
        out = [int(v) for v in line.split()]
        assert out[0] == ctypes.sizeof(cls), cls
        assert out[1:] == [getattr(cls, f).offset for f in fields], cls


def test_no_cpu_fallback(built_lib):
    from ccvs_amd import ops
    with pytest.raises(built_lib.CcvsError):
        ops.upfirdn2d(torch.zeros(1, 1, 8, 8), pad=(2, 2))
    with pytest.raises(built_lib.CcvsError):
        ops.vq_argmin(torch.zeros(1, 4, 2, 2), torch.zeros(4, 32), torch.zeros(32))
    if not torch.cuda.is_available():
        from ccvs_amd.tools.utils import to_cuda
        with pytest.raises(RuntimeError):
            to_cuda({"vid": torch.zeros(1)}, "vid")


def test_product_never_imports_the_oracle():
    for base, _, files in os.walk(os.path.join(ROOT, "ccvs_amd")):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(base, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", text, re.M), f"{f} imports the oracle"


def test_options_match_reference_flags():
    from ccvs_amd.tools.options import Options, BAIR_ARGV, KINETICS_ARGV
    # the reference's own launch line (scripts/bairhd/save_videos_p2p.sh) parses, training-only flags ignored
    script = ("--name save_videos_p2p_bairhd --vid_len 16 --vid_skip 16 --x_cond_len 64 --batch_size_vid 2 --batch_size_valid_mult 1 "
              "--num_workers 4 --n_iter 640 --x_sample --x_top_k 100 --x_temperature 1.0 --shuffle_valid "
              "--q_skip_context 1 2 3 4 5 6 7 8 9 10 11 12 13 14 15 --q_skip_memory 15 --dataset bairhd --max_dim 256 --is_seq --log_fps 1 "
              "--gpu_ids 0 --q_z_num 1024 --q_z_size 512 --q_z_shape 8 8 --q_lr 0.002 --q_beta1 0.0 --q_beta2 0.99 --q_gan_loss logistic "
              "--q_use_enc --q_use_dec --q_use_di --q_use_vgg_img --q_use_gan_feat_img --q_use_direct_recovery_img "
              "--q_necf 128 --q_necf_mult 1 1 2 2 4 4 --q_ndcf_mult 1 1 2 2 4 4 --q_ndcf 64 --q_enc_model skipgan --q_dec_model skipgan "
              "--q_use_inter --q_inter_p 0.75 --q_use_ema --x_z_num 1024 --x_z_len 1024 --x_n_layer 24 --x_n_head 16 --x_n_embd 1024 "
              "--x_lr 0.00001 --x_z_chunk 64 --x_p2p --p2p_len 16 --x_emb_mode temporal").split()
    o = Options()
    opt = o.parse(load_qvid_generator=True, load_transformer=True, argv=script)
    q, x = opt["qvid_generator"], opt["transformer"]
    assert "--q_lr" in o.ignored and "--q_use_di" in o.ignored
    assert q.necf_mult == [1, 1, 2, 2, 4, 4] and q.z_shape == [8, 8] and q.skip_memory == 15 and q.use_ema and q.inter_p == 0.75
    assert x.p2p and x.sample and x.top_k == 100 and x.z_len == 1024 and x.z_shape == [8, 8] and x.state_size == 0
    assert q.aspect_ratio == 1 and x.fps == 4 and q.max_dim == 256 and x.vid_len == 16   # bairhd preset + base copied into each
    assert opt["state_estimator"] is None
    b = Options().parse(True, True, argv=BAIR_ARGV)["transformer"]
    k = Options().parse(True, True, argv=KINETICS_ARGV)["qvid_generator"]
    assert b.cond_len == 64 and k.z_num == 16384 and k.necf == 256 and k.imagenet_norm


def test_engine_shard_and_single_process_gather():
    from ccvs_amd.tools.engine import Engine
    e = Engine(backend="gloo")
    assert e.shard_batch(16) == (0, 16) and e.is_main and not e.distributed
    t = torch.arange(6).view(2, 3)
    assert e.all_gather_clips(t) is t
    assert e.all_reduce_max(1.5) == 1.5


TINY_ARGV = ["--name", "tiny", "--dataset", "bairhd", "--max_dim", "32", "--vid_len", "4", "--q_z_num", "32", "--q_z_size", "16",
             "--q_z_shape", "8", "8", "--q_use_enc", "--q_use_dec", "--q_necf", "8", "--q_necf_mult", "1", "2", "2",
             "--q_enc_model", "skipgan", "--q_dec_model", "skipgan", "--q_use_inter", "--q_inter_p", "0.75",
             "--q_skip_context", "1", "2", "3", "--q_skip_memory", "3", "--x_z_num", "32", "--x_z_len", "256", "--x_n_layer", "2",
             "--x_n_head", "2", "--x_n_embd", "32", "--x_z_chunk", "64", "--x_cond_len", "64", "--x_emb_mode", "temporal",
             "--x_num_blocks", "4", "--batch_size_vid", "2"]


def test_state_dict_layout_and_initialiser_parity(golden_dir):
    """Built in the reference's order under the same seed, the MI355X modules carry the reference's
    parameter names AND values (golden weights came from the reference under torch.manual_seed(0))."""
    from ccvs_amd.tools.options import Options
    from ccvs_amd.models.skip_vid_generator.models import skip_autoencoder as sae, mingpt
    from ccvs_amd.models.skip_vid_generator.modules.quantize import VectorQuantizer
    gold = np.load(os.path.join(golden_dir, "tiny_e2e.npz"))
    opt = Options().parse(True, True, argv=TINY_ARGV)
    q, x = opt["qvid_generator"], opt["transformer"]
    torch.manual_seed(0)
    net_e = sae.SkipGANEncoder(q)
    net_q = VectorQuantizer(q.z_num, q.z_size, beta=0.25)
    net_g = sae.SkipGANDecoder(q)
    net_t = mingpt.GPT(vocab_size=x.z_num, block_size=x.z_len, n_layer=x.n_layer, n_head=x.n_head, n_embd=x.n_embd, emb_mode=x.emb_mode,
                       shape=x.z_shape, num_blocks=x.num_blocks)
    overridden = {"q/embedding.weight", "t/s_emb", "t/t_emb"}  # replaced after construction by make_golden.py
    for pre, net in (("e", net_e), ("q", net_q), ("g", net_g), ("t", net_t)):
        ref = {k[len(pre) + 1:]: gold[k] for k in gold.files if k.startswith(pre + "/")}
        own = {k: v for k, v in net.state_dict().items() if not k.endswith(".kernel")}
        assert set(own) == set(ref), set(own) ^ set(ref)
        for k, v in own.items():
            assert tuple(v.shape) == ref[k].shape, k
            if f"{pre}/{k}" not in overridden:
                assert np.array_equal(v.numpy(), ref[k]), f"{pre}/{k}: initialiser stream differs from the reference"


def test_synthetic_batch_independent_of_sharding():
    from ccvs_amd.tools.options import Options
    from ccvs_amd.helpers.generator import Generator
    gen = Generator(Options().parse(True, True, argv=TINY_ARGV))
    full = gen.synthetic_batch(4, seed=3)["vid"]
    lo, hi = gen.synthetic_batch(2, seed=3, first_clip=0)["vid"], gen.synthetic_batch(2, seed=3, first_clip=2)["vid"]
    assert full.shape == (4, 4, 3, 32, 32) and torch.equal(full, torch.cat([lo, hi]))
    assert full.min() >= -1 and full.max() <= 1
    with pytest.raises(NotImplementedError):
        o = Options().parse(True, True, argv=TINY_ARGV + ["--layout"])   # layouts stay outside the path and say so
        Generator(o)


def test_pos_emb_matches_oracle(golden_dir):
    from ccvs_amd.models.skip_vid_generator.models import mingpt
    from oracle import ccvs_oracle as O
    torch.manual_seed(0)
    for mode in ("temporal", "spatio-temporal", None):
        net = mingpt.GPT(vocab_size=20, block_size=48, num_blocks=3, n_layer=1, n_head=2, n_embd=32, emb_mode=mode, shape=[4, 4])
        with torch.no_grad():
            for n, p in net.named_parameters():
                if n.endswith("_emb"):
                    p.normal_(0, 1)
        cfg = O.namespace(z_shape=[4, 4], emb_mode=mode)
        sd = net.state_dict()
        for t, dl in [(48, None), (21, torch.tensor([1, 0, 1])), (16, torch.tensor([2]))]:
            want = O.gpt_pos_emb(sd, cfg, t, dl)
            assert torch.equal(net.get_pos_emb(t, dl), want)


def test_reference_import_paths_redirect():
    """with `models` / `tools` aliased to the ccvs_amd packages, the imports at the top of the
    reference's helpers/generator.py (:17-23) and models/__init__ resolve to the MI355X implementations."""
    prog = r'''
import sys
sys.path.insert(0, %r)
import ccvs_amd.models, ccvs_amd.tools
sys.modules["models"] = ccvs_amd.models
sys.modules["tools"] = ccvs_amd.tools
from tools.options import Options
from tools.engine import Engine
from tools.utils import mkdir, color_transfer, to_cuda, flatten_vid, unflatten_vid
from models.skip_vid_generator.models.quantized_video_model import QVidModel
from models.skip_vid_generator.models.state_model import StateModel
from models.skip_vid_generator.models.transformer_model import Transformer
from models.skip_vid_generator.models.stft_model import StftModel
from models.skip_vid_generator.models.skip_autoencoder import SkipGANEncoder, SkipGANDecoder, StateEstimator, StftEncoder
from models.skip_vid_generator.models.mingpt import GPT
from models.skip_vid_generator.modules.quantize import VectorQuantizer
from models import load_network, save_network, print_network
import ccvs_amd.ops
assert QVidModel.__module__ == "models.skip_vid_generator.models.quantized_video_model"
assert sys.modules["models.skip_vid_generator.models.mingpt"].ops is ccvs_amd.ops   # one kernel binding, whatever the alias
print("REDIRECT_OK")
''' % ROOT
    res = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "REDIRECT_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]


def test_conv_persistent_tiles_mode_is_a_host_switch(built_lib, monkeypatch):
    """`ccvs_conv_persistent_tiles` (include/ccvs_hip.h) is pure host state: query, set, the previous mode comes back, only bits 0-1
    are kept -- and `PipelinedRun.run` lowers it to 0 for a run of several batches and restores it, also when the run fails
    (no GPU call: the run is cut short at its first step)."""
    from ccvs_amd import ops
    from ccvs_amd.helpers import pipeline
    start = ops.conv_persistent_tiles()
    try:
        assert ops.conv_persistent_tiles(1) == start and ops.conv_persistent_tiles() == 1
        assert ops.conv_persistent_tiles(3) == 1 and ops.conv_persistent_tiles(7) == 3 and ops.conv_persistent_tiles() == 3
        assert ops.conv_persistent_tiles(1) == 3

        class Cut(Exception):
            pass

        seen = []
        run = pipeline.PipelinedRun.__new__(pipeline.PipelinedRun)
        run.dec_streams, run.s_enc, run.chain_list, run.entry = [], None, [], None
        monkeypatch.setattr(pipeline.PipelinedRun, "_run", lambda self, side: (seen.append(ops.conv_persistent_tiles()), (_ for _ in ()).throw(Cut()))[1])

        class NoStream:
            def wait_stream(self, other):
                pass
        run.s_enc = NoStream()
        for n_batches, want in ((20, 0), (None, 0), (1, 1)):
            run.n_batches = n_batches
            with pytest.raises(Cut):
                run.run()
            assert seen[-1] == want and ops.conv_persistent_tiles() == 1, (n_batches, seen)
    finally:
        ops.conv_persistent_tiles(start)
