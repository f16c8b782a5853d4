"""What `--x_kv_dtype bf16` costs and saves at BAIR sizes, random weights (no trained checkpoint ships with the repository):

  bytes    the KV cache per batch in both dtypes (arithmetic from the shapes, `GPT.kv_cache_bytes`);
  time     one decode step (`ccvs_gpt_decode_step` / `ccvs_gpt_decode_step_bf16kv`: embed .. pick), HIP events around runs of 8
           consecutive steps whose cache lengths straddle T (T - 4 .. T + 3), 2 warm-up runs, then the median / min / max of 9 runs, as
           eager launches and as the replayed 8-step hipGraph; rows in {16, 64}, T in {256, 1023}; sampled picks (Philox, top-k 100);
  quality  `--quality`: teacher-forced NLL of a random-token clip under both modes (mean and max |difference| per token) and the share
           of greedy tokens that differ over one 64 -> 1024 rollout (1 -> 15 frames of 64 tokens).

  e2e      `--e2e`: the Generator at the BAIR launch line (batch 16, synthetic clips, random weights), with and without the flag:
           one `generate_vid` on the serial and on the stream schedule, `run_pipelined` over 4 batches -- seconds, frames/s and
           torch.cuda.max_memory_allocated.

    python tools/kv_dtype_probe.py [--modes fp32,bf16] [--quality] [--e2e] [--no-steps] [--label TEXT]

A tree without the mode (the parent commit, for the same-session comparison) runs `--modes fp32`.  The clocks are not pinned: the
spread of the repeats is printed with every figure."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ccvs_amd.models.skip_vid_generator.models import mingpt  # noqa: E402

STEPS, WARM, REPS = 8, 2, 9
TMAX = 1088   # 17 frames of 64 positions: room for the 8 steps around T = 1023


def bair_gpt(seed=0):
    torch.manual_seed(seed)
    net = mingpt.GPT(vocab_size=1024, block_size=TMAX, num_blocks=17, n_layer=24, n_head=16, n_embd=1024, emb_mode="temporal", shape=(8, 8)).cuda()
    for p in net.parameters():   # (the initialiser leaves LayerNorm at identity and the biases at zero)
        p.data.add_(0.02 * torch.randn_like(p))
    return net.eval()


def set_mode(net, kv_dtype):
    net.drop_engine_state()
    if hasattr(net, "kv_dtype"):
        net.kv_dtype = kv_dtype
    else:
        assert kv_dtype == "fp32", "this tree has no bf16 KV cache"


def time_steps(net, rows, T, form):
    """-> ms per decode step: [median, min, max] over REPS runs of STEPS steps."""
    sampler = {"sample": True, "top_k": 100, "temperature": 1.0, "noise": "device", "top_p": None}
    c = net.begin(rows, TMAX)
    g = torch.Generator(device="cuda").manual_seed(1)
    for t in c["k"] + c["v"]:   # a filled cache: the values do not matter to the time, NaNs would
        t.copy_(torch.randn(t.shape, device="cuda", generator=g).to(t.dtype))
    c["tok"].copy_(torch.randint(0, 1024, c["tok"].shape, device="cuda", generator=g))
    net._set_decode_state([(1, 2, 0, 0)])
    key = ("probe", rows, T, form)
    graph = net._decode_graph(sampler, key + (STEPS,), steps=STEPS) if form == "graph" else None
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for rep in range(WARM + REPS):
        c["len_dev"].fill_(T - STEPS // 2)
        c["widx"].fill_(T - STEPS // 2)
        a.record()
        if graph is not None:
            graph.replay()
        else:
            for _ in range(STEPS):
                net._decode_body(sampler)
        b.record()
        b.synchronize()
        if rep >= WARM:
            out.append(a.elapsed_time(b) / STEPS)
    assert int(c["len_dev"][0]) == T + STEPS // 2
    return statistics.median(out), min(out), max(out)


def kv_bytes(net, rows):
    cfg = net.config
    item = 2 if getattr(net, "kv_dtype", "fp32") == "bf16" else 4
    return 2 * cfg.n_layer * rows * 1024 * cfg.n_embd * item


def quality(net):
    gen = torch.Generator().manual_seed(7)
    tokens = torch.randint(0, 1024, (4, 1024), generator=gen).cuda()
    nll = {}
    for kv in ("fp32", "bf16"):
        set_mode(net, kv)
        logits = net(tokens[:, :-1])                                   # teacher-forced, [B, 1023, V]
        lp = torch.log_softmax(logits.double(), -1)
        nll[kv] = -lp.gather(-1, tokens[:, 1:].unsqueeze(-1)).squeeze(-1)
        del logits, lp
    d = (nll["fp32"] - nll["bf16"]).abs()
    print(f"quality  teacher-forced NLL, random weights, 4 x 1023 random tokens: mean fp32 {nll['fp32'].mean().item():.6f}  bf16 {nll['bf16'].mean().item():.6f}"
          f"  |difference| per token: mean {d.mean().item():.3e}  max {d.max().item():.3e}")
    toks = {}
    for kv in ("fp32", "bf16"):
        set_mode(net, kv)
        toks[kv] = net.generate(tokens[:, :64].contiguous(), 1024 - 64, sample=False)
    torch.cuda.synchronize()
    diff = (toks["fp32"][:, 64:] != toks["bf16"][:, 64:])
    first = [int(r.nonzero()[0]) if r.any() else -1 for r in diff]
    print(f"quality  greedy rollout 64 -> 1024 tokens (1 -> 15 frames), random weights, 4 clips: share of tokens that differ {diff.float().mean().item():.4f}"
          f"  first differing step per clip {first}")
    print("quality  (random weights give near-flat distributions: after the first differing token the two rollouts are different sequences;"
          " the effect on samples of a trained model is NOT measured -- no checkpoint ships with the repository)")


def e2e(kv):
    import time
    from ccvs_amd.tools.options import Options, BAIR_ARGV
    from ccvs_amd.helpers.generator import Generator
    argv = list(BAIR_ARGV) + ["--batch_size_vid", "16", "--x_sample_noise", "device", "--rec_pass", "false"] + (["--x_kv_dtype", kv] if kv != "fp32" else [])
    opt = Options().parse(load_qvid_generator=True, load_transformer=True, argv=argv)
    torch.manual_seed(0)
    gen = Generator(opt).build_models()
    batches = [{"vid": gen.synthetic_batch(16, seed=1 + i)["vid"].cuda()} for i in range(4)]
    frames = 16 * gen.opt.vid_len

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    with torch.no_grad():
        for schedule in ("serial", "stream"):
            call = lambda: gen.generate_vid({"vid": batches[0]["vid"].clone()}, 0, schedule=schedule)   # noqa: E731
            timed(call)                                                                                 # warm-up: captures, packed weights
            torch.cuda.reset_peak_memory_stats()
            t = timed(call)
            print(f"e2e      {kv}  generate_vid({schedule}), batch 16: {t:6.3f} s  {frames / t:7.1f} frames/s  max_memory_allocated {torch.cuda.max_memory_allocated() / 2 ** 30:5.2f} GiB")
        run = lambda: gen.run_pipelined(({"vid": b["vid"].clone()} for b in batches), first_iter=0)    # noqa: E731
        timed(run)
        torch.cuda.reset_peak_memory_stats()
        t = timed(run)
        print(f"e2e      {kv}  run_pipelined, 4 batches of 16:     {t:6.3f} s  {4 * frames / t:7.1f} frames/s  max_memory_allocated {torch.cuda.max_memory_allocated() / 2 ** 30:5.2f} GiB")
    del gen
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="fp32,bf16")
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--no-steps", action="store_true", help="skip the decode-step timing")
    ap.add_argument("--label", default="this tree")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU: no fallback"
    dev = torch.cuda.get_device_properties(0)
    print(f"# {args.label}: {dev.name}, {dev.multi_processor_count} CUs, clocks not pinned; ms per decode step = median [min .. max] of {REPS} runs of {STEPS} steps")
    net = bair_gpt()
    with torch.no_grad():
        for kv in args.modes.split(","):
            set_mode(net, kv)
            for rows in (16, 64):
                print(f"bytes    {kv}  KV cache per batch of {rows} x 1024 positions: {kv_bytes(net, rows) / 2 ** 20:.0f} MiB")
            for rows in (16, 64) if not args.no_steps else ():
                for T in (256, 1023):
                    for form in ("eager", "graph"):
                        net.drop_engine_state()
                        med, lo, hi = time_steps(net, rows, T, form)
                        print(f"time     {kv}  rows {rows:3d}  T {T:4d}  {form:5s}  {med:7.3f} [{lo:7.3f} .. {hi:7.3f}] ms/step")
        if args.quality:
            quality(net)
    del net
    torch.cuda.empty_cache()
    if args.e2e:
        for kv in args.modes.split(","):
            e2e(kv)
    print(f"memory   torch.cuda.max_memory_allocated {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


if __name__ == "__main__":
    main()
