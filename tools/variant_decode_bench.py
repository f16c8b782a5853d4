#!/usr/bin/env python3
"""Cost of the flow-decoder variants of Matching at BAIR 256^2 geometry (random weights, batch 16, the default contexts):
one full-frame decode (`vid_decoder`, random tokens) per variant against the default decoder, and the deformable convolution
kernel alone at every level's shape: us per launch, algorithmic TFLOP/s and the fraction of the roofline bench.py prices the
convolutions against (dense bf16 MFMA peak for split-bf16, fp32 MFMA peak for the strict mode).

The `skiprgb` row is the --q_skip_rgb output head (a ToRGB per level) on the default flow decoder.

    python tools/variant_decode_bench.py [--batch 16] [--reps 3] [--variants default skiprgb] [--out profiles/variant_decode_bench.json]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ccvs_amd.tools.options import Options, BAIR_ARGV  # noqa: E402
from ccvs_amd.helpers.generator import Generator  # noqa: E402
from ccvs_amd import ops  # noqa: E402

BF16_MFMA_PEAK_TFLOPS, FP32_MFMA_PEAK_TFLOPS = 2500.0, 157.3   # the peaks of bench.py
VARIANTS = {
    "default": [],
    "masked": ["--q_use_masked_flow"],
    "deform": ["--q_use_deformed_conv"],
    "tradeoff": ["--q_use_tradeoff"],
    "nocorr": ["--q_no_corr"],
    "all": ["--q_use_masked_flow", "--q_use_deformed_conv", "--q_use_tradeoff", "--q_no_corr"],
    "skiprgb": ["--q_skip_rgb"],
}


def decode_ms(flags, batch, reps):
    opt = Options().parse(load_qvid_generator=True, load_transformer=True, argv=list(BAIR_ARGV) + ["--batch_size_vid", str(batch), "--rec_only"] + flags)
    torch.manual_seed(0)
    gen = Generator(opt).build_models()
    qv = gen.vid_model
    data = {"vid": gen.synthetic_batch(batch, seed=1)["vid"].cuda()}
    shapes = []
    with torch.no_grad():
        enc = qv(data, mode="vid_encoder")
        n_tok = enc["code"].shape[1]
        code = torch.randint(0, qv.net_q.embedding.weight.shape[0], (batch, n_tok), generator=torch.Generator().manual_seed(2)).cuda()
        inter = [f[:, :1].contiguous() for f in enc["inter"]]
        ops.KERNEL_TIMER = ops.KernelTimer()
        qv({"code": code, "inter": inter}, mode="vid_decoder")    # warm-up (weight packing, allocator); records the deform shapes
        torch.cuda.synchronize()
        shapes = sorted({r[6] for r in ops.KERNEL_TIMER.records if r[0].startswith("deform_")})
        ops.KERNEL_TIMER = None
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            qv({"code": code, "inter": inter}, mode="vid_decoder")
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
    del gen, qv, enc, data
    torch.cuda.empty_cache()
    return min(times), times, shapes


def deform_alone(shape, precision, flow_kind, iters=10):
    n, c, h, w = shape
    k = 2 if n % 2 == 0 else 1
    g = torch.Generator(device="cuda").manual_seed(0)
    ctxs = [torch.randn(n // k, c, h, w, device="cuda", generator=g) for _ in range(k)]
    if flow_kind == "random":   # independent per pixel: every lane of a wave gathers from its own cache lines (the worst case)
        flow = torch.randn(n, 2, h, w, device="cuda", generator=g) * 3
    else:                       # smooth, as a decoder's up-sampled flow is: a random 8 x 8 field, bilinearly enlarged
        flow = torch.nn.functional.interpolate(torch.randn(n, 2, 8, 8, device="cuda", generator=g) * 3, size=(h, w), mode="bilinear")
    wp = ops.pack_deform_weight(torch.randn(c, c, 3, 3, device="cuda", generator=g) * 0.02, precision=precision)
    bias = torch.zeros(c, device="cuda")
    for _ in range(3):
        ops.deform_conv3x3(ctxs, flow, 4.0, wp, bias, act=True)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        ops.deform_conv3x3(ctxs, flow, 4.0, wp, bias, act=True)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    flops = 2.0 * n * c * c * 9 * h * w
    tf = flops / (us * 1e-6) / 1e12
    peak = BF16_MFMA_PEAK_TFLOPS if precision == "bf16x3" else FP32_MFMA_PEAK_TFLOPS
    gather_bytes = 4.0 * n * c * h * w * (9 * 4 + 1)   # 4 corner reads per tap and channel (mostly cache hits) + the output
    return {"shape_NCHW": [n, c, h, w], "precision": precision, "flow": flow_kind, "us": us, "tflops": tf, "peak": peak, "frac": tf / peak,
            "gather_bytes_per_us_GBps": gather_bytes / (us * 1e-6) / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--variants", nargs="+", default=list(VARIANTS), choices=list(VARIANTS))
    args = ap.parse_args()
    assert torch.cuda.is_available()
    res = {"geometry": "BAIR 256x256 (ccvs_amd.tools.options.BAIR_ARGV), random weights and tokens", "batch": args.batch, "decode_ms": {},
           "deform_alone": []}
    all_shapes = set()
    for name, flags in VARIANTS.items():
        if name not in args.variants:
            continue
        t0 = time.time()
        best, times, shapes = decode_ms(flags, args.batch, args.reps)
        all_shapes.update(shapes)
        res["decode_ms"][name] = {"best": best, "all": times}
        print(f"decode {name:9s} {best:9.1f} ms  (runs {', '.join(f'{t:.1f}' for t in times)}; {time.time() - t0:.0f} s wall)", flush=True)
    base = res["decode_ms"]["default"]["best"]
    for name in res["decode_ms"]:
        res["decode_ms"][name]["vs_default"] = res["decode_ms"][name]["best"] / base
    largest = {}
    for n, c, h, w in all_shapes:   # one shape per level: the most context pairs
        largest[(c, h, w)] = max(n, largest.get((c, h, w), 0))
    for (c, h, w), n in sorted(largest.items(), key=lambda t: t[0][1]):
        for flow_kind in ("smooth", "random"):
            for prec in ("bf16x3", "f32"):
                r = deform_alone((n, c, h, w), prec, flow_kind)
                res["deform_alone"].append(r)
                print(f"deform {prec:6s} {flow_kind:6s} N,C,H,W={(n, c, h, w)}: {r['us']:9.1f} us  {r['tflops']:7.1f} TFLOP/s  frac {r['frac']:.4f} of "
                      f"{r['peak']:.0f}", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
