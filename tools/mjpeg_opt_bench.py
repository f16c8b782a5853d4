"""Measures the Motion-JPEG encoder with per-frame optimised Huffman tables on one GPU for
profiles/mjpeg_optimized.txt.  Quality 90 throughout; times are HIP-event medians around the call, two series each, the two forms
alternating (the difference between the series of one form is the run-to-run spread).

  batch    one batch of `Generator.run()`'s writer: 16 clips x 16 frames of 256 x 256 (the frames of tools/mjpeg_bench.py: a smooth field
           shifted per frame plus noise).  Per sampling: the standard encode beside gather + tables + emit, and the bytes of both.
  default  `ccvs_mjpeg_encode` / `ccvs_mjpeg_encode_sampled` on that batch, this library against another build of it (--parent-lib: the
           library of the parent commit), called through ctypes in the same process, alternating.
  clips    (--clips) the BAIR clips of a generator run as bench.py sets it up (random weights, seeded synthetic input: `real` is that
           input, `fake` what the generator makes of it): bytes per clip, header and scan apart, standard against optimised.
  profile  (--profile) nothing but ten optimised encodes of the batch at 4:4:4, for a run under rocprofv3 --kernel-trace --stats.

    python tools/mjpeg_opt_bench.py [--parent-lib FILE] [--clips] [--profile] [--out FILE]
"""
import ctypes
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))
import jpeg_opt_ref as O  # noqa: E402
from ccvs_amd import lib, ops  # noqa: E402
from ccvs_amd.tools import mjpeg  # noqa: E402

out = open(sys.argv[sys.argv.index("--out") + 1], "a") if "--out" in sys.argv else None
NAMES = ("444", "422", "420")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if out is not None:
        out.write(line + "\n")
        out.flush()


def fmt(ms):
    return f"median {statistics.median(ms):.3f} ms  min {min(ms):.3f}  max {max(ms):.3f}  (n={len(ms)})"


def timed(fn, reps=30, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def sizes(u8, s):
    """(frames, standard header bytes, standard scan bytes, optimised header bytes, optimised scan bytes) of uint8 frames [n, H, W, 3]."""
    h, w = u8.shape[-3:-1]
    _, off = ops.mjpeg_encode_to_host(u8, 90, sampling=s)
    _, ooff, tables = ops.mjpeg_encode_to_host(u8, 90, sampling=s, optimize=True)
    n = len(off) - 1
    head = len(mjpeg.jpeg_header(h, w, 90, sampling=s)) + 2                                 # (+ EOI)
    ohead = sum(len(mjpeg.jpeg_header(h, w, 90, sampling=s, huffman=mjpeg.huffman_from_spec(t))) + 2 for t in tables)
    return n, n * head, off[-1], ohead, ooff[-1]


def size_line(what, clips, u8, s):
    n, head, scan, ohead, oscan = sizes(u8, s)
    std, opt = head + scan, ohead + oscan
    say(f"  {what} {NAMES[s]}: per clip standard {std / clips:.0f} B (header {head / clips:.0f} + scan {scan / clips:.0f}), optimised {opt / clips:.0f} B "
        f"(header {ohead / clips:.0f} + scan {oscan / clips:.0f}): -{100 * (std - opt) / std:.1f} % (header -{100 * (head - ohead) / std:.1f} %, "
        f"scan -{100 * (scan - oscan) / std:.1f} % of the standard file)")


torch.manual_seed(0)
dev = torch.device("cuda")
base = torch.from_numpy(O._smooth(256, 256)).to(dev).float()
u8 = torch.stack([(torch.roll(base, shifts=(k % 61, (3 * k) % 97), dims=(0, 1)) + 4.0 * torch.randn(256, 256, 3, device=dev)).clamp(0, 255).to(torch.uint8)
                  for k in range(256)])
raw = u8.numel()
stream = torch.empty(raw, dtype=torch.uint8, device=dev)
say("library", lib.LIB_PATH, "; device", torch.cuda.get_device_name(0), "; frames", tuple(u8.shape), "raw bytes", raw, "; quality 90")

if "--profile" in sys.argv:
    for _ in range(10):
        ops.mjpeg_encode_optimized(u8, 90, out=stream)
    torch.cuda.synchronize()
    say("done")
    sys.exit(0)

# ---- batch
for s in (0, 1, 2):
    forms = (("standard ", lambda: ops.mjpeg_encode(u8, 90, out=stream, sampling=s)), ("optimised", lambda: ops.mjpeg_encode_optimized(u8, 90, out=stream, sampling=s)))
    for series in range(2):
        for name, fn in forms:
            say(f"batch {NAMES[s]} {name} series {series}: {fmt(timed(fn))}")
    _, off, tables = ops.mjpeg_encode_optimized(u8, 90, out=stream, sampling=s)
    off, host = off.tolist(), stream.cpu().numpy()
    scan, want, _ = O.encode_scan_optimized(u8[5].cpu().numpy(), 90, s)
    assert bytes(host[off[5]:off[6]]) == scan and (tables[5].cpu().numpy() == O.spec_bytes(want)).all(), s
    say(f"  frame 5 equals the mirror byte for byte ({off[6] - off[5]} bytes, tables too)")
    size_line("batch of 16 clips,", 16, u8, s)

# ---- default path, this library against the parent's
if "--parent-lib" in sys.argv:
    path = os.path.abspath(sys.argv[sys.argv.index("--parent-lib") + 1])
    libs = (("this  ", lib.load()), ("parent", ctypes.CDLL(path)))
    vp = ctypes.c_void_p
    offsets = torch.empty(257, dtype=torch.int64, device=dev)
    cur = vp(torch.cuda.current_stream().cuda_stream)
    for s in (0, 1, 2):
        r = (32, 16, 16)[s]
        work = torch.empty(12 * 256 * 1024 // r // (1, 2, 4)[s] + 64, dtype=torch.uint8, device=dev)
        got = []

        def call(L):
            if s == 0:
                f = L.ccvs_mjpeg_encode
                f.restype, f.argtypes = ctypes.c_int, [vp, ctypes.c_long] + [ctypes.c_int] * 5 + [vp, ctypes.c_long, vp, vp, vp]
                rc = f(vp(u8.data_ptr()), 256 * 256 * 3, 256, 256, 256, 90, r, vp(stream.data_ptr()), raw, vp(offsets.data_ptr()), vp(work.data_ptr()), cur)
            else:
                f = L.ccvs_mjpeg_encode_sampled
                f.restype, f.argtypes = ctypes.c_int, [vp, ctypes.c_long] + [ctypes.c_int] * 6 + [vp, ctypes.c_long, vp, vp, vp]
                rc = f(vp(u8.data_ptr()), 256 * 256 * 3, 256, 256, 256, 90, s, r, vp(stream.data_ptr()), raw, vp(offsets.data_ptr()), vp(work.data_ptr()), cur)
            assert rc == 0
        for series in range(3):
            for name, L in libs:
                say(f"default {NAMES[s]} {name} series {series}: {fmt(timed(lambda: call(L)))}")
        for name, L in libs:
            stream.zero_()
            call(L)
            got.append((offsets.tolist(), stream[:int(offsets[-1])].cpu().numpy().tobytes()))
        assert got[0] == got[1]
        say(f"  the two libraries write the same {got[0][0][-1]} bytes")

# ---- the clips of a generator run
if "--clips" in sys.argv:
    import types
    import bench
    from ccvs_amd.tools.engine import Engine
    args = types.SimpleNamespace(config="bair", batch=16, sample_noise="device", rec_pass=False, encode="all")
    with Engine() as engine, torch.no_grad():
        gen, opt = bench.build_generator(args)
        gen.engine = engine
        bench.calibrate_codebook(gen, {"vid": gen.synthetic_batch(2, seed=1, first_clip=0)["vid"].to(dev)})
        data = {"vid": gen.synthetic_batch(16, seed=1, first_clip=0)["vid"].to(dev)}
        torch.manual_seed(bench.noise_seed_of_rank(0))
        res = gen.generate_vid(data, 0)
        clips = {"real": ops.pack_u8(data["vid"].contiguous()), "fake": ops.pack_u8(res["fake"]["vid"].contiguous())}
    for kind, c in clips.items():
        say(f"clips of a generator run (bair, random weights, synthetic input), {kind}: {tuple(c.shape)}")
        for s in (0, 1, 2):
            size_line(kind, c.shape[0], c, s)
say("done")
