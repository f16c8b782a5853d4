"""Times the Motion-JPEG encoder per chrominance sampling on one GPU for profiles/mjpeg.txt, on the batch of
tools/mjpeg_bench.py: 768 frames of 256 x 256 (one BAIR batch of `Generator.run()`), a smooth field shifted per frame plus noise, quality
90.  Per sampling: the HIP-event median of the encode (both passes plus the scan), the compressed bytes, and the writer job per batch
(3 x `save_video_batch` of 16 x 16 frames as .avi).  One frame per sampling is checked against the mirror tests/jpeg_sub_ref.py.

    python tools/mjpeg_sub_bench.py [--tree DIR] [--out FILE]

--tree DIR: import `ccvs_amd` from another checkout (one from before the samplings existed is timed at 4:4:4 alone), so that two
commits are measured by the same script in the same session."""
import inspect
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv else HERE
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(HERE, "tests"))
import jpeg_sub_ref as S  # noqa: E402
from ccvs_amd import lib, ops  # noqa: E402
from ccvs_amd.helpers.generator import save_video_batch  # noqa: E402

out = open(sys.argv[sys.argv.index("--out") + 1], "a") if "--out" in sys.argv else None


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if out is not None:
        out.write(line + "\n")
        out.flush()


sampled = "sampling" in inspect.signature(ops.mjpeg_encode).parameters
torch.manual_seed(0)
dev = torch.device("cuda")
base = torch.from_numpy(S._smooth(256, 256)).to(dev).float()
u8 = torch.stack([(torch.roll(base, shifts=(k % 61, (3 * k) % 97), dims=(0, 1)) + 4.0 * torch.randn(256, 256, 3, device=dev)).clamp(0, 255).to(torch.uint8)
                  for k in range(768)])
raw = u8.numel()
say("tree", TREE, "; library", lib.LIB_PATH, "; samplings", "444 422 420" if sampled else "444 only")
say("device", torch.cuda.get_device_name(0), "; frames", tuple(u8.shape), "raw bytes", raw, "; quality 90")


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


clips = [(u8[256 * k:256 * (k + 1)].view(16, 16, 256, 256, 3).permute(0, 1, 4, 2, 3).float() / 127.5 - 1.0).contiguous() for k in range(3)]
tmp = tempfile.mkdtemp(prefix="mjpeg_sub_bench_")
for name, s in (("444", 0), ("422", 1), ("420", 2)) if sampled else (("444", 0),):
    kw = {"sampling": s} if sampled else {}
    stream = torch.empty(raw, dtype=torch.uint8, device=dev)
    _, off = ops.mjpeg_encode(u8, 90, out=stream, **kw)
    off = off.tolist()
    for series in range(2):                                          # two series: their difference is the run-to-run spread
        say(f"encode {name} series {series}: bytes out {off[-1]} (ratio {raw / off[-1]:.2f}); HIP events around the call: {fmt(timed(lambda: ops.mjpeg_encode(u8, 90, out=stream, **kw)))}")
    host = stream.cpu().numpy()
    assert bytes(host[off[5]:off[6]]) == S.encode_scan_sub(u8[5].cpu().numpy(), 90, s), name
    say(f"  frame 5 equals the mirror byte for byte ({off[6] - off[5]} bytes)")
    how = {"subsampling": name} if sampled else {}

    def writer():
        for k, c in enumerate(clips):
            save_video_batch(c, 16, 0, os.path.join(tmp, name, str(k)), 4, True, False, [-1, 1], "bairhd", video_format="avi", return_clip=False, **how)
    writer()
    ms = []
    for _ in range(5):
        t = time.perf_counter()
        writer()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t))
    disk = sum(os.path.getsize(os.path.join(b, f)) for b, _, fs in os.walk(os.path.join(tmp, name)) for f in fs)
    say(f"  writer job per batch, .avi {name}: {fmt(ms)}; bytes on disk {disk}")
shutil.rmtree(tmp)
say("done")
