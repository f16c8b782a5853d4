"""Times the Motion-JPEG output stage on one GPU for profiles/mjpeg.txt: `ccvs_mjpeg_encode` on one BAIR batch of
`Generator.run()` = 768 frames of 256 x 256 (16 clips x 16 frames x real / fake / rec), the device-to-host copies of the raw and of the
compressed batch, and the writer thread's job per batch as .npy and as .avi.  Synthetic frames (a smooth field, shifted per frame, plus
noise); two frames are checked against the mirror tests/jpeg_ref.py.    python tools/mjpeg_bench.py [--out FILE]"""
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import jpeg_ref as R
from ccvs_amd import ops
from ccvs_amd.helpers.generator import save_video_batch

out = open(sys.argv[sys.argv.index("--out") + 1], "w") if "--out" in sys.argv else None


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if out is not None:
        out.write(line + "\n")
        out.flush()



torch.manual_seed(0)
dev = torch.device("cuda")
base = torch.from_numpy(R._smooth(256, 256)).to(dev).float()
frames = []
for k in range(768):
    f = torch.roll(base, shifts=(k % 61, (3 * k) % 97), dims=(0, 1)) + 4.0 * torch.randn(256, 256, 3, device=dev)
    frames.append(f.clamp(0, 255).to(torch.uint8))
u8 = torch.stack(frames)
raw = u8.numel()
say("device", torch.cuda.get_device_name(0), "; frames", tuple(u8.shape), "raw bytes", raw)

def timed(fn, reps, warm=3):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms
def host_timed(fn, reps, warm=2):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); torch.cuda.synchronize(); ms.append(1e3 * (time.perf_counter() - t))
    return ms
def fmt(ms): return f"median {statistics.median(ms):.3f} ms  min {min(ms):.3f}  max {max(ms):.3f}  (n={len(ms)})"

for q in (90, 75):
    stream = torch.empty(raw, dtype=torch.uint8, device=dev)
    _, off = ops.mjpeg_encode(u8, q, out=stream)
    total = int(off[-1])
    ms = timed(lambda: ops.mjpeg_encode(u8, q, out=stream), 20)
    say(f"ccvs_mjpeg_encode q={q}: bytes in {raw} bytes out {total} (ratio {raw / total:.2f}); device events around the call (3 kernels + 2 allocations): {fmt(ms)}; "
        f"{raw / statistics.median(ms) / 1e6:.1f} GB/s of input")
# spot check: frames 0 and 767 equal the mirror
stream, off = ops.mjpeg_encode(u8, 90)
off = off.tolist(); s = stream.cpu().numpy()
for k in (0, 767):
    assert bytes(s[off[k]:off[k + 1]]) == R.encode_scan(u8[k].cpu().numpy(), 90), k
say("frames 0 and 767 of the batch equal the mirror byte for byte")
say("device-to-host copy of the raw uint8 batch (u8.cpu(), pageable, as save_video_batch does):", fmt(host_timed(lambda: u8.cpu(), 10)))
comp = stream[:off[-1]]
say(f"device-to-host copy of the compressed stream ({off[-1]} bytes, .cpu()):", fmt(host_timed(lambda: comp.cpu(), 10)))
say("mjpeg_encode_to_host (encode + offsets + compressed bytes to the host):", fmt(host_timed(lambda: ops.mjpeg_encode_to_host(u8, 90), 10)))

# the writer thread's job per batch: three save_video_batch calls of [16, 16, 3, 256, 256]
clips = [(u8[256 * k:256 * (k + 1)].view(16, 16, 256, 256, 3).permute(0, 1, 4, 2, 3).float() / 127.5 - 1.0).contiguous() for k in range(3)]
tmp = tempfile.mkdtemp(prefix="mjpeg_bench_")
def writer(fmt_, rc):
    for k, c in enumerate(clips):
        save_video_batch(c, 16, 0, os.path.join(tmp, fmt_ or "auto", str(k)), 4, True, False, [-1, 1], "bairhd", video_format=fmt_, return_clip=rc)
res = {"npy": [], "avi": []}
writer("npy", True); writer("avi", False)
for _ in range(5):
    for name, rc in (("npy", True), ("avi", False)):
        t = time.perf_counter(); writer(name, rc); torch.cuda.synchronize(); res[name].append(1e3 * (time.perf_counter() - t))
def du(d): return sum(os.path.getsize(os.path.join(b, f)) for b, _, fs in os.walk(d) for f in fs)
say(f"writer job per batch (3 x save_video_batch of 16 x 16 frames, files to {tempfile.gettempdir()}), alternating:")
say("  .npy:", fmt(res["npy"]), "; bytes on disk", du(os.path.join(tmp, "npy")))
say("  .avi (q=90, return_clip=False):", fmt(res["avi"]), "; bytes on disk", du(os.path.join(tmp, "avi")))
shutil.rmtree(tmp)
say("done")
