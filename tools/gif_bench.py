"""Measures the GIF output stage on one GPU for profiles/gif.txt.  Times of device work are HIP-event medians
around the call, two series each, the forms alternating (the difference between the series of one form is the run-to-run spread);
times that include the copy to the host are wall-clock medians around the call and a synchronise.

  batch    one batch of `Generator.run()`'s writer: 16 clips x 16 frames of 256 x 256 (the frames of tools/apng_bench.py: a smooth field
           shifted per frame plus noise).  `ops.gif_encode` (palette and LZW) and `ops.gif_palette` alone, beside `ops.png_encode` and
           `ops.mjpeg_encode` at 4:4:4 on the same batch in the same run; then what reaches the host: `gif_encode_to_host` beside
           `png_encode_to_host`, `mjpeg_encode_to_host` and the raw clip's `.cpu()` of the .npy path.
  sizes    bytes of the batch in each form; clip 3 equals the mirror byte for byte.

    python tools/gif_bench.py [--out FILE]
"""
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))
import gif_ref as G  # noqa: E402
import jpeg_opt_ref as O  # noqa: E402
from ccvs_amd import lib, ops  # noqa: E402

out = open(sys.argv[sys.argv.index("--out") + 1], "a") if "--out" in sys.argv else None


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


def walled(fn, reps=10, warm=2):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t))
    return ms


torch.manual_seed(0)
dev = torch.device("cuda")
base = torch.from_numpy(O._smooth(256, 256)).to(dev).float()
u8 = torch.stack([(torch.roll(base, shifts=(k % 61, (3 * k) % 97), dims=(0, 1)) + 4.0 * torch.randn(256, 256, 3, device=dev)).clamp(0, 255).to(torch.uint8)
                  for k in range(256)])
clips = u8.view(16, 16, 256, 256, 3)
raw = u8.numel()
L = lib.load()
gif_stream = torch.empty(int(L.ccvs_gif_stream_bound(256, 256, 256, 0)), dtype=torch.uint8, device=dev)
png_stream = torch.empty(int(L.ccvs_apng_stream_bound(256, 256, 256, 0)), dtype=torch.uint8, device=dev)
say("library", os.path.relpath(lib.LIB_PATH, HERE), "; device", torch.cuda.get_device_name(0), "; clips", tuple(clips.shape), "raw bytes", raw,
    "; gif workspace", int(L.ccvs_gif_workspace_bytes(16, 16, 256, 256, 0)), "bytes")

forms = (("gif palette + LZW", lambda: ops.gif_encode(clips, out=gif_stream)), ("gif palette only ", lambda: ops.gif_palette(clips)),
         ("apng adaptive    ", lambda: ops.png_encode(u8, -1, out=png_stream)), ("mjpeg 444 q90    ", lambda: ops.mjpeg_encode(u8, 90, out=png_stream[:raw])))
for series in range(2):
    for name, fn in forms:
        say(f"device  {name} series {series}: {fmt(timed(fn))}")
hosts = (("gif_encode_to_host  ", lambda: ops.gif_encode_to_host(clips)), ("png_encode_to_host  ", lambda: ops.png_encode_to_host(u8)),
         ("mjpeg_encode_to_host", lambda: ops.mjpeg_encode_to_host(u8, 90)), ("raw clip .cpu()     ", lambda: u8.cpu()))
for series in range(2):
    for name, fn in hosts:
        say(f"to host {name} series {series}: {fmt(walled(fn))}")

data, off, pals = ops.gif_encode_to_host(clips)
_, off_png = ops.png_encode_to_host(u8)
_, off_jpg = ops.mjpeg_encode_to_host(u8, 90)
want, off_w, pal_w, table_w, used_w = G.encode(clips[3].cpu().numpy(), 0)
assert data[off[48]:off[64]] == want and np.array_equal(pals[3], pal_w)
say(f"  clip 3 equals the mirror byte for byte ({off[64] - off[48]} bytes, {used_w} colours)")
shown = torch.from_numpy(pal_w[G.indices(clips[3].cpu().numpy(), table_w)]).double()
mse = ((shown - clips[3].cpu().double()) ** 2).mean().item()
say(f"  clip 3 quantisation PSNR {10 * np.log10(255.0 ** 2 / mse):.2f} dB")
say(f"  batch of 16 clips: raw {raw} B; gif payloads {off[-1]} B ({off[-1] / raw:.4f} of raw); apng streams {off_png[-1]} B ({off_png[-1] / raw:.4f}); "
    f"mjpeg 4:4:4 q90 scans {off_jpg[-1]} B ({off_jpg[-1] / raw:.4f})")
say("done")
