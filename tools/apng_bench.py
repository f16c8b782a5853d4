"""Measures the lossless output stage on one GPU for profiles/apng.txt.  Times of device work are HIP-event
medians around the call, two series each, the forms alternating (the difference between the series of one form is the run-to-run
spread); times that include the copy to the host are wall-clock medians around the call and a synchronise.

  batch    one batch of `Generator.run()`'s writer: 16 clips x 16 frames of 256 x 256 (the frames of tools/mjpeg_opt_bench.py: a smooth
           field shifted per frame plus noise).  `ops.png_encode` with the adaptive filter and with Sub forced, beside `ops.mjpeg_encode`
           at 4:4:4; then what reaches the host: `png_encode_to_host`, `mjpeg_encode_to_host`, and the raw clip's `.cpu()` of the .npy path.
  sizes    bytes of the batch, and on eight of its frames zlib's Huffman-only and level-6 streams of the same filtered bytes and
           Pillow's default PNG; frame 5 equals the mirror byte for byte.
  profile  (--profile) nothing but ten adaptive encodes of the batch, for a run under rocprofv3 --kernel-trace --stats.

    python tools/apng_bench.py [--profile] [--out FILE]
"""
import io
import os
import statistics
import sys
import time
import zlib

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))
import apng_ref as R  # noqa: E402
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
raw = u8.numel()
L = lib.load()
stream = torch.empty(int(L.ccvs_apng_stream_bound(256, 256, 256, 0)), dtype=torch.uint8, device=dev)
say("library", os.path.relpath(lib.LIB_PATH, HERE), "; device", torch.cuda.get_device_name(0), "; frames", tuple(u8.shape), "raw bytes", raw,
    "; workspace", int(L.ccvs_apng_workspace_bytes(256, 256, 256, 0)), "bytes")

if "--profile" in sys.argv:
    for _ in range(10):
        ops.png_encode(u8, -1, out=stream)
    torch.cuda.synchronize()
    say("done")
    sys.exit(0)

forms = (("apng adaptive ", lambda: ops.png_encode(u8, -1, out=stream)), ("apng Sub      ", lambda: ops.png_encode(u8, 1, out=stream)),
         ("mjpeg 444 q90 ", lambda: ops.mjpeg_encode(u8, 90, out=stream[:raw])))
for series in range(2):
    for name, fn in forms:
        say(f"device  {name} series {series}: {fmt(timed(fn))}")
hosts = (("png_encode_to_host  ", lambda: ops.png_encode_to_host(u8)), ("mjpeg_encode_to_host", lambda: ops.mjpeg_encode_to_host(u8, 90)),
         ("raw clip .cpu()     ", lambda: u8.cpu()))
for series in range(2):
    for name, fn in hosts:
        say(f"to host {name} series {series}: {fmt(walled(fn))}")

data, off = ops.png_encode_to_host(u8)
sub, off_sub = ops.png_encode_to_host(u8, 1)
_, off_jpg = ops.mjpeg_encode_to_host(u8, 90)
frame = u8[5].cpu().numpy()
assert data[off[5]:off[6]] == R.encode_frame(frame, -1, 0)["stream"]
say(f"  frame 5 equals the mirror byte for byte ({off[6] - off[5]} bytes)")
say(f"  batch of 16 clips: raw {raw} B; apng streams adaptive {off[-1]} B ({off[-1] / raw:.4f} of raw), Sub {off_sub[-1]} B ({off_sub[-1] / raw:.4f}); "
    f"mjpeg 4:4:4 q90 scans {off_jpg[-1]} B ({off_jpg[-1] / raw:.4f})")
ours = huff = lvl6 = pil = 0
try:
    from PIL import Image
except ImportError:
    Image = None
for k in range(0, 256, 32):
    f = u8[k].cpu().numpy()
    filtered = R.filter_rows(f, -1)[0].tobytes()
    assert zlib.decompress(data[off[k]:off[k + 1]]) == filtered
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
    huff += len(c.compress(filtered) + c.flush())
    lvl6 += len(zlib.compress(filtered, 6))
    ours += off[k + 1] - off[k]
    if Image is not None:
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, format="PNG")
        pil += buf.tell()
say(f"  eight frames: ours {ours} B; zlib Huffman-only on the same filtered bytes {huff} B (ours / it {ours / huff:.4f}); zlib level 6 {lvl6} B "
    f"({ours / lvl6:.4f}); Pillow's default PNG files {pil} B ({ours / pil:.4f})" if pil else f"  eight frames: ours {ours} B; zlib Huffman-only {huff} B; level 6 {lvl6} B")
say("done")
