"""Times the PNG decoder on one GPU for profiles/png_decode.txt.  The batch is that of tools/apng_bench.py: 16 clips x
16 frames of 256 x 256 (a smooth field shifted per frame plus noise), (a) as the zlib streams `ops.png_encode` makes of it (Huffman-only
deflate: every byte a literal) and (b) as the streams of Pillow's default PNG files of the same pixels (zlib level 6: LZ77 matches).

  device   HIP events around the call, median of 30 after 5 warm-up calls, two series, the forms alternating: `ccvs_png_decode` (inflate
           and un-filter) and `ccvs_zlib_inflate` alone on the same streams, the blob already on the device;
  host     wall clock around `ops.png_decode` from host bytes (pack, one upload, decode, the status read-back) and a synchronise; for
           context `tools.apng.read_apng` on the 16 APNG files and Pillow on the 256 PNG files, one thread and 16 threads, and the bytes
           that cross to the device either way;
  profile  (--profile) nothing but ten decodes of each form, for a run under rocprofv3 --kernel-trace --stats.

    python tools/png_decode_bench.py [--profile] [--out FILE]
"""
import ctypes as C
import io
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))
import jpeg_opt_ref as O  # noqa: E402
from ccvs_amd import lib, ops  # noqa: E402
from ccvs_amd.tools import apng  # noqa: E402

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
H = W = 256
base = torch.from_numpy(O._smooth(H, W)).to(dev).float()
u8 = torch.stack([(torch.roll(base, shifts=(k % 61, (3 * k) % 97), dims=(0, 1)) + 4.0 * torch.randn(H, W, 3, device=dev)).clamp(0, 255).to(torch.uint8)
                  for k in range(256)])
host_frames = u8.cpu().numpy()
L = lib.load()
data, off = ops.png_encode_to_host(u8)
own = [data[off[i]:off[i + 1]] for i in range(256)]
try:
    from PIL import Image
except ImportError:
    Image = None
forms = [("own streams   ", own)]
pil_files = []
if Image is not None:
    for f in host_frames:
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, format="PNG")
        pil_files.append(buf.getvalue())
    forms.append(("Pillow streams", [apng.apng_streams(b)[2][0] for b in pil_files]))
say("library", os.path.relpath(lib.LIB_PATH, HERE), "; device", torch.cuda.get_device_name(0), "; frames", tuple(u8.shape), "raw bytes", u8.numel(),
    "; workspace", int(L.ccvs_png_decode_workspace_bytes(256, H, W)), "bytes")

frames_out = torch.empty(256, H, W, 3, dtype=torch.uint8, device=dev)
status = torch.empty(256, dtype=torch.int32, device=dev)
work = torch.empty(int(L.ccvs_png_decode_workspace_bytes(256, H, W)), dtype=torch.uint8, device=dev)
fb = H * (3 * W + 1)
calls = []
for name, streams in forms:
    meta, blob = ops.png_decode_pack(streams, H, W)
    meta["blob"] = torch.from_numpy(blob).to(dev)
    rows4 = np.ascontiguousarray([(r[0], r[1], i * fb, fb) for i, r in enumerate(meta["rows_host"].tolist())], dtype=np.int64)
    rows4_dev = torch.from_numpy(rows4).to(dev)

    def decode(meta=meta):
        ops.png_decode_uploaded(meta, frames_out, status, work)

    def inflate(meta=meta, rows4=rows4, rows4_dev=rows4_dev):
        lib.check(L.ccvs_zlib_inflate(C.c_void_p(meta["blob"].data_ptr() + meta["o_data"]), meta["data_bytes"], C.c_void_p(rows4_dev.data_ptr()),
                                      rows4.ctypes.data_as(C.c_void_p), 256, C.c_void_p(work.data_ptr()), 256 * fb, C.c_void_p(status.data_ptr()),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ccvs_zlib_inflate")
    decode()
    assert not status.any() and torch.equal(frames_out, u8), name
    calls.append((name, streams, decode, inflate, blob.nbytes))

if "--profile" in sys.argv:
    for name, streams, decode, inflate, nbytes in calls:
        for _ in range(10):
            decode()
    torch.cuda.synchronize()
    say("done")
    sys.exit(0)

for series in range(2):
    for name, streams, decode, inflate, nbytes in calls:
        say(f"device  {name} inflate + un-filter series {series}: {fmt(timed(decode))}")
        say(f"device  {name} inflate alone       series {series}: {fmt(timed(inflate))}")
for series in range(2):
    for name, streams, decode, inflate, nbytes in calls:
        say(f"from host bytes {name} ops.png_decode (pack, upload, decode, status) series {series}: {fmt(walled(lambda: ops.png_decode(streams, H, W)))}")
    say(f"from host bytes raw frames .cuda()                                        series {series}: {fmt(walled(lambda: torch.from_numpy(host_frames).cuda()))}")
for name, streams, decode, inflate, nbytes in calls:
    say(f"  {name}: {sum(len(s) for s in streams)} B of streams, {nbytes} B uploaded ({nbytes / u8.numel():.4f} of the raw frames' {u8.numel()} B)")

# the host decoders on the same files, for context
with tempfile.TemporaryDirectory() as tmp:
    clips = []
    for c in range(16):
        clips.append(os.path.join(tmp, f"vid_{c:05d}.png"))
        apng.write_apng(clips[-1], own[16 * c:16 * c + 16], 4, H, W)
    assert np.array_equal(apng.read_apng(clips[3]), host_frames[48:64])
    assert torch.equal(ops.read_apng_clips(clips).view(256, H, W, 3), u8)
    pool = ThreadPoolExecutor(16)
    say(f"host    read_apng, 16 APNG files of 16 frames, one thread : {fmt(walled(lambda: [apng.read_apng(p) for p in clips], reps=3, warm=1))}")
    say(f"host    read_apng, 16 APNG files of 16 frames, 16 threads : {fmt(walled(lambda: list(pool.map(apng.read_apng, clips)), reps=3, warm=1))}")
    say(f"device  ops.read_apng_clips on the same 16 files           : {fmt(walled(lambda: ops.read_apng_clips(clips), reps=5, warm=1))}")
    if Image is not None:
        files = []
        for i, b in enumerate(pil_files):
            files.append(os.path.join(tmp, f"{i:03d}.png"))
            with open(files[-1], "wb") as f:
                f.write(b)
        pil = lambda p: np.asarray(Image.open(p).convert("RGB"))
        say(f"host    Pillow, 256 PNG files, one thread : {fmt(walled(lambda: [pil(p) for p in files], reps=3, warm=1))}")
        say(f"host    Pillow, 256 PNG files, 16 threads : {fmt(walled(lambda: list(pool.map(pil, files)), reps=5, warm=1))}")
    pool.shutdown()
say("done")
