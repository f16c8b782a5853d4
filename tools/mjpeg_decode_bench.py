"""Times the JPEG decoder on one GPU for profiles/mjpeg_decode.txt: 16 clips x 16 frames of 256 x 256 written by
`save_video_batch(..., video_format="avi")` at quality 90 (restart interval 32 MCUs: 8192 units), then
  1. `ccvs_mjpeg_decode` alone on the uploaded plan (device events);
  2. file to pixels on the device: `ops.read_avi_clips` = read, parse, upload, decode (host clock, ends in a synchronise);
  3. beside them, where Pillow imports: `mjpeg.decode_frames` on 16 threads plus the upload of the pixels;
  4. the same frames as files without restart markers (Pillow writes them: one unit per frame), decode call alone.
Synthetic frames as in tools/mjpeg_bench.py; the decoded clips are checked against Pillow's where it imports.
    python tools/mjpeg_decode_bench.py [--out FILE] [--decode-only]       (--decode-only: step 1 alone, for a kernel trace)"""
import io
import os
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import jpeg_ref as R
from ccvs_amd import ops
from ccvs_amd.helpers.generator import save_video_batch
from ccvs_amd.tools import mjpeg

out = open(sys.argv[sys.argv.index("--out") + 1], "w") if "--out" in sys.argv else None
decode_only = "--decode-only" in sys.argv


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if out is not None:
        out.write(line + "\n")
        out.flush()


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


torch.manual_seed(0)
dev = torch.device("cuda")
base = torch.from_numpy(R._smooth(256, 256)).to(dev).float()
frames = []
for k in range(256):
    f = torch.roll(base, shifts=(k % 61, (3 * k) % 97), dims=(0, 1)) + 4.0 * torch.randn(256, 256, 3, device=dev)
    frames.append(f.clamp(0, 255).to(torch.uint8))
u8 = torch.stack(frames)
tmp = tempfile.mkdtemp(prefix="mjpeg_decode_bench_")
vid = (u8.view(16, 16, 256, 256, 3).permute(0, 1, 4, 2, 3).float() / 127.5 - 1.0).contiguous()
save_video_batch(vid, 16, 0, tmp, 4, True, False, [-1, 1], "bairhd", video_format="avi", return_clip=False)
paths = [os.path.join(tmp, n) for n in sorted(os.listdir(tmp))]
files = [f for p in paths for f in mjpeg.read_avi(p)[3]]
say("device", torch.cuda.get_device_name(0), "; files", len(paths), "frames", len(files), "bytes", sum(len(f) for f in files), "-> pixels", u8.numel())

plan = mjpeg.plan_frames(files)
up = ops.mjpeg_decode_upload(plan)
pixels, status = ops.mjpeg_decode_uploaded(up)
work = torch.empty(max(ops._lib.load().ccvs_mjpeg_decode_workspace_bytes(256, 256, 256, 0), 16), dtype=torch.uint8, device=dev)
assert not status.any()
ms = timed(lambda: ops.mjpeg_decode_uploaded(up, pixels, status, work), 20)
say(f"1. ccvs_mjpeg_decode alone ({plan['units'].shape[0]} units, {plan['tables'].size // 4008} table record(s), buffers preallocated): device events around the call "
    f"(memset + 3 kernels): {fmt(ms)}; {u8.numel() / statistics.median(ms) / 1e6:.1f} GB/s of pixels")
if decode_only:
    shutil.rmtree(tmp)
    say("done")
    sys.exit(0)

say("2. file to pixels on the device (ops.read_avi_clips: read 16 files, parse 256 frames, one upload, one decode, status read back):",
    fmt(host_timed(lambda: ops.read_avi_clips(paths), 10)))
say("   of which the host's parse + unit tables + table records (mjpeg.plan_frames):", fmt(host_timed(lambda: mjpeg.plan_frames(files), 10)))
try:
    from PIL import Image
except ImportError:
    Image = None
if Image is None:
    say("3. Pillow is not installed here: decode_frames not measured")
    say("4. files without restart markers need Pillow to write them: not measured")
else:
    pool = ThreadPoolExecutor(16)
    def pillow():
        clips = list(pool.map(lambda p: mjpeg.decode_frames(mjpeg.read_avi(p)[3]), paths))
        return torch.from_numpy(np.stack(clips)).to(dev)
    ref = pillow()
    assert torch.equal(ref.view(256, 256, 256, 3), pixels), "the GPU decoder's pixels differ from Pillow's"
    say("   the 256 decoded frames equal Pillow's byte for byte")
    say("3. Pillow beside it (mjpeg.decode_frames per file on 16 threads, np.stack, one upload):", fmt(host_timed(pillow, 10)))
    plain = []
    for f in ref.view(256, 256, 256, 3).cpu().numpy():
        buf = io.BytesIO()
        Image.fromarray(f, "RGB").save(buf, format="JPEG", quality=90, subsampling=0)
        plain.append(buf.getvalue())
    plan1 = mjpeg.plan_frames(plain)
    up1 = ops.mjpeg_decode_upload(plan1)
    ms1 = timed(lambda: ops.mjpeg_decode_uploaded(up1, pixels, status[:256], work), 10)
    assert not status[:256].any()
    say(f"4. the same call on files without restart markers ({plan1['units'].shape[0]} units of 1024 MCUs, Pillow's files at quality 90): {fmt(ms1)}; "
        f"{statistics.median(ms1) / statistics.median(ms):.1f} x the time with 32-MCU units")
shutil.rmtree(tmp)
say("done")
