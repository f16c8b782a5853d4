"""Measures the GIF output stage with and without changed-rectangle frames on one GPU for profiles/gif_delta.txt.
Times of device work are HIP-event medians around the call (30 after 5 warm-up calls), two series each, the forms alternating: the
difference between the two series of one form is the run-to-run spread.

  noisy    the batch of tools/gif_bench.py: 16 clips x 16 frames of 256 x 256, a smooth field shifted per frame plus noise -- every pixel of
           every frame changes;
  frozen   a copy whose frames are frame 0 of their clip outside a 96 x 96 box that moves 8 pixels per frame and shows the noisy batch's
           pixels: a static background, one moving object.
  times    `ops.gif_encode` without and with `delta=True`, and `ops.gif_palette` at 256 and 255 colours, on both batches;
  sizes    the payload bytes of both batches without and with the flag, and the share of the later frames written as rectangles; clip 3 of
           the frozen batch equals the mirror (tests/gif_delta_ref.py) byte for byte.

    python tools/gif_delta_bench.py [--out FILE] [--plain-only]

--plain-only measures the flag-less calls alone: the form that also runs in a checkout from before the flag, for the comparison of the
flag-less path across the change (copy this file into that checkout's tools/ and run it there, in the same session).
"""
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))
import jpeg_opt_ref as O  # noqa: E402
from ccvs_amd import lib, ops  # noqa: E402

out = open(sys.argv[sys.argv.index("--out") + 1], "a") if "--out" in sys.argv else None
plain_only = "--plain-only" in sys.argv


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


torch.manual_seed(0)
dev = torch.device("cuda")
base = torch.from_numpy(O._smooth(256, 256)).to(dev).float()
u8 = torch.stack([(torch.roll(base, shifts=(k % 61, (3 * k) % 97), dims=(0, 1)) + 4.0 * torch.randn(256, 256, 3, device=dev)).clamp(0, 255).to(torch.uint8)
                  for k in range(256)])
noisy = u8.view(16, 16, 256, 256, 3)
frozen = noisy[:, :1].repeat(1, 16, 1, 1, 1)
for f in range(1, 16):
    y, x = 20 + 8 * f, 10 + 8 * f
    frozen[:, f, y:y + 96, x:x + 96] = noisy[:, f, y:y + 96, x:x + 96]
batches = (("noisy ", noisy), ("frozen", frozen))
L = lib.load()
stream = torch.empty(int(L.ccvs_gif_stream_bound(256, 256, 256, 0)), dtype=torch.uint8, device=dev)
say("library", os.path.relpath(lib.LIB_PATH, HERE), "; device", torch.cuda.get_device_name(0), "; clips", tuple(noisy.shape), "; plain only" if plain_only else "")

forms = []
for tag, clips in batches:
    forms.append((f"{tag} gif_encode             ", lambda clips=clips: ops.gif_encode(clips, out=stream)))
    forms.append((f"{tag} gif_palette            ", lambda clips=clips: ops.gif_palette(clips)))
    if not plain_only:
        forms.append((f"{tag} gif_encode delta=True  ", lambda clips=clips: ops.gif_encode(clips, out=stream, delta=True)))
        forms.append((f"{tag} gif_palette 255 colours", lambda clips=clips: ops.gif_palette(clips, 255)))
for series in range(2):
    for name, fn in forms:
        say(f"device  {name} series {series}: {fmt(timed(fn))}")

raw = noisy.numel()
for tag, clips in batches:
    _, off, _ = ops.gif_encode_to_host(clips)
    line = f"  {tag}: raw {raw} B; full frames {off[-1]} B ({off[-1] / raw:.4f} of raw)"
    if not plain_only:
        _, off_d, _, rects = ops.gif_encode_to_host(clips, delta=True)
        later = rects.reshape(16, 16, 4)[:, 1:].reshape(-1, 4)
        as_rect = int((later != np.array([0, 0, 256, 256])).any(1).sum())
        line += f"; changed rectangles {off_d[-1]} B ({off_d[-1] / raw:.4f} of raw, {off_d[-1] / off[-1]:.3f} of full); {as_rect} of {len(later)} later frames as rectangles"
    say(line)
if not plain_only:
    import gif_delta_ref as D  # noqa: E402
    data, off, pals, rects = ops.gif_encode_to_host(frozen, delta=True)
    want = D.encode(frozen[3].cpu().numpy(), 0)
    assert data[off[48]:off[64]] == want[0] and np.array_equal(pals[3], want[2]) and np.array_equal(rects[48:64], want[5])
    say(f"  frozen clip 3 equals the mirror byte for byte ({off[64] - off[48]} bytes, {want[4]} colours, rectangles {rects[49].tolist()} ... {rects[63].tolist()})")
say("done")
