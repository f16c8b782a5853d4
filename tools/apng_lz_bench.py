"""Measures the lossless output stage with LZ77 matches against the default writer on one GPU, for
profiles/apng_lz.txt.  Times of device work are HIP-event medians around the call, two series each, the forms alternating in one
process (the difference between the series of one form is the run-to-run spread); times that include the copy to the host are
wall-clock medians around the call and a synchronise.

  smooth   the batch of tools/apng_bench.py: 16 clips x 16 frames of 256 x 256, a smooth field shifted per frame plus noise -- content
           on which matches do not pay, so the per-band choice is expected to fall back to literal-only almost everywhere;
  pasted   the same clips with a flat border of 24 pixels and a flat object of 96 x 80 pixels that moves per frame: real matches.
  Per batch: `ops.png_encode` with lz77 off and on, `png_encode_to_host` both ways, the batch's bytes both ways, and on eight frames
  zlib's Huffman-only, Z_RLE and level-6 streams of the same filtered bytes, Pillow's default PNG, and the mirror: the same bytes, and
  how many of the bands took the match block.
  profile  (--profile) nothing but ten lz77 encodes of each batch, for a run under rocprofv3 --kernel-trace --stats.

    python tools/apng_lz_bench.py [--profile] [--out FILE]
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
import apng_lz_ref as Z  # noqa: E402
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
smooth = torch.stack([(torch.roll(base, shifts=(k % 61, (3 * k) % 97), dims=(0, 1)) + 4.0 * torch.randn(256, 256, 3, device=dev)).clamp(0, 255).to(torch.uint8)
                      for k in range(256)])
pasted = smooth.clone()
pasted[:, :24] = pasted[:, -24:] = 16
pasted[:, :, :24] = pasted[:, :, -24:] = 16
for k in range(256):
    y, x = 40 + (5 * k) % 80, 40 + (7 * k) % 90
    pasted[k, y:y + 80, x:x + 96] = torch.tensor([200, 60, 30], dtype=torch.uint8, device=dev)
raw = smooth.numel()
L = lib.load()
stream = torch.empty(int(L.ccvs_apng_stream_bound(256, 256, 256, 0)), dtype=torch.uint8, device=dev)
say("library", os.path.relpath(lib.LIB_PATH, HERE), "; device", torch.cuda.get_device_name(0), "; frames", tuple(smooth.shape), "raw bytes", raw,
    "; workspace", int(L.ccvs_apng_workspace_bytes(256, 256, 256, 0)), "bytes, with lz77", int(L.ccvs_apng_lz_workspace_bytes(256, 256, 256, 0)))
batches = (("smooth", smooth), ("pasted", pasted))

if "--profile" in sys.argv:
    for _, u8 in batches:
        for _ in range(10):
            ops.png_encode(u8, -1, out=stream, lz77=True)
    torch.cuda.synchronize()
    say("done")
    sys.exit(0)


for tag, u8 in batches:
    forms = ((f"{tag} lz77 off", lambda: ops.png_encode(u8, -1, out=stream)), (f"{tag} lz77 on ", lambda: ops.png_encode(u8, -1, out=stream, lz77=True)))
    med = {}
    for series in range(2):
        for name, fn in forms:
            ms = timed(fn)
            med.setdefault(name, []).append(statistics.median(ms))
            say(f"device  {name} series {series}: {fmt(ms)}")
    off_ms, on_ms = (statistics.mean(med[name]) for name, _ in forms)
    say(f"  {tag}: lz77 on / off = {on_ms / off_ms:.2f} (medians {on_ms:.3f} ms / {off_ms:.3f} ms)")
    hosts = ((f"{tag} png_encode_to_host lz77 off", lambda: ops.png_encode_to_host(u8)), (f"{tag} png_encode_to_host lz77 on ", lambda: ops.png_encode_to_host(u8, lz77=True)))
    for series in range(2):
        for name, fn in hosts:
            say(f"to host {name} series {series}: {fmt(walled(fn))}")
    plain, off_p = ops.png_encode_to_host(u8)
    data, off = ops.png_encode_to_host(u8, lz77=True)
    assert all(off[i + 1] - off[i] <= off_p[i + 1] - off_p[i] for i in range(256))
    shrank = sum(off[i + 1] - off[i] < off_p[i + 1] - off_p[i] for i in range(256))
    say(f"  {tag}: raw {raw} B; streams lz77 off {off_p[-1]} B ({off_p[-1] / raw:.4f} of raw), on {off[-1]} B ({off[-1] / raw:.4f} of raw, {off[-1] / off_p[-1]:.4f} of off); "
        f"{shrank} of 256 frames shrank")
    ours = huff = rle = lvl6 = pil = took = bands = 0
    try:
        from PIL import Image
    except ImportError:
        Image = None
    for k in range(0, 256, 32):
        f = u8[k].cpu().numpy()
        filtered = R.filter_rows(f, -1)[0].tobytes()
        assert zlib.decompress(data[off[k]:off[k + 1]]) == filtered
        for strategy in (zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE):
            c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, strategy)
            size = len(c.compress(filtered) + c.flush())
            huff, rle = (huff + size, rle) if strategy == zlib.Z_HUFFMAN_ONLY else (huff, rle + size)
        lvl6 += len(zlib.compress(filtered, 6))
        ours += off[k + 1] - off[k]
        if Image is not None:
            buf = io.BytesIO()
            Image.fromarray(f).save(buf, format="PNG")
            pil += buf.tell()
        m = Z.encode_frame(f, -1, 0)                                     # the mirror: the same bytes, and it says which blocks hold matches
        assert m["stream"] == data[off[k]:off[k + 1]]
        took += m["choice"].count("lz")
        bands += m["bands"]
    say(f"  {tag}, eight frames: lz77 on {ours} B; zlib Huffman-only on the same filtered bytes {huff} B; Z_RLE {rle} B; level 6 {lvl6} B; Pillow's default PNG files {pil} B; "
        f"all eight equal the mirror byte for byte, {took} of their {bands} bands took the match block")
say("done")
