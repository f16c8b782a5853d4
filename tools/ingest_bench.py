"""Time the input stage (`ops.ingest_u8`) at two batches of 256 frames (BAIR's 16 clips of 16 frames):

  bair      256 x 256 frames -> 256 x 256: no resample, uint8 HWC -> fp32 planar (one launch);
  resample  240 x 320 frames -> Resize(256) 256 x 341 -> CenterCrop(256) -> fp32 (two launches: the resample to uint8, then the crop +
            convert; the crop follows the resize, so the first launch also resamples the columns the crop drops).

Per case: the kernel time (HIP events around 20 back-to-back calls, warm, median and best of 50), the algorithmic bytes (uint8 frames in
+ fp32 clip out), the GB/s they amount to and their fraction of the chip's 8 TB/s HBM peak; beside them a device-to-device copy of
the fp32 clip (the rate a plain copy reaches), the host-to-device upload of the uint8 and of the fp32 batch from pinned memory, and
the wall time of the same batch through PIL + ToTensor + Normalize on 16 host threads (the reference's per-frame work).  The results of
the GPU path and of the host chain are compared (they must be equal).

    python tools/ingest_bench.py > profiles/ingest_bench.txt"""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccvs_amd import ops  # noqa: E402
from ccvs_amd.data.frame_dataset import resize_target, run_plan  # noqa: E402
from to_rgb_bench import timed  # noqa: E402

HBM_PEAK = 8.0e12
MEAN = STD = (0.5, 0.5, 0.5)


def pil_chain(frames, resize, crop, threads=16):
    """The reference's per-frame transform on the host: (fp32 [N, 3, H, W], wall seconds), or None without Pillow."""
    try:
        from PIL import Image
    except ImportError:
        return None
    mean, std = torch.tensor(MEAN)[:, None, None], torch.tensor(STD)[:, None, None]

    def one(f):
        img = Image.fromarray(f, "RGB")
        if resize is not None:
            img = img.resize((resize[1], resize[0]), Image.BILINEAR)
        if crop is not None:
            img = img.crop((crop[1], crop[0], crop[1] + crop[3], crop[0] + crop[2]))
        t = torch.from_numpy(np.asarray(img)).permute(2, 0, 1).to(torch.float32).div(255)
        return t.sub_(mean).div_(std)

    torch.set_num_threads(1)
    with ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(one, frames[:threads]))
        t0 = time.perf_counter()
        out = list(pool.map(one, frames))
        dt = time.perf_counter() - t0
    return torch.stack(out), dt


def case(name, hs, ws, plan, resize, crop, n=256):
    rng = np.random.RandomState(1)
    host = rng.randint(0, 256, size=(n, hs, ws, 3)).astype(np.uint8)
    pinned = torch.from_numpy(host).pin_memory()
    u8 = pinned.cuda()
    ho, wo = (plan[-1][1] or plan[-1][0][2:]) if plan else (hs, ws)
    clip = torch.empty(n, 3, ho, wo, device="cuda")
    fn = lambda: run_plan(u8, plan, clip, MEAN, STD)
    fn()
    t, best = timed(fn, reps=50, inner=20)
    nbytes = u8.numel() + 4 * clip.numel()
    dst = torch.empty_like(clip)
    t_copy, _ = timed(lambda: dst.copy_(clip), reps=50, inner=20)
    pinned_f32 = torch.empty(clip.shape, dtype=torch.float32).pin_memory()
    t_up8, _ = timed(lambda: u8.copy_(pinned, non_blocking=True), reps=10, inner=2)
    t_up32, _ = timed(lambda: dst.copy_(pinned_f32, non_blocking=True), reps=10, inner=2)
    row = {"case": name, "frames": n, "src": [hs, ws], "out": [ho, wo], "launches": max(1, len(plan)), "ms": t, "best_ms": best,
           "MB_u8_in": u8.numel() / 1e6, "MB_f32_out": 4 * clip.numel() / 1e6, "GBps": nbytes / t / 1e6, "hbm_fraction": nbytes / (t * 1e-3) / HBM_PEAK,
           "copy_f32_clip_ms": t_copy, "copy_GBps_read_plus_written": 8 * clip.numel() / t_copy / 1e6,
           "upload_u8_ms": t_up8, "upload_f32_ms": t_up32}
    ref = pil_chain(host, resize, crop)
    if ref is not None:
        row["pil_16_threads_ms"] = ref[1] * 1e3
        row["equal_to_pil_chain"] = bool(torch.equal(clip.cpu(), ref[0]))
    else:
        row["pil_16_threads_ms"] = None
    print(f"{name:9s} {n} x {hs}x{ws} -> {ho}x{wo}  {row['launches']} launch(es)  {t:.4f} ms (best {best:.4f})  "
          f"{nbytes / 1e6:.1f} MB (uint8 in {row['MB_u8_in']:.1f} + fp32 out {row['MB_f32_out']:.1f})  {row['GBps']:.0f} GB/s = "
          f"{100 * row['hbm_fraction']:.1f} % of 8 TB/s   copy of the fp32 clip {t_copy:.4f} ms ({row['copy_GBps_read_plus_written']:.0f} GB/s read + written)   "
          f"upload uint8 {t_up8:.3f} ms / fp32 {t_up32:.3f} ms   PIL + ToTensor + Normalize, 16 threads: "
          + (f"{row['pil_16_threads_ms']:.1f} ms, equal: {row['equal_to_pil_chain']}" if ref is not None else "not measured (no Pillow)"))
    return row


def main():
    assert torch.cuda.is_available(), "ingest_bench measures on the GPU"
    rows = [case("bair", 256, 256, [], None, None)]
    h, w = resize_target(240, 320, 256)
    left = int(round((w - 256) / 2.))
    rows.append(case("resample", 240, 320, [(None, (h, w)), ((0, left, 256, 256), (256, 256))], (h, w), (0, left, 256, 256)))
    print(json.dumps({"cases": rows}))


if __name__ == "__main__":
    main()
