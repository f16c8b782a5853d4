"""Time the video-file datasets' transform kernel (`ops.ingest_f32`), fused against staged, at the two real
geometries:

  kinetics  16 clips x 16 frames of 64 x 64 -> Resize(256) 256 x 256 -> Resize(64) 64 x 64, ImageNet normalisation;
  ucf101    2 clips x 16 frames of 240 x 320 -> Resize(256) 256 x 341 -> CenterCrop(256), 0.5 / 0.5 normalisation.

Per case and form: HIP events around 20 back-to-back `ops.ingest_f32` calls through the Python wrapper (warm, median and best of 50
windows -- the bracket of tools/to_rgb_bench.py), the intermediate fp32 tensor the staged form writes and reads, and whether the two
forms gave the same bits.  The calls go through the wrapper, as the loader's do, so a form's launches count with their host cost.

    python tools/video_ingest_bench.py > profiles/video_ingest_bench.txt"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccvs_amd import ops  # noqa: E402
from ccvs_amd.data.transform_plan import IMAGENET_MEAN, IMAGENET_STD, resize_target  # noqa: E402
from to_rgb_bench import timed  # noqa: E402


def case(name, n, hs, ws, stages, mean, std):
    rng = np.random.RandomState(1)
    u8 = torch.from_numpy(rng.randint(0, 256, size=(n, hs, ws, 3)).astype(np.uint8)).cuda()
    rows = ops.ingest_stages(hs, ws, stages)
    ho, wo = rows[-1][4:]
    out = {form: torch.empty(n, 3, ho, wo, device="cuda") for form in ("fused", "staged")}
    row = {"case": name, "frames": n, "src": [hs, ws], "stages": rows, "out": [ho, wo], "MB_u8_in": u8.numel() / 1e6,
           "MB_f32_out": 4 * n * 3 * ho * wo / 1e6, "MB_f32_intermediate_staged": sum(4 * n * 3 * r[4] * r[5] for r in rows[:-1]) / 1e6}
    for form in ("fused", "staged"):
        fn = lambda: ops.ingest_f32(u8, stages, out=out[form], pre="div255", mean=mean, std=std, fused=form == "fused")
        fn()
        row[form + "_ms"], row[form + "_best_ms"] = timed(fn, reps=50, inner=20)
    row["same_bits"] = bool(torch.equal(out["fused"].view(torch.int32), out["staged"].view(torch.int32)))
    print(f"{name:9s} {n} x {hs}x{ws} -> {' -> '.join(f'{r[4]}x{r[5]}' for r in rows)}   fused {row['fused_ms']:.4f} ms (best {row['fused_best_ms']:.4f})   "
          f"staged {row['staged_ms']:.4f} ms (best {row['staged_best_ms']:.4f}, {len(rows)} launches, {row['MB_f32_intermediate_staged']:.1f} MB of fp32 "
          f"intermediate written and read)   uint8 in {row['MB_u8_in']:.1f} MB, fp32 out {row['MB_f32_out']:.1f} MB   same bits: {row['same_bits']}")
    return row


def main():
    assert torch.cuda.is_available(), "video_ingest_bench measures on the GPU"
    rows = [case("kinetics", 256, 64, 64, [(None, (256, 256)), (None, (64, 64))], IMAGENET_MEAN, IMAGENET_STD)]
    h, w = resize_target(240, 320, 256)
    left = int(round((w - 256) / 2.))
    rows.append(case("ucf101", 32, 240, 320, [(None, (h, w)), ((0, left, 256, 256), None)], (0.5,) * 3, (0.5,) * 3))
    print(json.dumps({"cases": rows}))


if __name__ == "__main__":
    main()
