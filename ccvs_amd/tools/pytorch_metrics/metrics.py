"""PSNR / SSIM of generated clips against the real ones, on the GPU that produced them
(mirror of the reference's tools/pytorch_metrics/metrics.py).

Same function names and argument meaning as the reference:

  get_psnr(x, y)      piq.psnr(x, y, data_range=1., reduction='mean')                       metrics.py:24-25 -> ccvs_psnr
  get_ssim(x, y)      mean over images of the mean over the 3 channel planes of
                      skimage.metrics.structural_similarity (scikit-image 0.17.2 defaults)  metrics.py:15-22 -> ccvs_ssim
  upscale(videos)     F.interpolate(..., mode='bilinear') up to 161 pixels                  metrics.py:115-124 -> ccvs_resize_bilinear
  metrics_from_files  the batching / aggregation of metrics.py:27-78; `metrics_from_videos` is the same loop on uint8 tensors
                      [N, T, H, W, 3] such as `save_video_batch` packs.  Files named .avi (the Motion-JPEG files `--video_format avi`
                      writes) or .npy are loaded by `load_videos` below, on the GPU; for .mp4 the caller brings a `loader=` (the
                      reference's decoder is OpenCV, absent here).
  load_video(s)       metrics.py:80-97: .avi through `read_avi` and `ops.mjpeg_decode` (the JPEG decoder in HIP, DESIGN.md section
                      4.16: libjpeg's pixels), .npy the uint8 [T, H, W, 3] arrays `run()` writes, .png the lossless animated PNGs of
                      `--video_format apng` (`tools.apng.read_apng`: inflated and un-filtered on the host, or with png_decode="gpu" on
                      the device by `ops.read_apng_clips`, DESIGN.md sections 4.22 and 4.23 -- the exact clips, so the scores are those of the clips the model produced); the clips stay on the device.
                      `resize` other than None raises NotImplementedError (the reference's is OpenCV INTER_AREA, not reproduced).
  get_video_files, get_folder(s), print_scores, main, and the argparse block      metrics.py:92-186:
                      python -m ccvs_amd.tools.pytorch_metrics.metrics --exp_tag TAG [--real_tag --real_folder --fake_folder
                      --num_folds --idx --print_256 --lpips_weights] prints the reference's lines for results/*TAG/{real,fake};
                      without LPIPS weights the LPIPS lines say "not available (needs pretrained weights)".
  get_lpips(x, y)     piq.LPIPS(reduction='mean')(x, y)                                     metrics.py:12-13 -> lpips.LPIPS
                      piq downloads a pretrained VGG16 and learned linear heads; nothing is downloaded here and no weights are in
                      the repository, so the user names a file: `set_lpips_weights(path | dict | None)`, the environment variable
                      CCVS_LPIPS_WEIGHTS (read on first use), or `--lpips_weights PATH` of the command.  The file is what
                      `python -m ccvs_amd.tools.pytorch_metrics.lpips --vgg ... --lin ... --out ...` writes (lpips.py has the
                      algorithm).  Without weights get_lpips raises NotImplementedError, before it looks at its arguments, and the
                      aggregate functions return None in its place.  Parity with piq itself is not pinned (piq is not installed
                      where the tests run), as for PSNR and SSIM: the float64 mirror tests/lpips_ref.py is.

x, y: [N, 3, H, W] fp32 CUDA tensors in [0, 1].  No CPU fallback: the kernels live in libccvs_hip.so.
"""
import argparse
import os
from glob import glob

import numpy as np
import torch

from ccvs_amd import ops


_LPIPS_SOURCE = None   # what `set_lpips_weights` was given; None: the environment variable, if it is set
_LPIPS_MODEL = None    # the lpips.LPIPS built from it on first use


def set_lpips_weights(weights):
    """Configure LPIPS for this process: a weight file's path, the dict `lpips.load_lpips_weights` takes, or None (no weights: the
    environment variable CCVS_LPIPS_WEIGHTS, if set, is read on the next use).  The network is built on first use."""
    global _LPIPS_SOURCE, _LPIPS_MODEL
    _LPIPS_SOURCE, _LPIPS_MODEL = weights, None


def _lpips_model():
    """The configured lpips.LPIPS, or None without weights."""
    global _LPIPS_MODEL
    if _LPIPS_MODEL is None:
        source = _LPIPS_SOURCE if _LPIPS_SOURCE is not None else (os.environ.get("CCVS_LPIPS_WEIGHTS") or None)
        if source is None:
            return None
        from ccvs_amd.tools.pytorch_metrics.lpips import LPIPS
        _LPIPS_MODEL = LPIPS(source)
    return _LPIPS_MODEL


def get_lpips(x, y):
    """metrics.py:12-13, from the weights `set_lpips_weights` / CCVS_LPIPS_WEIGHTS name: a 0-dim fp32 device tensor."""
    model = _lpips_model()
    if model is None:
        raise NotImplementedError("LPIPS needs piq's pretrained VGG16 + linear-head weights (downloaded by piq.LPIPS); none are configured: "
                                  "name a weight file with set_lpips_weights, CCVS_LPIPS_WEIGHTS or --lpips_weights")
    return model(x, y)


def get_ssim(x, y):
    """metrics.py:15-22.  Returns a 0-dim float64 tensor like the reference's `torch.tensor(ssim)`."""
    s = ops.ssim_planes(x, y, data_range=2.0)     # [N, 3] float64; float planes and no data_range: skimage 0.17.2 takes dmax - dmin = 2
    return s.mean(dim=1).mean().cpu()              # (sum of three planes) / 3 per image, then / N


def get_psnr(x, y):
    """metrics.py:24-25."""
    return ops.psnr(x, y, data_range=1.0).mean()


def upscale(videos, min_size=161):
    """metrics.py:115-124."""
    h, w = videos.shape[-2:]
    if h >= min_size and w >= min_size:
        return videos
    size = [min_size, int(min_size * w / h)] if h < w else [int(min_size * h / w), min_size]
    return ops.resize_bilinear(videos, size)


def _scores(real_videos, generated_videos, idx, lpips, ssim, psnr):
    """One batch of metrics.py:46-59: real_videos / generated_videos [B, T, H, W, 3] in [0, 1].  lpips: the LPIPS lists, or None
    without weights."""
    if len(idx) == 0:
        real = real_videos.view(-1, *real_videos.shape[2:]).permute(0, 3, 1, 2).contiguous()
        fake = generated_videos.view(-1, *generated_videos.shape[2:]).permute(0, 3, 1, 2).contiguous()
        if lpips is not None:
            lpips.append(get_lpips(real, fake).cpu())
        ssim.append(get_ssim(real, fake).cpu())
        psnr.append(get_psnr(real, fake).cpu())
    else:
        for k, frame_idx in enumerate(idx):
            real = upscale(real_videos[:, frame_idx].permute(0, 3, 1, 2).contiguous())
            fake = upscale(generated_videos[:, frame_idx].permute(0, 3, 1, 2).contiguous())
            if lpips is not None:
                lpips[k].append(get_lpips(real, fake).cpu())
            ssim[k].append(get_ssim(real, fake).cpu())
            psnr[k].append(get_psnr(real, fake).cpu())


def _aggregate(ssim, psnr, print_256, idx, batch_size, lpips=None):
    """metrics.py:61-78.  lpips: the LPIPS lists; None without weights -- LPIPS is then left out of the line and returned as None."""
    lpips_m = None
    if print_256 and len(idx) == 0:
        ssim = torch.stack(ssim).view(-1, 256 // batch_size)
        psnr = torch.stack(psnr).view(-1, 256 // batch_size)
        ssim_m, psnr_m = ssim.mean(), psnr.mean()
        head = ""
        if lpips is not None:
            lpips = torch.stack(lpips).view(-1, 256 // batch_size)
            lpips_m = lpips.mean()
            head = f"LPIPS is: {lpips_m} (+- {lpips.mean(1).std()}), "
        print(f"(256) {head}SSIM is {ssim_m} (+- {ssim.mean(1).std()}), PSNR is {psnr_m} (+- {psnr.mean(1).std()})")
    elif len(idx) == 0:
        ssim_m, psnr_m = torch.stack(ssim).mean(), torch.stack(psnr).mean()
        if lpips is not None:
            lpips_m = torch.stack(lpips).mean()
    else:
        ssim_m = [torch.stack(e).mean() for e in ssim]
        psnr_m = [torch.stack(e).mean() for e in psnr]
        if lpips is not None:
            lpips_m = [torch.stack(e).mean() for e in lpips]
    return lpips_m, ssim_m, psnr_m


def _lpips_lists(idx):
    """The LPIPS lists of a run of the loop, or None without weights."""
    if _lpips_model() is None:
        return None
    return [] if len(idx) == 0 else [[] for _ in idx]


def metrics_from_videos(real_videos_u8, generated_videos_u8, print_256=False, idx=(), batch_size=16, device="cuda"):
    """The loop of `metrics_from_files` on clips already in memory: uint8 [N, T, H, W, 3] (numpy or torch), batches of 16 as in the
    reference (a ragged tail is dropped like its `total_size // batch_size`).  Returns (lpips, ssim, psnr); lpips is None without
    LPIPS weights (`set_lpips_weights`)."""
    idx = list(idx)
    total = len(real_videos_u8)
    assert len(generated_videos_u8) == total
    ssim, psnr = ([], []) if len(idx) == 0 else ([[] for _ in idx], [[] for _ in idx])
    lpips = _lpips_lists(idx)
    with torch.no_grad():
        for i in range(total // batch_size):
            sl = slice(i * batch_size, min((i + 1) * batch_size, total))
            real = torch.as_tensor(real_videos_u8[sl]).to(device) / 255
            fake = torch.as_tensor(generated_videos_u8[sl]).to(device) / 255
            _scores(real, fake, idx, lpips, ssim, psnr)
    return _aggregate(ssim, psnr, print_256, idx, batch_size, lpips)


def metrics_from_files(real_video_files, generated_video_files, resize, num_workers, print_256, idx, loader=None, png_decode="host"):
    """metrics.py:27-78.  png_decode: where `load_videos` decodes .png clips ("host" or "gpu").  loader: `loader(files, resize) -> uint8 [B, T, H, W, 3]` (numpy or torch) in place of `load_videos`; it is
    needed for .mp4 names only -- the reference decodes those with OpenCV (metrics.py:80-97), which this image does not have, so
    without a loader they raise."""
    if loader is None:
        if any(os.path.splitext(str(f))[1].lower() not in (".avi", ".npy", ".png") for f in list(real_video_files) + list(generated_video_files)):
            raise RuntimeError("metrics_from_files: no mp4 decoder here (the reference uses OpenCV); pass loader=..., or call "
                               "metrics_from_videos on the uint8 clips")
        loader = lambda files, size: load_videos(files, size, num_workers, png_decode=png_decode)  # noqa: E731
    batch_size = 16
    total = len(real_video_files)
    ssim, psnr = ([], []) if len(idx) == 0 else ([[] for _ in idx], [[] for _ in idx])
    lpips = _lpips_lists(idx)
    with torch.no_grad():
        for i in range(total // batch_size):
            sl = slice(i * batch_size, min((i + 1) * batch_size, total))
            real = torch.as_tensor(loader(real_video_files[sl], resize)).cuda() / 255
            fake = torch.as_tensor(loader(generated_video_files[sl], resize)).cuda() / 255
            _scores(real, fake, idx, lpips, ssim, psnr)
    return _aggregate(ssim, psnr, print_256, idx, batch_size, lpips)


def load_video(file, resize):
    """metrics.py:80-90: uint8 [T, H, W, 3] on the device of one .avi (Motion-JPEG, decoded on the GPU) or .npy file."""
    return load_videos([file], resize, 1)[0]


def get_video_files(folder):
    """metrics.py:92-93, for the kinds of file a run writes here: the folder's *.mp4, else its *.avi, else its *.npy, else its *.png
    (the animated PNGs of `--video_format apng`), sorted."""
    for ext in ("mp4", "avi", "npy", "png"):
        files = sorted(glob(os.path.join(folder, "*." + ext)))
        if files:
            return files
    return []


def load_videos(video_files, resize, num_workers, png_decode="host"):
    """metrics.py:95-97: uint8 [B, T, H, W, 3] on the device.  The .avi files of a batch are decoded by one call; `num_workers` is
    accepted and unused (the files are read by this process, the frames decoded by the GPU).  png_decode: "host" inflates and
    un-filters the .png clips of a batch with zlib and numpy and uploads the frames; "gpu" uploads their zlib streams and decodes all
    frames of the batch in one call (`ops.read_apng_clips`) -- the same bytes either way."""
    if png_decode not in ("host", "gpu"):
        raise ValueError(f"load_videos: png_decode is 'host' or 'gpu', not {png_decode!r}")
    if resize is not None:
        raise NotImplementedError("load_videos: resize is OpenCV's INTER_AREA in the reference, which is not reproduced here; pass resize=None")
    kinds = {os.path.splitext(str(f))[1].lower() for f in video_files}
    if kinds == {".avi"}:
        return ops.read_avi_clips([str(f) for f in video_files])
    if kinds == {".npy"}:
        clips = [np.load(str(f)) for f in video_files]
        for f, c in zip(video_files, clips):
            if c.dtype != np.uint8 or c.ndim != 4 or c.shape[-1] != 3 or c.shape != clips[0].shape:
                raise ValueError(f"load_videos: {f} holds {c.dtype} {c.shape}, not a uint8 [T, H, W, 3] clip of the batch's shape")
        return torch.from_numpy(np.stack(clips)).cuda()
    if kinds == {".png"} and png_decode == "gpu":
        return ops.read_apng_clips([str(f) for f in video_files])
    if kinds == {".png"}:                                               # the lossless clips: inflated and un-filtered on the host, one upload
        from ccvs_amd.tools.apng import read_apng
        clips = [read_apng(str(f)) for f in video_files]
        for f, c in zip(video_files, clips):
            if c.shape != clips[0].shape:
                raise ValueError(f"load_videos: {f} holds a clip of shape {c.shape}, not the batch's {clips[0].shape}")
        return torch.from_numpy(np.stack(clips)).cuda()
    raise RuntimeError(f"load_videos: files of kind(s) {sorted(kinds)}: one batch is all .avi or all .npy or all .png (no mp4 decoder here)")


def get_folder(exp_tag, fold_i=None):
    """metrics.py:99-104."""
    if fold_i is not None:
        exp_tag += f"_{fold_i}"
    all_folders = glob(f"results/*{exp_tag}")
    assert len(all_folders) == 1, f"Too many possibilities for this tag {exp_tag}:\n{all_folders}"
    return all_folders[0]


def get_folders(exp_tag, num_folds):
    """metrics.py:106-113."""
    if num_folds is not None:
        return [get_folder(exp_tag, i) for i in range(num_folds)]
    return [get_folder(exp_tag)]


def print_scores(scores, name):
    """metrics.py:126-130; a metric that is not available here (LPIPS: its scores are None) says so instead of a number."""
    if any(s is None for s in scores):
        print(f"{name} scores: not available (needs pretrained weights)")
        return
    print(f"Individual {name} scores")
    print(scores)
    print(f"Mean/std of {name} across {len(scores)} runs")
    print(np.mean(scores), np.std(scores))


def main(args):
    """metrics.py:132-172."""
    if getattr(args, "lpips_weights", None):
        set_lpips_weights(args.lpips_weights)
    fake_folders = get_folders(args.exp_tag, args.num_folds)
    real_tag = args.exp_tag if args.real_tag is None else args.real_tag
    real_folders = get_folders(real_tag, args.num_folds)

    if len(args.idx) == 0:
        lpips, ssim, psnr = [], [], []
    else:
        lpips, ssim, psnr = [[] for _ in args.idx], [[] for _ in args.idx], [[] for _ in args.idx]
    for i, (real_root, fake_root) in enumerate(zip(sorted(real_folders), sorted(fake_folders))):
        print(f"[{i}] Loading real")
        real_video_files = get_video_files(os.path.join(real_root, args.real_folder))
        print(f"Found {len(real_video_files)} {args.real_folder} video files")

        print(f"[{i}] Loading fake")
        fake_video_files = get_video_files(os.path.join(fake_root, args.fake_folder))
        print(f"Found {len(fake_video_files)} {args.fake_folder} video files")

        assert len(real_video_files) == len(fake_video_files)

        print(f"[{i}] Computing metrics")
        lpips_i, ssim_i, psnr_i = metrics_from_files(real_video_files, fake_video_files, args.resize, args.num_workers, args.print_256, args.idx,
                                                      png_decode=getattr(args, "png_decode", "host"))
        if len(args.idx) == 0:
            lpips.append(lpips_i)
            ssim.append(ssim_i)
            psnr.append(psnr_i)
        else:
            for k in range(len(args.idx)):
                lpips[k].append(None if lpips_i is None else lpips_i[k])
                ssim[k].append(ssim_i[k])
                psnr[k].append(psnr_i[k])

    if len(args.idx) == 0:
        print_scores(lpips, "LPIPS")
        print_scores(ssim, "SSIM")
        print_scores(psnr, "PSNR")
    else:
        for k in range(len(args.idx)):
            print_scores(lpips[k], f"LPIPS-{k}")
            print_scores(ssim[k], f"SSIM-{k}")
            print_scores(psnr[k], f"PSNR-{k}")


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--exp_tag', type=str, default=None)
    parser.add_argument('--real_tag', type=str, default=None)
    parser.add_argument('--real_folder', type=str, default="real")
    parser.add_argument('--fake_folder', type=str, default="fake")
    parser.add_argument('--num_folds', type=int, default=None)
    parser.add_argument('--idx', type=int, nargs="+", default=[])
    parser.add_argument('--num_workers', type=int, default=8)
    parser.add_argument('--print_256', action='store_true')
    parser.add_argument('--resize', type=int, nargs="+", default=None)
    parser.add_argument('--lpips_weights', type=str, default=None, help="the LPIPS weight file (tools/pytorch_metrics/lpips.py writes it)")
    parser.add_argument('--png_decode', type=str, default="host", choices=("host", "gpu"),
                        help="where .png clips are inflated and un-filtered: host (zlib and numpy) or gpu (one decode call per batch); the same bytes")
    return parser.parse_args(argv)


if __name__ == "__main__":
    main(parse_args())
