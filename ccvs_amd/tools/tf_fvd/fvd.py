"""The Frechet Video Distance of generated clips against the real ones, on the GPU (mirror of the reference's tools/tf_fvd/fvd.py).

Same function names and argument meaning as the reference:

  preprocess(videos, target_resolution)   fvd.py:34-51: uint8 [N, T, H, W, 3] -> fp32 [N, T, 3, 224, 224] in [-1, 1]: TF1's
                                          tf.image.resize_bilinear and 2 v / 255 - 1                          -> ops.fvd_prep
  create_id3_embedding(videos)            fvd.py:63-122: the Kinetics-400 RGB I3D's time-averaged logits
                                          (`RGB/inception_i3d/Mean:0`), float64 [N, 400] on the device      -> i3d.I3D
  compute_fvd_given_acts(acts_1, acts_2)  fvd.py:136-143: np.mean, np.cov(rowvar=False) and the Frechet distance, float64 on the host
                                          (`tools.utils.calculate_frechet_distance`, numpy only)
  emb_from_files                          fvd.py:145-173: embeddings in batches of 16, the remainder dropped; `emb_from_videos` is the
                                          same loop on uint8 clips in memory, `fvd_from_videos(real_u8, fake_u8)` their distance.
                                          (The reference's `fvd_from_files` calls `emb_from_files` with an argument missing and cannot
                                          run; it is not mirrored.)
  fvd_size, fvd_full, main, parse_args    fvd.py:216-275: python -m ccvs_amd.tools.tf_fvd.fvd --exp_tag TAG [--real_tag --real_folder
                                          --fake_folder --num_folds --mode size|full|both --size 256 --fvd_weights --channel_order]
                                          prints the reference's lines for results/*TAG/{real,fake}.
  load_videos, get_video_files, get_folder(s)   those of tools/pytorch_metrics/metrics.py: .avi (Motion-JPEG, decoded on the GPU), .npy
                                          and .png (lossless APNG, read on the host) clips; `--resize` raises as it does there (OpenCV's INTER_AREA is not reproduced), and
                                          .mp4 needs a `loader=`.

The network's weights come from TF-Hub in the reference.  Nothing is downloaded here and no weights are in the repository, so the
user names a file: `set_fvd_weights(path | dict | None)`, the environment variable CCVS_FVD_WEIGHTS (read on first use), or
`--fvd_weights PATH`.  The file is what `python -m ccvs_amd.tools.tf_fvd.i3d --state_dict rgb_imagenet.pt --out i3d_kinetics400.pt`
writes (i3d.py has the network).  Without weights everything that needs the network raises NotImplementedError.

Channel order: the reference reads its frames with OpenCV, which gives BGR, and feeds them to the network unconverted -- its published
figures are computed so.  This project's readers give RGB; `channel_order="bgr"` (the default everywhere here) reverses the channels to
reproduce the reference, `"rgb"` feeds the network the order it was trained on.

Parity with TensorFlow itself is not pinned (TensorFlow is not installed where the tests run): the float64 mirror tests/fvd_ref.py is.
No CPU fallback: the kernels live in libccvs_hip.so.
"""
import argparse
import os

import numpy as np
import torch

from ccvs_amd import ops
from ccvs_amd.tools.pytorch_metrics.metrics import get_folder, get_folders, get_video_files, load_video, load_videos  # noqa: F401
from ccvs_amd.tools.utils import calculate_frechet_distance

BATCH_SIZE = 16     # fvd.py:77,147

_FVD_SOURCE = None   # what `set_fvd_weights` was given; None: the environment variable, if it is set
_FVD_MODEL = None    # the i3d.I3D built from it on first use


def set_fvd_weights(weights):
    """Configure the I3D network for this process: a weight file's path, the dict `i3d.load_i3d_weights` takes, an `i3d.I3D` already
    built (another precision or width table), or None (no weights: the environment variable CCVS_FVD_WEIGHTS, if set, is read on the
    next use).  The network is built on first use."""
    global _FVD_SOURCE, _FVD_MODEL
    _FVD_SOURCE, _FVD_MODEL = weights, None


def _fvd_model():
    global _FVD_MODEL
    if _FVD_MODEL is None:
        source = _FVD_SOURCE if _FVD_SOURCE is not None else (os.environ.get("CCVS_FVD_WEIGHTS") or None)
        if source is None:
            raise NotImplementedError("FVD needs the pretrained Kinetics-400 I3D network (the reference downloads it from TF-Hub); no weights "
                                      "are configured: name a weight file with set_fvd_weights, CCVS_FVD_WEIGHTS or --fvd_weights")
        from ccvs_amd.tools.tf_fvd.i3d import I3D
        _FVD_MODEL = source if isinstance(source, I3D) else I3D(source)
    return _FVD_MODEL


def preprocess(videos, target_resolution=(224, 224), channel_order="bgr"):
    """fvd.py:34-51.  videos: uint8 [N, T, H, W, 3] (numpy or torch) -> fp32 [N, T, 3, h, w] on the device, channel-first."""
    if channel_order not in ("bgr", "rgb"):
        raise ValueError(f"preprocess: channel_order is 'bgr' or 'rgb', not {channel_order!r}")
    u8 = torch.as_tensor(videos)
    if u8.dim() != 5 or u8.shape[-1] != 3 or u8.dtype != torch.uint8:
        raise ValueError(f"preprocess: videos are uint8 [N, T, H, W, 3], got {tuple(u8.shape)} {u8.dtype}")
    return ops.fvd_prep(u8.cuda(), target_resolution, flip=channel_order == "bgr")


def create_id3_embedding(videos):
    """fvd.py:63-122.  videos: fp32 [N, T, 3, 224, 224] in [-1, 1] (what `preprocess` returns) -> float64 [N, 400] on the device."""
    return _fvd_model().features(videos)


def compute_fvd_given_acts(acts_1, acts_2):
    """fvd.py:136-143, float64 on the host."""
    acts_1, acts_2 = (np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64) for a in (acts_1, acts_2))
    m1, s1 = np.mean(acts_1, axis=0), np.cov(acts_1, rowvar=False)
    m2, s2 = np.mean(acts_2, axis=0), np.cov(acts_2, rowvar=False)
    return calculate_frechet_distance(m1, s1, m2, s2)


def _embed_batches(total, real_batch, fake_batch, channel_order):
    """The loop of fvd.py:163-172: batches of 16, the remainder dropped.  The real and the fake clips of a batch go through launches of
    the same shape, so equal clips give equal embeddings, bit for bit."""
    model = _fvd_model()
    if total < BATCH_SIZE:
        raise ValueError(f"FVD: {total} clips; the embeddings are computed in batches of {BATCH_SIZE} and the remainder is dropped, so none would be left")
    real_emb, fake_emb = [], []
    with torch.no_grad():
        for i in range(total // BATCH_SIZE):
            sl = slice(i * BATCH_SIZE, (i + 1) * BATCH_SIZE)
            real_emb.append(model.embed(real_batch(sl), channel_order).cpu().numpy())
            fake_emb.append(model.embed(fake_batch(sl), channel_order).cpu().numpy())
    return np.concatenate(real_emb, axis=0), np.concatenate(fake_emb, axis=0)


def emb_from_videos(real_u8, fake_u8, channel_order="bgr"):
    """`emb_from_files` on clips already in memory: uint8 [N, T, H, W, 3] (numpy or torch).  Returns two float64 numpy [N // 16 * 16, 400]."""
    assert len(real_u8) == len(fake_u8)
    return _embed_batches(len(real_u8), lambda sl: real_u8[sl], lambda sl: fake_u8[sl], channel_order)


def emb_from_files(real_video_files, fake_video_files, resize, num_workers, channel_order="bgr", loader=None, png_decode="host"):
    """fvd.py:145-173.  loader: `loader(files, resize) -> uint8 [B, T, H, W, 3]` in place of `load_videos` (needed for .mp4 names only);
    png_decode: where `load_videos` decodes .png clips ("host" or "gpu")."""
    if loader is None:
        loader = lambda files, size: load_videos(files, size, num_workers, png_decode=png_decode)  # noqa: E731
    assert len(real_video_files) == len(fake_video_files)
    return _embed_batches(len(real_video_files), lambda sl: loader(real_video_files[sl], resize), lambda sl: loader(fake_video_files[sl], resize),
                          channel_order)


def fvd_from_videos(real_u8, fake_u8, channel_order="bgr"):
    """The FVD of uint8 clips [N, T, H, W, 3] in memory (N >= 16; a ragged tail of N % 16 clips is dropped): a float."""
    real_emb, fake_emb = emb_from_videos(real_u8, fake_u8, channel_order)
    return float(compute_fvd_given_acts(real_emb, fake_emb))


def fvd_size(real_emb, fake_emb, size):
    """fvd.py:216-226."""
    fvds = []
    n = real_emb.shape[0] // size
    for i in range(n):
        fvds.append(compute_fvd_given_acts(real_emb[i * size:(i + 1) * size], fake_emb[i * size:(i + 1) * size]))
    print("Individual FVD scores")
    print(fvds)
    print(f"Mean/std of FVD across {n} runs of size {size}")
    print(np.mean(fvds), np.std(fvds))
    return fvds


def fvd_full(real_emb, fake_emb):
    """fvd.py:228-230."""
    fvd = compute_fvd_given_acts(real_emb, fake_emb)
    print(f"FVD score: {fvd}")
    return fvd


def main(args):
    """fvd.py:232-260."""
    if args.mode not in ("size", "full", "both"):
        raise ValueError(f"--mode is size, full or both, not {args.mode!r}")
    if getattr(args, "fvd_weights", None):
        set_fvd_weights(args.fvd_weights)
    fake_folders = get_folders(args.exp_tag, args.num_folds)
    real_tag = args.exp_tag if args.real_tag is None else args.real_tag
    real_folders = get_folders(real_tag, args.num_folds)

    real_emb, fake_emb = [], []
    for i, (real_root, fake_root) in enumerate(zip(sorted(real_folders), sorted(fake_folders))):
        print(f"[{i}] Loading real")
        real_video_files = get_video_files(os.path.join(real_root, args.real_folder))
        print(f"Found {len(real_video_files)} {args.real_folder} video files")

        print(f"[{i}] Loading fake")
        fake_video_files = get_video_files(os.path.join(fake_root, args.fake_folder))
        print(f"Found {len(fake_video_files)} {args.fake_folder} video files")

        assert len(real_video_files) == len(fake_video_files)

        print(f"[{i}] Computing embeddings")
        real_emb_i, fake_emb_i = emb_from_files(real_video_files, fake_video_files, args.resize, args.num_workers, args.channel_order,
                                                png_decode=getattr(args, "png_decode", "host"))
        real_emb.append(real_emb_i)
        fake_emb.append(fake_emb_i)

    print(f"Computing FVD with {args.mode} mode")
    real_emb = np.concatenate(real_emb, axis=0)
    fake_emb = np.concatenate(fake_emb, axis=0)
    if args.mode == "size" or args.mode == "both":
        fvd_size(real_emb, fake_emb, args.size)
    if args.mode == "full" or args.mode == "both":
        fvd_full(real_emb, fake_emb)


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--exp_tag', type=str, default=None)
    parser.add_argument('--real_tag', type=str, default=None)
    parser.add_argument('--real_folder', type=str, default="real")
    parser.add_argument('--fake_folder', type=str, default="fake")
    parser.add_argument('--num_folds', type=int, default=None)
    parser.add_argument('--mode', type=str, default="size", help="(size | full | both)")
    parser.add_argument('--size', type=int, default=256)
    parser.add_argument('--resize', type=int, nargs="+", default=None)
    parser.add_argument('--num_workers', type=int, default=8)
    parser.add_argument('--fvd_weights', type=str, default=None, help="the I3D weight file (tools/tf_fvd/i3d.py writes it)")
    parser.add_argument('--channel_order', type=str, default="bgr", choices=("bgr", "rgb"),
                        help="bgr: the channels reversed, as the reference feeds them (OpenCV frames, unconverted); rgb: the canonical order")
    parser.add_argument('--png_decode', type=str, default="host", choices=("host", "gpu"),
                        help="where .png clips are inflated and un-filtered: host (zlib and numpy) or gpu (one decode call per batch); the same bytes")
    return parser.parse_args(argv)


if __name__ == "__main__":
    main(parse_args())
