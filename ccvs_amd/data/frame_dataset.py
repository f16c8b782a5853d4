"""The frame-folder datasets of the reference (data/base_dataset.py, data/bairhd_dataset.py), validation phase, `from_vid=False`:
which frames make an item and what the per-frame transform chain amounts to, on the host; the pixels' work on the GPU.

`FrameDataset` restates the reference: discovery and grouping (bairhd_dataset.py:22-32), the clip choice (base_dataset.py:243-250), the
crop geometry (`get_augmentation_parameters`, :120-165) and the chain Resize / Resize + CenterCrop / Resize / crop / Resize(dim)
(`get_transform`, :341-357) with torchvision 0.8.1's size rules, and the order of the draws from Python's `random`.  It does not run
the chain: `plan` folds it into stages (box, size) that `ops.ingest_u8` executes -- every Resize a `PIL.Image.resize(BILINEAR)`,
bit for bit.  `FrameLoader` batches items, decodes ahead in threads, uploads the uint8 frames and returns the fp32 clip.

The datasets of video files (`from_vid=True`: kinetics600, drums, ucf101) and their STFT stream are `video_dataset.py`'s: Motion-JPEG
AVI files decoded on the GPU, the reference's tensor transform chain (`ops.ingest_f32`); `frames_root` routes them there when the
dataset's folder holds at least one `.avi` and raises when it holds none.  `--load_state` and layouts are outside both paths and raise.
The geometry both share (`resize_target`, `_Chain`, the crop parameters, `plan`) lives in `transform_plan.py`."""
import os
import random
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .folder_dataset import NPY_EXTENSION, make_dataset
from .transform_plan import IMAGENET_MEAN, IMAGENET_STD, ChainGeometry, _Chain, resize_target   # noqa: F401  (moved there; still importable from here)

# --dataset -> the folder of frames under dataroot for the validation phase (bairhd_dataset.py:10,23: "valid" reads "test")
FRAME_FOLDERS = {"bairhd": os.path.join("original_frames_256", "test")}
# datasets the reference reads from video files (tools/options.py:421-449: from_vid)
VIDEO_DATASETS = ("kinetics600", "drums", "ucf101")


def frames_root(opt):
    """The folder `FrameDataset` would read for `opt` (for a dataset of video files: the dataroot `VideoDataset` reads), or None when `opt.dataroot` is no directory (then there is no dataset on disk
    and the caller keeps its synthetic input).  A directory that cannot be read as frames raises, naming the reason."""
    root = getattr(opt, "dataroot", None)
    if not root or not os.path.isdir(root):
        return None
    if getattr(opt, "layout", False):
        raise NotImplementedError("--layout: label-map inputs are not on the MI355X path")
    if getattr(opt, "load_state", False):
        raise NotImplementedError("--load_state: the annotated-frames dataset (frame states) is not read here")
    if opt.dataset in VIDEO_DATASETS:
        from .video_dataset import find_videos
        if find_videos(opt) is None:
            raise NotImplementedError(f"--dataset {opt.dataset} is read from video files: no Motion-JPEG .avi file of it was found under {root} "
                                      f"(.mp4 and MPEG-4 files are not decoded on this path; re-encode the clips once as Motion-JPEG AVI, "
                                      f"INTEGRATION.md, or export them as frame folders and use a frame-folder dataset)")
        return root                                                      # `ccvs_amd.data.VideoDataset` reads it (video_dataset.py)
    if getattr(opt, "stft", False):
        raise NotImplementedError(f"--x_stft reads STFT pickles beside video files: --dataset {opt.dataset} under {root} is not a video dataset")
    if opt.dataset not in FRAME_FOLDERS:
        raise NotImplementedError(f"--dataset {opt.dataset}: no frame-folder layout is known for it (known: {sorted(FRAME_FOLDERS)})")
    path = os.path.join(root, FRAME_FOLDERS[opt.dataset])
    if not os.path.isdir(path):
        raise FileNotFoundError(f"--dataroot {root} exists but holds no {FRAME_FOLDERS[opt.dataset]} folder of frames for --dataset {opt.dataset}")
    return path


class FrameDataset(ChainGeometry):
    def __init__(self, opt, phase="valid", load_vid=True):
        if phase != "valid":
            raise NotImplementedError("FrameDataset is the validation-phase dataset (no flips, zooms, colour jitter): phase must be 'valid'")
        if opt.dataset in VIDEO_DATASETS:
            raise NotImplementedError(f"--dataset {opt.dataset} is read from video files: that is `ccvs_amd.data.VideoDataset`")
        self.opt, self.phase, self.load_vid = opt, phase, bool(load_vid)
        root = frames_root(opt)
        if root is None:
            raise FileNotFoundError(f"--dataroot {getattr(opt, 'dataroot', None)} is not a directory")
        self.frame_paths = make_dataset(root, recursive=True)
        if not self.frame_paths:
            raise FileNotFoundError(f"no frames found under {root}")
        groups = {}
        for path in sorted(self.frame_paths):                           # bairhd_dataset.py:24-31: one directory is one video
            groups.setdefault(os.path.dirname(path), []).append(path)
        self.vid_frame_paths = list(groups.values())
        self.init_geometry()

    def __len__(self):
        return len(self.vid_frame_paths) if self.load_vid else len(self.frame_paths)

    # ---- items
    def choose(self, index):
        """The draws of item `index` in the reference's order (crop offsets, then the clip's first frame; with categories one
        `torch.randint` for `tgt_vid_lbl`) and what they select: {"paths", "offsets"[, "tgt_vid_lbl"]}.  Call it from one thread,
        in item order; `decode` is free of draws."""
        o = self.opt
        item = {"offsets": self.crop_offsets()}
        if self.load_vid:
            paths = self.vid_frame_paths[index]
            n, step = int(o.vid_len), int(o.one_every_n)                 # p2p_len / load_vid_len apply to training only (:246-247)
            if len(paths) < n or len(paths) - n * step + 1 <= 0:
                raise ValueError(f"{os.path.dirname(paths[0])}: {len(paths)} frames, a clip needs {n} frames, one every {step}")
            idx = random.randrange(len(paths) - n * step + 1)
            item["paths"] = paths[idx:idx + n * step:step]
        else:
            item["paths"] = [self.frame_paths[index]]
        if getattr(o, "categories", None) is not None:
            item["tgt_vid_lbl"] = torch.randint(low=0, high=len(o.categories), size=torch.Size([]))
        return item

    @staticmethod
    def read_frame(path):
        """uint8 [H, W, 3] RGB: `PIL.Image.open(path).convert('RGB')` (:196), or `np.load` for a .npy frame."""
        if path.endswith(NPY_EXTENSION):
            frame = np.load(path)
            if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
                raise ValueError(f"{path}: a .npy frame must hold uint8 [H, W, 3], not {frame.dtype} {frame.shape}")
            return frame
        try:
            from PIL import Image
        except ImportError as exc:
            raise ImportError(f"reading {path} needs Pillow, which is not installed (frames may also be .npy files of uint8 [H, W, 3])") from exc
        with Image.open(path) as img:
            return np.asarray(img.convert("RGB"))

    def compressed(self, item):
        """`PngStreams` of a chosen item all of whose frames are single-image 8-bit RGB non-interlaced PNG files of one size, else None
        (.npy, .jpg, palette / grey / alpha / 16-bit / interlaced or animated PNG, mixed sizes, a file the chunk walk refuses)."""
        from ccvs_amd.tools import apng
        streams, size = [], None
        for p in item["paths"]:
            if not p.lower().endswith(".png") or not apng.png_gpu_decodable(p):
                return None
            try:
                h, w, zs = apng.apng_streams(p)
            except ValueError:
                return None
            if len(zs) != 1 or (size or (h, w)) != (h, w):
                return None
            size = (h, w)
            streams.append(zs[0])
        return PngStreams(streams, size[0], size[1], list(item["paths"]))

    def decode(self, item):
        """(uint8 [T, H, W, 3], plan) of a chosen item (T = 1 for single frames).  With `--png_decode gpu` an item of PNG frames the GPU
        decodes comes as (`PngStreams`, plan): the files' zlib streams, which `FrameLoader.assemble` uploads and decodes."""
        if getattr(self.opt, "png_decode", "host") == "gpu":
            packed = self.compressed(item)
            if packed is not None:
                return packed, self.plan(packed.shape[1], packed.shape[2], item["offsets"])
        frames = [self.read_frame(p) for p in item["paths"]]
        if any(f.shape != frames[0].shape for f in frames):
            raise ValueError(f"{os.path.dirname(item['paths'][0])}: frames of one clip differ in size")
        frames = np.stack(frames)
        return frames, self.plan(frames.shape[1], frames.shape[2], item["offsets"])

    def load(self, index):
        return self.decode(self.choose(index))


class PngStreams:
    """The frames of an item still compressed: the zlib stream of every frame, `shape` as the decoded uint8 array would have it."""

    def __init__(self, streams, h, w, paths):
        self.streams, self.paths, self.shape = streams, paths, (len(streams), h, w, 3)


def run_plan(frames_u8, plan, out, mean, std):
    """uint8 device frames [N, Hs, Ws, 3] through the stages of `plan` into the fp32 tensor `out` [N, 3, H, W] (dense rows, any frame /
    channel strides), on the current stream: uint8 between the stages, ToTensor + Normalize folded into the last."""
    from ccvs_amd import ops
    plan = list(plan) or [(None, None)]
    for box, size in plan[:-1]:
        frames_u8 = ops.ingest_u8(frames_u8, box=box, size=size, as_u8=True)
    return ops.ingest_u8(frames_u8, box=plan[-1][0], size=plan[-1][1], out=out, mean=mean, std=std)


class FrameLoader:
    """Batches of a `FrameDataset` as the synthesis path reads them: {"vid": fp32 [B, T, 3, H, W]} (or {"img": [B, 3, H, W]}) on the
    current device, `tgt_vid_lbl` [B] where the reference gives it.

    Items go in sequential order, `global_batch` per step, the last incomplete step dropped (the reference's DataLoader: drop_last);
    this process takes items [lo, hi) of every step (`Engine.shard_batch`).  `--shuffle_valid` orders the items by a `torch.randperm`
    seeded from `--seed`: the same on every rank, and OURS -- not the stream of the reference's RandomSampler.  The draws of an item
    (`FrameDataset.choose`) are made by the iterating thread in item order; its frames are decoded ahead by at most
    min(num_workers, 16) threads (none: inline).  A batch is stacked into one pinned uint8 buffer, uploaded with one non-blocking
    copy and run through `ops.ingest_u8` on the caller's current stream: no side stream, no synchronisation.  Frames of a batch that
    differ in source size or plan are launched group by group.  With `--png_decode gpu` the items that come compressed
    (`FrameDataset.decode`) form groups of their own: a group's zlib streams go into one pinned blob, up in one non-blocking copy and
    through one `ops.png_decode_uploaded` on the same stream, whose uint8 frames take the place of the uploaded ones; the status words
    of a batch are read back once, after its last launch (the one synchronisation this mode adds), and a failed frame raises
    ValueError naming its file."""

    def __init__(self, dataset, global_batch, lo=0, hi=None, cycle=False, ahead=2):
        self.dataset, self.global_batch = dataset, int(global_batch)
        self.lo, self.hi = int(lo), int(global_batch if hi is None else hi)
        self.cycle, self.ahead = bool(cycle), max(1, int(ahead))
        self.steps = len(dataset) // self.global_batch
        if self.steps == 0:
            raise ValueError(f"the dataset has {len(dataset)} items, fewer than one batch of {self.global_batch}")
        self.workers = min(int(getattr(dataset.opt, "num_workers", 0)), 16)

    def __len__(self):
        return self.steps

    def order(self, epoch=0):
        n = len(self.dataset)
        if getattr(self.dataset.opt, "shuffle_valid", False):
            g = torch.Generator().manual_seed(int(getattr(self.dataset.opt, "seed", 0)) * 1000003 + epoch)
            return torch.randperm(n, generator=g).tolist()
        return list(range(n))

    def _steps(self):
        epoch = 0
        while True:
            order = self.order(epoch)
            for s in range(self.steps):
                yield order[s * self.global_batch + self.lo:s * self.global_batch + self.hi]
            if not self.cycle:
                return
            epoch += 1

    def __iter__(self):
        ds = self.dataset
        pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="ccvs-frame-decode") if self.workers > 0 else None
        try:
            queue, steps = deque(), self._steps()

            def fill():
                while len(queue) < self.ahead:
                    idxs = next(steps, None)
                    if idxs is None:
                        return
                    items = [ds.choose(i) for i in idxs]                 # the draws: this thread, item order
                    queue.append((items, [pool.submit(ds.decode, it) for it in items] if pool is not None else None))

            fill()
            while queue:
                items, futures = queue.popleft()
                decoded = [f.result() for f in futures] if futures is not None else [ds.decode(it) for it in items]
                fill()                                                   # the next steps decode while this one is uploaded
                yield self.assemble(items, decoded)
        finally:
            if pool is not None:
                pool.shutdown(wait=True, cancel_futures=True)

    def assemble(self, items, decoded):
        ds = self.dataset
        b, t = len(items), decoded[0][0].shape[0]
        dev = torch.device("cuda", torch.cuda.current_device())
        clip = torch.empty(b, t, 3, *ds.out_size, dtype=torch.float32, device=dev)
        groups, checks = {}, []
        for i, (frames, plan) in enumerate(decoded):
            groups.setdefault((tuple(frames.shape), tuple(plan), isinstance(frames, PngStreams)), []).append(i)
        for (shape, plan, packed), idxs in groups.items():
            if packed:
                from ccvs_amd import ops
                meta, blob = ops.png_decode_pack([z for i in idxs for z in decoded[i][0].streams], shape[1], shape[2])
                pinned = torch.empty(blob.size, dtype=torch.uint8, pin_memory=True)
                pinned.copy_(torch.from_numpy(blob))
                meta["blob"] = pinned.to(dev, non_blocking=True)
                u8, status = ops.png_decode_uploaded(meta)
                checks.append((status, [p for i in idxs for p in decoded[i][0].paths]))
            else:
                pinned = torch.empty(len(idxs), *shape, dtype=torch.uint8, pin_memory=True)
                for k, i in enumerate(idxs):
                    pinned[k].copy_(torch.from_numpy(decoded[i][0]))
                u8 = pinned.to(dev, non_blocking=True).view(len(idxs) * t, *shape[1:])
            if len(groups) == 1:
                run_plan(u8, plan, clip.view(b * t, 3, *ds.out_size), *ds.norm)
            else:
                part = run_plan(u8, plan, torch.empty(len(idxs) * t, 3, *ds.out_size, dtype=torch.float32, device=dev), *ds.norm)
                clip[torch.tensor(idxs, device=dev)] = part.view(len(idxs), t, 3, *ds.out_size)
        if checks:
            from ccvs_amd import ops
            st = torch.cat([c[0] for c in checks]).cpu().numpy()
            if st.any():
                k = int(st.nonzero()[0][0])
                word, why = ops.PD_STATUS.get(int(st[k]), ("?", "unknown"))
                raise ValueError(f"{[p for c in checks for p in c[1]][k]}: the PNG decoder failed with status {int(st[k])} ({word}: {why}); "
                                 f"{int((st != 0).sum())} of {st.size} frames of the batch failed")
        out = {"vid": clip} if ds.load_vid else {"img": clip[:, 0]}
        if "tgt_vid_lbl" in items[0]:
            out["tgt_vid_lbl"] = torch.stack([it["tgt_vid_lbl"] for it in items])
        return out
