"""The frame-folder datasets of the reference (data/base_dataset.py, data/bairhd_dataset.py), validation phase, `from_vid=False`:
which frames make an item and what the per-frame transform chain amounts to, on the host; the pixels' work on the GPU.

`FrameDataset` restates the reference: discovery and grouping (bairhd_dataset.py:22-32), the clip choice (base_dataset.py:243-250), the
crop geometry (`get_augmentation_parameters`, :120-165) and the chain Resize / Resize + CenterCrop / Resize / crop / Resize(dim)
(`get_transform`, :341-357) with torchvision 0.8.1's size rules, and the order of the draws from Python's `random`.  It does not run
the chain: `plan` folds it into stages (box, size) that `ops.ingest_u8` executes -- every Resize a `PIL.Image.resize(BILINEAR)`,
bit for bit.  `FrameLoader` batches items, decodes ahead in threads, uploads the uint8 frames and returns the fp32 clip.

Video files (`from_vid=True`: kinetics600, drums, ucf101), `--load_state`, STFT inputs and layouts are outside this path and raise."""
import os
import random
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .folder_dataset import NPY_EXTENSION, make_dataset

# --dataset -> the folder of frames under dataroot for the validation phase (bairhd_dataset.py:10,23: "valid" reads "test")
FRAME_FOLDERS = {"bairhd": os.path.join("original_frames_256", "test")}
# datasets the reference reads from video files (tools/options.py:421-449: from_vid)
VIDEO_DATASETS = ("kinetics600", "drums", "ucf101")

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def frames_root(opt):
    """The folder `FrameDataset` would read for `opt`, or None when `opt.dataroot` is no directory (then there is no dataset on disk
    and the caller keeps its synthetic input).  A directory that cannot be read as frames raises, naming the reason."""
    root = getattr(opt, "dataroot", None)
    if not root or not os.path.isdir(root):
        return None
    if getattr(opt, "layout", False):
        raise NotImplementedError("--layout: label-map inputs are not on the MI355X path")
    if getattr(opt, "load_state", False):
        raise NotImplementedError("--load_state: the annotated-frames dataset (frame states) is not read here")
    if getattr(opt, "stft", False):
        raise NotImplementedError(f"--x_stft reads STFT pickles beside video files: not read from {root} (no video decoder on this path)")
    if opt.dataset in VIDEO_DATASETS:
        raise NotImplementedError(f"--dataset {opt.dataset} is read from video files (.mp4 / .avi through a video decoder), which this "
                                  f"path does not decode; export the clips as frame folders and use a frame-folder dataset")
    if opt.dataset not in FRAME_FOLDERS:
        raise NotImplementedError(f"--dataset {opt.dataset}: no frame-folder layout is known for it (known: {sorted(FRAME_FOLDERS)})")
    path = os.path.join(root, FRAME_FOLDERS[opt.dataset])
    if not os.path.isdir(path):
        raise FileNotFoundError(f"--dataroot {root} exists but holds no {FRAME_FOLDERS[opt.dataset]} folder of frames for --dataset {opt.dataset}")
    return path


def resize_target(h, w, size):
    """Output (h, w) of torchvision 0.8.1's `Resize(size)` on an h x w frame: an int or a one-element list sizes the smaller edge, the
    other edge is int(size * long / short), a frame whose smaller edge already has that size is returned untouched; a two-element
    list is exactly (h, w)."""
    if isinstance(size, (list, tuple)) and len(size) == 1:
        size = size[0]
    if isinstance(size, (list, tuple)):
        assert len(size) == 2, size
        return int(size[0]), int(size[1])
    size = int(size)
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


class _Chain:
    """Folds the reference's chain into stages (box, size): a crop that follows a resize waits for the next resize and becomes its
    box; steps that change nothing are dropped."""

    def __init__(self, h, w):
        self.h, self.w, self.box, self.stages = h, w, None, []

    def resize(self, size):
        th, tw = resize_target(self.h, self.w, size)
        if (th, tw) != (self.h, self.w):
            self.stages.append((self.box, (th, tw)))
            self.box, self.h, self.w = None, th, tw

    def crop(self, top, left, h, w, what):
        if not (0 <= top and 0 <= left and h > 0 and w > 0 and top + h <= self.h and left + w <= self.w):
            raise ValueError(f"{what}: the crop (top {top}, left {left}, {h} x {w}) leaves the {self.h} x {self.w} image -- PIL would pad "
                             f"it with black; --true_dim / --true_ratio do not describe these frames")
        if (top, left, h, w) == (0, 0, self.h, self.w):
            return
        base = self.box or (0, 0, self.h, self.w)
        self.box, self.h, self.w = (base[0] + top, base[1] + left, h, w), h, w

    def done(self):
        if self.box is not None:
            self.stages.append((self.box, (self.h, self.w)))
            self.box = None
        return self.stages


class FrameDataset:
    def __init__(self, opt, phase="valid", load_vid=True):
        if phase != "valid":
            raise NotImplementedError("FrameDataset is the validation-phase dataset (no flips, zooms, colour jitter): phase must be 'valid'")
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
        dims = [2 ** k for k in range(2, int(np.log2(opt.max_dim)) + 1)]  # base_dataset.py:74-75
        self.dim = dims[int(np.log2(opt.dim)) - 2]
        self.out_size = (self.dim, int(self.dim * opt.aspect_ratio))    # the clip the reference allocates (:265)
        self.norm = (IMAGENET_MEAN, IMAGENET_STD) if getattr(opt, "imagenet_norm", False) else ((0.5,) * 3, (0.5,) * 3)

    def __len__(self):
        return len(self.vid_frame_paths) if self.load_vid else len(self.frame_paths)

    # ---- geometry
    def crop_offsets(self):
        """The draws of `get_augmentation_parameters` in validation (:141): two `random.random()` for `fixed_crop` without
        `centered_crop`, none otherwise."""
        o = self.opt
        if not o.fixed_top_centered_zoom and o.fixed_crop and not o.centered_crop:
            return random.random(), random.random()
        return 0.5, 0.5

    def augmentation(self, offsets=(0.5, 0.5)):
        """(top, left, h_crop, w_crop, scale) of `get_augmentation_parameters` in validation (:120-165)."""
        o = self.opt
        h, w = int(o.true_dim), int(o.true_dim * o.true_ratio)
        if o.fixed_top_centered_zoom:
            h_crop = int(h / o.fixed_top_centered_zoom)
            w_crop = int(h_crop * o.aspect_ratio)
            assert w >= w_crop, (w, w_crop)
            return 0, int((w - w_crop) / 2), h_crop, w_crop, None
        if o.fixed_crop:
            h_crop, w_crop = o.fixed_crop[0], o.fixed_crop[1]
            h_scaled, w_scaled = int(h * 1.), int(w * 1.)
            assert h_scaled - h_crop >= 0 and w_scaled - w_crop >= 0, (h_scaled, w_scaled, o.fixed_crop)
            return int(offsets[0] * (h_scaled - h_crop)), int(offsets[1] * (w_scaled - w_crop)), h_crop, w_crop, (h_scaled, w_scaled)
        zoom = max(1., o.aspect_ratio / o.true_ratio)
        h_crop = int(h / zoom)
        w_crop = int(h_crop * o.aspect_ratio)
        assert h >= h_crop and w >= w_crop, (h, w, h_crop, w_crop)
        return 0, 0, h_crop, w_crop, None

    def plan(self, src_h, src_w, offsets=(0.5, 0.5)):
        """The stages [(box, size), ...] the reference's chain (`get_transform`, :348-357) amounts to for a src_h x src_w frame: each
        is a crop to `box` = (top, left, h, w) (None: the whole image) followed by a bilinear resize to `size` = (h, w).  [] when the
        frame already is the clip's frame.  Raises when a crop leaves the image or the result is not the clip's frame size."""
        o = self.opt
        top, left, h_crop, w_crop, scale = self.augmentation(offsets)
        c = _Chain(int(src_h), int(src_w))
        if o.resize_img is not None:
            c.resize(list(o.resize_img))
        if o.resize_center_crop_img is not None:
            s = int(o.resize_center_crop_img)
            c.resize(s)
            c.crop(int(round((c.h - s) / 2.)), int(round((c.w - s) / 2.)), s, s, "--resize_center_crop_img")
        if scale is not None:
            c.resize(list(scale))
        c.crop(top, left, h_crop, w_crop, "the crop of --true_dim / --fixed_crop / --fixed_top_centered_zoom")
        c.resize(self.dim)
        if (c.h, c.w) != self.out_size:
            raise ValueError(f"the transform chain turns a {src_h} x {src_w} frame into {c.h} x {c.w}, not the clip's {self.out_size[0]} x "
                             f"{self.out_size[1]} (--dim {self.dim}, --aspect_ratio {o.aspect_ratio})")
        return c.done()

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

    def decode(self, item):
        """(uint8 [T, H, W, 3], plan) of a chosen item (T = 1 for single frames)."""
        frames = [self.read_frame(p) for p in item["paths"]]
        if any(f.shape != frames[0].shape for f in frames):
            raise ValueError(f"{os.path.dirname(item['paths'][0])}: frames of one clip differ in size")
        frames = np.stack(frames)
        return frames, self.plan(frames.shape[1], frames.shape[2], item["offsets"])

    def load(self, index):
        return self.decode(self.choose(index))


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
    differ in source size or plan are launched group by group."""

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
        groups = {}
        for i, (frames, plan) in enumerate(decoded):
            groups.setdefault((frames.shape, tuple(plan)), []).append(i)
        for (shape, plan), idxs in groups.items():
            pinned = torch.empty(len(idxs), *shape, dtype=torch.uint8, pin_memory=True)
            for k, i in enumerate(idxs):
                pinned[k].copy_(torch.from_numpy(decoded[i][0]))
            u8 = pinned.to(dev, non_blocking=True).view(len(idxs) * t, *shape[1:])
            if len(groups) == 1:
                run_plan(u8, plan, clip.view(b * t, 3, *ds.out_size), *ds.norm)
            else:
                part = run_plan(u8, plan, torch.empty(len(idxs) * t, 3, *ds.out_size, dtype=torch.float32, device=dev), *ds.norm)
                clip[torch.tensor(idxs, device=dev)] = part.view(len(idxs), t, 3, *ds.out_size)
        out = {"vid": clip} if ds.load_vid else {"img": clip[:, 0]}
        if "tgt_vid_lbl" in items[0]:
            out["tgt_vid_lbl"] = torch.stack([it["tgt_vid_lbl"] for it in items])
        return out
