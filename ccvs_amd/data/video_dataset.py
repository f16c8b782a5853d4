"""The video-file datasets of the reference (`from_vid=True`: data/ucf101_dataset.py, data/drum_dataset.py, data/kinetics600_dataset.py over
data/base_dataset.py), validation phase, read from Motion-JPEG AVI files: which frames make an item on the host, the pixels' work on
the GPU.

`VideoDataset` restates the reference: discovery (ucf101_dataset.py:12, drum_dataset.py:12-17; kinetics600 through the serialised
`{data_specs}_{phase}_data.pkl`, base_dataset.py:30-33, 81-88, since its `get_data` raises by design), the clip table of torchvision
0.8.1's `VideoClips(paths, clip_length_in_frames=L, frames_between_clips=--vid_skip)` without frame-rate resampling
(base_dataset.py:58-64, 114-118), the draws and the frame selection of `__getitem__` (:169, 203-231, 332-333) and the STFT slice
(:223-231).  The transform chain is the TENSOR one (`get_transform(..., is_PIL=False)`): the geometry of `ChainGeometry.plan`, every
Resize an `F.interpolate(bilinear, align_corners=False)` on `vid.float() / 255` -- `ops.ingest_f32`, not Pillow's resampler.

`VideoLoader` batches items like `FrameLoader`: workers fetch the chosen frames' JPEG bytes (`read_avi_frames`: seek + read) and parse
them (`plan_frames`); the batch's compressed bytes go up in one pinned buffer and one non-blocking copy, `ccvs_mjpeg_decode` turns them
into uint8 frames and `ccvs_ingest_f32` into the clip.

Not reproduced: the training phase, `.mp4` / MPEG-4 files (only `.avi` files are listed; re-encode once), and the
reference's metadata pickle cache (`{phase}_metadata.pkl`: frame counts come from the AVI headers, a seek per file, every time)."""
import bisect
import os
import pickle
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ..tools import mjpeg
from .folder_dataset import make_dataset
from .frame_dataset import VIDEO_DATASETS, FrameLoader
from .transform_plan import ChainGeometry

# --dataset -> the folder of video files under dataroot for the validation phase (ucf101_dataset.py:12; drum_dataset.py:12-14: "valid" reads "test")
VIDEO_FOLDERS = {"ucf101": "videos", "drums": os.path.join("AudioSet_Dataset", "test", "mp4")}
AVI = ".avi"
STFT_SIZE = (64, 16)                                                     # base_dataset.py:230


def serialized_path(opt, data_str, phase):
    """base_dataset.py:81-88 (no folds)."""
    name = f"{phase}_{data_str}.pkl" if getattr(opt, "data_specs", None) is None else f"{opt.data_specs}_{phase}_{data_str}.pkl"
    return os.path.join(opt.dataroot, name)


def find_videos(opt, phase="valid"):
    """The reference's `self.data` for a video dataset -- {"vid_paths"[, "stft_paths", "vid_id", "vid_labels"]} -- restricted to the
    `.avi` files, in `make_dataset(..., from_vid=True)`'s order (directories sorted; the files of a directory sorted too, where the
    reference takes the file system's order).  None when there is no `.avi` to read (no folder, an empty one, `.mp4` only)."""
    root = opt.dataroot
    if opt.dataset == "kinetics600":                                     # the serialised lists (--load_data), the only route the reference has
        path = serialized_path(opt, "data", phase)
        if not os.path.isfile(path):
            return None
        with open(path, "rb") as fh:
            data = pickle.load(fh)
        paths = [p if os.path.isabs(p) else os.path.join(root, p) for p in data["vid_paths"]]
        keep = [k for k, p in enumerate(paths) if p.endswith(AVI)]
        out = {"vid_paths": [paths[k] for k in keep]}
        if "vid_labels" in data:
            out["vid_labels"] = [int(data["vid_labels"][k]) for k in keep]
        return out if keep else None
    folder = os.path.join(root, VIDEO_FOLDERS[opt.dataset])
    if not os.path.isdir(folder):
        return None
    paths = [p for p in make_dataset(folder, recursive=True, from_vid=True) if p.endswith(AVI)]
    if not paths:
        return None
    out = {"vid_paths": paths}
    if opt.dataset == "drums":                                           # drum_dataset.py:15-16
        out["stft_paths"] = [p.replace("/mp4/", "/stft_pickle/").replace(".mp4", ".pickle").replace(AVI, ".pickle") for p in paths]
        out["vid_id"] = [int(os.path.basename(p).split(".")[0]) for p in paths]
    return out


def clip_table(frame_counts, length, skip):
    """Cumulative clip counts of `VideoClips`: video v holds the clips `arange(n_v).unfold(0, length, skip)`, numbered through the videos."""
    counts = [(n - length) // skip + 1 if n >= length else 0 for n in frame_counts]
    return np.cumsum(counts, dtype=np.int64)


class VideoDataset(ChainGeometry):
    def __init__(self, opt, phase="valid", load_vid=True):
        if phase != "valid":
            raise NotImplementedError("VideoDataset is the validation-phase dataset (no flips, zooms, colour jitter, start = 0): phase must be 'valid'")
        if opt.dataset not in VIDEO_DATASETS:
            raise NotImplementedError(f"--dataset {opt.dataset} is not read from video files (those are {list(VIDEO_DATASETS)})")
        self.opt, self.phase, self.load_vid = opt, phase, bool(load_vid)
        if not getattr(opt, "dataroot", None) or not os.path.isdir(opt.dataroot):
            raise FileNotFoundError(f"--dataroot {getattr(opt, 'dataroot', None)} is not a directory")
        self.data = find_videos(opt, phase)
        if self.data is None:
            raise FileNotFoundError(f"no Motion-JPEG .avi video files of --dataset {opt.dataset} under {opt.dataroot}")
        paths = self.data["vid_paths"]
        with ThreadPoolExecutor(max_workers=min(16, len(paths))) as pool:      # headers and index only: no frame is read
            probed = list(pool.map(mjpeg.probe_avi, paths))
        self.indexes = [p[4] for p in probed]
        self.frame_counts = [p[3] for p in probed]
        if self.load_vid:                                                # base_dataset.py:58-62 (validation)
            self.clip_len = int(opt.load_vid_len) if opt.load_vid_len is not None else int(opt.vid_len)
        else:
            self.clip_len = 1
        self.vid_skip = int(opt.vid_skip)
        self.cum = clip_table(self.frame_counts, self.clip_len, self.vid_skip)
        if len(self) == 0:
            raise ValueError(f"no video under {opt.dataroot} has the {self.clip_len} frames of a clip (the longest has {max(self.frame_counts)})")
        self.init_geometry()

    def __len__(self):
        return int(self.cum[-1])

    def get_clip(self, index):
        """(video index, frame numbers) of clip `index`: `VideoClips.get_clip`'s choice."""
        if not 0 <= index < len(self):
            raise IndexError(f"clip {index} of {len(self)}")
        video = bisect.bisect_right(self.cum, index)
        start = (index - (int(self.cum[video - 1]) if video else 0)) * self.vid_skip
        return video, list(range(start, start + self.clip_len))

    def choose(self, index):
        """The draws of item `index` in the reference's order (base_dataset.py:169, 211-221, 332-333) and what they select: {"video",
        "path", "frames", "offsets"[, "vid_lbl", "vid_id", "delta_length", "stft", "tgt_vid_lbl"]}.  Call it from one thread, in item
        order; `decode` is free of draws."""
        o = self.opt
        item = {"offsets": self.crop_offsets()}                          # :169
        video, frames = self.get_clip(index)                            # :204
        item["video"], item["path"] = video, self.data["vid_paths"][video]
        if "vid_labels" in self.data:                                    # :206-209
            item["vid_lbl"] = self.data["vid_labels"][video]
        if "vid_id" in self.data:
            item["vid_id"] = self.data["vid_id"][video]
        if self.load_vid:
            start = end = step = None
            if o.load_vid_len is not None:                               # :211-216
                vid_len = o.vid_len if o.p2p_len is None else o.p2p_len
                step = min(max(1, int(random.random() * (o.load_vid_len - 1) / (vid_len - 1))), o.max_vid_step)
                start = 0                                                # (validation)
                end = start + step * (vid_len - 1) + 1
                frames = frames[start:end:step]
            if o.p2p_len is not None:                                    # :217-221 -- not gated on the phase in this branch
                idx = random.randrange(o.p2p_len - o.vid_len + 1)
                idx_end_frame = random.randrange(idx + o.vid_len - 1, o.p2p_len)
                if idx_end_frame >= len(frames):
                    raise ValueError(f"--p2p_len {o.p2p_len}: the item holds {len(frames)} frames, the end frame drawn is {idx_end_frame} "
                                     f"(the reference fails there too: load --load_vid_len / --vid_len frames of at least --p2p_len)")
                frames = frames[idx:idx + o.vid_len - 1] + [frames[idx_end_frame]]
                item["delta_length"] = torch.tensor(idx_end_frame - idx)
            if "stft_paths" in self.data and o.load_vid_len is not None and o.p2p_len is None:   # :223-224
                item["stft"] = (self.data["stft_paths"][video], start, end, step)
        else:
            frames = frames[:1]                                          # :175 img_idx = [0]
        item["frames"] = frames
        if getattr(o, "categories", None) is not None:                   # :332-333
            item["tgt_vid_lbl"] = torch.randint(low=0, high=len(o.categories), size=torch.Size([]))
        return item

    @staticmethod
    def read_stft(path, start, end, step):
        """fp32 [T, Hf, Wf]: the pickle's array (a `.npy` of the same name where there is no pickle) sliced [start:end:step] -- counted
        from the start of the FILE, not from the clip's first frame, as base_dataset.py:228 does."""
        if os.path.isfile(path):
            with open(path, "rb") as fh:
                stft = pickle.load(fh)
        elif os.path.isfile(os.path.splitext(path)[0] + ".npy"):
            path = os.path.splitext(path)[0] + ".npy"
            stft = np.load(path)
        else:
            raise FileNotFoundError(f"{path}: no STFT pickle (nor a .npy of that name) beside the video")
        stft = np.asarray(stft)
        if stft.ndim != 3:
            raise ValueError(f"{path}: the STFT array must be [frames, H, W], not {stft.shape}")
        return np.ascontiguousarray(stft[start:end:step].astype(np.float32))

    def decode(self, item):
        """The host's share of an item: the chosen frames' JPEG bytes (seek + read), parsed into the decoder's plan, the stages of the
        transform chain for their size, the STFT slice."""
        jpegs = mjpeg.read_avi_frames(item["path"], item["frames"], self.indexes[item["video"]])
        try:
            plan = mjpeg.plan_frames(jpegs)
        except ValueError as exc:
            raise ValueError(f"{item['path']} (frames {item['frames']}): {exc}") from None
        out = {"plan": plan, "stages": tuple(self.plan(plan["h"], plan["w"], item["offsets"])), "raw_bytes": plan["n"] * plan["h"] * plan["w"] * 3}
        if "stft" in item:
            out["stft"] = self.read_stft(*item["stft"])
            if out["stft"].shape[0] != len(item["frames"]):
                raise ValueError(f"{item['stft'][0]}: {out['stft'].shape[0]} STFT frames in [{item['stft'][1]}:{item['stft'][2]}:{item['stft'][3]}], the clip has {len(item['frames'])}")
        return out

    def load(self, index):
        return self.decode(self.choose(index))


def merge_plans(plans):
    """One `plan_frames` plan of several (same size and sampling): frames, units and scans one behind the other, table records shared."""
    if len(plans) == 1:
        return plans[0]
    records, tables, frame_table, units, scans, frame0, byte0 = {}, [], [], [], [], 0, 0
    for p in plans:
        own = [bytes(p["tables"][k * mjpeg.TABLE_BYTES:(k + 1) * mjpeg.TABLE_BYTES]) for k in range(p["tables"].size // mjpeg.TABLE_BYTES)]
        remap = np.asarray([records.setdefault(r, len(records)) for r in own], dtype=np.int32)
        frame_table.append(remap[p["frame_table"]])
        u = np.array(p["units"], dtype=np.int64)
        u[:, 0] += frame0
        u[:, 1] += byte0
        units.append(u)
        scans.append(p["scans"])
        frame0, byte0 = frame0 + p["n"], byte0 + p["scans"].size
    first = plans[0]
    return {"n": frame0, "h": first["h"], "w": first["w"], "sampling": first["sampling"], "scans": np.concatenate(scans), "units": np.concatenate(units),
            "tables": np.frombuffer(b"".join(records), dtype=np.uint8), "frame_table": np.concatenate(frame_table)}


class VideoLoader(FrameLoader):
    """Batches of a `VideoDataset`, with `FrameLoader`'s contract (order, `--shuffle_valid`, sharding [lo, hi), `cycle`, the draws by the
    iterating thread in item order, decode-ahead by at most min(num_workers, 16) threads, no side stream, no synchronisation):
    {"vid": fp32 [B, T, 3, H, W]} (or {"img"}), "stft" fp32 [B, T, 1, 64, 16] for drums under --load_vid_len, "vid_lbl" / "vid_id" /
    "delta_length" / "tgt_vid_lbl" where the reference gives them.

    Everything a batch needs on the device -- the decoder's unit tables, table records and COMPRESSED scans of every group of clips,
    the STFT slices -- is packed into ONE pinned buffer and goes up in ONE non-blocking copy; `ccvs_mjpeg_decode` writes the uint8
    frames, `ccvs_ingest_f32` the clip.  Clips of a batch that differ in source size, sampling or plan are launched group by group.

    The decoder's status words are NOT read back per batch.  Each batch adds its count of failed restart units to a counter on the
    device (`bad_units`); `check()` reads it -- the one synchronisation, at a point the caller chooses -- and raises, naming the last
    batch's files where the failure is theirs.  An iteration that runs to its end calls `check()` itself.  `bytes_up` / `bytes_raw`
    count what went up against what the same frames are as raw uint8."""

    def __init__(self, dataset, global_batch, lo=0, hi=None, cycle=False, ahead=2):
        super().__init__(dataset, global_batch, lo, hi, cycle, ahead)
        self.bad_units, self.last, self.bytes_up, self.bytes_raw = None, [], 0, 0

    def __iter__(self):
        yield from super().__iter__()
        self.check()

    def check(self):
        """Reads the failed-unit counter back (synchronises) and raises ValueError where a unit of a batch since the last call failed."""
        if self.bad_units is None:
            return
        bad, self.bad_units = int(self.bad_units.item()), None
        if bad:
            named = []
            for paths, status in self.last:
                st = status.cpu()
                if bool((st != 0).any()):
                    named.append(f"{paths}: {int((st != 0).sum())} unit(s), first status {int(st[st != 0][0])}")
            raise ValueError(f"{bad} restart unit(s) of the decoded batches failed (corrupt or unsupported JPEG data)"
                             + ("; in the last batch: " + "; ".join(named) if named else "; none of them in the last batch"))

    def assemble(self, items, decoded):
        from ccvs_amd import ops
        ds = self.dataset
        b, t = len(items), len(items[0]["frames"])
        if any(len(it["frames"]) != t for it in items):
            raise ValueError("the clips of a batch differ in length")
        dev = torch.device("cuda", torch.cuda.current_device())
        groups = {}
        for i, d in enumerate(decoded):
            p = d["plan"]
            groups.setdefault((p["h"], p["w"], p["sampling"], d["stages"]), []).append(i)
        # ---- pack: per group the decoder's blob, then the STFT slices, each part 16-byte aligned
        parts, offset = [], 0
        for key, idxs in groups.items():
            meta, blob = ops.mjpeg_decode_pack(merge_plans([decoded[i]["plan"] for i in idxs]))
            parts.append((offset, blob))
            meta["at"] = offset
            groups[key] = (idxs, meta)
            offset += (blob.size + 15) & ~15
        stft_groups = {}
        if "stft" in decoded[0]:
            for i, d in enumerate(decoded):
                stft_groups.setdefault(d["stft"].shape, []).append(i)
            for shape, idxs in stft_groups.items():
                block = np.stack([decoded[i]["stft"] for i in idxs]).reshape(-1).view(np.uint8)
                parts.append((offset, block))
                stft_groups[shape] = (idxs, offset, block.size)
                offset += (block.size + 15) & ~15
        pinned = torch.empty(offset, dtype=torch.uint8, pin_memory=True)
        host = pinned.numpy()
        for at, part in parts:
            host[at:at + part.size] = part
        up = pinned.to(dev, non_blocking=True)
        self.bytes_up += offset
        self.bytes_raw += sum(d["raw_bytes"] for d in decoded)
        # ---- decode and transform, group by group
        clip = torch.empty(b, t, 3, *ds.out_size, dtype=torch.float32, device=dev)
        self.last = []
        for (h, w, sampling, stages), (idxs, meta) in groups.items():
            meta["blob"] = up[meta["at"]:]
            u8, status = ops.mjpeg_decode_uploaded(meta)
            bad = (status != 0).sum()
            self.bad_units = bad if self.bad_units is None else self.bad_units + bad
            self.last.append((", ".join(items[i]["path"] for i in idxs), status))
            if len(groups) == 1:
                ops.ingest_f32(u8, stages, out=clip.view(b * t, 3, *ds.out_size), pre="div255", mean=ds.norm[0], std=ds.norm[1])
            else:
                part = ops.ingest_f32(u8, stages, pre="div255", mean=ds.norm[0], std=ds.norm[1])
                clip[torch.tensor(idxs, device=dev)] = part.view(len(idxs), t, 3, *ds.out_size)
        out = {"vid": clip} if ds.load_vid else {"img": clip[:, 0]}
        if stft_groups:
            stft = torch.empty(b, t, 1, *STFT_SIZE, dtype=torch.float32, device=dev)
            for (_, hf, wf), (idxs, at, nbytes) in stft_groups.items():
                src = up[at:at + nbytes].view(torch.float32).view(len(idxs) * t, 1, hf, wf)
                if len(stft_groups) == 1:
                    ops.ingest_f32(src, [(None, STFT_SIZE)], out=stft.view(b * t, 1, *STFT_SIZE), pre="x2m1")
                else:
                    stft[torch.tensor(idxs, device=dev)] = ops.ingest_f32(src, [(None, STFT_SIZE)], pre="x2m1").view(len(idxs), t, 1, *STFT_SIZE)
            out["stft"] = stft
        for key in ("vid_lbl", "vid_id"):
            if key in items[0]:
                out[key] = torch.tensor([it[key] for it in items])
        for key in ("delta_length", "tgt_vid_lbl"):
            if key in items[0]:
                out[key] = torch.stack([it[key] for it in items])
        return out
