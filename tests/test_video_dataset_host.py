"""not gpu: the host side of the video-file datasets.

  1. the mirror tests/video_ingest_ref.py against the literal torch chain of the reference (`x.float() / 255 -> permute ->
     F.interpolate(size, mode="bilinear", align_corners=False)` per Resize `-> crop -> sub / div`) on every row of `ROWS`: the two may
     differ in the last bits of the fp32 source coordinate (torch's CPU kernel is free to contract), so the bound is the one
     tests/test_metrics_gpu.py::test_resize_bilinear_vs_torch uses for the same arithmetic, 1e-5, divided by the smallest std behind
     the post-op;
  2. the clip table against `torch.arange(n).unfold(0, L, skip)` concatenated over the videos;
  3. the draws and the selected frame numbers against a restatement of base_dataset.py:169-231, 332-333 written out here;
  4. `probe_avi` / `read_avi_frames` on files of `write_avi` and on variants other writers produce, and every refusal;
  5. routing: tiny ucf101 / drums / kinetics600 trees give a `VideoDataset`, `.mp4`-only and empty folders still raise;
  6. the C ABI: `ccvs_ingest_f32` declared through include/ccvs_hip.h, exported, and refusing bad arguments before any GPU call.
"""
import ctypes
import os
import pickle
import random
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import video_ingest_ref as R  # noqa: E402

from ccvs_amd.tools import mjpeg  # noqa: E402


def options(dataset, extra=()):
    from ccvs_amd.tools.options import Options
    return Options().parse(load_qvid_generator=True, load_transformer=True, argv=R.tiny_argv(dataset) + [str(v) for v in extra])


# ------------------------------------------------------------------ 1: the mirror against torch
@pytest.mark.parametrize("row", R.ROWS, ids=[r[0] for r in R.ROWS])
def test_mirror_within_the_bound_of_the_torch_chain(row):
    name, kind, (n, c, hs, ws), stages, pre = row
    src = R.row_source(row)
    norms = [None, R.HALF, R.IMAGENET] if c == 3 else [None, ((0.5,), (0.5,))]
    for norm in norms:
        mean, std = norm if norm else (None, None)
        got = R.chain(src, stages, pre, mean, std)
        want = R.torch_chain(src, stages, pre, mean, std).numpy()
        assert got.shape == want.shape and got.dtype == want.dtype == np.float32
        bound = 1e-5 / (min(std) if std else 1.0)
        worst = float(np.abs(got - want).max())
        print(f"{name} norm={norm}: max |mirror - torch| {worst:.3e} (bound {bound:.3e}), {int((got != want).sum())} of {got.size} differ")
        assert worst <= bound


def test_mirror_identity_axes_copy_exactly():
    src = R.row_source(R.ROWS[5])
    x = R.pre_op(src, "div255")
    assert np.array_equal(R.stage(x, None, None), x) and np.array_equal(R.stage(x, (1, 2, 7, 8), None), x[..., 1:8, 2:10])
    wide = R.stage(x, None, (9, 20))                                  # rows are an identity axis: an output row reads ONE source row
    assert np.array_equal(wide[..., 0], x[..., 0])                      # (column 0: source coordinate clamped to 0, weight 1)
    assert np.array_equal(wide, np.stack([R.stage(x[..., r:r + 1, :], None, (1, 20))[..., 0, :] for r in range(9)], axis=-2))


# ------------------------------------------------------------------ 2: the clip table
@pytest.mark.parametrize("length,skip", [(4, 1), (4, 3), (9, 2), (1, 1)])
def test_clip_table_equals_unfold(tmp_path, length, skip):
    from ccvs_amd.data.video_dataset import VideoDataset, clip_table
    counts = [length - 1, length, length + skip - 1, length + skip, 57] if length > 1 else [1, 2, 57]
    want = []
    for v, n in enumerate(counts):
        if n >= length:
            want += [(v, row.tolist()) for row in torch.arange(n).unfold(0, length, skip)]
    cum = clip_table(counts, length, skip)
    assert int(cum[-1]) == len(want)
    ds = VideoDataset.__new__(VideoDataset)
    ds.cum, ds.clip_len, ds.vid_skip = cum, length, skip
    assert [ds.get_clip(i) for i in range(len(want))] == want
    with pytest.raises(IndexError):
        ds.get_clip(len(want))


# ------------------------------------------------------------------ 3: the draws
def fake_jpeg(k, size):
    return b"\xff\xd8" + bytes([k % 251]) * size + b"\xff\xd9"


def tree(root, dataset, counts, sizes=None):
    clips = {}
    for k, n in enumerate(counts):
        name = {"ucf101": f"g{k % 2}/v{k}.avi", "drums": f"{100 + k}.avi", "kinetics600": f"k{k}.avi"}[dataset]
        clips[name] = ([fake_jpeg(k * 100 + f, 20 + 3 * f) for f in range(n)], 16, 24)
    return R.write_video_tree(str(root), dataset, clips)


def restated_item(o, clips, index, data):
    """base_dataset.py:169-231, 332-333 for phase "valid", from_vid and load_vid, restated: the draws in the reference's order and the
    frame numbers they select.  `clips`: the (video, frame numbers) rows of the unfold table."""
    out = {}
    # :169 -> :141: two draws only for a fixed crop that is not centred
    if not o.fixed_top_centered_zoom and o.fixed_crop:
        out["offsets"] = (0.5, 0.5) if o.centered_crop else (random.random(), random.random())
    else:
        out["offsets"] = (0.5, 0.5)
    video, numbers = clips[index]                                        # :204
    out["video"] = video
    if "vid_labels" in data:
        out["vid_lbl"] = data["vid_labels"][video]
    if "vid_id" in data:
        out["vid_id"] = data["vid_id"][video]
    if o.load_vid_len is not None:                                       # :211-216
        length = o.vid_len if o.p2p_len is None else o.p2p_len
        step = min(max(1, int(random.random() * (o.load_vid_len - 1) / (length - 1))), o.max_vid_step)
        start = 0
        end = start + step * (length - 1) + 1
        numbers = numbers[start:end:step]
        out["slice"] = (start, end, step)
    if o.p2p_len is not None:                                            # :217-221
        first = random.randrange(o.p2p_len - o.vid_len + 1)
        last = random.randrange(first + o.vid_len - 1, o.p2p_len)
        numbers = numbers[first:first + o.vid_len - 1] + [numbers[last]]
        out["delta_length"] = last - first
    out["frames"] = numbers
    if o.categories is not None:                                         # :332-333
        out["tgt_vid_lbl"] = int(torch.randint(low=0, high=len(o.categories), size=torch.Size([])))
    return out


DRAW_CONFIGS = {
    "plain": [],
    "load9_step1": ["--load_vid_len", 9, "--max_vid_step", 1],
    "load9_step3": ["--load_vid_len", 9, "--max_vid_step", 3],
    "p2p": ["--p2p_len", 7],
    "load9_p2p": ["--load_vid_len", 9, "--p2p_len", 6],
    "fixed_crop": ["--fixed_crop", 12, 12, "--true_dim", 16, "--true_ratio", 1.5],
    "fixed_crop_centered": ["--fixed_crop", 12, 12, "--true_dim", 16, "--true_ratio", 1.5, "--centered_crop"],
    "categories": ["--categories", "a", "b", "c"],
}


@pytest.mark.parametrize("name", list(DRAW_CONFIGS))
def test_draws_and_selection_equal_the_restatement(tmp_path, name):
    from ccvs_amd.data import VideoDataset
    extra = DRAW_CONFIGS[name]
    if name == "p2p":
        extra = extra + ["--vid_len", 4, "--load_vid_len", 7, "--max_vid_step", 1]   # (the item must hold --p2p_len frames, or the reference fails)
    tree(tmp_path, "drums", [12, 3, 15])
    opt = options("drums", ["--dataroot", tmp_path, "--true_dim", 16, "--true_ratio", 1.5, "--vid_skip", 2] + extra)["transformer"]
    ds = VideoDataset(opt)
    length = opt.load_vid_len if opt.load_vid_len is not None else opt.vid_len
    clips = [(v, row.tolist()) for v, n in enumerate(ds.frame_counts) if n >= length for row in torch.arange(n).unfold(0, length, 2)]
    assert len(ds) == len(clips) and ds.frame_counts == [12, 3, 15]
    order = list(range(len(ds)))[::-1] + [0, 0, 1]
    random.seed(31)
    torch.manual_seed(31)
    want = [restated_item(opt, clips, i, ds.data) for i in order]
    tail = (random.random(), int(torch.randint(0, 1000, ())))
    random.seed(31)
    torch.manual_seed(31)
    got = [ds.choose(i) for i in order]
    assert (random.random(), int(torch.randint(0, 1000, ()))) == tail, "the number of draws differs"
    steps = set()
    for g, w in zip(got, want):
        assert g["frames"] == w["frames"] and g["offsets"] == w["offsets"] and g["video"] == w["video"] and g["vid_id"] == w["vid_id"]
        assert ("delta_length" in g) == ("delta_length" in w) and ("tgt_vid_lbl" in g) == ("tgt_vid_lbl" in w)
        if "delta_length" in w:
            assert int(g["delta_length"]) == w["delta_length"]
        if "tgt_vid_lbl" in w:
            assert int(g["tgt_vid_lbl"]) == w["tgt_vid_lbl"]
        if "slice" in w and opt.p2p_len is None:
            assert g["stft"][1:] == w["slice"]                          # the STFT slice counts from the start of the FILE (:228)
            steps.add(w["slice"][2])
        else:
            assert "stft" not in g
        assert len(g["frames"]) == opt.vid_len
    if name == "load9_step1":
        assert steps == {1}
    if name == "load9_step3":
        assert steps == {1, 2}                                           # int(r * 8 / 3) is 0, 1 or 2
    if name.startswith("fixed_crop"):
        assert (got[0]["offsets"] == (0.5, 0.5)) == (name == "fixed_crop_centered")


def test_stft_slice_counts_from_the_file_start_and_npy_is_accepted(tmp_path):
    from ccvs_amd.data import VideoDataset
    paths = tree(tmp_path, "drums", [14, 14])
    rng = np.random.RandomState(2)
    arrays = [rng.rand(14, 20, 6) for _ in range(2)]
    os.makedirs(tmp_path / "AudioSet_Dataset" / "test" / "stft_pickle")
    with open(tmp_path / "AudioSet_Dataset" / "test" / "stft_pickle" / "100.pickle", "wb") as fh:
        pickle.dump(arrays[0], fh)
    np.save(tmp_path / "AudioSet_Dataset" / "test" / "stft_pickle" / "101.npy", arrays[1])
    opt = options("drums", ["--dataroot", tmp_path, "--true_dim", 16, "--true_ratio", 1.5, "--load_vid_len", 9, "--max_vid_step", 2, "--vid_skip", 5])["transformer"]
    ds = VideoDataset(opt)
    assert ds.data["stft_paths"][0].endswith("/stft_pickle/100.pickle") and ds.data["vid_id"] == [100, 101] and len(ds) == 4
    random.seed(5)
    for index in range(4):
        item = ds.choose(index)
        video, numbers = ds.get_clip(index)
        path, start, end, step = item["stft"]
        assert start == 0 and item["frames"] == numbers[0:end:step]
        got = ds.read_stft(*item["stft"])
        assert got.dtype == np.float32 and np.array_equal(got, arrays[video][0:end:step].astype(np.float32))   # NOT arrays[video][numbers]
    os.remove(tmp_path / "AudioSet_Dataset" / "test" / "stft_pickle" / "101.npy")
    with pytest.raises(FileNotFoundError, match="101.pickle"):
        ds.read_stft(ds.data["stft_paths"][1], 0, 4, 1)


# ------------------------------------------------------------------ 4: the container
def chunk(tag, payload):
    return tag + struct.pack("<I", len(payload)) + payload + (b"\x00" if len(payload) & 1 else b"")


def lst(kind, payload):
    return b"LIST" + struct.pack("<I", len(payload) + 4) + kind + payload


def build_avi(frames, fps=5, h=16, w=24, junk=False, info=False, odml=False, rec=False, audio=False, idx="movi", fourcc=b"MJPG", riff_delta=0, avix=False):
    """An MJPG AVI as another writer might lay it out; idx: "movi" (offsets from the 'movi' tag), "abs" (from the file start), None."""
    avih = struct.pack("<14I", 1000000 // fps, 0, 0, 0x10 if idx else 0, len(frames), 0, 2 if audio else 1, 0, w, h, 0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIIIhhhh", b"vids", fourcc, 0, 0, 0, 0, 1, fps, 0, len(frames), 0, 0xFFFFFFFF, 0, 0, 0, w, h)
    strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, fourcc, w * h * 3, 0, 0, 0, 0)
    streams = lst(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf) + (chunk(b"JUNK", b"\0" * 9) if junk else b""))
    if audio:
        auds = struct.pack("<4s4sIHHIIIIIIIIhhhh", b"auds", b"\0\0\0\0", 0, 0, 0, 0, 1, 8000, 0, 0, 0, 0xFFFFFFFF, 1, 0, 0, 0, 0)
        streams += lst(b"strl", chunk(b"strh", auds) + chunk(b"strf", struct.pack("<HHIIHH", 1, 1, 8000, 8000, 1, 8)))
    hdrl = lst(b"hdrl", chunk(b"avih", avih) + streams + (lst(b"odml", chunk(b"dmlh", struct.pack("<I", len(frames)))) if odml else b""))
    front = b"AVI " + hdrl + (lst(b"INFO", chunk(b"ISFT", b"another writer\0")) if info else b"") + (chunk(b"JUNK", b"\0" * 101) if junk else b"")
    movi_tag = 8 + len(front) + 8                                       # file offset of the 'movi' fourcc
    body, entries = b"", []
    for k, f in enumerate(frames):
        group = b""
        if audio:
            group += chunk(b"01wb", bytes([k]) * 7)
        at = len(body) + 4 + (12 if rec else 0) + len(group)            # from the 'movi' tag to this frame's chunk header
        group += chunk(b"00dc", f)
        if rec:
            entries.append((b"rec ", len(body) + 4, len(group) + 4))
            group = lst(b"rec ", group)
        if audio:
            entries.append((b"01wb", at - 16, 7))
        entries.append((b"00dc", at, len(f)))
        body += group
    base = movi_tag if idx == "abs" else 0
    index = b"".join(struct.pack("<4sIII", tag, 0x10, base + off, n) for tag, off, n in entries)
    data = front + lst(b"movi", body) + (chunk(b"idx1", index) if idx else b"") + (chunk(b"JUNK", b"\0" * 4) if junk else b"")
    out = b"RIFF" + struct.pack("<I", len(data) + riff_delta) + data
    if avix:
        out += b"RIFF" + struct.pack("<I", 4 + 12) + b"AVIX" + lst(b"movi", b"")
    return out


FRAMES = [fake_jpeg(k, 31 + 7 * k) for k in range(6)]
VARIANTS = {
    "junk_and_info": dict(junk=True, info=True),
    "odml_header": dict(odml=True),
    "rec_groups": dict(rec=True),
    "rec_groups_no_index": dict(rec=True, idx=None),
    "interleaved_audio": dict(audio=True),
    "interleaved_audio_no_index": dict(audio=True, idx=None, junk=True),
    "no_index": dict(idx=None),
    "absolute_index": dict(idx="abs"),
    "absolute_index_everything": dict(idx="abs", junk=True, info=True, rec=True, audio=True, odml=True),
    "lower_case_handler": dict(fourcc=b"mjpg"),
}


def test_probe_and_read_frames_of_write_avi(tmp_path):
    path = str(tmp_path / "own.avi")
    mjpeg.write_avi(path, FRAMES, 4, 16, 24)
    before = open(path, "rb").read()
    fps, h, w, n, index = mjpeg.probe_avi(path)
    assert (fps, h, w, n) == (4, 16, 24, 6) and mjpeg.read_avi(path) == (4, 16, 24, FRAMES)
    assert [before[o:o + s] for o, s in index] == FRAMES
    assert mjpeg.read_avi_frames(path, range(6), index) == FRAMES and mjpeg.read_avi_frames(path, [4, 1, 4]) == [FRAMES[4], FRAMES[1], FRAMES[4]]
    with pytest.raises(IndexError, match="own.avi"):
        mjpeg.read_avi_frames(path, [6], index)
    assert open(path, "rb").read() == before


@pytest.mark.parametrize("name", list(VARIANTS))
def test_probe_accepts_other_writers_layouts(tmp_path, name):
    path = str(tmp_path / (name + ".avi"))
    with open(path, "wb") as fh:
        fh.write(build_avi(FRAMES, **VARIANTS[name]))
    fps, h, w, n, index = mjpeg.probe_avi(path)
    assert (fps, h, w, n) == (5, 16, 24, 6)
    assert mjpeg.read_avi_frames(path, range(6), index) == FRAMES and mjpeg.read_avi_frames(path, [5, 0]) == [FRAMES[5], FRAMES[0]]
    if not set(VARIANTS[name]) & {"rec", "audio", "fourcc"}:            # (`read_avi` reads `write_avi`'s layout: one stream, flat, "MJPG")
        assert mjpeg.read_avi(path)[3] == FRAMES


def test_probe_never_reads_a_payload(tmp_path, monkeypatch):
    """With and without idx1: every read of the probe is a header, the header list or the index -- no byte of a frame."""
    import builtins
    for name in ("junk_and_info", "interleaved_audio_no_index"):
        path = str(tmp_path / (name + ".avi"))
        data = build_avi(FRAMES, **VARIANTS[name])
        with open(path, "wb") as fh:
            fh.write(data)
        _, _, _, _, index = mjpeg.probe_avi(path)
        touched = []
        real_open = builtins.open

        class Spy:
            def __init__(self, fh):
                self.fh = fh

            def __enter__(self):
                return self

            def __exit__(self, *a):
                self.fh.close()

            def seek(self, pos):
                return self.fh.seek(pos)

            def read(self, n):
                at = self.fh.tell()
                out = self.fh.read(n)
                touched.append((at, at + len(out)))
                return out

        monkeypatch.setattr(builtins, "open", lambda p, mode="r", *a, **k: Spy(real_open(p, mode, *a, **k)) if p == path else real_open(p, mode, *a, **k))
        assert mjpeg.probe_avi(path)[4] == index
        monkeypatch.undo()
        for lo, hi in touched:
            assert all(hi <= o or lo >= o + s for o, s in index), (lo, hi)


def test_probe_refusals_name_the_file(tmp_path):
    def refused(name, data, match):
        path = str(tmp_path / (name + ".avi"))
        with open(path, "wb") as fh:
            fh.write(data)
        with pytest.raises(ValueError, match=match) as exc:
            mjpeg.probe_avi(path)
        assert path in str(exc.value)

    refused("mpeg4", build_avi(FRAMES, fourcc=b"XVID"), "not MJPG.*re-encode")
    refused("avix", build_avi(FRAMES, avix=True), "AVIX")
    refused("short", build_avi(FRAMES)[:-10], "RIFF length")
    refused("long", build_avi(FRAMES) + b"\0\0", "RIFF length")
    refused("riff_lies", build_avi(FRAMES, riff_delta=2), "RIFF length")
    refused("dropped", build_avi(FRAMES[:2] + [b""] + FRAMES[3:]), "zero length")
    refused("dropped_no_index", build_avi(FRAMES[:2] + [b""] + FRAMES[3:], idx=None), "zero length")
    refused("not_avi", b"RIFF" + struct.pack("<I", 4) + b"WAVE", "not a RIFF AVI")
    refused("mp4", b"\0\0\0\x18ftypmp42" + b"\0" * 16, "not a RIFF AVI.*re-encode")


# ------------------------------------------------------------------ 5: routing
def test_video_trees_route_to_the_video_dataset(tmp_path):
    from ccvs_amd.data import VideoDataset, VideoLoader
    from ccvs_amd.helpers.generator import Generator
    want_paths = {}
    for dataset in ("ucf101", "drums", "kinetics600"):
        root = tmp_path / dataset
        os.makedirs(root)
        paths = tree(root, dataset, [6, 9, 5])
        if dataset != "kinetics600":                                     # an .mp4 beside the .avi files is not listed
            open(os.path.join(os.path.dirname(list(paths.values())[0]), "zzz.mp4"), "wb").close()
        extra = ["--dataroot", root, "--true_dim", 16, "--true_ratio", 1.5]
        opts = options(dataset, extra)
        gen = Generator(opts)
        info = gen.get_data_info("valid", "vid")
        loader = info["dataloader"]
        assert isinstance(loader, VideoLoader) and isinstance(loader.dataset, VideoDataset) and info["batch_size_per_gpu"] == 2
        ds = loader.dataset
        want_paths[dataset] = ds.data["vid_paths"]
        assert sorted(ds.frame_counts) == [5, 6, 9] and len(ds) == 3 + 6 + 2 and len(loader) == 5
        assert [ds.get_clip(i)[0] for i in range(11)] == [v for v, n in enumerate(ds.frame_counts) for _ in range(n - 3)]   # every clip maps back to its video
    u = [os.path.relpath(p, tmp_path / "ucf101" / "videos") for p in want_paths["ucf101"]]
    assert u == ["g0/v0.avi", "g0/v2.avi", "g1/v1.avi"]                  # directories in sorted order, then the files
    assert [os.path.basename(p) for p in want_paths["drums"]] == ["100.avi", "101.avi", "102.avi"]
    k = [os.path.basename(p) for p in want_paths["kinetics600"]]
    assert k == ["k2.avi", "k1.avi", "k0.avi"]                           # the pickle's order, not the folder's


def test_drums_ids_and_kinetics_labels(tmp_path):
    from ccvs_amd.data import VideoDataset
    tree(tmp_path / "d", "drums", [5, 5])
    ds = VideoDataset(options("drums", ["--dataroot", tmp_path / "d", "--true_dim", 16, "--true_ratio", 1.5, "--x_stft"])["transformer"])   # --x_stft no longer raises
    assert ds.data["vid_id"] == [100, 101] and [ds.choose(i)["vid_id"] for i in range(4)] == [100, 100, 101, 101]
    assert ds.data["stft_paths"] == [p.replace("/mp4/", "/stft_pickle/").replace(".avi", ".pickle") for p in ds.data["vid_paths"]]
    tree(tmp_path / "k", "kinetics600", [4, 6])
    opt = options("kinetics600", ["--dataroot", tmp_path / "k", "--true_dim", 16, "--true_ratio", 1.5, "--resize_center_crop_img", 16, "--load_data"])["transformer"]
    ds = VideoDataset(opt)
    assert ds.frame_counts == [6, 4] and ds.data["vid_labels"] == [0, 1]
    assert [ds.choose(i)["vid_lbl"] for i in range(len(ds))] == [0, 0, 0, 1]
    os.rename(tmp_path / "k" / "valid_data.pkl", tmp_path / "k" / "spec_valid_data.pkl")            # --data_specs names the file
    with pytest.raises(FileNotFoundError):
        VideoDataset(opt)
    opt.data_specs = "spec"
    assert VideoDataset(opt).frame_counts == [6, 4]


def test_folders_without_avi_still_raise(tmp_path):
    from ccvs_amd.helpers.generator import Generator
    for dataset, folder in (("ucf101", "videos"), ("drums", "AudioSet_Dataset/test/mp4"), ("kinetics600", "clips")):
        for fill in ("empty", "mp4"):
            root = tmp_path / f"{dataset}_{fill}"
            os.makedirs(root / folder)
            if fill == "mp4":
                open(root / folder / "7.mp4", "wb").close()
                if dataset == "kinetics600":
                    with open(root / "valid_data.pkl", "wb") as fh:
                        pickle.dump({"vid_paths": [str(root / folder / "7.mp4")], "vid_labels": [0]}, fh)
            with pytest.raises(NotImplementedError, match="video"):
                Generator(options(dataset, ["--dataroot", root])).get_data_info("valid", "vid")
    root = tmp_path / "ucf101_mp4"
    for flag, match in (("--load_state", "load_state"), ("--layout", "layout")):
        with pytest.raises(NotImplementedError, match=match):
            Generator(options("ucf101", ["--dataroot", root, flag])).get_data_info("valid", "vid")
    # an .avi that is not Motion-JPEG: probe_avi's refusal, with the file name and the pointer to re-encoding
    bad = tmp_path / "ucf101_xvid"
    os.makedirs(bad / "videos")
    with open(bad / "videos" / "a.avi", "wb") as fh:
        fh.write(build_avi(FRAMES, fourcc=b"XVID"))
    with pytest.raises(ValueError, match="a.avi.*not MJPG.*re-encode"):
        Generator(options("ucf101", ["--dataroot", bad])).get_data_info("valid", "vid")


def test_transform_plan_is_the_frame_datasets(tmp_path):
    """The geometry moved to `transform_plan.py` unchanged: the same stages for both datasets, and still importable from frame_dataset."""
    from ccvs_amd.data import VideoDataset, frame_dataset, transform_plan
    assert frame_dataset.resize_target is transform_plan.resize_target and frame_dataset._Chain is transform_plan._Chain
    tree(tmp_path, "ucf101", [5])
    ds = VideoDataset(options("ucf101", ["--dataroot", tmp_path, "--resize_center_crop_img", 32, "--true_dim", 32])["transformer"])
    assert ds.plan(30, 40) == [(None, (32, 42)), ((0, 5, 32, 32), (32, 32))] and ds.out_size == (32, 32)
    assert ds.plan(32, 32) == [] and ds.norm == ((0.5,) * 3, (0.5,) * 3)


# ------------------------------------------------------------------ 6: the C ABI
def test_video_symbol_declared_and_exported(tmp_path):
    from ccvs_amd import lib, ops
    header = open(os.path.join(ROOT, "include", "ccvs_hip_video.h")).read()
    assert re.search(r'^#include "ccvs_hip_video.h"', open(os.path.join(ROOT, "include", "ccvs_hip.h")).read(), re.M)
    assert sorted(set(re.findall(r"^int (ccvs_[a-zA-Z0-9_]+)\s*\(", header, re.M))) == sorted(lib.VIDEO_EXPORTS) == ["ccvs_ingest_f32"]
    handle = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(handle, "ccvs_ingest_f32")
    c = tmp_path / "p.c"
    c.write_text('#include "ccvs_hip.h"\nvoid* p[] = {(void*)ccvs_ingest_f32};\nint n = CCVS_INGEST_MAX_STAGES + CCVS_INGEST_PRE_X2M1;\n')
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "p.o")], check=True)
    L = lib.load()
    assert L.ccvs_abi_version() == 6
    one = ctypes.c_void_p(16)
    st = lambda *rows: (ctypes.c_int32 * (6 * len(rows)))(*[v for r in rows for v in r])
    call = lambda u8, c, pre, stages, n_st, sc=64: L.ccvs_ingest_f32(one, u8, 192, sc, 1, c, 8, 8, pre, stages, n_st, None, one, 192, 64, None)
    for args, word in (((1, 3, 1, st((0, 4, 8, 8, 8, 8)), 1), "leaves"), ((1, 1, 1, st((0, 0, 8, 8, 8, 8)), 1), "channels"), ((0, 2, 0, st((0, 0, 8, 8, 8, 8)), 1), "channels"),
                       ((1, 3, 3, st((0, 0, 8, 8, 8, 8)), 1), "pre-op"), ((1, 3, 1, st((0, 0, 8, 8, 8, 8)), 4), "stages"), ((1, 3, 1, st((0, 0, 8, 8, 4, 4), (0, 0, 5, 4, 2, 2)), 2), "leaves"),
                       ((0, 3, 0, st((0, 0, 8, 8, 8, 8)), 1, 63), "stride")):
        assert call(*args) != 0 and word in L.ccvs_last_error().decode(), word
    with pytest.raises(lib.CcvsError):
        ops.ingest_f32(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    assert ops.ingest_stages(30, 40, [(None, (32, 42)), ((0, 5, 32, 32), None)]) == [(0, 0, 30, 40, 32, 42), (0, 5, 32, 32, 32, 32)]
    with pytest.raises(ValueError, match="leaves its"):
        ops.ingest_stages(8, 8, [(None, (4, 4)), ((0, 0, 5, 4), None)])
