"""not gpu: the host side of the input stage.

  1. `ops.resample_tables` (vectorised, torch float64) equals the tables of the restatement tests/ingest_ref.py (Python doubles, one
     output sample at a time) for every (in, out) pair of `ingest_ref.SHAPES`;
  2. the restatement equals Pillow's own `Image.resize(..., BILINEAR)` on every shape (the one test here that needs Pillow), and the
     stored tests/golden/ingest_pil.npz is what the installed restatement gives;
  3. `FrameDataset.plan`, applied with the restatement, equals the reference's chain written out with `Image.resize` / `crop` under
     torchvision 0.8.1's size rules, for the default branch, --resize_center_crop_img, --resize_img + --fixed_crop + --centered_crop,
     --fixed_top_centered_zoom and a source that already has the target size (empty plan);
  4. discovery order and grouping, the clip choice under `random.seed` against the restated draws, --one_every_n, a too-short video;
  5. no dataroot: the synthetic batch, as before; a video-file dataset raises;
  6. `lib.INPUT_EXPORTS` equals what include/ccvs_hip_input.h declares, and the built library exports it.
"""
import ctypes
import hashlib
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ingest_ref as R  # noqa: E402

TINY = ["--name", "tiny", "--dataset", "bairhd", "--max_dim", "32", "--vid_len", "4", "--q_z_num", "32", "--q_z_size", "16",
        "--q_z_shape", "8", "8", "--q_use_enc", "--q_use_dec", "--q_necf", "8", "--q_necf_mult", "1", "2", "2",
        "--q_enc_model", "skipgan", "--q_dec_model", "skipgan", "--q_use_inter", "--q_inter_p", "0.75",
        "--q_skip_context", "1", "2", "3", "--q_skip_memory", "3", "--x_z_num", "32", "--x_z_len", "256", "--x_n_layer", "2",
        "--x_n_head", "2", "--x_n_embd", "32", "--x_z_chunk", "64", "--x_cond_len", "64", "--x_emb_mode", "temporal",
        "--x_num_blocks", "4", "--batch_size_vid", "2"]


def axis_pairs():
    pairs = set()
    for (hs, ws), box, (ho, wo) in R.SHAPES:
        hc, wc = (hs, ws) if box is None else box[2:]
        pairs.update([(hc, ho), (wc, wo)])
    return sorted(pairs)


def write_tree(root, videos, frames, shape=(40, 56), ext=".npy", seed=5):
    """<root>/original_frames_256/test/<video>/<k>.npy with seeded random frames; returns {video: uint8 [frames, H, W, 3]}."""
    rng = np.random.RandomState(seed)
    out = {}
    for v in videos:
        d = os.path.join(root, "original_frames_256", "test", v)
        os.makedirs(d)
        out[v] = rng.randint(0, 256, size=(frames, *shape, 3)).astype(np.uint8)
        for k in range(frames):
            if ext == ".npy":
                np.save(os.path.join(d, f"{k:03d}.npy"), out[v][k])
            else:
                from PIL import Image
                Image.fromarray(out[v][k], "RGB").save(os.path.join(d, f"{k:03d}{ext}"))
    return out


def options(extra):
    from ccvs_amd.tools.options import Options
    return Options().parse(load_qvid_generator=True, load_transformer=True, argv=TINY + [str(v) for v in extra])


# ------------------------------------------------------------------ 1, 2: the resampler
@pytest.mark.parametrize("pair", axis_pairs(), ids=lambda p: f"{p[0]}to{p[1]}")
def test_resample_tables_equal_the_restatement(pair):
    from ccvs_amd import ops
    coef, bounds = ops.resample_tables(*pair)
    want_coef, want_bounds = R.tables(*pair)
    assert coef.dtype == bounds.dtype == torch.int32 and coef.device.type == "cpu"
    assert np.array_equal(coef.numpy(), want_coef) and np.array_equal(bounds.numpy(), want_bounds)
    scale = pair[0] / pair[1]
    assert coef.shape == (pair[1], 2 * int(np.ceil(max(scale, 1.0))) + 1) and bounds.shape == (pair[1], 2)
    assert int(bounds[:, 0].min()) >= 0 and int((bounds[:, 0] + bounds[:, 1]).max()) <= pair[0]       # no tap outside the input
    assert int((coef.sum(dim=1) - (1 << 22)).abs().max()) <= coef.shape[1]                             # weights sum to one, up to rounding
    assert ops.resample_tables(*pair)[0] is coef                                                       # cached


def test_restatement_equals_pillow_on_every_shape(golden_dir):
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    gold = np.load(os.path.join(golden_dir, "ingest_pil.npz"))
    print("Pillow", PIL.__version__, "; golden file made with", str(gold["pillow_version"]))
    for shape in R.SHAPES:
        _, box, size = shape
        frame = R.source(shape)[0]
        img = Image.fromarray(frame, "RGB")
        if box is not None:
            img = img.crop((box[1], box[0], box[1] + box[3], box[0] + box[2]))
        want = np.asarray(img.resize((size[1], size[0]), Image.BILINEAR))
        got = R.stage(frame, box, size)
        diff = int(np.abs(got.astype(int) - want.astype(int)).max())
        print(R.shape_id(shape), "max |restatement - Pillow| =", diff)
        assert diff == 0 and got.shape == want.shape
        assert np.array_equal(want, gold[R.shape_id(shape) + "/out"])


def test_golden_file_is_what_the_restatement_gives(golden_dir):
    """Needs no Pillow: the stored outputs, the stored inputs and the digests of the regenerated ones."""
    path = os.path.join(golden_dir, "ingest_pil.npz")
    assert os.path.getsize(path) < 300 << 10
    gold = np.load(path)
    assert str(gold["pillow_version"])
    for shape in R.SHAPES:
        key = R.shape_id(shape)
        frame = R.source(shape)[0]
        assert hashlib.sha256(frame.tobytes()).hexdigest() == str(gold[key + "/sha"]), key
        if key + "/in" in gold.files:
            assert np.array_equal(gold[key + "/in"], frame)
        assert np.array_equal(R.stage(frame, shape[1], shape[2]), gold[key + "/out"]), key
    assert sum((R.shape_id(s) + "/in") in gold.files for s in R.SHAPES) >= 8


# ------------------------------------------------------------------ 3: the chain
def tv_resize(img, size):
    """torchvision 0.8.1 `Resize(size, BILINEAR)` on a PIL image."""
    from PIL import Image
    if isinstance(size, (list, tuple)) and len(size) == 1:
        size = size[0]
    if isinstance(size, int):
        w, h = img.size
        if (w <= h and w == size) or (h <= w and h == size):
            return img
        if w < h:
            return img.resize((size, int(size * h / w)), Image.BILINEAR)
        return img.resize((int(size * w / h), size), Image.BILINEAR)
    return img.resize((size[1], size[0]), Image.BILINEAR)


def tv_crop(img, top, left, h, w):
    return img.crop((left, top, left + w, top + h))


def pil_chain(frame, opt, dim, offsets=(0.5, 0.5)):
    """data/base_dataset.py:120-165 (validation) and :348-357 on one frame, with PIL."""
    from PIL import Image
    img = Image.fromarray(frame, "RGB")
    h, w = int(opt.true_dim), int(opt.true_dim * opt.true_ratio)
    scale = None
    if opt.fixed_top_centered_zoom:
        h_crop = int(h / opt.fixed_top_centered_zoom)
        w_crop = int(h_crop * opt.aspect_ratio)
        top, left = 0, int((w - w_crop) / 2)
    elif opt.fixed_crop:
        h_crop, w_crop = opt.fixed_crop
        scale = (int(h * 1.), int(w * 1.))
        top, left = int(offsets[0] * (scale[0] - h_crop)), int(offsets[1] * (scale[1] - w_crop))
    else:
        zoom = max(1., opt.aspect_ratio / opt.true_ratio)
        h_crop = int(h / zoom)
        w_crop = int(h_crop * opt.aspect_ratio)
        top, left = 0, 0
    if opt.resize_img is not None:
        img = tv_resize(img, list(opt.resize_img))
    if opt.resize_center_crop_img is not None:
        s = opt.resize_center_crop_img
        img = tv_resize(img, s)
        iw, ih = img.size
        img = tv_crop(img, int(round((ih - s) / 2.)), int(round((iw - s) / 2.)), s, s)
    if scale is not None:
        img = tv_resize(img, list(scale))
    img = tv_crop(img, top, left, h_crop, w_crop)
    img = tv_resize(img, dim)
    return np.asarray(img)


CHAINS = {
    # name: (source (h, w), extra flags, number of stages)
    "default": ((40, 56), ["--true_dim", 40, "--true_ratio", 1.4, "--aspect_ratio", 1.0], 1),
    "default_wide": ((48, 96), ["--true_dim", 48, "--true_ratio", 2.0, "--aspect_ratio", 2.0, "--dim", 16], 1),
    "resize_center_crop": ((40, 56), ["--resize_center_crop_img", 36, "--true_dim", 36], 2),
    "resize_fixed_centered": ((45, 71), ["--resize_img", 50, 64, "--fixed_crop", 32, 32, "--centered_crop", "--true_dim", 50, "--true_ratio", 1.28], 2),
    "fixed_random_offsets": ((50, 64), ["--fixed_crop", 32, 32, "--true_dim", 50, "--true_ratio", 1.28], 1),
    "top_centered_zoom": ((60, 80), ["--fixed_top_centered_zoom", 1.5, "--true_dim", 60, "--true_ratio", 1.3333334], 1),
    "already_the_target": ((32, 32), ["--true_dim", 32], 0),
}


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_plan_equals_the_pil_chain(tmp_path, name):
    pytest.importorskip("PIL")
    from ccvs_amd.data import FrameDataset
    (h, w), extra, n_stages = CHAINS[name]
    write_tree(str(tmp_path), ["v"], 4, shape=(h, w))
    opt = options(["--dataroot", tmp_path] + extra)["transformer"]
    ds = FrameDataset(opt, phase="valid", load_vid=True)
    frame = np.random.RandomState(9).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    offsets = (0.3, 0.8) if name == "fixed_random_offsets" else (0.5, 0.5)
    plan = ds.plan(h, w, offsets)
    print(name, plan)
    assert len(plan) == n_stages
    want = pil_chain(frame, opt, ds.dim, offsets)
    got = R.run_plan(frame, plan)
    assert got.shape == want.shape == (*ds.out_size, 3) and np.array_equal(got, want)
    if name == "fixed_random_offsets":   # the two draws the reference makes even in validation
        random.seed(3)
        a, b = random.random(), random.random()
        random.seed(3)
        assert ds.crop_offsets() == (a, b)
    else:
        state = random.getstate()
        assert ds.crop_offsets() == (0.5, 0.5) and random.getstate() == state


def test_plan_refuses_a_crop_that_leaves_the_image(tmp_path):
    from ccvs_amd.data import FrameDataset
    write_tree(str(tmp_path), ["v"], 4, shape=(40, 56))
    ds = FrameDataset(options(["--dataroot", tmp_path, "--true_dim", 64])["transformer"])
    with pytest.raises(ValueError, match="leaves the 40 x 56 image"):
        ds.plan(40, 56)
    ds = FrameDataset(options(["--dataroot", tmp_path, "--true_dim", 40, "--true_ratio", 1.4, "--aspect_ratio", 1.4])["transformer"])
    assert ds.out_size == (32, 44) and ds.plan(40, 56) == [(None, (32, 44))]
    # a portrait crop: Resize(dim) sizes the smaller edge, the width, and the 64 x 32 result is not the 32 x 16 clip the reference allocates
    ds = FrameDataset(options(["--dataroot", tmp_path, "--true_dim", 40, "--true_ratio", 1.4, "--aspect_ratio", 0.5])["transformer"])
    with pytest.raises(ValueError, match="not the clip's 32 x 16"):
        ds.plan(40, 56)


# ------------------------------------------------------------------ 4: discovery and clip choice
def test_discovery_grouping_and_clip_choice(tmp_path):
    from ccvs_amd.data import FrameDataset, make_dataset, IMG_EXTENSIONS
    assert IMG_EXTENSIONS == ['.jpg', '.JPG', '.jpeg', '.JPEG', '.png', '.PNG', '.ppm', '.PPM', '.bmp', '.BMP', '.tiff', '.webp']
    vids = write_tree(str(tmp_path), ["b", "a/x"], 9)
    root = os.path.join(str(tmp_path), "original_frames_256", "test")
    open(os.path.join(root, "b", "notes.txt"), "w").write("not a frame")
    paths = make_dataset(root)
    want = [os.path.join(root, v, f"{k:03d}.npy") for v in ("a/x", "b") for k in range(9)]
    assert paths == want
    opt = options(["--dataroot", tmp_path, "--true_dim", 40, "--true_ratio", 1.4])["transformer"]
    ds = FrameDataset(opt, phase="valid", load_vid=True)
    assert len(ds) == 2 and ds.vid_frame_paths == [want[:9], want[9:]]
    assert len(FrameDataset(opt, phase="valid", load_vid=False)) == 18
    # the clip choice: idx = random.randrange(len - vid_len * one_every_n + 1), frames idx : idx + vid_len * n : n
    for seed in (0, 1, 2):
        random.seed(seed)
        idx = [random.randrange(9 - 4 + 1) for _ in range(2)]
        random.seed(seed)
        for v, (i, name) in enumerate(zip(idx, ("a/x", "b"))):
            item = ds.choose(v)
            assert item["paths"] == want[9 * v + i:9 * v + i + 4] and item["offsets"] == (0.5, 0.5) and "tgt_vid_lbl" not in item
            frames, plan = ds.decode(item)
            assert np.array_equal(frames, vids[name][i:i + 4]) and plan == ds.plan(40, 56)
    ds2 = FrameDataset(options(["--dataroot", tmp_path, "--true_dim", 40, "--true_ratio", 1.4, "--one_every_n", 2])["transformer"])
    random.seed(4)
    i = random.randrange(9 - 8 + 1)
    random.seed(4)
    assert ds2.choose(1)["paths"] == want[9 + i:9 + i + 8:2]
    ds3 = FrameDataset(options(["--dataroot", tmp_path, "--true_dim", 40, "--true_ratio", 1.4, "--one_every_n", 3])["transformer"])
    with pytest.raises(ValueError, match="9 frames, a clip needs 4 frames, one every 3"):
        ds3.choose(0)
    # a single frame item: the 'img' branch draws nothing
    state = random.getstate()
    item = FrameDataset(opt, phase="valid", load_vid=False).choose(10)
    assert item["paths"] == [want[10]] and random.getstate() == state


def test_loader_order_and_sharding(tmp_path):
    from ccvs_amd.data import FrameDataset, FrameLoader
    write_tree(str(tmp_path), [f"v{k}" for k in range(5)], 4)
    opt = options(["--dataroot", tmp_path, "--true_dim", 40, "--true_ratio", 1.4])["transformer"]
    ds = FrameDataset(opt)
    steps = lambda ld, n: [s for s, _ in zip(ld._steps(), range(n))]
    assert steps(FrameLoader(ds, 2), 9) == [[0, 1], [2, 3]]                                    # drop_last
    assert steps(FrameLoader(ds, 2, 1, 2), 9) == [[1], [3]]                                    # rank 1 of 2
    assert steps(FrameLoader(ds, 2, cycle=True), 5) == [[0, 1], [2, 3], [0, 1], [2, 3], [0, 1]]
    opt.shuffle_valid, opt.seed = True, 7
    perm = torch.randperm(5, generator=torch.Generator().manual_seed(7 * 1000003)).tolist()
    assert steps(FrameLoader(ds, 2), 9) == [perm[0:2], perm[2:4]] and sorted(perm) == list(range(5))
    with pytest.raises(ValueError, match="fewer than one batch"):
        FrameLoader(ds, 6)


# ------------------------------------------------------------------ 5: the switch in get_data_info
def test_missing_dataroot_is_the_synthetic_batch_and_video_datasets_raise(tmp_path):
    from ccvs_amd.helpers.generator import Generator
    for extra in ([], ["--dataroot", os.path.join(str(tmp_path), "nowhere")]):
        gen = Generator(options(extra))
        info = gen.get_data_info("valid", "vid")
        assert info["dataloader"] is None and info["batch_size_per_gpu"] == 2
        for it in range(2):
            batch = gen.next_batch(info)
            assert list(batch) == ["vid"] and torch.equal(batch["vid"], gen.synthetic_batch(2, seed=1 + it, first_clip=0)["vid"])
    os.makedirs(os.path.join(str(tmp_path), "vids"))
    for dataset in ("kinetics600", "drums", "ucf101"):
        argv = [a if a != "bairhd" else dataset for a in TINY] + ["--dataroot", os.path.join(str(tmp_path), "vids")]
        from ccvs_amd.tools.options import Options
        gen = Generator(Options().parse(True, True, argv=argv))
        with pytest.raises(NotImplementedError, match="video"):
            gen.get_data_info("valid", "vid")
    with pytest.raises(FileNotFoundError, match="original_frames_256"):
        Generator(options(["--dataroot", os.path.join(str(tmp_path), "vids")])).get_data_info("valid", "vid")
    with pytest.raises(NotImplementedError, match="load_state"):
        Generator(options(["--dataroot", os.path.join(str(tmp_path), "vids"), "--load_state"])).get_data_info("valid", "vid")


def test_new_flags_have_the_reference_defaults():
    from ccvs_amd.tools.options import Options
    o = Options()
    b = o.parse(True, True, argv=TINY)["transformer"]
    assert (b.resize_img, b.resize_center_crop_img, b.fixed_crop, b.centered_crop, b.fixed_top_centered_zoom, b.one_every_n, b.shuffle_valid) == \
        (None, None, None, False, None, 1, False)
    k = Options().parse(True, True, argv=[a if a != "bairhd" else "kinetics600" for a in TINY] + ["--shuffle_valid", "--centered_crop"])["qvid_generator"]
    assert k.resize_center_crop_img == 256 and k.shuffle_valid and k.centered_crop and k.imagenet_norm
    u = Options().parse(True, True, argv=[a if a != "bairhd" else "ucf101" for a in TINY])["transformer"]
    assert u.resize_center_crop_img == 256
    f = Options().parse(True, True, argv=TINY + ["--fixed_crop", "24", "40", "--one_every_n", "2"])["transformer"]
    assert f.fixed_crop == [24, 40] and (f.height_size, f.width_size) == (24, 40) and f.one_every_n == 2


# ------------------------------------------------------------------ 6: the C ABI
def test_input_symbol_declared_and_exported(tmp_path):
    from ccvs_amd import lib, ops
    header = open(os.path.join(ROOT, "include", "ccvs_hip_input.h")).read()
    assert re.search(r'^#include "ccvs_hip_input.h"', open(os.path.join(ROOT, "include", "ccvs_hip.h")).read(), re.M)
    assert sorted(set(re.findall(r"\b(ccvs_[a-zA-Z0-9_]+)\s*\(", header))) == sorted(lib.INPUT_EXPORTS) == ["ccvs_ingest_u8"]
    assert not set(lib.INPUT_EXPORTS) & (set(lib.EXPORTS) | set(lib.EVAL_EXPORTS)) and len(lib.EXPORTS) == 51
    handle = ctypes.CDLL(lib.LIB_PATH)
    for sym in lib.INPUT_EXPORTS:
        assert hasattr(handle, sym), sym
    c = tmp_path / "p.c"
    c.write_text('#include "ccvs_hip.h"\nvoid* p[] = {' + ", ".join("(void*)" + s for s in lib.INPUT_EXPORTS) + "};\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "p.o")], check=True)
    L = lib.load()
    assert L.ccvs_abi_version() == 6
    # refused before any GPU call: a crop box that leaves the frame, both outputs at once, a missing table with a size change
    one = ctypes.c_void_p(16)
    assert L.ccvs_ingest_u8(one, 0, 1, 8, 8, 0, 4, 8, 8, None, None, 0, None, None, 0, 8, 8, one, None, 0, 0, None, None) != 0
    assert "leaves" in L.ccvs_last_error().decode()
    assert L.ccvs_ingest_u8(one, 0, 1, 8, 8, 0, 0, 8, 8, None, None, 0, None, None, 0, 8, 8, one, one, 64, 64, one, None) != 0
    assert L.ccvs_ingest_u8(one, 0, 1, 8, 8, 0, 0, 8, 8, None, None, 0, None, None, 0, 4, 8, one, None, 0, 0, None, None) != 0
    with pytest.raises(lib.CcvsError):
        ops.ingest_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    lut = ops.norm_table((0.5,) * 3, (0.5,) * 3, "cpu")
    assert lut.shape == (3, 256) and lut[0, 0] == -1.0 and lut[2, 255] == 1.0
    assert torch.equal(lut, R.normalize(np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, axis=2))[:, 0])
