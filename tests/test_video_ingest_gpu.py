"""-m gpu: the video-file datasets' input stage on the MI355X (`ccvs_ingest_f32`, `ops.ingest_f32`, `ccvs_amd.data.VideoDataset` /
`VideoLoader`).  Every comparison is exact (torch.equal): the kernel's operations are single correctly rounded
fp32 ones in the order of the mirror tests/video_ingest_ref.py, which tests/test_video_dataset_host.py holds against torch's own chain.

  1. `ops.ingest_f32` == mirror for every row of `video_ingest_ref.ROWS` (uint8 C = 3, fp32 C = 1 and C = 3, boxes at every edge, a row
     past one block's width, output widths that are and are not multiples of 4, N = 1 .. 5), without a post-op and with both
     normalisations, written into the middle frames of a NaN-filled clip from a strided source: outside the slice everything stays NaN;
  2. fused == staged, bit for bit, on every multi-stage row (three stages included), and the default form is the documented one;
  3. the datasets end to end: tiny Motion-JPEG AVI trees (Pillow-encoded 4:2:0 / 4:4:4 / restart-marker frames of 16 x 24 and 30 x 40
     wrapped by `write_avi`) through `VideoLoader`: `batch["vid"]` equals mirror(Pillow-decoded frames of the chosen numbers), the drums
     batch's `stft` equals the mirror on the pickles and `vid_id` is passed through; two source sizes in one batch;
  4. `Generator.get_data_info` + `next_batch` on the ucf101 tree feed `generate_vid`, and `run()` writes the ingested frames to `real/`.
"""
import io
import os
import pickle
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import video_ingest_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [r[0] for r in R.ROWS]
MULTI = [r for r in R.ROWS if len(r[3]) > 1]


@pytest.fixture(scope="module")
def sources():
    """Per row, made once and left unchanged: the source array."""
    return {r[0]: R.row_source(r) for r in R.ROWS}


def device_source(src):
    """uint8 frames as a view of a larger device buffer with an odd frame stride > H * W * 3; fp32 planes as they are."""
    if src.dtype != np.uint8:
        return torch.from_numpy(src).cuda()
    n, per = src.shape[0], src[0].size
    stride = per + 7 if per % 2 == 0 else per + 8
    buf = torch.full((n * stride + 16,), 255, dtype=torch.uint8, device="cuda")
    view = buf.as_strided(src.shape, (stride, src.shape[2] * 3, 3, 1))
    view.copy_(torch.from_numpy(src).cuda())
    assert n == 1 or not view.is_contiguous()
    return view


def norms_of(c):
    return [None, R.HALF, R.IMAGENET] if c == 3 else [None, ((0.5,), (0.5,)), ((0.25,), (0.75,))]


@pytest.mark.parametrize("row", R.ROWS, ids=IDS)
def test_ingest_f32_equals_the_mirror_inside_a_nan_clip(sources, row):
    from ccvs_amd import ops
    name, kind, (n, c, hs, ws), stages, pre = row
    src = sources[name]
    dev = device_source(src)
    for norm in norms_of(c):
        mean, std = norm if norm else (None, None)
        want = torch.from_numpy(R.chain(src, stages, pre, mean, std))
        ho, wo = want.shape[-2:]
        clip = torch.full((2, n + 2, c, ho, wo), float("nan"), device="cuda")
        ret = ops.ingest_f32(dev, stages, out=clip[1, 1:n + 1], pre=pre, mean=mean, std=std)
        assert ret.data_ptr() == clip[1, 1:n + 1].data_ptr()
        got = clip[1, 1:n + 1].cpu()
        bad = int((got != want).sum())
        print(f"{name} norm={norm is not None}: {bad} of {want.numel()} values differ, max |diff| {float((got - want).abs().max()):.3e}")
        assert torch.equal(got, want)
        mask = torch.ones(clip.shape, dtype=torch.bool, device="cuda")
        mask[1, 1:n + 1] = False
        assert bool(torch.isnan(clip[mask]).all()) and not bool(torch.isnan(clip[1, 1:n + 1]).any())
    fresh = ops.ingest_f32(dev, stages, pre=pre)                                       # a new tensor when none is given
    assert fresh.is_contiguous() and torch.equal(fresh.cpu(), torch.from_numpy(R.chain(src, stages, pre)))


def test_output_into_a_clip_slice_of_the_issue_shape(sources):
    """`clip[b, 1:3]` of a [2, 4, 3, H, W] clip, N = 2, both normalisations."""
    from ccvs_amd import ops
    row = R.ROWS[1]
    src = sources[row[0]]
    for mean, std in (R.HALF, R.IMAGENET):
        want = torch.from_numpy(R.chain(src, row[3], row[4], mean, std))
        clip = torch.full((2, 4, 3, 8, 8), float("nan"), device="cuda")
        ops.ingest_f32(torch.from_numpy(src).cuda(), row[3], out=clip[0, 1:3], mean=mean, std=std)
        assert torch.equal(clip[0, 1:3].cpu(), want)
        assert bool(torch.isnan(clip[1]).all()) and bool(torch.isnan(clip[0, 0]).all()) and bool(torch.isnan(clip[0, 3]).all())


@pytest.mark.parametrize("row", MULTI, ids=[r[0] for r in MULTI])
def test_fused_equals_staged(sources, row):
    from ccvs_amd import ops
    name, kind, (n, c, hs, ws), stages, pre = row
    dev = device_source(sources[name])
    mean, std = (R.IMAGENET if c == 3 else ((0.25,), (0.75,)))
    fused = ops.ingest_f32(dev, stages, pre=pre, mean=mean, std=std, fused=True)
    staged = ops.ingest_f32(dev, stages, pre=pre, mean=mean, std=std, fused=False)
    assert torch.equal(fused.view(torch.int32), staged.view(torch.int32))             # the same bits, not only the same values
    assert torch.equal(fused.cpu(), torch.from_numpy(R.chain(sources[name], stages, pre, mean, std)))
    default = ops.ingest_f32(dev, stages, pre=pre, mean=mean, std=std)
    assert torch.equal(default.view(torch.int32), staged.view(torch.int32))


def test_refused_arguments():
    from ccvs_amd import lib, ops
    frames = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="leaves its"):
        ops.ingest_f32(frames, [((0, 4, 8, 8), None)])
    with pytest.raises(ValueError, match="at most 3"):
        ops.ingest_f32(frames, [(None, (4, 4))] * 4)
    with pytest.raises(ValueError, match="pre-op"):
        ops.ingest_f32(frames, pre="sqrt")
    with pytest.raises(lib.CcvsError):
        ops.ingest_f32(frames.cpu())


# ------------------------------------------------------------------ 3: the datasets end to end
def encode(frames, subsampling, restart=0):
    from PIL import Image
    out = []
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(f, "RGB").save(buf, format="JPEG", quality=90, subsampling=subsampling, restart_marker_blocks=restart)
        out.append(buf.getvalue())
    return out


def pillow_decode(jpegs):
    from PIL import Image
    return np.stack([np.asarray(Image.open(io.BytesIO(j)).convert("RGB")) for j in jpegs])


# three clips per dataset: (frames, (h, w), Pillow's subsampling number, restart interval in MCUs)
CLIPS = [(6, (16, 24), 2, 0), (5, (30, 40), 0, 0), (6, (16, 24), 2, 2)]
NAMES = {"ucf101": ["a/x.avi", "b/y.avi", "c/z.avi"], "drums": ["100.avi", "101.avi", "102.avi"], "kinetics600": ["k0.avi", "k1.avi", "k2.avi"]}


def make_tree(root, dataset):
    """Writes the dataset's three clips; returns [(path, jpeg files)] in the order the dataset lists them."""
    rng = np.random.RandomState(len(dataset))
    clips, files = {}, {}
    for name, (n, (h, w), sub, rst) in zip(NAMES[dataset], CLIPS):
        smooth = rng.randint(0, 256, size=(n, h // 4 + 1, w // 4 + 1, 3)).astype(np.uint8).repeat(4, axis=1).repeat(4, axis=2)[:, :h, :w]
        files[name] = encode(smooth ^ rng.randint(0, 16, size=smooth.shape).astype(np.uint8), sub, rst)
        clips[name] = (files[name], h, w)
    paths = R.write_video_tree(str(root), dataset, clips)
    order = sorted(NAMES[dataset], reverse=dataset == "kinetics600")    # kinetics600: the pickle's order (write_video_tree reverses it)
    return [(paths[n], files[n]) for n in order]


def parse(dataset, extra):
    from ccvs_amd.tools.options import Options
    return Options().parse(load_qvid_generator=True, load_transformer=True, argv=R.tiny_argv(dataset) + [str(v) for v in extra])


def stages_for(h, w, mode):
    if mode == "rcc32":      # Resize(32) -> CenterCrop(32) -> the true_dim crop and Resize(32) change nothing
        return [(None, (32, 48)), ((0, 8, 32, 32), (32, 32))] if (h, w) == (16, 24) else [(None, (32, 42)), ((0, 5, 32, 32), (32, 32))]
    return [((0, 0, 16, 16), (32, 32))]                                  # drums: the 16 x 16 crop of --true_dim 16, Resize(32)


@pytest.mark.parametrize("dataset", ["ucf101", "kinetics600", "drums"])
def test_loader_equals_the_mirror_on_pillow_frames(tmp_path, dataset):
    pytest.importorskip("PIL")
    from ccvs_amd.data import VideoDataset, VideoLoader
    videos = make_tree(tmp_path, dataset)
    if dataset == "drums":
        extra, mode, length = ["--true_dim", 16, "--true_ratio", 1.5, "--load_vid_len", 5, "--max_vid_step", 2, "--x_stft"], "crop16", 5
        rng = np.random.RandomState(9)
        stfts = [rng.rand(len(f), 20, 6) for _, f in videos]
        os.makedirs(tmp_path / "AudioSet_Dataset" / "test" / "stft_pickle")
        for (path, _), arr in zip(videos, stfts):
            with open(path.replace("/mp4/", "/stft_pickle/").replace(".avi", ".pickle"), "wb") as fh:
                pickle.dump(arr, fh)
    else:
        extra, mode, length = ["--resize_center_crop_img", 32, "--true_dim", 32], "rcc32", 4
    opt = parse(dataset, ["--dataroot", tmp_path, "--num_workers", 2] + extra)["transformer"]
    ds = VideoDataset(opt)
    assert [p for p, _ in videos] == ds.data["vid_paths"]
    clips = [(v, list(range(s, s + length))) for v, (_, f) in enumerate(videos) for s in range(len(f) - length + 1)]
    assert len(ds) == len(clips)
    loader = VideoLoader(ds, 2)
    random.seed(3)
    batches = list(loader)
    assert len(batches) == len(clips) // 2 and loader.bad_units is None             # (the finished iteration checked the status words)
    norm = R.IMAGENET if dataset == "kinetics600" else R.HALF
    random.seed(3)
    sizes_in_a_batch, raw = set(), 0
    for s, batch in enumerate(batches):
        assert batch["vid"].shape == (2, 4, 3, 32, 32) and batch["vid"].dtype == torch.float32 and batch["vid"].is_cuda
        shapes = set()
        for k in range(2):
            video, numbers = clips[2 * s + k]
            sl = slice(None)
            if dataset == "drums":
                step = min(max(1, int(random.random() * (5 - 1) / (4 - 1))), 2)
                sl = slice(0, step * 3 + 1, step)
                numbers = numbers[sl]
            frames = pillow_decode([videos[video][1][f] for f in numbers])
            shapes.add(frames.shape[1:3])
            raw += frames.nbytes
            want = R.chain(frames, stages_for(*frames.shape[1:3], mode), "div255", *norm)
            assert torch.equal(batch["vid"][k].cpu(), torch.from_numpy(want)), (s, k)
            if dataset == "drums":
                want_stft = R.chain(stfts[video][sl].astype(np.float32)[:, None], [(None, (64, 16))], "x2m1")
                assert batch["stft"].shape == (2, 4, 1, 64, 16) and torch.equal(batch["stft"][k].cpu(), torch.from_numpy(want_stft)), (s, k)
                assert int(batch["vid_id"][k]) == 100 + video
            if dataset == "kinetics600":
                assert int(batch["vid_lbl"][k]) == video
        sizes_in_a_batch.add(len(shapes))
    assert sizes_in_a_batch == {1, 2}, "no batch mixed two source sizes"
    assert 0 < loader.bytes_up and loader.bytes_raw == raw
    print(f"{dataset}: {loader.bytes_up} bytes uploaded (tables + compressed scans + STFT) for {loader.bytes_raw} bytes of raw uint8 frames")


def test_corrupt_scan_is_reported_by_check_not_per_batch(tmp_path):
    pytest.importorskip("PIL")
    from ccvs_amd.data import VideoDataset, VideoLoader
    from ccvs_amd.tools import mjpeg
    rng = np.random.RandomState(1)
    files = encode(rng.randint(0, 256, size=(4, 16, 24, 3)).astype(np.uint8), 2)
    scan = mjpeg.parse_jpeg(files[2])["scan_offset"]
    files[2] = files[2][:scan] + bytes(b if b != 0xFF else 0x7F for b in files[2][scan:scan + 40]) + files[2][scan + 200:]   # a scan cut short
    R.write_video_tree(str(tmp_path), "ucf101", {"bad.avi": (files, 16, 24)})
    ds = VideoDataset(parse("ucf101", ["--dataroot", tmp_path, "--resize_center_crop_img", 32, "--true_dim", 32, "--batch_size_vid", 1])["transformer"])
    loader = VideoLoader(ds, 1)
    it = iter(loader)
    batch = next(it)                                                     # the batch is returned: nothing was read back
    assert batch["vid"].shape == (1, 4, 3, 32, 32) and loader.bad_units is not None
    with pytest.raises(ValueError, match="bad.avi"):
        loader.check()


# ------------------------------------------------------------------ 4: the generator on a video dataset
def test_generator_reads_the_ucf101_tree_and_run_writes_its_frames(tmp_path, golden_dir):
    pytest.importorskip("PIL")
    from ccvs_amd.helpers.generator import Generator
    from ccvs_amd.models.skip_vid_generator.models.quantized_video_model import QVidModel
    from ccvs_amd.models.skip_vid_generator.models.transformer_model import Transformer
    videos = make_tree(tmp_path / "data", "ucf101")
    clips = [(v, list(range(s, s + 4))) for v, (_, f) in enumerate(videos) for s in range(len(f) - 3)]
    argv = ["--dataroot", tmp_path / "data", "--resize_center_crop_img", 32, "--true_dim", 32, "--num_workers", 2]
    opt = parse("ucf101", argv)
    gen = Generator(opt)
    info = gen.get_data_info("valid", "vid")
    batch = gen.next_batch(info)
    want = []
    for video, numbers in clips[:2]:
        frames = pillow_decode([videos[video][1][f] for f in numbers])
        want.append(torch.from_numpy(R.chain(frames, stages_for(*frames.shape[1:3], "rcc32"), "div255", *R.HALF)))
    assert list(batch) == ["vid"] and torch.equal(batch["vid"].cpu(), torch.stack(want))
    gold = np.load(os.path.join(golden_dir, "tiny_e2e.npz"))
    sd = lambda pre: {k[len(pre) + 1:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(pre + "/")}
    gen.vid_model = QVidModel(opt["qvid_generator"], is_train=False, is_main=True).eval()
    gen.transformer_model = Transformer(opt["transformer"], is_train=False, is_main=True).eval()
    for net, pre in ((gen.vid_model.net_e, "e"), (gen.vid_model.net_q, "q"), (gen.vid_model.net_g, "g"), (gen.transformer_model.net_t, "t")):
        assert not net.load_state_dict(sd(pre), strict=False).unexpected_keys
    out = gen.generate_vid({"vid": batch["vid"].clone()})
    torch.cuda.synchronize()
    assert torch.equal(out["real"], batch["vid"])
    for name in ("fake", "rec"):
        assert out[name]["vid"].shape == (2, 4, 3, 32, 32) and bool(torch.isfinite(out[name]["vid"]).all()), name
    info["dataloader"].check()
    # run(): the real/ files are the ingested frames, packed as save_video_batch packs them
    opt = parse("ucf101", argv + ["--n_iter", 3, "--save_path", tmp_path / "out", "--video_format", "npy"])
    torch.manual_seed(0)
    Generator(opt).run()
    real = os.path.join(opt["transformer"].result_path, "real")
    names = sorted(os.listdir(real))
    assert len(names) == 6 and all(n.endswith(".npy") for n in names), names
    for i, name in enumerate(names):
        video, numbers = clips[i]
        frames = pillow_decode([videos[video][1][f] for f in numbers])
        x = torch.from_numpy(R.chain(frames, stages_for(*frames.shape[1:3], "rcc32"), "div255", *R.HALF))
        packed = (((x.clamp(-1, 1) - (-1.0)) / 2.0) * 255.0).to(torch.uint8).permute(0, 2, 3, 1).numpy()
        assert np.array_equal(np.load(os.path.join(real, name)), packed), name
