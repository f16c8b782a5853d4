"""-m gpu: the input stage on the MI355X (`ccvs_ingest_u8`, `ops.ingest_u8`, `ccvs_amd.data`).  Every comparison is exact (torch.equal):
the kernel's arithmetic is integer and its fp32 values come from a table.

  1. uint8 form: N = 3 frames, a strided view of a larger buffer (odd frame stride), equal the restatement of tests/ingest_ref.py for
     every shape of `ingest_ref.SHAPES`, and frame 0 equals Pillow's own output stored in tests/golden/ingest_pil.npz;
  2. fp32 form: written through a slice into the middle frames of a NaN-filled [2, 5, 3, Ho, Wo] clip; the written part equals
     ((u8 / 255) - mean) / std computed by torch on the device from the uint8 form's result, for 0.5 / 0.5 and the ImageNet constants,
     and everything outside the slice is still NaN.  The division by 255 is written as a division by a 0-dim DEVICE tensor: torch's GPU
     kernel for `tensor / python_scalar` multiplies by the reciprocal instead (one bit off for about 110 of the 256 byte values), and
     the reference's ToTensor runs on the CPU, where the division is a true one.  The same values are also compared with torch's CPU
     result (`ingest_ref.normalize`);
  3. chained stages: a two-stage plan, uint8 intermediate then fp32 final, equals the same chain in the restatement;
  4. the dataset end to end: a tmp_path dataset of .npy frames through `Generator.get_data_info` -> `next_batch` equals the
     restatement's clip normalised by torch, `generate_vid` on it returns finite clips of the right shape; the same frames as PNG files
     equal the PIL chain where Pillow is importable; two videos of different frame sizes in one batch are launched group by group;
  5. `Generator.run()` on a folder of frames writes `real/` clips that are the folder's frames (the pipelined schedule reads the
     loader's clips while it runs).
"""
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ingest_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
HALF = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
IDS = [R.shape_id(s) for s in R.SHAPES]


@pytest.fixture(scope="module")
def cases(golden_dir):
    """Per shape, computed once and left unchanged: the 3 source frames, the restatement's uint8 result, Pillow's stored frame 0."""
    gold = np.load(os.path.join(golden_dir, "ingest_pil.npz"))
    out = {}
    for shape in R.SHAPES:
        _, box, size = shape
        src = R.source(shape, frames=3)
        out[R.shape_id(shape)] = dict(src=src, want=R.stage(src, box, size), pil=gold[R.shape_id(shape) + "/out"])
    return out


def strided_frames(src):
    """The frames as a view of a larger device buffer whose frame stride is odd (no frame but the first starts dword-aligned)."""
    n, per = src.shape[0], src[0].size
    stride = per + 7 if per % 2 == 0 else per + 8
    buf = torch.full((n * stride + 16,), 255, dtype=torch.uint8, device="cuda")
    view = buf.as_strided(src.shape, (stride, src.shape[2] * 3, 3, 1))
    view.copy_(torch.from_numpy(src).cuda())
    return view


def device_normalize(u8, mean, std):
    dev = u8.device
    x = u8.permute(0, 3, 1, 2).float() / torch.full((), 255.0, device=dev)
    m = torch.tensor(mean, dtype=torch.float32, device=dev)[:, None, None]
    s = torch.tensor(std, dtype=torch.float32, device=dev)[:, None, None]
    return (x - m) / s


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_uint8_form(cases, shape):
    from ccvs_amd import ops
    _, box, size = shape
    c = cases[R.shape_id(shape)]
    assert np.array_equal(c["want"][0], c["pil"]), "the restatement no longer equals Pillow's stored output"
    frames = strided_frames(c["src"])
    assert not frames.is_contiguous()
    got = ops.ingest_u8(frames, box=box, size=size, as_u8=True)
    assert got.shape == (3, size[0], size[1], 3) and got.dtype == torch.uint8
    got = got.cpu()
    diff = (got.int() - torch.from_numpy(c["want"]).int()).abs()
    print(f"{R.shape_id(shape)}: max |uint8 diff| {int(diff.max())}, differing bytes {int((diff > 0).sum())} of {diff.numel()}")
    assert torch.equal(got, torch.from_numpy(c["want"]))
    assert torch.equal(got[0], torch.from_numpy(c["pil"]))


@pytest.mark.parametrize("norm", [HALF, IMAGENET], ids=["half", "imagenet"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_fp32_form_into_a_clip_slice(cases, shape, norm):
    from ccvs_amd import ops
    _, box, size = shape
    mean, std = norm
    c = cases[R.shape_id(shape)]
    frames = strided_frames(c["src"])
    u8 = ops.ingest_u8(frames, box=box, size=size, as_u8=True)
    clip = torch.full((2, 5, 3, size[0], size[1]), float("nan"), device="cuda")
    ret = ops.ingest_u8(frames, box=box, size=size, out=clip[1, 1:4], mean=mean, std=std)
    assert ret.data_ptr() == clip[1, 1:4].data_ptr()
    want = device_normalize(u8, mean, std)
    assert torch.equal(clip[1, 1:4], want)
    assert torch.equal(clip[1, 1:4].cpu(), R.normalize(c["want"], mean, std)), "differs from torch's CPU ToTensor + Normalize"
    mask = torch.ones(clip.shape, dtype=torch.bool, device="cuda")
    mask[1, 1:4] = False
    assert bool(torch.isnan(clip[mask]).all()) and not bool(torch.isnan(clip[1, 1:4]).any())
    if norm is HALF:   # a new tensor when none is given
        fresh = ops.ingest_u8(frames, box=box, size=size)
        assert fresh.shape == (3, 3, size[0], size[1]) and torch.equal(fresh, want)


def test_chained_stages():
    from ccvs_amd import ops
    rng = np.random.RandomState(77)
    src = rng.randint(0, 256, size=(3, 41, 67, 3)).astype(np.uint8)
    plan = [((2, 3, 36, 48), (20, 27)), ((1, 2, 16, 24), (32, 32))]
    want = R.normalize(R.run_plan(src, plan))
    mid = ops.ingest_u8(torch.from_numpy(src).cuda(), box=plan[0][0], size=plan[0][1], as_u8=True)
    assert torch.equal(mid.cpu(), torch.from_numpy(R.stage(src, *plan[0])))
    got = ops.ingest_u8(mid, box=plan[1][0], size=plan[1][1])
    assert got.shape == (3, 3, 32, 32) and torch.equal(got.cpu(), want)
    # a crop with no resample at all, at a box whose left edge is not a multiple of 4 pixels (byte loads) and at one that is (dword loads)
    for box in ((3, 5, 32, 56), (3, 4, 32, 56), (0, 0, 41, 67)):
        got = ops.ingest_u8(torch.from_numpy(src).cuda(), box=box)
        assert torch.equal(got.cpu(), R.normalize(R.crop(src, box))), box
        got = ops.ingest_u8(torch.from_numpy(src).cuda(), box=box, as_u8=True)
        assert torch.equal(got.cpu(), torch.from_numpy(np.ascontiguousarray(R.crop(src, box)))), box


def test_refused_arguments():
    from ccvs_amd import lib, ops
    frames = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="leaves the"):
        ops.ingest_u8(frames, box=(0, 4, 8, 8))
    with pytest.raises(lib.CcvsError):
        ops.ingest_u8(frames.cpu())


# ------------------------------------------------------------------ 4: the dataset end to end
# the tiny configuration of tests/test_e2e_gpu.py
TINY_ARGV = [
    "--name", "tiny", "--dataset", "bairhd", "--max_dim", "32", "--vid_len", "4",
    "--q_z_num", "32", "--q_z_size", "16", "--q_z_shape", "8", "8",
    "--q_use_enc", "--q_use_dec", "--q_necf", "8", "--q_necf_mult", "1", "2", "2",
    "--q_enc_model", "skipgan", "--q_dec_model", "skipgan", "--q_use_inter", "--q_inter_p", "0.75",
    "--q_skip_context", "1", "2", "3", "--q_skip_memory", "3",
    "--x_z_num", "32", "--x_z_len", "256", "--x_n_layer", "2", "--x_n_head", "2", "--x_n_embd", "32",
    "--x_z_chunk", "64", "--x_cond_len", "64", "--x_emb_mode", "temporal", "--x_num_blocks", "4",
    "--batch_size_vid", "2",
]
# a centre crop and a resize to the tiny configuration's 32 x 32 frames: 40 x 56 -> Resize(36) 36 x 50 -> CenterCrop 36 x 36 -> Resize(32)
CHAIN_ARGV = ["--resize_center_crop_img", "36", "--true_dim", "36", "--num_workers", "2"]
WANT_PLAN = [(None, (36, 50)), ((0, 7, 36, 36), (32, 32))]


def write_dataset(root, ext):
    rng = np.random.RandomState(11)
    vids = []
    for v in ("clip_a", "clip_b"):
        d = os.path.join(root, "original_frames_256", "test", v)
        os.makedirs(d)
        vids.append(rng.randint(0, 256, size=(6, 40, 56, 3)).astype(np.uint8))
        for k in range(6):
            if ext == ".npy":
                np.save(os.path.join(d, f"{k:02d}.npy"), vids[-1][k])
            else:
                from PIL import Image
                Image.fromarray(vids[-1][k], "RGB").save(os.path.join(d, f"{k:02d}{ext}"))
    return vids


def first_batch(root, seed):
    from ccvs_amd.tools.options import Options
    from ccvs_amd.helpers.generator import Generator
    opt = Options().parse(load_qvid_generator=True, load_transformer=True, argv=TINY_ARGV + CHAIN_ARGV + ["--dataroot", root])
    gen = Generator(opt)
    info = gen.get_data_info("valid", "vid")
    assert info["batch_size_per_gpu"] == 2 and len(info["dataloader"]) == 1
    random.seed(seed)
    batch = gen.next_batch(info)
    with pytest.raises(StopIteration):       # two videos, one batch of two, --iter_function iter
        gen.next_batch(info)
    return gen, opt, batch


def restated_starts(seed):
    random.seed(seed)
    return [random.randrange(6 - 4 + 1) for _ in range(2)]


def test_dataset_end_to_end_npy(tmp_path, golden_dir):
    vids = write_dataset(str(tmp_path), ".npy")
    gen, opt, batch = first_batch(str(tmp_path), seed=13)
    assert list(batch) == ["vid"] and batch["vid"].is_cuda and batch["vid"].shape == (2, 4, 3, 32, 32) and batch["vid"].dtype == torch.float32
    assert info_plan(gen, opt) == WANT_PLAN
    starts = restated_starts(13)
    want = torch.stack([R.normalize(R.run_plan(vids[v][s:s + 4], WANT_PLAN)) for v, s in enumerate(starts)])
    assert torch.equal(batch["vid"].cpu(), want)
    # the clip through the synthesis path, with the golden run's weights
    from ccvs_amd.models.skip_vid_generator.models.quantized_video_model import QVidModel
    from ccvs_amd.models.skip_vid_generator.models.transformer_model import Transformer
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
    assert out["enc_code"].shape == (2, 4 * 64)


def info_plan(gen, opt):
    from ccvs_amd.data import FrameDataset
    return FrameDataset(opt["transformer"]).plan(40, 56)


def test_dataset_end_to_end_png_equals_the_pil_chain(tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image
    vids = write_dataset(str(tmp_path), ".png")
    _, _, batch = first_batch(str(tmp_path), seed=17)
    want = []
    for v, s in enumerate(restated_starts(17)):
        frames = []
        for f in vids[v][s:s + 4]:
            img = Image.fromarray(f, "RGB").resize((50, 36), Image.BILINEAR)      # Resize(36): the smaller edge, int(36 * 56 / 40) = 50
            img = img.crop((7, 0, 7 + 36, 36))                                    # CenterCrop(36): int(round((50 - 36) / 2.)) = 7
            frames.append(np.asarray(img.resize((32, 32), Image.BILINEAR)))      # Resize(dim)
        want.append(R.normalize(np.stack(frames)))
    assert torch.equal(batch["vid"].cpu(), torch.stack(want))


def test_loader_groups_frames_of_different_source_sizes(tmp_path):
    """Two videos of different frame sizes in one batch: launched group by group, each clip equal to the restatement's."""
    from ccvs_amd.tools.options import Options
    from ccvs_amd.helpers.generator import Generator
    rng = np.random.RandomState(3)
    vids = []
    for v, shape in (("a", (40, 56)), ("b", (36, 36))):
        d = os.path.join(str(tmp_path), "original_frames_256", "test", v)
        os.makedirs(d)
        vids.append(rng.randint(0, 256, size=(4, *shape, 3)).astype(np.uint8))
        for k in range(4):
            np.save(os.path.join(d, f"{k}.npy"), vids[-1][k])
    opt = Options().parse(True, True, argv=TINY_ARGV + ["--resize_center_crop_img", "36", "--true_dim", "36", "--num_workers", "0", "--imagenet_norm",
                                                       "--dataroot", str(tmp_path)])
    gen = Generator(opt)
    batch = gen.next_batch(gen.get_data_info("valid", "vid"))
    plans = [WANT_PLAN, [(None, (32, 32))]]
    want = torch.stack([R.normalize(R.run_plan(vids[v], plans[v]), *IMAGENET) for v in range(2)])
    assert torch.equal(batch["vid"].cpu(), want)


def test_run_writes_the_folders_frames(tmp_path):
    """`Generator(opt).run()` -- the entry point of `python -m ccvs_amd.helpers.generator` -- on a folder of frames that already have
    the clip's size (BAIR's case: no resample): the several-batches-in-flight schedule reads the loader's clips while it runs, and
    the `real/` files it writes are the folder's frames (--vid_len 4 of 4 frames per video: the clip choice has one outcome).  A real
    clip is saved as trunc(255 (x + 1) / 2) of x = (v / 255 - 0.5) / 0.5: v itself, or v - 1 where fp32 lands just below it."""
    from ccvs_amd.tools.options import Options
    from ccvs_amd.helpers.generator import Generator
    rng = np.random.RandomState(23)
    root = tmp_path / "data"
    vids = []
    for v in range(6):
        d = root / "original_frames_256" / "test" / f"traj_{v}"
        os.makedirs(d)
        vids.append(rng.randint(0, 256, size=(4, 32, 32, 3)).astype(np.uint8))
        for k in range(4):
            np.save(d / f"{k}.npy", vids[-1][k])
    opt = Options().parse(load_qvid_generator=True, load_transformer=True,
                          argv=TINY_ARGV + ["--true_dim", "32", "--n_iter", "3", "--dataroot", str(root), "--save_path", str(tmp_path / "out"), "--num_workers", "2"])
    torch.manual_seed(0)
    Generator(opt).run()
    real = os.path.join(opt["transformer"].result_path, "real")
    names = sorted(os.listdir(real))
    assert len(names) == 6, names
    if not names[0].endswith(".npy"):   # written as .mp4 where torchvision is installed: lossy, nothing to compare byte for byte
        return
    for v, name in enumerate(names):
        got = np.load(os.path.join(real, name))
        x = R.normalize(vids[v])
        want = (((x.clamp(-1, 1) - (-1.0)) / 2.0) * 255.0).to(torch.uint8).permute(0, 2, 3, 1).numpy()
        assert np.array_equal(got, want), name
        assert int(np.abs(got.astype(int) - vids[v].astype(int)).max()) <= 1
