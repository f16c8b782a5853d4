"""gpu: the lossless output stage (`ccvs_apng_encode`, csrc/png.hip) against the spec mirror tests/apng_ref.py,
which tests/test_apng_host.py holds against zlib's inflate and Pillow.  Every comparison is byte for byte.

  1. every row of the image table (and the row whose tree runs the length limiter): offsets and stream equal the mirror's, written
     into a stream pre-filled with 0xFF from a workspace filled with garbage; nothing at or beyond offsets[n] is touched;
  2. five frames in one launch equal their five single launches, also under a CU budget that makes the workgroups walk across frames;
     twice, the same bytes; a clip with frame_stride > 3 w h whose padding holds garbage;
  3. capacity 0, 1, one band short and exactly enough: complete offsets, nothing at or beyond `capacity`, status 0 as the mjpeg
     encoders give it; `ops.png_encode_to_host` runs again where the default capacity is too small;
  4. `save_video_batch(video_format="apng")`: Pillow's frames of the files equal the returned clip, for both normalisation branches,
     with a state marker and with cat / idx suffixes; `return_clip=False`; the other formats write what they wrote;
  5. `Generator(opt).run()` with `--video_format apng`: serial == pipelined file for file, the files hold the clips of the `.npy` run,
     the metrics command prints exactly `metrics_from_videos` of those clips -- and not on the avi tree; the FVD loader reads them.
"""
import ctypes
import os
import sys
import zlib

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import apng_ref as R  # noqa: E402
from tests.test_e2e_gpu import TINY_ARGV  # noqa: E402
from tests.test_mjpeg_opt_gpu import budgeted  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xFF


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def encode(frames, flt, band_rows, capacity, stride=None, extra=0):
    """`ccvs_apng_encode` on frames [n, H, W, 3] (or one frame) into a stream of `capacity` bytes, with `extra` more behind it to look
    at, all pre-filled with FILL; the workspace holds garbage.  (status, the whole stream on the host, the offsets)."""
    from ccvs_amd import lib
    L = lib.load()
    frames = frames[None] if frames.dim() == 3 else frames
    n, h, w = frames.shape[:3]
    out = torch.full((capacity + extra,), FILL, dtype=torch.uint8, device="cuda")
    offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    work = torch.randint(0, 256, (L.ccvs_apng_workspace_bytes(n, h, w, band_rows),), dtype=torch.uint8, device="cuda",
                         generator=torch.Generator("cuda").manual_seed(n * h + w))
    rc = L.ccvs_apng_encode(_p(frames), frames.stride(0) if stride is None else stride, n, h, w, flt, band_rows, _p(out), capacity, _p(offsets),
                            _p(work), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.ccvs_last_error().decode()
    return rc, out.cpu().numpy(), offsets.cpu().tolist()


# ------------------------------------------------------------------ 1
def test_every_row_equals_the_mirror():
    dev = {name: torch.from_numpy(img).cuda() for name, img in R.images().items()}
    for key, name, flt, r in R.rows():
        want = R.mirrored(key)["stream"]
        _, got, off = encode(dev[name], flt, r, len(want) + 37)
        assert off == [0, len(want)], (key, off, len(want))
        diff = np.flatnonzero(got[:len(want)] != np.frombuffer(want, np.uint8))
        assert diff.size == 0, (key, "first differing byte", int(diff[0]), "of", len(want))
        assert (got[len(want):] == FILL).all(), key
    print("rows", len(R.rows()))


def test_deep_row_through_the_limiter():
    img = R.deep_row()                                                  # one row of 43690 pixels: a band of 131071 bytes, 64 tiles, a tree 17 deep
    want = R.encode_frame(img, 0, 0)["stream"]
    _, got, off = encode(torch.from_numpy(img).cuda(), 0, 0, len(want) + 5)
    assert off == [0, len(want)] and got[:len(want)].tobytes() == want and (got[len(want):] == FILL).all()
    assert zlib.decompress(got[:len(want)].tobytes()) == b"\x00" + img.tobytes()


# ------------------------------------------------------------------ 2
def _five():
    return np.stack([R.images()[k + "_33x65"] for k in ("zeros", "noise", "smooth", "mixed", "dramp")])


def test_five_frames_in_one_launch_equal_their_single_launches():
    clip = _five()
    dev = torch.from_numpy(clip).cuda()
    for flt, r in ((-1, 0), (-1, 5), (4, 1), (3, 32), (0, 33)):        # 1, 7, 33, 2 and 1 bands per frame
        singles = [R.encode_frame(clip[i], flt, r)["stream"] for i in range(5)]
        for i in (1, 3):
            _, got, off = encode(dev[i], flt, r, len(singles[i]))
            assert off == [0, len(singles[i])] and got.tobytes() == singles[i], (flt, r, i)
        want = b"".join(singles)
        for lim in (0, 1):                                              # 1: at most 8 workgroups for up to 165 bands: each walks on into later frames
            runs = [budgeted(lim, lambda: encode(dev, flt, r, len(want) + 5)) for _ in range(2)]
            _, got, off = runs[0]
            assert off == list(np.cumsum([0] + [len(x) for x in singles])), (flt, r, lim)
            assert got[:len(want)].tobytes() == want and (got[len(want):] == FILL).all(), (flt, r, lim)
            assert runs[1][2] == off and np.array_equal(runs[1][1], got)                         # the same bytes on every run


def test_frame_stride_with_garbage_between_the_frames():
    from ccvs_amd import ops
    clip = _five()
    raw = 33 * 65 * 3
    stride = raw + 61                                                   # frames at odd addresses
    buf = torch.randint(0, 256, (5 * stride,), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    padded = buf.view(5, stride)
    padded[:, :raw] = torch.from_numpy(clip).cuda().view(5, raw)
    frames = padded[:, :raw].view(5, 33, 65, 3)
    assert frames.stride(0) == stride and not frames.is_contiguous()
    want, off_w = R.encode(clip, -1, 4)
    _, got, off = encode(frames, -1, 4, len(want) + 3)
    assert off == off_w and got[:len(want)].tobytes() == want and (got[len(want):] == FILL).all()
    stream, offsets = ops.png_encode(frames, -1, 4)                     # through ops: the view is passed on as it is
    assert offsets.tolist() == off_w and stream[:off_w[-1]].cpu().numpy().tobytes() == want
    # a time-strided view of a clip batch, as `mjpeg_encode` takes it
    batch = torch.from_numpy(np.stack([clip, clip[::-1]]).copy()).cuda()
    got_b, off_b = ops.png_encode_to_host(batch[:, 1::2], 2, 0)
    want_b, off_wb = R.encode([clip[1], clip[3], clip[3], clip[1]], 2, 0)
    assert off_b == off_wb and got_b == want_b


# ------------------------------------------------------------------ 3
def test_capacity_keeps_offsets_and_writes_nothing_beyond():
    from ccvs_amd import ops
    clip = np.stack([R.images()["noise_33x65"], R.images()["smooth_33x65"]])
    dev = torch.from_numpy(clip).cuda()
    want, off_w = R.encode(clip, -1, 8)                                 # 5 bands per frame
    want = np.frombuffer(want, np.uint8)
    last_band = len(R.encode_frame(clip[1][32:], 0, 8)["stream"])       # (about the size of the second frame's last band)
    for capacity in (0, 1, off_w[1] + 3, len(want) - last_band, len(want) - 1, len(want)):
        rc, got, off = encode(dev, -1, 8, capacity, extra=64)
        assert rc == 0 and off == off_w, capacity                       # the mjpeg encoders' status in that case: 0, the offsets say it
        assert (got[capacity:] == FILL).all(), capacity
        assert np.array_equal(got[:capacity], want[:capacity]), capacity
    # a null stream goes with capacity 0
    from ccvs_amd import lib
    L = lib.load()
    offsets = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    work = torch.empty(L.ccvs_apng_workspace_bytes(2, 33, 65, 8), dtype=torch.uint8, device="cuda")
    assert L.ccvs_apng_encode(_p(dev), dev.stride(0), 2, 33, 65, -1, 8, None, 0, _p(offsets), _p(work), None) == 0
    torch.cuda.synchronize()
    assert offsets.tolist() == off_w
    # through ops: a capacity that is too small is reported by the offsets; the host form runs again
    stream, offsets = ops.png_encode(dev, -1, 8, capacity=100)
    assert stream.numel() == 100 and offsets.tolist() == off_w and np.array_equal(stream.cpu().numpy(), want[:100])
    data, off = ops.png_encode_to_host(dev, -1, 8)
    assert off == off_w and data == want.tobytes()


# ------------------------------------------------------------------ 4
def _pil_frames(path):
    from PIL import Image
    with Image.open(path) as im:
        out = []
        for t in range(getattr(im, "n_frames", 1)):
            im.seek(t)
            out.append(np.asarray(im.convert("RGB")).copy())
        return np.stack(out), im.info.get("duration")


def test_save_video_batch_apng(tmp_path):
    pytest.importorskip("PIL")
    from ccvs_amd.helpers.generator import save_video_batch
    from ccvs_amd.tools import apng
    vid = torch.rand(2, 3, 3, 24, 40, generator=torch.Generator().manual_seed(5)) * 2.4 - 1.2
    vid[1, 2] = 0.25                                                    # a flat frame among them
    state = torch.tensor([[[0.1, 0.2], [0.5, 0.5], [0.99, 0.0]], [[0.3, 0.9], [0.0, 0.0], [0.7, 0.4]]])
    cases = {"span": dict(imagenet_norm=False), "imagenet": dict(imagenet_norm=True), "state": dict(imagenet_norm=False, state=state),
             "named": dict(imagenet_norm=False, cat=["a", "b"], idx=[7, 8])}
    for tag, kw in cases.items():
        norm = kw.pop("imagenet_norm")
        d = tmp_path / tag
        dataset = "bair" if tag == "state" else "kinetics600"          # (bair: the marker is drawn on a 64-pixel grid, clipped at the border)
        u8 = save_video_batch(vid.cuda(), 2, 3, str(d), 4, True, norm, [-1, 1], dataset, video_format="apng", quality=10, subsampling="420", optimize=True, **kw)
        assert u8.shape == (2, 3, 24, 40, 3) and u8.dtype == torch.uint8 and not u8.is_cuda
        names = [f"vid_{6 + i:05d}" + (f"_{'ab'[i]}_{7 + i}" if tag == "named" else "") + ".png" for i in range(2)]
        assert sorted(os.listdir(d)) == names
        for i, n in enumerate(names):
            frames, duration = _pil_frames(str(d / n))
            assert duration == 250.0 and np.array_equal(frames, u8[i].numpy()), (tag, i)
            assert np.array_equal(apng.read_apng(str(d / n)), u8[i].numpy()), (tag, i)
        e = tmp_path / (tag + "_nc")                                    # return_clip=False (what `save_results` asks for): the same files, no clip
        assert save_video_batch(vid.cuda(), 2, 3, str(e), 4, True, norm, [-1, 1], dataset, video_format="apng", return_clip=False, **kw) is None or tag == "state"
        assert all(open(e / n, "rb").read() == open(d / n, "rb").read() for n in names)
    plain = save_video_batch(vid.cuda(), 2, 3, str(tmp_path / "npy"), 4, True, False, [-1, 1], "kinetics600", video_format="npy")
    assert np.array_equal(np.load(tmp_path / "npy" / "vid_00006.npy"), plain[0].numpy())
    frames, _ = _pil_frames(str(tmp_path / "span" / "vid_00006.png"))
    assert np.array_equal(frames, plain[0].numpy())                     # the lossless file holds the .npy file's clip
    assert not np.array_equal(_pil_frames(str(tmp_path / "state" / "vid_00006.png"))[0], plain[0].numpy())     # ... and the marked one its marker


def test_other_formats_write_what_they_wrote(tmp_path):
    """The avi bytes are pinned by the mirror tests of tests/test_mjpeg_*_gpu.py; here: the default and "npy" still give the arrays (or mp4
    where torchvision imports) and "avi" the files `read_avi` opens, unchanged by the new branch."""
    from ccvs_amd import ops
    from ccvs_amd.helpers.generator import save_video_batch
    from ccvs_amd.tools import mjpeg
    vid = torch.rand(2, 3, 3, 24, 40, generator=torch.Generator().manual_seed(6)) * 2 - 1
    u8 = save_video_batch(vid.cuda(), 2, 0, str(tmp_path / "npy"), 4, True, False, [-1, 1], "kinetics600", video_format="npy")
    assert sorted(os.listdir(tmp_path / "npy")) == ["vid_00000.npy", "vid_00001.npy"] and np.array_equal(np.load(tmp_path / "npy" / "vid_00001.npy"), u8[1].numpy())
    save_video_batch(vid.cuda(), 2, 0, str(tmp_path / "auto"), 4, True, False, [-1, 1], "kinetics600")
    assert sorted(os.path.splitext(n)[1] for n in os.listdir(tmp_path / "auto")) in ([".npy", ".npy"], [".mp4", ".mp4"])
    save_video_batch(vid.cuda(), 2, 0, str(tmp_path / "avi"), 4, True, False, [-1, 1], "kinetics600", video_format="avi", quality=80)
    scans, off = ops.mjpeg_encode_to_host(u8.cuda(), 80)
    head = mjpeg.jpeg_header(24, 40, 80)
    for i in range(2):
        fps, h, w, frames = mjpeg.read_avi(str(tmp_path / "avi" / f"vid_{i:05d}.avi"))
        assert (fps, h, w) == (4, 24, 40) and frames == [head + scans[off[k]:off[k + 1]] + mjpeg.EOI for k in range(3 * i, 3 * i + 3)]


# ------------------------------------------------------------------ 5
def _run(root, mode, extra):
    """`Generator(opt).run()` at the tiny geometry, 8 batches of 2 clips (the metrics command scores batches of 16): {(folder, file): bytes}."""
    from ccvs_amd.tools.options import Options
    from ccvs_amd.helpers.generator import Generator
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("CCVS_RUN_SCHEDULE", mode)
        torch.manual_seed(0)
        argv = TINY_ARGV + ["--n_iter", "8", "--x_top_k", "10", "--x_sample", "--save_path", str(root)] + extra
        opt = Options().parse(load_qvid_generator=True, load_transformer=True, argv=argv)
        gen = Generator(opt)
        torch.manual_seed(9)
        gen.run()
    top, files = opt["transformer"].result_path, {}
    for kind in sorted(os.listdir(top)):
        for n in sorted(os.listdir(os.path.join(top, kind))):
            files[kind, n] = open(os.path.join(top, kind, n), "rb").read()
    return top, files


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    base = tmp_path_factory.mktemp("apng_runs")
    return {tag: _run(base / tag, mode, extra) for tag, mode, extra in (
        ("apng", "pipelined", ["--video_format", "apng", "--video_quality", "5", "--video_subsampling", "420", "--video_optimize"]),
        ("serial", "serial", ["--video_format", "apng"]), ("npy", "pipelined", ["--video_format", "npy"]),
        ("avi", "pipelined", ["--video_format", "avi"]))}


def test_run_writes_apng_files_pipelined_equals_serial(runs, tmp_path):
    pytest.importorskip("PIL")
    from ccvs_amd.tools.tf_fvd import fvd
    files = runs["apng"][1]
    assert files == runs["serial"][1]                                   # (and the avi flags beside apng moved nothing)
    assert sorted(files) == sorted((kind, f"vid_{i:05d}.png") for kind in ("real", "fake", "rec") for i in range(16))
    arrays = runs["npy"][1]
    total = raw = huff = 0
    for (kind, name), data in files.items():
        want = np.load(os.path.join(runs["npy"][0], kind, name[:-4] + ".npy"))
        frames, duration = _pil_frames(os.path.join(runs["apng"][0], kind, name))
        assert np.array_equal(frames, want) and frames.shape == (4, 32, 32, 3), (kind, name)
        total += len(data)
        raw += want.size
        for f in want:                                                  # recorded: zlib's Huffman-only stream of the same filtered bytes
            c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
            huff += len(c.compress(R.filter_rows(f, -1)[0].tobytes()) + c.flush())
    assert sorted(arrays) == sorted((kind, name[:-4] + ".npy") for kind, name in files)
    print(f"tiny run: {len(files)} apng files {total} bytes, raw clips {raw} bytes ({total / raw:.4f}), zlib Huffman-only streams {huff} ({total / huff:.4f} with the containers)")
    # the FVD command's loader reads the same clips from the files as the run had on the device
    for kind in ("real", "fake"):
        got = fvd.load_videos(fvd.get_video_files(os.path.join(runs["apng"][0], kind)), None, 1)
        want = np.stack([np.load(os.path.join(runs["npy"][0], kind, f"vid_{i:05d}.npy")) for i in range(16)])
        assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), kind


def _metric_lines(top, monkeypatch, capsys):
    from ccvs_amd.tools.pytorch_metrics import metrics as M
    monkeypatch.chdir(os.path.dirname(os.path.dirname(top)))
    assert os.path.dirname(top).endswith("results")
    capsys.readouterr()
    M.main(M.parse_args(["--exp_tag", os.path.basename(top)]))
    out = capsys.readouterr().out.splitlines()
    assert "Found 16 real video files" in out and "Found 16 fake video files" in out
    return [out[out.index(f"Mean/std of {m} across 1 runs") + 1] for m in ("SSIM", "PSNR")]


def test_metrics_command_prints_the_clips_own_scores(runs, monkeypatch, capsys):
    from ccvs_amd.tools.pytorch_metrics import metrics as M
    clips = {kind: np.stack([np.load(os.path.join(runs["npy"][0], kind, f"vid_{i:05d}.npy")) for i in range(16)]) for kind in ("real", "fake")}
    _, ssim, psnr = M.metrics_from_videos(torch.from_numpy(clips["real"]).cuda(), torch.from_numpy(clips["fake"]).cuda())
    want = [f"{np.mean([s])!s} {np.std([s])!s}" for s in (ssim, psnr)]
    lossless = _metric_lines(runs["apng"][0], monkeypatch, capsys)
    lossy = _metric_lines(runs["avi"][0], monkeypatch, capsys)
    print("clips", want, "apng", lossless, "avi", lossy)
    assert lossless == want                                             # exactly the scores of the clips the model produced
    assert lossy != want                                                # ... which the Motion-JPEG files at quality 90, 4:4:4 do not give
