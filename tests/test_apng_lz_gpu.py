"""gpu: the lossless output stage with LZ77 matches (`ccvs_apng_encode_lz`, csrc/png_lz.hip) against the spec
mirror tests/apng_lz_ref.py, which tests/test_apng_lz_host.py holds against zlib's inflate and Pillow.  Every comparison is byte for byte.

  1. every row of the mirror's table: offsets and stream equal the mirror's, written into a stream pre-filled with 0xFF from a workspace
     filled with garbage; nothing at or beyond offsets[n] is touched;
  2. five frames in one launch equal their single launches, with no CU budget and under a budget of one CU; twice, the same bytes; a
     frame stride larger than the frame with garbage between the frames;
  3. capacity 0, 1, one band short and exactly enough: complete offsets, nothing at or beyond `capacity`; `png_encode_to_host(lz77=True)`;
  4. `ops.png_encode(x)` without the argument still gives `apng_ref`'s bytes;
  5. the device's own inflate (`ops.png_decode`) of the new streams returns the frames, the distance-32768 row among them;
  6. `save_video_batch(video_format="apng", lz77=True)`: Pillow and `read_apng` give the returned clip, `return_clip=False` writes the
     same files, no file is larger than without the flag;
  7. `Generator(opt).run()` with `--video_format apng --video_lz77`: serial == pipelined, the files hold the `.npy` run's clips,
     `ops.read_apng_clips` reads them back.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import apng_lz_ref as Z  # noqa: E402
import apng_ref as R  # noqa: E402
from tests.test_apng_gpu import FILL, _pil_frames, _run  # noqa: E402
from tests.test_mjpeg_opt_gpu import budgeted  # noqa: E402

pytestmark = pytest.mark.gpu


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def encode(frames, flt, band_rows, capacity, stride=None, extra=0):
    """`ccvs_apng_encode_lz` on frames [n, H, W, 3] (or one frame) into a stream of `capacity` bytes, with `extra` more behind it to look
    at, all pre-filled with FILL; the workspace holds garbage.  (status, the whole stream on the host, the offsets)."""
    from ccvs_amd import lib
    L = lib.load()
    frames = frames[None] if frames.dim() == 3 else frames
    n, h, w = frames.shape[:3]
    out = torch.full((capacity + extra,), FILL, dtype=torch.uint8, device="cuda")
    offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    work = torch.randint(0, 256, (L.ccvs_apng_lz_workspace_bytes(n, h, w, band_rows),), dtype=torch.uint8, device="cuda",
                         generator=torch.Generator("cuda").manual_seed(n * h + w))
    rc = L.ccvs_apng_encode_lz(_p(frames), frames.stride(0) if stride is None else stride, n, h, w, flt, band_rows, _p(out), capacity, _p(offsets),
                               _p(work), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.ccvs_last_error().decode()
    return rc, out.cpu().numpy(), offsets.cpu().tolist()


# ------------------------------------------------------------------ 1
def test_every_row_equals_the_mirror():
    dev = {name: torch.from_numpy(img).cuda() for name, img in Z.images().items()}
    chosen = set()
    for key, name, flt, r in Z.rows():
        m = Z.mirrored(key)
        want = m["stream"]
        chosen |= set(m["choice"])
        _, got, off = encode(dev[name], flt, r, len(want) + 37)
        assert off == [0, len(want)], (key, off, len(want))
        diff = np.flatnonzero(got[:len(want)] != np.frombuffer(want, np.uint8))
        assert diff.size == 0, (key, "first differing byte", int(diff[0]), "of", len(want))
        assert (got[len(want):] == FILL).all(), key
    assert chosen == {"lz", "literal"}
    print("rows", len(Z.rows()))


# ------------------------------------------------------------------ 2
def _five():
    return np.stack([Z.images()[k + "_33x65"] for k in ("zeros", "noise", "smooth", "mixed", "dramp")])


def test_five_frames_in_one_launch_equal_their_single_launches():
    clip = _five()
    dev = torch.from_numpy(clip).cuda()
    for flt, r in ((-1, 0), (-1, 5), (4, 1), (0, 33)):                  # 1, 7, 33 and 1 bands per frame
        singles = [Z.encode_frame(clip[i], flt, r)["stream"] for i in range(5)]
        for i in (0, 3):
            _, got, off = encode(dev[i], flt, r, len(singles[i]))
            assert off == [0, len(singles[i])] and got.tobytes() == singles[i], (flt, r, i)
        want = b"".join(singles)
        for lim in (0, 1):                                              # 1: a few workgroups for up to 165 bands: each walks on into later frames
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
    want, off_w = Z.encode(clip, -1, 4)
    _, got, off = encode(frames, -1, 4, len(want) + 3)
    assert off == off_w and got[:len(want)].tobytes() == want and (got[len(want):] == FILL).all()
    stream, offsets = ops.png_encode(frames, -1, 4, lz77=True)          # through ops: the view is passed on as it is
    assert offsets.tolist() == off_w and stream[:off_w[-1]].cpu().numpy().tobytes() == want


# ------------------------------------------------------------------ 3, 4
def test_capacity_keeps_offsets_and_writes_nothing_beyond():
    from ccvs_amd import ops
    clip = np.stack([Z.images()["mixed_33x65"], Z.images()["smooth_33x65"]])
    dev = torch.from_numpy(clip).cuda()
    want, off_w = Z.encode(clip, -1, 8)                                 # 5 bands per frame
    want = np.frombuffer(want, np.uint8)
    last_band = len(Z.encode_frame(clip[1][32:], 0, 8)["stream"])       # (about the size of the second frame's last band)
    for capacity in (0, 1, off_w[1] + 3, len(want) - last_band, len(want) - 1, len(want)):
        rc, got, off = encode(dev, -1, 8, capacity, extra=64)
        assert rc == 0 and off == off_w, capacity
        assert (got[capacity:] == FILL).all(), capacity
        assert np.array_equal(got[:capacity], want[:capacity]), capacity
    stream, offsets = ops.png_encode(dev, -1, 8, capacity=100, lz77=True)
    assert stream.numel() == 100 and offsets.tolist() == off_w and np.array_equal(stream.cpu().numpy(), want[:100])
    data, off = ops.png_encode_to_host(dev, -1, 8, lz77=True)
    assert off == off_w and data == want.tobytes()
    # the default capacity is the default writer's, and its bytes did not move
    stream, offsets = ops.png_encode(dev, -1, 8, lz77=True)
    plain, plain_off = ops.png_encode(dev, -1, 8)
    assert stream.numel() == plain.numel() and offsets[-1].item() <= plain_off[-1].item() <= plain.numel()
    ref, ref_off = R.encode(clip, -1, 8)
    assert plain_off.tolist() == ref_off and plain[:ref_off[-1]].cpu().numpy().tobytes() == ref
    assert ops.png_encode_to_host(dev, -1, 8) == (ref, ref_off)


# ------------------------------------------------------------------ 5
def test_the_device_inflates_what_the_device_wrote():
    from ccvs_amd import ops
    for names in (("zeros_64x64", "mixed_64x64", "dramp_64x64", "noise_64x64", "smooth_64x64"), ("period_32768",), ("run_517",), ("run_to_band_end",)):
        clip = np.stack([Z.images()[k] for k in names])
        h, w = clip.shape[1:3]
        for flt, r in ((-1, 0), (0, 1)):
            data, off = ops.png_encode_to_host(torch.from_numpy(clip).cuda(), flt, r, lz77=True)
            frames, status = ops.png_decode([data[off[i]:off[i + 1]] for i in range(len(names))], h, w, check=False)
            assert status.cpu().tolist() == [0] * len(names), (names, flt, r)
            assert np.array_equal(frames.cpu().numpy(), clip), (names, flt, r)
    far = Z.mirrored("period_32768/f0/b1")
    assert any(isinstance(t, tuple) and t[1] == 32768 for t in far["tokens"][0])


# ------------------------------------------------------------------ 6
def test_save_video_batch_apng_lz77(tmp_path):
    pytest.importorskip("PIL")
    from ccvs_amd.helpers.generator import save_video_batch
    from ccvs_amd.tools import apng
    vid = torch.rand(2, 3, 3, 24, 40, generator=torch.Generator().manual_seed(5)) * 2.4 - 1.2
    vid[1, 2] = 0.25                                                    # a flat frame among them
    vid[0, :, :, :6] = -1.0                                             # a flat border
    for tag, norm in (("span", False), ("imagenet", True)):
        args = (vid.cuda(), 2, 3, str(tmp_path / tag), 4, True, norm, [-1, 1], "kinetics600")
        u8 = save_video_batch(*args, video_format="apng", lz77=True)
        names = ["vid_00006.png", "vid_00007.png"]
        assert sorted(os.listdir(tmp_path / tag)) == names
        for i, n in enumerate(names):
            frames, duration = _pil_frames(str(tmp_path / tag / n))
            assert duration == 250.0 and np.array_equal(frames, u8[i].numpy()), (tag, i)
            assert np.array_equal(apng.read_apng(str(tmp_path / tag / n)), u8[i].numpy()), (tag, i)
        args = args[:3] + (str(tmp_path / (tag + "_nc")),) + args[4:]
        assert save_video_batch(*args, video_format="apng", lz77=True, return_clip=False) is None
        args = args[:3] + (str(tmp_path / (tag + "_off")),) + args[4:]
        save_video_batch(*args, video_format="apng")
        for n in names:
            on = open(tmp_path / tag / n, "rb").read()
            assert open(tmp_path / (tag + "_nc") / n, "rb").read() == on
            assert len(on) <= os.path.getsize(tmp_path / (tag + "_off") / n), (tag, n)
        assert sum(os.path.getsize(tmp_path / tag / n) for n in names) < sum(os.path.getsize(tmp_path / (tag + "_off") / n) for n in names)


# ------------------------------------------------------------------ 7
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    base = tmp_path_factory.mktemp("apng_lz_runs")
    return {tag: _run(base / tag, mode, extra) for tag, mode, extra in (
        ("lz", "pipelined", ["--video_format", "apng", "--video_lz77"]), ("serial", "serial", ["--video_format", "apng", "--video_lz77"]),
        ("npy", "pipelined", ["--video_format", "npy"]))}


def test_run_writes_lz77_files_pipelined_equals_serial(runs):
    pytest.importorskip("PIL")
    from ccvs_amd import ops
    files = runs["lz"][1]
    assert files == runs["serial"][1]
    assert sorted(files) == sorted((kind, f"vid_{i:05d}.png") for kind in ("real", "fake", "rec") for i in range(16))
    for kind, name in files:
        want = np.load(os.path.join(runs["npy"][0], kind, name[:-4] + ".npy"))
        frames, _ = _pil_frames(os.path.join(runs["lz"][0], kind, name))
        assert np.array_equal(frames, want), (kind, name)
    for kind in ("real", "fake"):
        got = ops.read_apng_clips([os.path.join(runs["lz"][0], kind, f"vid_{i:05d}.png") for i in range(16)])
        want = np.stack([np.load(os.path.join(runs["npy"][0], kind, f"vid_{i:05d}.npy")) for i in range(16)])
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want), kind
