"""gpu: the JPEG encoder of the output stage (csrc/jpeg.hip) against the fixture tests/golden/mjpeg_cases.npz --
the files Pillow (libjpeg) wrote -- and against the spec mirror tests/jpeg_ref.py, which tests/test_mjpeg_host.py holds against both.
Every comparison is byte for byte.

  1. every fixture row: scan bytes and offsets equal Pillow's; the stream behind offsets[n] is untouched;
  2. several frames of different content in one launch, contiguous and as a strided view: each equals its single-frame encode;
  3. the scan larger than the raw frame: complete offsets, nothing at or beyond `capacity`, the bytes below it right, the re-run exact;
  4. bad arguments are refused with a status and a message, and nothing is launched: the buffers stay as they were;
  5. `save_video_batch(..., video_format="avi")`: the files' scans equal the mirror's encode of the uint8 clip the call returned, also
     with the imagenet de-normalisation and with a state marker on a 256 x 256 clip;
  6. `Generator(opt).run()` with `--video_format avi`: the pipelined and the serial schedule write the same bytes; without the flag the
     run writes the files it wrote before;
  7. two runs give identical bytes.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jpeg_ref as R  # noqa: E402
from tests.test_e2e_gpu import TINY_ARGV  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xA5


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "mjpeg_cases.npz"))


@pytest.fixture(scope="module")
def wanted(gold):
    """{row key: Pillow's scan}."""
    return {key: R.scan_of(gold[key].tobytes()) for key, _, _, _ in R.rows()}


def encode(frames, quality, r, capacity):
    """(the whole stream on the host, the offsets) of one call into a stream of `capacity` bytes pre-filled with FILL."""
    from ccvs_amd import ops
    out = torch.full((capacity,), FILL, dtype=torch.uint8, device="cuda")
    stream, offsets = ops.mjpeg_encode(frames, quality, r, out=out)
    assert stream is out and offsets.dtype == torch.int64 and offsets.is_cuda
    return stream.cpu().numpy(), offsets.cpu().tolist()


def test_every_fixture_row_equals_pillow_and_runs_repeat(gold, wanted):
    worst = 0
    for key, name, q, r in R.rows():
        img = torch.from_numpy(gold[name + "/in"]).cuda()
        want = wanted[key]
        slack = 37
        got, off = encode(img, q, r, len(want) + slack)
        assert off == [0, len(want)], (key, off, len(want))
        diff = np.flatnonzero(got[:len(want)] != np.frombuffer(want, dtype=np.uint8))
        worst = max(worst, diff.size)
        assert diff.size == 0, (key, "first differing byte", int(diff[0]), "of", len(want))
        assert (got[len(want):] == FILL).all(), key                                       # nothing behind the scan
        again, off2 = encode(img[None], q, r, len(want) + slack)                            # 7: the same bytes on every run
        assert off2 == off and np.array_equal(again, got), key
    print("rows", len(R.rows()), "differing bytes", worst)


def test_default_interval_and_capacity(gold, wanted):
    from ccvs_amd import ops
    img = torch.from_numpy(gold["noise_13x21/in"]).cuda()
    stream, offsets = ops.mjpeg_encode(img, 75)                                             # R = None: a row of MCUs; capacity = the raw size
    assert stream.numel() == 13 * 21 * 3 and offsets.tolist() == [0, len(wanted["noise_13x21/q75"])]
    assert bytes(stream[:offsets[1]].cpu().numpy()) == wanted["noise_13x21/q75"]
    data, off = ops.mjpeg_encode_to_host(img, 75)
    assert data == wanted["noise_13x21/q75"] and off == [0, len(data)]


def test_several_frames_contiguous_and_strided(gold):
    from ccvs_amd import ops
    rng = np.random.RandomState(11)
    smooth = R.CASES["smooth_64x64"][0]()[:24, :40]
    clip = np.stack([rng.randint(0, 256, size=(24, 40, 3)).astype(np.uint8), smooth, np.zeros((24, 40, 3), np.uint8), smooth[::-1].copy(),
                     R.CASES["checker_16x16"][0]().repeat(2, axis=0).repeat(3, axis=1)[:24, :40], np.full((24, 40, 3), 255, np.uint8)])
    clip = np.stack([clip, clip[::-1]])                                                     # [2, 6, 24, 40, 3]
    dev = torch.from_numpy(clip.copy()).cuda()
    single = {}
    for b in range(2):
        for t in range(6):
            data, off = ops.mjpeg_encode_to_host(dev[b, t], 90)
            single[b, t] = data
            assert data == R.encode_scan(clip[b, t], 90), (b, t)
    assert len({len(v) for v in single.values()}) >= 4                                      # scans of different lengths
    for view, frames in ((dev, [(b, t) for b in range(2) for t in range(6)]), (dev[:, 1::2], [(b, t) for b in range(2) for t in (1, 3, 5)])):
        assert view.is_contiguous() == (len(frames) == 12)
        want = b"".join(single[f] for f in frames)
        got, off = encode(view, 90, None, len(want) + 5)
        assert off == list(np.cumsum([0] + [len(single[f]) for f in frames]))
        assert bytes(got[:len(want)]) == want and (got[len(want):] == FILL).all()


def test_overflow_keeps_offsets_and_writes_nothing_beyond_capacity(gold, wanted):
    from ccvs_amd import ops
    img = torch.from_numpy(gold["noise_24x40/in"]).cuda()
    want = wanted["noise_24x40/q100"]
    raw = 24 * 40 * 3
    assert len(want) > raw
    # two frames: the first one fits, the second one does not.  The stream is longer than `capacity` so that "beyond" can be looked at.
    frames = torch.stack([img, img])
    out = torch.full((2 * len(want) + 64,), FILL, dtype=torch.uint8, device="cuda")
    capacity = 2 * raw
    L = __import__("ccvs_amd.lib", fromlist=["load"]).load()
    offsets = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    work = torch.empty(L.ccvs_mjpeg_workspace_bytes(2, 24, 40, 5), dtype=torch.uint8, device="cuda")
    rc = L.ccvs_mjpeg_encode(ctypes.c_void_p(frames.data_ptr()), raw, 2, 24, 40, 100, 5, ctypes.c_void_p(out.data_ptr()), capacity,
                             ctypes.c_void_p(offsets.data_ptr()), ctypes.c_void_p(work.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    got = out.cpu().numpy()
    assert offsets.tolist() == [0, len(want), 2 * len(want)] and 2 * len(want) > capacity > len(want)
    assert (got[capacity:] == FILL).all()                                                   # untouched at and beyond capacity
    assert bytes(got[:len(want)]) == want                                                   # the complete frame
    assert bytes(got[len(want):capacity]) == want[:capacity - len(want)]                    # ... and what fits of the other one
    # the single frame at capacity = raw, through ops: same offsets, then the exact re-run
    stream, off = ops.mjpeg_encode(img, 100, 5)
    assert stream.numel() == raw and off.tolist() == [0, len(want)] and bytes(stream.cpu().numpy()) == want[:raw]
    data, off = ops.mjpeg_encode_to_host(img, 100, 5)
    assert data == want and off == [0, len(want)]


def test_bad_arguments_are_refused_before_any_launch():
    from ccvs_amd import lib, ops
    L = lib.load()
    torch.cuda.synchronize()
    img = torch.zeros(8, 8, 3, dtype=torch.uint8, device="cuda")
    for kw, word in (({"quality": 0}, "quality"), ({"quality": 101}, "quality"), ({"restart_mcus": 0}, "restart"), ({"restart_mcus": 33}, "restart")):
        with pytest.raises(lib.CcvsError, match=word):
            ops.mjpeg_encode(img, **kw)
    # through the ABI, on real buffers: a status and a message, the buffers stay as they were
    out = torch.full((256,), FILL, dtype=torch.uint8, device="cuda")
    offsets = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    work = torch.zeros(64, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for h, w in ((0, 8), (8, 0), (65536, 8), (8, 65536)):
        assert L.ccvs_mjpeg_encode(p(img), 192, 1, h, w, 90, 1, p(out), 256, p(offsets), p(work), None) != 0 and "size" in L.ccvs_last_error().decode()
    assert L.ccvs_mjpeg_encode(p(img), 192, 1, 8, 8, 0, 1, p(out), 256, p(offsets), p(work), None) != 0 and "quality" in L.ccvs_last_error().decode()
    assert L.ccvs_mjpeg_encode(p(img), 192, 1, 8, 8, 90, 33, p(out), 256, p(offsets), p(work), None) != 0 and "restart" in L.ccvs_last_error().decode()
    torch.cuda.synchronize()
    assert (out == FILL).all() and offsets.tolist() == [-7, -7] and int(work.sum()) == 0
    torch.cuda.synchronize()
    assert int(img.sum()) == 0


def _avi_scans(path, h, w, quality):
    from ccvs_amd.tools import mjpeg
    fps, hh, ww, frames = mjpeg.read_avi(path)
    head = mjpeg.jpeg_header(h, w, quality)
    assert (hh, ww) == (h, w) and all(f.startswith(head) and f.endswith(mjpeg.EOI) for f in frames)
    return fps, [f[len(head):-2] for f in frames]


def test_save_video_batch_avi(tmp_path):
    from ccvs_amd.helpers.generator import save_video_batch
    vid = torch.rand(2, 3, 3, 24, 40, generator=torch.Generator().manual_seed(5)) * 2.4 - 1.2
    for name, inet, dataset, q in (("plain", False, "bairhd", 90), ("inet", True, "kinetics600", 60)):
        u8 = save_video_batch(vid.cuda(), 2, 3, str(tmp_path / name), 4, True, inet, [-1, 1], dataset, video_format="avi", quality=q)
        assert u8.dtype == torch.uint8 and u8.device.type == "cpu" and u8.shape == (2, 3, 24, 40, 3)
        assert sorted(os.listdir(tmp_path / name)) == ["vid_00006.avi", "vid_00007.avi"]
        for i in range(2):
            fps, scans = _avi_scans(str(tmp_path / name / f"vid_{6 + i:05d}.avi"), 24, 40, q)
            assert fps == 4 and scans == [R.encode_scan(u8[i, t].numpy(), q) for t in range(3)], (name, i)
    # return_clip=False (what `save_results` asks for): the same files, no clip
    assert save_video_batch(vid.cuda(), 2, 3, str(tmp_path / "nc"), 4, True, False, [-1, 1], "bairhd", video_format="avi", return_clip=False) is None
    for i in range(2):
        assert open(tmp_path / "nc" / f"vid_{6 + i:05d}.avi", "rb").read() == open(tmp_path / "plain" / f"vid_{6 + i:05d}.avi", "rb").read()
    # the state marker on a 256 x 256 clip: the marked host clip is what the file holds
    big = torch.rand(1, 2, 3, 256, 256, generator=torch.Generator().manual_seed(6)) * 2 - 1
    state = torch.tensor([[[0.5, 0.25], [0.999, 0.0]]])
    plain = save_video_batch(big.cuda(), 1, 0, str(tmp_path / "p"), 4, True, False, [-1, 1], "bairhd", video_format="npy")
    marked = save_video_batch(big.cuda(), 1, 0, str(tmp_path / "s"), 4, True, False, [-1, 1], "bairhd", state=state, video_format="avi", return_clip=False)
    assert marked is not None and not torch.equal(marked, plain) and (marked[0, 0, 64, 127:130] == 255).all()
    fps, scans = _avi_scans(str(tmp_path / "s" / "vid_00000.avi"), 256, 256, 90)
    assert scans == [R.encode_scan(marked[0, t].numpy(), 90) for t in range(2)]


def _run_files(tmp_path, monkeypatch, mode, extra):
    from ccvs_amd.tools.options import Options
    from ccvs_amd.helpers.generator import Generator
    monkeypatch.setenv("CCVS_RUN_SCHEDULE", mode)
    torch.manual_seed(0)
    argv = TINY_ARGV + ["--n_iter", "5", "--x_top_k", "10", "--x_sample", "--save_path", str(tmp_path)] + extra
    opt = Options().parse(load_qvid_generator=True, load_transformer=True, argv=argv)
    gen = Generator(opt)
    torch.manual_seed(9)
    gen.run()
    root, files = opt["transformer"].result_path, {}
    for kind in sorted(os.listdir(root)):
        for n in sorted(os.listdir(os.path.join(root, kind))):
            files[kind, n] = open(os.path.join(root, kind, n), "rb").read()
    return files


def test_run_writes_avi_files_pipelined_equals_serial(tmp_path, monkeypatch):
    from ccvs_amd.tools import mjpeg
    avi = {mode: _run_files(tmp_path / mode, monkeypatch, mode, ["--video_format", "avi", "--video_quality", "80"]) for mode in ("serial", "pipelined")}
    assert avi["serial"] == avi["pipelined"]
    assert sorted(avi["serial"]) == sorted((kind, f"vid_{i:05d}.avi") for kind in ("real", "fake", "rec") for i in range(10))
    # without the flag: the files the run wrote before (.npy arrays, or mp4 where torchvision imports), and the .avi files hold those clips
    try:
        import torchvision.io  # noqa: F401
        ext = ".mp4"
    except ImportError:
        ext = ".npy"
    plain = _run_files(tmp_path / "plain", monkeypatch, "pipelined", [])
    assert sorted(plain) == sorted((kind, f"vid_{i:05d}{ext}") for kind in ("real", "fake", "rec") for i in range(10))
    if ext == ".npy":
        import io
        for (kind, name), data in plain.items():
            clip = np.load(io.BytesIO(data))
            path = os.path.join(str(tmp_path), "x.avi")
            open(path, "wb").write(avi["pipelined"][kind, name.replace(".npy", ".avi")])
            fps, h, w, frames = mjpeg.read_avi(path)
            head = mjpeg.jpeg_header(h, w, 80)
            assert (fps, h, w) == (4, *clip.shape[1:3]) and [f[len(head):-2] for f in frames] == [R.encode_scan(c, 80) for c in clip], (kind, name)
