"""gpu: the subsampled modes of the JPEG encoder (4:2:2 and 4:2:0: `ccvs_mjpeg_encode_sampled`, csrc/jpeg.hip)
against the fixture tests/golden/mjpeg_sub_cases.npz -- the files Pillow (libjpeg) wrote -- and against the spec mirror
tests/jpeg_sub_ref.py, which tests/test_mjpeg_sub_host.py holds against both.  Every comparison is byte for byte; every image comes from
the mirror's case table.

  1. every fixture row, both samplings: scan bytes and offsets equal Pillow's; the stream behind offsets[n] is untouched;
  2. several frames of different content in one launch, contiguous and as a strided view: each equals the mirror's scan;
  3. a stream that is too small: complete offsets, nothing at or beyond `capacity`, then `mjpeg_encode_to_host` exact;
  4. `ccvs_mjpeg_encode_sampled(sampling=0)` is byte-equal to `ccvs_mjpeg_encode`;
  5. the way back on the device: `ops.mjpeg_decode` of header + scan + EOI equals Pillow's decode of those bytes for every row wider than
     4 pixels; `ops.read_avi_clips` of files `save_video_batch(subsampling="420")` wrote equals it too;
  6. `save_video_batch(video_format="avi", subsampling=...)`: the files' scans equal the mirror's encode of the returned clip, for 422 and
     420, both normalisations and with a state marker; `return_clip=False` returns None;
  7. `Generator(opt).run()` with `--video_format avi --video_subsampling 420`: the serial and the pipelined schedule write the same
     bytes, whose SOF says 2 x 2; without the flag it says 1 x 1;
  8. the metrics command on a results/ tree of 4:2:0 files prints the PSNR / SSIM of the clips the decoder mirror decodes.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jpeg_decode_ref as D  # noqa: E402
import jpeg_ref as R  # noqa: E402
import jpeg_sub_ref as S  # noqa: E402
from tests.test_mjpeg_gpu import _run_files  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xA5


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "mjpeg_sub_cases.npz"))


@pytest.fixture(scope="module")
def wanted(gold):
    """{row key: Pillow's scan}."""
    return {row[0]: R.scan_of(gold[row[0]].tobytes()) for row in S.rows()}


def encode(frames, quality, r, sampling, capacity):
    """(the whole stream on the host, the offsets) of one call into a stream of `capacity` bytes pre-filled with FILL."""
    from ccvs_amd import ops
    out = torch.full((capacity,), FILL, dtype=torch.uint8, device="cuda")
    stream, offsets = ops.mjpeg_encode(frames, quality, r, out=out, sampling=sampling)
    assert stream is out and offsets.dtype == torch.int64 and offsets.is_cuda
    return stream.cpu().numpy(), offsets.cpu().tolist()


# ------------------------------------------------------------------ 1
def test_every_fixture_row_equals_pillow(gold, wanted):
    worst = 0
    for key, name, s, q, r in S.rows():
        img = torch.from_numpy(gold[name + "/in"]).cuda()
        want = wanted[key]
        got, off = encode(img, q, r, s, len(want) + 37)
        assert off == [0, len(want)], (key, off, len(want))
        diff = np.flatnonzero(got[:len(want)] != np.frombuffer(want, dtype=np.uint8))
        worst = max(worst, diff.size)
        assert diff.size == 0, (key, "first differing byte", int(diff[0]), "of", len(want))
        assert (got[len(want):] == FILL).all(), key                                       # nothing behind the scan
    print("rows", len(S.rows()), "differing bytes", worst)


def test_default_interval_and_repeat(gold, wanted):
    from ccvs_amd import ops
    img = torch.from_numpy(gold["noise_13x21/in"]).cuda()
    for s in S.SAMPLINGS:
        want = wanted[f"noise_13x21/s{s}/q75"]
        stream, offsets = ops.mjpeg_encode(img, 75, sampling=s)                             # R = None: a row of MCUs; capacity = the raw size
        assert stream.numel() == 13 * 21 * 3 and offsets.tolist() == [0, len(want)] and bytes(stream[:len(want)].cpu().numpy()) == want
        assert ops.mjpeg_encode_to_host(img, 75, sampling=s) == (want, [0, len(want)]) == ops.mjpeg_encode_to_host(img[None], 75, None, s)
    with pytest.raises(ValueError, match="sampling"):
        ops.mjpeg_encode(img, 75, sampling=3)


# ------------------------------------------------------------------ 2
def test_several_frames_contiguous_and_strided(gold):
    from ccvs_amd import ops
    noise, smooth = gold["noise_24x40/in"], gold["smooth_24x40/in"]
    clip = np.stack([noise, smooth, np.zeros((24, 40, 3), np.uint8), smooth[::-1].copy(), gold["noise_25x72/in"][:24, 20:60], np.full((24, 40, 3), 255, np.uint8)])
    clip = np.stack([clip, clip[::-1]])                                                     # [2, 6, 24, 40, 3]
    dev = torch.from_numpy(clip.copy()).cuda()
    for s in S.SAMPLINGS:
        single = {(b, t): S.encode_scan_sub(clip[b, t], 90, s) for b in range(2) for t in range(6)}
        assert len({len(v) for v in single.values()}) >= 4                                  # scans of different lengths
        for view, frames in ((dev, [(b, t) for b in range(2) for t in range(6)]), (dev[:, 1::2], [(b, t) for b in range(2) for t in (1, 3, 5)])):
            assert view.is_contiguous() == (len(frames) == 12)
            want = b"".join(single[f] for f in frames)
            got, off = encode(view, 90, None, s, len(want) + 5)
            assert off == list(np.cumsum([0] + [len(single[f]) for f in frames])), s
            assert bytes(got[:len(want)]) == want and (got[len(want):] == FILL).all(), s


# ------------------------------------------------------------------ 3
def test_too_small_stream_keeps_offsets_and_writes_nothing_beyond_capacity(gold, wanted):
    from ccvs_amd import lib, ops
    L = lib.load()
    img = torch.from_numpy(gold["noise_24x40/in"]).cuda()
    frames = torch.stack([img, img])
    raw = 24 * 40 * 3
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for s in S.SAMPLINGS:
        want = wanted[f"noise_24x40/s{s}/q100"]
        capacity = len(want) + len(want) // 3                                               # the first frame fits, the second does not
        out = torch.full((2 * len(want) + 64,), FILL, dtype=torch.uint8, device="cuda")
        offsets = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        work = torch.empty(L.ccvs_mjpeg_sampled_workspace_bytes(2, 24, 40, s, 3), dtype=torch.uint8, device="cuda")
        rc = L.ccvs_mjpeg_encode_sampled(p(frames), raw, 2, 24, 40, 100, s, 3, p(out), capacity, p(offsets), p(work),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        got = out.cpu().numpy()
        assert offsets.tolist() == [0, len(want), 2 * len(want)] and 2 * len(want) > capacity > len(want)
        assert (got[capacity:] == FILL).all()                                               # untouched at and beyond capacity
        assert bytes(got[:len(want)]) == want and bytes(got[len(want):capacity]) == want[:capacity - len(want)]
        # through ops: a capacity below the scan gives the same offsets and the bytes that fit, the host form then the exact bytes
        stream, off = ops.mjpeg_encode(img, 100, 3, capacity=len(want) - 9, sampling=s)
        assert stream.numel() == len(want) - 9 and off.tolist() == [0, len(want)] and bytes(stream.cpu().numpy()) == want[:-9]
        assert ops.mjpeg_encode_to_host(img, 100, 3, sampling=s) == (want, [0, len(want)])
    # the host form's own second run: scans larger than the raw frame
    for name in ("noise_1x1", "noise_9x9"):
        tiny = torch.from_numpy(gold[name + "/in"]).cuda()
        for s in S.SAMPLINGS:
            want = wanted[f"{name}/s{s}/q100"]
            assert len(want) > tiny.numel() and ops.mjpeg_encode_to_host(tiny, 100, sampling=s) == (want, [0, len(want)])


# ------------------------------------------------------------------ 4
def test_sampling_0_equals_the_444_entry_point(gold):
    from ccvs_amd import lib
    L = lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    cur = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, q, r in (("noise_24x40", 100, 5), ("noise_13x21", 30, 2), ("noise_16x520", 90, 32)):
        img = torch.from_numpy(gold[name + "/in"]).cuda()
        h, w = img.shape[:2]
        want = R.encode_scan(gold[name + "/in"], q, r)
        res = []
        for sampled in (False, True):
            out = torch.full((len(want) + 16,), FILL, dtype=torch.uint8, device="cuda")
            offsets = torch.full((2,), -1, dtype=torch.int64, device="cuda")
            if sampled:
                n_work = L.ccvs_mjpeg_sampled_workspace_bytes(1, h, w, 0, r)
                work = torch.empty(n_work, dtype=torch.uint8, device="cuda")
                rc = L.ccvs_mjpeg_encode_sampled(p(img), h * w * 3, 1, h, w, q, 0, r, p(out), out.numel(), p(offsets), p(work), cur)
            else:
                n_work = L.ccvs_mjpeg_workspace_bytes(1, h, w, r)
                work = torch.empty(n_work, dtype=torch.uint8, device="cuda")
                rc = L.ccvs_mjpeg_encode(p(img), h * w * 3, 1, h, w, q, r, p(out), out.numel(), p(offsets), p(work), cur)
            assert rc == 0
            res.append((n_work, offsets.tolist(), out.cpu().numpy().tobytes()))
        assert res[0] == res[1] and res[0][1] == [0, len(want)] and res[0][2] == want + bytes([FILL]) * 16, name


# ------------------------------------------------------------------ 5
def test_round_trip_on_the_device(gold, wanted, tmp_path):
    pytest.importorskip("PIL")
    from ccvs_amd import ops
    from ccvs_amd.helpers.generator import save_video_batch
    from ccvs_amd.tools import mjpeg
    rows = [row for row in S.rows() if gold[row[1] + "/in"].shape[1] > 4]
    assert len(rows) >= len(S.rows()) - 30
    for key, name, s, q, r in rows:
        h, w = gold[name + "/in"].shape[:2]
        scan, off = ops.mjpeg_encode_to_host(torch.from_numpy(gold[name + "/in"]).cuda(), q, r, sampling=s)
        data = mjpeg.jpeg_header(h, w, q, r, s) + scan + mjpeg.EOI
        assert np.array_equal(ops.mjpeg_decode([data])[0].cpu().numpy(), mjpeg.decode_frames([data])[0]), key
    # the decoder refuses subsampled frames at most 4 wide: that stays
    with pytest.raises(ValueError, match="chrominance"):
        ops.mjpeg_decode([mjpeg.jpeg_header(1, 1, 90, 1, 2) + wanted["noise_1x1/s2/q90"] + mjpeg.EOI])
    # files of our own writer through `read_avi_clips`
    clips = np.stack([np.stack([gold["noise_25x72/in"][:24, k:k + 40], gold["smooth_24x40/in"], gold["noise_24x40/in"]]) for k in (0, 9)])
    vid = torch.from_numpy(clips).cuda().permute(0, 1, 4, 2, 3).float() / 255
    u8 = save_video_batch(vid, 2, 0, str(tmp_path), 4, True, False, [0, 1], "kinetics600", video_format="avi", subsampling="420")
    assert np.array_equal(u8.numpy(), clips)
    paths = [str(tmp_path / f"vid_{i:05d}.avi") for i in range(2)]
    back = ops.read_avi_clips(paths)
    assert back.shape == (2, 3, 24, 40, 3) and back.is_cuda
    files = [mjpeg.read_avi(p)[3] for p in paths]
    assert all(mjpeg.parse_jpeg(f)["sampling"] == 2 for fs in files for f in fs)
    assert np.array_equal(back.cpu().numpy(), np.stack([mjpeg.decode_frames(fs) for fs in files]))


# ------------------------------------------------------------------ 6
def _avi_scans(path, h, w, quality, sampling):
    from ccvs_amd.tools import mjpeg
    fps, hh, ww, frames = mjpeg.read_avi(path)
    head = mjpeg.jpeg_header(h, w, quality, sampling=sampling)
    assert (hh, ww) == (h, w) and all(f.startswith(head) and f.endswith(mjpeg.EOI) for f in frames)
    return fps, [f[len(head):-2] for f in frames]


def test_save_video_batch_subsampled(tmp_path):
    from ccvs_amd.helpers.generator import save_video_batch
    vid = torch.rand(2, 3, 3, 24, 40, generator=torch.Generator().manual_seed(5)) * 2.4 - 1.2
    for sub, s in (("422", 1), ("420", 2)):
        for name, inet, dataset, q in (("plain", False, "bairhd", 90), ("inet", True, "kinetics600", 60)):
            d = tmp_path / (name + sub)
            u8 = save_video_batch(vid.cuda(), 2, 3, str(d), 4, True, inet, [-1, 1], dataset, video_format="avi", quality=q, subsampling=sub)
            assert u8.dtype == torch.uint8 and u8.device.type == "cpu" and u8.shape == (2, 3, 24, 40, 3)
            assert sorted(os.listdir(d)) == ["vid_00006.avi", "vid_00007.avi"]
            for i in range(2):
                fps, scans = _avi_scans(str(d / f"vid_{6 + i:05d}.avi"), 24, 40, q, s)
                assert fps == 4 and scans == [S.encode_scan_sub(u8[i, t].numpy(), q, s) for t in range(3)], (sub, name, i)
        # return_clip=False (what `save_results` asks for): the same files, no clip
        d = tmp_path / ("nc" + sub)
        assert save_video_batch(vid.cuda(), 2, 3, str(d), 4, True, False, [-1, 1], "bairhd", video_format="avi", return_clip=False, subsampling=sub) is None
        for i in range(2):
            assert open(d / f"vid_{6 + i:05d}.avi", "rb").read() == open(tmp_path / ("plain" + sub) / f"vid_{6 + i:05d}.avi", "rb").read()
        # the state marker on a 256 x 256 clip: the marked host clip is what the file holds
        big = torch.rand(1, 2, 3, 256, 256, generator=torch.Generator().manual_seed(6)) * 2 - 1
        state = torch.tensor([[[0.5, 0.25], [0.999, 0.0]]])
        d = tmp_path / ("s" + sub)
        marked = save_video_batch(big.cuda(), 1, 0, str(d), 4, True, False, [-1, 1], "bairhd", state=state, video_format="avi", return_clip=False, subsampling=sub)
        assert marked is not None and (marked[0, 0, 64, 127:130] == 255).all()
        fps, scans = _avi_scans(str(d / "vid_00000.avi"), 256, 256, 90, s)
        assert scans == [S.encode_scan_sub(marked[0, t].numpy(), 90, s) for t in range(2)], sub
    # the default is full chrominance: the bytes of a call that does not name the keyword
    a = tmp_path / "a444"
    save_video_batch(vid.cuda(), 2, 3, str(a), 4, True, False, [-1, 1], "bairhd", video_format="avi", subsampling="444")
    b = tmp_path / "b444"
    save_video_batch(vid.cuda(), 2, 3, str(b), 4, True, False, [-1, 1], "bairhd", video_format="avi")
    assert open(a / "vid_00006.avi", "rb").read() == open(b / "vid_00006.avi", "rb").read()


# ------------------------------------------------------------------ 7
def _sof_factors(files, tmp_path):
    """The sampling numbers of all frames of AVI files given as bytes."""
    from ccvs_amd.tools import mjpeg
    out = set()
    for data in files:
        open(tmp_path / "one.avi", "wb").write(data)
        out |= {mjpeg.parse_jpeg(f)["sampling"] for f in mjpeg.read_avi(str(tmp_path / "one.avi"))[3]}
    return out


def test_run_writes_420_files_pipelined_equals_serial(tmp_path, monkeypatch):
    avi = {mode: _run_files(tmp_path / mode, monkeypatch, mode, ["--video_format", "avi", "--video_quality", "80", "--video_subsampling", "420"])
           for mode in ("serial", "pipelined")}
    assert avi["serial"] == avi["pipelined"]
    assert sorted(avi["serial"]) == sorted((kind, f"vid_{i:05d}.avi") for kind in ("real", "fake", "rec") for i in range(10))
    assert _sof_factors(avi["serial"].values(), tmp_path) == {2}                                      # luminance 2 x 2
    plain = _run_files(tmp_path / "plain", monkeypatch, "pipelined", ["--video_format", "avi", "--video_quality", "80"])
    assert sorted(plain) == sorted(avi["serial"]) and _sof_factors(plain.values(), tmp_path) == {0}   # without the flag: 1 x 1
    assert all(len(avi["serial"][k]) < len(plain[k]) for k in plain)


# ------------------------------------------------------------------ 8
def test_metrics_command_on_420_files(gold, tmp_path, monkeypatch, capsys):
    from ccvs_amd.helpers.generator import save_video_batch
    from ccvs_amd.tools import mjpeg
    from ccvs_amd.tools.pytorch_metrics import metrics as M
    smooth, noise = gold["smooth_256x256/in"], gold["noise_25x72/in"]
    real = np.stack([np.stack([smooth[8 * i + t:8 * i + t + 24, 5 * t + i:5 * t + i + 40] if i % 2 else noise[t % 2:t % 2 + 24, i + 7 * t:i + 7 * t + 40] for t in range(3)]) for i in range(16)])    # the command scores batches of 16 clips
    fake = np.clip(real.astype(int) + np.random.RandomState(13).randint(-20, 21, size=real.shape), 0, 255).astype(np.uint8)
    want = {}
    for kind, clips in (("real", real), ("fake", fake)):
        vid = torch.from_numpy(clips).cuda().permute(0, 1, 4, 2, 3).float() / 255
        d = tmp_path / "results" / "0001_clips_420" / kind
        save_video_batch(vid, 16, 0, str(d), 4, True, False, [0, 1], "kinetics600", video_format="avi", return_clip=False, subsampling="420")
        files = sorted(os.listdir(d))
        assert files == [f"vid_{i:05d}.avi" for i in range(16)]
        frames = [mjpeg.read_avi(str(d / n))[3] for n in files]
        assert all(mjpeg.parse_jpeg(f)["sampling"] == 2 for fs in frames for f in fs)
        want[kind] = np.stack([np.stack([D.decode(f) for f in fs]) for fs in frames])
    _, ssim_w, psnr_w = M.metrics_from_videos(want["real"], want["fake"])
    assert 10 < psnr_w.item() < 40
    monkeypatch.chdir(tmp_path)
    M.main(M.parse_args(["--exp_tag", "clips_420"]))
    lines = capsys.readouterr().out.splitlines()
    assert "Found 16 real video files" in lines and "Found 16 fake video files" in lines
    mean_std = lambda score: f"{np.mean([score])!s} {np.std([score])!s}"
    assert lines[lines.index("Mean/std of SSIM across 1 runs") + 1] == mean_std(ssim_w)
    assert lines[lines.index("Mean/std of PSNR across 1 runs") + 1] == mean_std(psnr_w)
