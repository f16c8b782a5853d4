"""gpu: the JPEG decoder (csrc/jpeg_decode.hip) against the fixture tests/golden/mjpeg_decode_cases.npz -- the
pixels Pillow (libjpeg-turbo) decoded -- and against the spec mirror tests/jpeg_decode_ref.py, which tests/test_mjpeg_decode_host.py
holds against both.  Every comparison is byte for byte.

  a. every fixture row: the pixels equal Pillow's, decoded into a slice of a larger buffer pre-filled with 0xA5 whose other bytes stay
     untouched; a second run gives the same bytes;
  b. several frames in one call -- the encoder's own scans at two qualities, and two files with Huffman tables of their own: each frame
     equals its single-frame decode and the mirror;
  c. the round trip at the workload's frame size: four 256 x 256 frames encoded by `ops.mjpeg_encode`, decoded, against the mirror;
  d. status words: a unit whose recorded length is cut short, a unit with one byte altered -- exactly the units the mirror fails report
     a non-zero status, the other units' pixels are right, `ops.mjpeg_decode` names the frame and the unit; bad arguments are refused
     before any launch;
  e. the metrics from files: `metrics_from_files` and `main` on .avi and .npy folders give exactly the values of `metrics_from_videos`
     on the mirror-decoded clips.
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

pytestmark = pytest.mark.gpu
FILL = 0xA5


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return D.load_fixture(os.path.join(golden_dir, "mjpeg_decode_cases.npz"))[0]


def project_files(frames_u8, quality):
    """The frames as the project writes them: its header, the scan `ops.mjpeg_encode` gives, EOI."""
    from ccvs_amd import ops
    from ccvs_amd.tools import mjpeg
    frames_u8 = np.asarray(frames_u8)
    data, off = ops.mjpeg_encode_to_host(torch.from_numpy(frames_u8).cuda(), quality)
    head = mjpeg.jpeg_header(frames_u8.shape[-3], frames_u8.shape[-2], quality)
    return [head + data[off[i]:off[i + 1]] + mjpeg.EOI for i in range(len(off) - 1)]


# ------------------------------------------------------------------ a
def test_every_fixture_row_equals_pillow_and_runs_repeat(fixture):
    from ccvs_amd import ops
    worst = 0
    for key, (data, rgb) in fixture.items():
        h, w = rgb.shape[:2]
        big = torch.full((3, h, w, 3), FILL, dtype=torch.uint8, device="cuda")
        out = ops.mjpeg_decode([data], out=big[1:2])
        assert out.data_ptr() == big[1].data_ptr() and out.shape == (1, h, w, 3)
        got = big.cpu().numpy()
        diff = int((got[1] != rgb).sum())
        worst = max(worst, diff)
        assert diff == 0, (key, "differing bytes", diff, "of", rgb.size)
        assert (got[0] == FILL).all() and (got[2] == FILL).all(), key                       # nothing around the frame
        again = ops.mjpeg_decode([data])                                                     # the same bytes on every run
        assert again.shape == (1, h, w, 3) and again.dtype == torch.uint8 and np.array_equal(again[0].cpu().numpy(), got[1]), key
    print("rows", len(fixture), "differing bytes", worst)


# ------------------------------------------------------------------ b
def test_several_frames_in_one_call(fixture):
    from ccvs_amd import ops
    rng = np.random.RandomState(11)
    smooth = R.CASES["smooth_64x64"][0]()[:24, :40]
    clip = np.stack([rng.randint(0, 256, size=(24, 40, 3)).astype(np.uint8), smooth, np.zeros((24, 40, 3), np.uint8), np.full((24, 40, 3), 255, np.uint8)])
    files = project_files(clip, 90) + project_files(clip, 100)                               # two quantisers in one call
    sets = [files, [fixture[k][0] for k in ("noise_13x21/q90/s2/opt", "noise_13x21/q5/s2/opt", "noise_13x21/q90/s2/r3")]]
    for files in sets:
        want = np.stack([D.decode(f) for f in files])
        got, status = ops.mjpeg_decode(files, check=False)
        assert status.dtype == torch.int32 and status.is_cuda and not status.any()
        assert np.array_equal(got.cpu().numpy(), want)
        for i, f in enumerate(files):
            assert np.array_equal(ops.mjpeg_decode([f])[0].cpu().numpy(), want[i]), i
    from ccvs_amd.tools import mjpeg
    assert mjpeg.plan_frames(sets[0])["frame_table"].tolist() == [0] * 4 + [1] * 4 and mjpeg.plan_frames(sets[1])["frame_table"].tolist() == [0, 1, 2]


# ------------------------------------------------------------------ c
def test_round_trip_at_the_workload_frame_size():
    from ccvs_amd import ops
    smooth = R.CASES["smooth_256x256"][0]()
    rng = np.random.RandomState(12)
    grain = np.clip(smooth.astype(int) + rng.randint(-6, 7, size=smooth.shape), 0, 255).astype(np.uint8)
    clip = np.stack([smooth, smooth[::-1].copy(), grain, np.ascontiguousarray(smooth.transpose(1, 0, 2))])
    files = project_files(clip, 90)
    got = ops.mjpeg_decode(files)
    assert got.shape == (4, 256, 256, 3)
    want = np.stack([D.decode(f) for f in files])
    assert np.array_equal(got.cpu().numpy(), want)
    assert int(np.abs(want.astype(int) - clip.astype(int)).max()) <= 40                      # quality 90: the clip comes back
    import tempfile
    from ccvs_amd.tools import mjpeg
    with tempfile.TemporaryDirectory() as d:
        for i in range(2):
            mjpeg.write_avi(os.path.join(d, f"v{i}.avi"), files[2 * i:2 * i + 2], 4, 256, 256)
        clips = ops.read_avi_clips([os.path.join(d, "v0.avi"), os.path.join(d, "v1.avi")])
        assert clips.shape == (2, 2, 256, 256, 3) and np.array_equal(clips.cpu().numpy().reshape(4, 256, 256, 3), want)
        mjpeg.write_avi(os.path.join(d, "short.avi"), files[:1], 4, 256, 256)
        with pytest.raises(ValueError, match="short.avi holds 1 frames"):
            ops.read_avi_clips([os.path.join(d, "v0.avi"), os.path.join(d, "short.avi")])


# ------------------------------------------------------------------ d
def unit_mask(p, unit):
    """True at the pixels of a 4:4:4 frame that the MCUs of a unit (offset, length, first MCU, MCUs) cover."""
    _, _, mcux, _ = D.geometry(p["h"], p["w"], 0)
    mask = np.zeros((p["h"], p["w"]), dtype=bool)
    for m in range(unit[2], unit[2] + unit[3]):
        mask[8 * (m // mcux):8 * (m // mcux) + 8, 8 * (m % mcux):8 * (m % mcux) + 8] = True
    return mask


def test_status_words_name_the_units_that_fail(fixture):
    from ccvs_amd import ops
    from ccvs_amd.tools import mjpeg
    key = "noise_16x40_r3/q100/s0/r3"
    data, rgb = fixture[key]
    p = D.parse(data)
    units = D.split_units(p["scan"], p["ri"], 10)
    assert len(units) == 4
    # 1. the recorded length of unit 2 cut short by the host; the bytes themselves stay
    plan = mjpeg.plan_frames([data])
    plan["units"] = plan["units"].copy()
    plan["units"][2, 2] -= 3
    got, status = ops.mjpeg_decode_planned(plan)
    status = status.cpu().numpy()
    assert (status != 0).tolist() == [False, False, True, False], status
    keep = ~unit_mask(p, units[2])
    assert keep.sum() == 16 * 40 - 3 * 64 and np.array_equal(got[0].cpu().numpy()[keep], rgb[keep])
    # 2. one byte of unit 1 altered: the first position at which the mirror fails unit 1 (an alteration may also just change pixels)
    off, length = units[1][:2]
    for at in range(off + 4, off + length - 4):
        if 0xFF in (p["scan"][at - 1], p["scan"][at], p["scan"][at] ^ 0x10):
            continue
        scan = p["scan"][:at] + bytes([p["scan"][at] ^ 0x10]) + p["scan"][at + 1:]
        _, mirror_status = D.decode_coefficients(p, scan=scan)
        if mirror_status[1]:
            break
    assert [s != 0 for s in mirror_status] == [False, True, False, False]
    bad = data[:p["scan_offset"]] + scan + data[-2:]
    got, status = ops.mjpeg_decode([bad], check=False)
    assert (status.cpu().numpy() != 0).tolist() == [False, True, False, False], status
    keep = ~unit_mask(p, units[1])
    assert np.array_equal(got[0].cpu().numpy()[keep], rgb[keep])
    with pytest.raises(ValueError, match=r"frame 0, unit 1 \(MCUs 3 \.\. 5\) failed with status [2-5]"):
        ops.mjpeg_decode([bad])
    with pytest.raises(ValueError, match=r"frame 1, unit 1 .*1 of 8 units failed"):
        ops.mjpeg_decode([data, bad])


def test_bad_arguments_are_refused_before_any_launch(fixture):
    from ccvs_amd import lib
    from ccvs_amd.tools import mjpeg
    L = lib.load()
    data, rgb = fixture["noise_13x21/q90/s2/r3"]
    plan = mjpeg.plan_frames([data])
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    scans, units, tables, ft = dev(plan["scans"]), dev(plan["units"]), dev(plan["tables"]), dev(plan["frame_table"])
    out = torch.full((13, 21, 3), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    work = torch.zeros(L.ccvs_mjpeg_decode_workspace_bytes(1, 13, 21, 2), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    host = plan["units"].copy()

    def call(n=1, sampling=2, scan_bytes=scans.numel(), scans_=scans, units_=units, host_=host, out_=out, w=21):
        rc = L.ccvs_mjpeg_decode(p(scans_), scan_bytes, p(units_), host_.ctypes.data_as(ctypes.c_void_p) if host_ is not None else None, 1, p(tables), 1, p(ft),
                                 n, 13, w, sampling, p(out_), 13 * 21 * 3, p(status), p(work), None)
        return rc, L.ccvs_last_error().decode()

    outside = host.copy()
    outside[0, 2] += 1
    for kw, word in (({"scans_": None}, "null"), ({"units_": None}, "null"), ({"host_": None}, "null"), ({"out_": None}, "null"), ({"n": 0}, "no frames"),
                     ({"sampling": 3}, "sampling"), ({"sampling": 1, "w": 4}, "chrominance"), ({"host_": outside}, "outside the stream"),
                     ({"scan_bytes": scans.numel() - 1}, "outside the stream")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert (out == FILL).all() and status.tolist() == [-7] and int(work.sum()) == 0
    rc, msg = call()
    assert rc == 0, msg
    assert status.tolist() == [0] and np.array_equal(out.cpu().numpy(), rgb)
    # the kernel checks the device copy of the unit table too: it differs from the host's here and is refused there, nothing is read
    units[0, 2] += 5
    status.fill_(-7)
    rc, msg = call()
    assert rc == 0 and status.tolist() == [1]


# ------------------------------------------------------------------ e
def mean_std(score):
    """The line `print_scores` prints under "Mean/std of ..." for one run."""
    return f"{np.mean([score])!s} {np.std([score])!s}"


def test_metrics_from_files_equal_the_mirror(fixture, tmp_path, monkeypatch, capsys):
    from ccvs_amd.helpers.generator import save_video_batch
    from ccvs_amd.tools import mjpeg
    from ccvs_amd.tools.pytorch_metrics import metrics as M
    imgs = D.images()
    smooth, noise, sparse = imgs["smooth_64x64"], imgs["noise_24x40"], imgs["sparse_32x32"]
    real = np.stack([np.stack([smooth[2 * i + t:2 * i + t + 16, 3 * t + i:3 * t + i + 24] if i % 3 else
                               (noise[t:t + 16, i:i + 24] if i % 2 else sparse[i:i + 16, t:t + 24]) for t in range(3)]) for i in range(16)])
    rng = np.random.RandomState(13)
    fake = np.clip(real.astype(int) + rng.randint(-20, 21, size=real.shape), 0, 255).astype(np.uint8)
    assert real.shape == (16, 3, 16, 24, 3)
    want = {}
    for tag, fmt in (("0001_clips_avi", "avi"), ("0002_clips_npy", "npy")):
        for kind, clips in (("real", real), ("fake", fake)):
            vid = torch.from_numpy(clips).cuda().permute(0, 1, 4, 2, 3).float() / 255
            d = tmp_path / "results" / tag / kind
            save_video_batch(vid, 16, 0, str(d), 4, True, False, [0, 1], "kinetics600", video_format=fmt)
            files = sorted(os.listdir(d))
            assert files == [f"vid_{i:05d}.{fmt}" for i in range(16)]
            if fmt == "avi":
                want[tag, kind] = np.stack([np.stack([D.decode(f) for f in mjpeg.read_avi(str(d / n))[3]]) for n in files])
            else:
                want[tag, kind] = np.stack([np.load(d / n) for n in files])
            assert want[tag, kind].shape == (16, 3, 16, 24, 3)
    monkeypatch.chdir(tmp_path)
    for tag in ("0001_clips_avi", "0002_clips_npy"):
        real_files = M.get_video_files(os.path.join("results", tag, "real"))
        fake_files = M.get_video_files(os.path.join("results", tag, "fake"))
        assert len(real_files) == len(fake_files) == 16
        loaded = M.load_videos(real_files, None, 8)
        assert loaded.is_cuda and loaded.dtype == torch.uint8 and np.array_equal(loaded.cpu().numpy(), want[tag, "real"])
        assert np.array_equal(M.load_video(fake_files[5], None).cpu().numpy(), want[tag, "fake"][5])
        lp, ssim, psnr = M.metrics_from_files(real_files, fake_files, None, 1, False, [])
        _, ssim_w, psnr_w = M.metrics_from_videos(want[tag, "real"], want[tag, "fake"])
        assert lp is None and ssim.item() == ssim_w.item() and psnr.item() == psnr_w.item() and 10 < psnr.item() < 40
        _, ssim_k, psnr_k = M.metrics_from_files(real_files, fake_files, None, 1, False, [0, 2])
        _, ssim_kw, psnr_kw = M.metrics_from_videos(want[tag, "real"], want[tag, "fake"], idx=[0, 2])
        assert [s.item() for s in ssim_k] == [s.item() for s in ssim_kw] and [s.item() for s in psnr_k] == [s.item() for s in psnr_kw]
        capsys.readouterr()
        M.main(M.parse_args(["--exp_tag", tag[5:]]))
        lines = capsys.readouterr().out.splitlines()
        assert "Found 16 real video files" in lines and "Found 16 fake video files" in lines
        assert "LPIPS scores: not available (needs pretrained weights)" in lines
        at = lines.index("Mean/std of SSIM across 1 runs")
        assert lines[at - 2] == "Individual SSIM scores" and lines[at + 1] == mean_std(ssim_w)
        at = lines.index("Mean/std of PSNR across 1 runs")
        assert lines[at - 2] == "Individual PSNR scores" and lines[at + 1] == mean_std(psnr_w)
        M.main(M.parse_args(["--exp_tag", tag[5:], "--idx", "0", "2"]))
        lines = capsys.readouterr().out.splitlines()
        assert lines[lines.index("Mean/std of SSIM-1 across 1 runs") + 1] == mean_std(ssim_kw[1])
        assert lines[lines.index("Mean/std of PSNR-0 across 1 runs") + 1] == mean_std(psnr_kw[0])
