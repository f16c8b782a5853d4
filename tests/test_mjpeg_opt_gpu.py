"""gpu: the JPEG encoder with per-frame optimised Huffman tables (`ccvs_mjpeg_encode_optimized`, csrc/jpeg.hip)
against the fixture tests/golden/mjpeg_opt_cases.npz -- the files Pillow (libjpeg) wrote with optimize=True -- and the spec mirror
tests/jpeg_opt_ref.py, which tests/test_mjpeg_opt_host.py holds against Pillow.  Every comparison is byte for byte.

  1. every fixture row: the tables tensor and the scan equal Pillow's, into buffers pre-filled with 0xAA -- the stream behind
     offsets[n] is untouched, a table's bytes behind its symbols are zero; the 256 x 256 row whose tree is 17 deep before limiting;
  2. five frames of different content (flat, noise, smooth, sparse, other noise) in one launch, with and without a CU budget that makes
     the workgroups walk across frame boundaries: each frame's tables and scan equal its single-frame launch; twice, the same bytes;
  3. a strided clip view (`clip[:, 1::2]`) is not copied;
  4. a stream that is too small: complete offsets, nothing at or beyond `capacity`, then `mjpeg_encode_to_host(optimize=True)` exact;
  5. `ops.mjpeg_encode` still gives the bytes of `ccvs_mjpeg_encode` / `ccvs_mjpeg_encode_sampled` and of the standard-table mirror;
  6. the way back: `ops.mjpeg_decode` of the optimised files (a table set per frame in one call) equals that of the standard files;
  7. `save_video_batch(video_format="avi", optimize=True)`: files that `read_avi` opens, the same pixels, not larger;
  8. `Generator(opt).run()` with `--video_format avi --video_optimize`: pipelined == serial, file for file;
  9. the metrics command prints the same PSNR / SSIM lines on optimised files as on standard ones.
"""
import ctypes
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jpeg_opt_ref as O  # noqa: E402
import jpeg_sub_ref as S  # noqa: E402
from tests.test_mjpeg_gpu import _run_files  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xAA
_SIDE = []


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "mjpeg_opt_cases.npz"))


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def encode(frames, quality, r, sampling, capacity, stride=None):
    """`ccvs_mjpeg_encode_optimized` on dense frames [n, H, W, 3] (or one frame) into a stream of `capacity` bytes and a tables tensor,
    both pre-filled with FILL: (the whole stream, the offsets, the tables uint8 [n, 4, 272]) on the host."""
    from ccvs_amd import lib
    L = lib.load()
    frames = frames[None] if frames.dim() == 3 else frames
    n, h, w = frames.shape[:3]
    out = torch.full((capacity,), FILL, dtype=torch.uint8, device="cuda")
    tables = torch.full((n, 4, 272), FILL, dtype=torch.uint8, device="cuda")
    offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    work = torch.empty(L.ccvs_mjpeg_optimized_workspace_bytes(n, h, w, sampling, r), dtype=torch.uint8, device="cuda")
    rc = L.ccvs_mjpeg_encode_optimized(_p(frames), frames.stride(0) if stride is None else stride, n, h, w, quality, sampling, r, _p(out), capacity,
                                       _p(offsets), _p(tables), _p(work), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.ccvs_last_error().decode()
    return out.cpu().numpy(), offsets.cpu().tolist(), tables.cpu().numpy()


def budgeted(lim, fn):
    """fn() on a side stream under a budget of `lim` CUs (0: none), behind everything queued on the current stream."""
    from ccvs_amd import ops
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream())
    side = _SIDE[0]
    ops.stream_cu_limit(side, lim)
    try:
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            res = fn()
        torch.cuda.synchronize()
        return res
    finally:
        ops.stream_cu_limit(side, 0)


# ------------------------------------------------------------------ 1
def test_every_fixture_row_equals_pillow(gold):
    worst = 0
    for key, name, s, q, r in O.rows():
        data = gold[key].tobytes()
        segs, start = O.segments(data)
        want, want_tables = data[start:-2], O.spec_bytes(O.dht_tables(segs))
        got, off, tables = encode(torch.from_numpy(gold[name + "/in"]).cuda(), q, r, s, len(want) + 37)
        assert np.array_equal(tables[0], want_tables), (key, "tables", np.argwhere(tables[0] != want_tables)[:4].tolist())
        assert off == [0, len(want)], (key, off, len(want))
        diff = np.flatnonzero(got[:len(want)] != np.frombuffer(want, dtype=np.uint8))
        worst = max(worst, diff.size)
        assert diff.size == 0, (key, "first differing byte", int(diff[0]), "of", len(want))
        assert (got[len(want):] == FILL).all(), key                                       # nothing behind the scan
    print("rows", len(O.rows()), "differing bytes", worst)


def test_limiter_row(gold):
    key, name, s, q, r = O.LIMITER_ROW
    n = int(gold[key + "/scan_len"])
    got, off, tables = encode(torch.from_numpy(O.image(name)).cuda(), q, r, s, n + 64)
    assert np.array_equal(tables[0], gold[key + "/dht"]) and tables[0, :, 15].any()        # Pillow's tables, 16-bit codes among them
    assert off == [0, n] and hashlib.sha256(got[:n].tobytes()).hexdigest() == str(gold[key + "/scan_sha256"])
    assert (got[n:] == FILL).all()


def test_ops_default_interval_and_host_form(gold):
    from ccvs_amd import ops
    from ccvs_amd.tools import mjpeg
    img = gold["noise_21x33/in"]
    for s in (0, 1, 2):
        r = S.default_restart(33, s)
        data = gold[f"noise_21x33/s{s}/q90/r{r}"].tobytes()
        segs, start = O.segments(data)
        want, want_tables = data[start:-2], O.spec_bytes(O.dht_tables(segs))
        stream, offsets, tables = ops.mjpeg_encode_optimized(torch.from_numpy(img).cuda(), 90, sampling=s)       # R = None, capacity = the raw size
        assert stream.numel() == img.size and offsets.tolist() == [0, len(want)] and bytes(stream[:len(want)].cpu().numpy()) == want
        assert tables.shape == (1, 4, 272) and tables.is_cuda and np.array_equal(tables[0].cpu().numpy(), want_tables)
        scans, off, host_tables = ops.mjpeg_encode_to_host(torch.from_numpy(img).cuda()[None], 90, None, s, optimize=True)
        assert (scans, off) == (want, [0, len(want)]) and np.array_equal(host_tables[0], want_tables)
        head = mjpeg.jpeg_header(21, 33, 90, sampling=s, huffman=mjpeg.huffman_from_spec(host_tables[0]))
        assert head + scans + mjpeg.EOI == data[:2] + data[20:]                            # Pillow's file but for its 18-byte JFIF APP0
    with pytest.raises(ValueError, match="sampling"):
        ops.mjpeg_encode_optimized(torch.from_numpy(img).cuda(), 90, sampling=3)


# ------------------------------------------------------------------ 2, 3
def _five(gold, h=24, w=40):
    return np.stack([O._flat(h, w), O._noise(h, w, 41), O._smooth(h, w), O._sparse(h, w, 42), O._noise(h, w, 43)])


def test_five_frames_in_one_launch_equal_their_single_launches(gold):
    clip = _five(gold)
    dev = torch.from_numpy(clip).cuda()
    for s, r in ((0, 5), (1, 2), (2, 1), (0, 1), (2, 16)):     # 3, 5, 6, 15 intervals per frame, and one (the interval is larger than the frame)
        single = [encode(dev[i], 90, r, s, 4096) for i in range(5)]
        scans = [g[:off[1]].tobytes() for g, off, _ in single]
        assert len({len(x) for x in scans}) == 5 and len({t.tobytes() for _, _, t in single}) == 5   # different lengths, different tables
        mirror = [O.encode_scan_optimized(clip[i], 90, s, r) for i in (0, 3)]
        assert [scans[0], scans[3]] == [m[0] for m in mirror] and np.array_equal(single[3][2][0], O.spec_bytes(mirror[1][1]))
        want = b"".join(scans)
        for lim in (0, 1):             # 1: at most 8 workgroups for the 15 .. 75 intervals: each walks on into later frames
            runs = [budgeted(lim, lambda: encode(dev, 90, r, s, len(want) + 5)) for _ in range(2)]
            got, off, tables = runs[0]
            assert off == list(np.cumsum([0] + [len(x) for x in scans])), (s, r, lim)
            assert np.array_equal(tables, np.concatenate([t for _, _, t in single])), (s, r, lim)
            assert got[:len(want)].tobytes() == want and (got[len(want):] == FILL).all(), (s, r, lim)
            assert runs[1][1] == off and np.array_equal(runs[1][0], got) and np.array_equal(runs[1][2], tables)      # the same bytes on every run


def test_strided_clip_view_is_not_copied(gold):
    from ccvs_amd import ops
    five = _five(gold)
    clip = np.stack([np.concatenate([five, five[:1]]), np.concatenate([five[::-1], five[2:3]])])       # [2, 6, 24, 40, 3]
    dev = torch.from_numpy(clip.copy()).cuda()
    view = dev[:, 1::2]
    assert not view.is_contiguous()
    for s in (0, 2):
        frames = [(b, t) for b in range(2) for t in (1, 3, 5)]
        single = {f: encode(dev[f], 90, S.default_restart(40, s), s, 4096) for f in frames}
        stream, offsets, tables = ops.mjpeg_encode_optimized(view, 90, sampling=s)
        off = offsets.tolist()
        assert off == list(np.cumsum([0] + [single[f][1][1] for f in frames]))
        assert stream[:off[-1]].cpu().numpy().tobytes() == b"".join(single[f][0][:single[f][1][1]].tobytes() for f in frames)
        assert np.array_equal(tables.cpu().numpy(), np.concatenate([single[f][2] for f in frames]))
        # the C entry point reads the view in place: the frame stride of the first axis' view
        got, off2, t2 = encode(dev[0, 1::2], 90, S.default_restart(40, s), s, off[3] + 3)
        assert off2 == off[:4] and got[:off[3]].tobytes() == stream[:off[3]].cpu().numpy().tobytes() and dev[0, 1::2].stride(0) == 2 * 24 * 40 * 3


# ------------------------------------------------------------------ 4
def test_too_small_stream_keeps_offsets_and_writes_nothing_beyond_capacity(gold):
    from ccvs_amd import ops
    img = torch.from_numpy(gold["noise_40x24/in"]).cuda()
    frames = torch.stack([img, img])
    for s in (0, 1, 2):
        data = gold[f"noise_40x24/s{s}/q100/r{S.default_restart(24, s)}"].tobytes()
        segs, start = O.segments(data)
        want, want_tables = data[start:-2], O.spec_bytes(O.dht_tables(segs))
        r = S.default_restart(24, s)
        capacity = len(want) + len(want) // 3                                               # the first frame fits, the second does not
        got, off, tables = encode(frames, 100, r, s, 2 * len(want) + 64)
        assert off == [0, len(want), 2 * len(want)] and got[:2 * len(want)].tobytes() == want + want
        from ccvs_amd import lib
        L = lib.load()
        out = torch.full((2 * len(want) + 64,), FILL, dtype=torch.uint8, device="cuda")
        tab = torch.full((2, 4, 272), FILL, dtype=torch.uint8, device="cuda")
        offsets = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        work = torch.empty(L.ccvs_mjpeg_optimized_workspace_bytes(2, 40, 24, s, r), dtype=torch.uint8, device="cuda")
        rc = L.ccvs_mjpeg_encode_optimized(_p(frames), 40 * 24 * 3, 2, 40, 24, 100, s, r, _p(out), capacity, _p(offsets), _p(tab), _p(work),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        got = out.cpu().numpy()
        assert offsets.tolist() == [0, len(want), 2 * len(want)] and 2 * len(want) > capacity > len(want)
        assert (got[capacity:] == FILL).all()                                               # untouched at and beyond capacity
        assert got[:capacity].tobytes() == (want + want)[:capacity]
        assert np.array_equal(tab.cpu().numpy(), np.stack([want_tables, want_tables]))     # the tables do not depend on the capacity
        # through ops: the bytes that fit, then the host form's second run is exact
        stream, off, _ = ops.mjpeg_encode_optimized(img, 100, r, capacity=len(want) - 9, sampling=s)
        assert stream.numel() == len(want) - 9 and off.tolist() == [0, len(want)] and bytes(stream.cpu().numpy()) == want[:-9]
    # the host form's own second run: a scan larger than the raw frame (21 x 33 is padded to 24 x 40; noise at quality 100, full chrominance)
    odd = torch.from_numpy(gold["noise_21x33/in"]).cuda()
    data = gold["noise_21x33/s0/q100/r5"].tobytes()
    segs, start = O.segments(data)
    want = data[start:-2]
    assert len(want) > odd.numel()
    scans, off, tables = ops.mjpeg_encode_to_host(odd, 100, optimize=True)
    assert (scans, off) == (want, [0, len(want)]) and np.array_equal(tables[0], O.spec_bytes(O.dht_tables(segs)))


# ------------------------------------------------------------------ 5
def test_default_path_bytes_did_not_move(gold):
    from ccvs_amd import lib, ops
    L = lib.load()
    cur = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    clip = _five(gold, 21, 33)
    dev = torch.from_numpy(clip).cuda()
    for s in (0, 1, 2):
        r = S.default_restart(33, s)
        want = [S.encode_scan_sub(clip[i], 90, s, r) for i in range(5)]
        stream, offsets = ops.mjpeg_encode(dev, 90, sampling=s)
        off = offsets.tolist()
        assert off == list(np.cumsum([0] + [len(x) for x in want])) and stream[:off[-1]].cpu().numpy().tobytes() == b"".join(want)
        assert ops.mjpeg_encode_to_host(dev, 90, sampling=s) == (b"".join(want), off)       # two results, as before
        out = torch.full((off[-1] + 16,), FILL, dtype=torch.uint8, device="cuda")
        offsets = torch.full((6,), -1, dtype=torch.int64, device="cuda")
        work = torch.empty(L.ccvs_mjpeg_sampled_workspace_bytes(5, 21, 33, s, r), dtype=torch.uint8, device="cuda")
        if s == 0:
            assert L.ccvs_mjpeg_workspace_bytes(5, 21, 33, r) == work.numel()
            rc = L.ccvs_mjpeg_encode(_p(dev), 21 * 33 * 3, 5, 21, 33, 90, r, _p(out), out.numel(), _p(offsets), _p(work), cur)
        else:
            rc = L.ccvs_mjpeg_encode_sampled(_p(dev), 21 * 33 * 3, 5, 21, 33, 90, s, r, _p(out), out.numel(), _p(offsets), _p(work), cur)
        assert rc == 0 and offsets.tolist() == off and out.cpu().numpy().tobytes() == b"".join(want) + bytes([FILL]) * 16


# ------------------------------------------------------------------ 6
def test_round_trip_on_the_device(gold):
    from ccvs_amd import ops
    from ccvs_amd.tools import mjpeg
    clip = _five(gold)
    dev = torch.from_numpy(clip).cuda()
    for s in (0, 1, 2):
        scans, off, tables = ops.mjpeg_encode_to_host(dev, 75, sampling=s, optimize=True)
        std_scans, std_off = ops.mjpeg_encode_to_host(dev, 75, sampling=s)
        opt = [mjpeg.jpeg_header(24, 40, 75, sampling=s, huffman=mjpeg.huffman_from_spec(tables[i])) + scans[off[i]:off[i + 1]] + mjpeg.EOI for i in range(5)]
        std = [mjpeg.jpeg_header(24, 40, 75, sampling=s) + std_scans[std_off[i]:std_off[i + 1]] + mjpeg.EOI for i in range(5)]
        assert len(mjpeg.plan_frames(opt)["tables"]) == 5 * mjpeg.TABLE_BYTES              # five table sets in one decode call
        a, b = ops.mjpeg_decode(opt), ops.mjpeg_decode(std)
        assert a.shape == (5, 24, 40, 3) and torch.equal(a, b), s
        assert off[-1] < std_off[-1]
    # every fixture row through the decoder: Pillow's own optimised files decode to what our standard files decode to
    for key, name, s, q, r in O.rows()[::7]:
        img = gold[name + "/in"]
        h, w = img.shape[:2]
        scan, _ = ops.mjpeg_encode_to_host(torch.from_numpy(img).cuda(), q, r, sampling=s)
        assert torch.equal(ops.mjpeg_decode([gold[key].tobytes()]), ops.mjpeg_decode([mjpeg.jpeg_header(h, w, q, r, s) + scan + mjpeg.EOI])), key


# ------------------------------------------------------------------ 7
def test_save_video_batch_optimized(tmp_path):
    from ccvs_amd import ops
    from ccvs_amd.helpers.generator import save_video_batch
    from ccvs_amd.tools import mjpeg
    vid = torch.rand(2, 3, 3, 24, 40, generator=torch.Generator().manual_seed(5)) * 2.4 - 1.2
    vid[1, 2] = 0.25                                                                       # a flat frame among them
    for sub, s in (("444", 0), ("422", 1), ("420", 2)):
        a, b = tmp_path / ("std" + sub), tmp_path / ("opt" + sub)
        u8 = save_video_batch(vid.cuda(), 2, 3, str(a), 4, True, False, [-1, 1], "bairhd", video_format="avi", quality=80, subsampling=sub)
        u8o = save_video_batch(vid.cuda(), 2, 3, str(b), 4, True, False, [-1, 1], "bairhd", video_format="avi", quality=80, subsampling=sub, optimize=True)
        assert torch.equal(u8, u8o) and sorted(os.listdir(b)) == ["vid_00006.avi", "vid_00007.avi"]
        for i in range(2):
            name = f"vid_{6 + i:05d}.avi"
            fps, h, w, frames = mjpeg.read_avi(str(b / name))
            _, _, _, std = mjpeg.read_avi(str(a / name))
            assert (fps, h, w, len(frames)) == (4, 24, 40, 3)
            assert os.path.getsize(b / name) <= os.path.getsize(a / name) and all(len(x) <= len(y) for x, y in zip(frames, std))
            assert torch.equal(ops.mjpeg_decode(frames), ops.mjpeg_decode(std)), (sub, i)
            for t, f in enumerate(frames):                                                  # every frame carries the tables the mirror builds for it
                scan, tables, _ = O.encode_scan_optimized(u8[i, t].numpy(), 80, s)
                head = mjpeg.jpeg_header(24, 40, 80, sampling=s, huffman=mjpeg.huffman_from_spec(O.spec_bytes(tables)))
                assert f == head + scan + mjpeg.EOI, (sub, i, t)
        # return_clip=False (what `save_results` asks for): the same files, no clip
        c = tmp_path / ("nc" + sub)
        assert save_video_batch(vid.cuda(), 2, 3, str(c), 4, True, False, [-1, 1], "bairhd", video_format="avi", quality=80, return_clip=False,
                                subsampling=sub, optimize=True) is None
        assert all(open(c / n, "rb").read() == open(b / n, "rb").read() for n in os.listdir(b))


# ------------------------------------------------------------------ 8
def test_run_writes_optimized_files_pipelined_equals_serial(tmp_path, monkeypatch):
    from ccvs_amd.tools import mjpeg
    avi = {mode: _run_files(tmp_path / mode, monkeypatch, mode, ["--video_format", "avi", "--video_quality", "80", "--video_optimize"])
           for mode in ("serial", "pipelined")}
    assert avi["serial"] == avi["pipelined"]
    assert sorted(avi["serial"]) == sorted((kind, f"vid_{i:05d}.avi") for kind in ("real", "fake", "rec") for i in range(10))
    plain = _run_files(tmp_path / "plain", monkeypatch, "pipelined", ["--video_format", "avi", "--video_quality", "80"])
    assert sorted(plain) == sorted(avi["serial"]) and all(len(avi["serial"][k]) < len(plain[k]) for k in plain)
    # without the flag every frame carries the Annex K tables; with it, tables of its own
    standard = {k: (bytes(b), bytes(v)) for k, (b, v) in mjpeg.HUFF.items()}
    for files, own in ((plain, False), (avi["serial"], True)):
        open(tmp_path / "one.avi", "wb").write(files["fake", "vid_00003.avi"])
        for f in mjpeg.read_avi(str(tmp_path / "one.avi"))[3]:
            assert (mjpeg.parse_jpeg(f)["huffman"] != standard) == own


# ------------------------------------------------------------------ 9
def test_metrics_command_prints_the_same_lines(gold, tmp_path, monkeypatch, capsys):
    from ccvs_amd.helpers.generator import save_video_batch
    from ccvs_amd.tools.pytorch_metrics import metrics as M
    five = _five(gold)
    real = np.stack([np.stack([np.roll(five[(i + t) % 5], 3 * i + t, axis=1) for t in range(3)]) for i in range(16)])    # the command scores batches of 16 clips
    fake = np.clip(real.astype(int) + np.random.RandomState(13).randint(-20, 21, size=real.shape), 0, 255).astype(np.uint8)
    lines = {}
    for tag, optimize in (("std", False), ("opt", True)):
        for kind, clips in (("real", real), ("fake", fake)):
            vid = torch.from_numpy(clips).cuda().permute(0, 1, 4, 2, 3).float() / 255
            d = tmp_path / "results" / f"0001_clips_{tag}" / kind
            save_video_batch(vid, 16, 0, str(d), 4, True, False, [0, 1], "kinetics600", video_format="avi", return_clip=False, optimize=optimize)
            assert sorted(os.listdir(d)) == [f"vid_{i:05d}.avi" for i in range(16)]
        monkeypatch.chdir(tmp_path)
        M.main(M.parse_args(["--exp_tag", f"clips_{tag}"]))
        out = capsys.readouterr().out.splitlines()
        assert "Found 16 real video files" in out and "Found 16 fake video files" in out
        lines[tag] = [out[out.index(f"Mean/std of {m} across 1 runs") + 1] for m in ("SSIM", "PSNR")]
    print(lines)
    assert lines["std"] == lines["opt"] and 10 < float(lines["opt"][1].split()[0]) < 40
    size = lambda tag: sum(os.path.getsize(os.path.join(r, f)) for r, _, fs in os.walk(tmp_path / "results" / f"0001_clips_{tag}") for f in fs)
    assert size("opt") < size("std")
