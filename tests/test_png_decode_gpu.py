"""-m gpu: the PNG decoder on the MI355X (`ccvs_zlib_inflate`, `ccvs_png_decode`).  Every comparison is exact.

  1. `ops.zlib_inflate` equals zlib on every plain and hand-assembled stream of tests/png_decode_ref.py, in one launch each, into an
     output pre-filled with 0xA5 with gaps between the streams' ranges: every byte outside a range is still 0xA5.  The planted buffer,
     the 256 x 256 frames and the stored stream are several times 32 KiB long;
  2. the status words equal the spec mirror's on the hand-assembled streams and on the 2000 mutations the sanitizer program runs
     (tests/test_png_decode_core.py); good streams in the same launch still decode, nothing is written outside any stream's range;
  3. `ops.png_decode`: random residuals under a random filter type per row and under each type forced, flat and ramp residuals (Paeth
     ties), at 1x1, 1x70, 65x1, 2x2, 63x63, 64x64, 65x67, 129x33 and 256x256 equal `apng.unfilter`; a type byte 5 gives BAD_FILTER on
     that frame only; five frames per launch equal their single launches, also under a budget of 8 workgroups; a frame stride with
     0xA5 between the frames;
  4. `ops.read_apng_clips` on the files of `save_video_batch(video_format="apng")` equals the returned clip, and on Pillow's LZ77-coded
     PNG / APNG files of the same pixels; `png_encode` then `png_decode` round-trips a 256 x 256 x 4 clip;
  5. the metrics and fvd commands with `--png_decode gpu` print the lines they print with `host`;
  6. frame folders through `FrameLoader` with `--png_decode gpu` and `host`: equal fp32 batches (a video of .npy frames and one of
     palette PNGs among them), also with `--num_workers 2` and a resize / crop plan; `Generator.run()` writes the same `real/` files.
"""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import apng_ref as R  # noqa: E402
import png_decode_ref as D  # noqa: E402
from tests.test_ingest_gpu import TINY_ARGV  # noqa: E402
from tests.test_mjpeg_opt_gpu import budgeted  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xA5


def inflate_poisoned(cases):
    """`ops.zlib_inflate` on (name, stream, expect, ...) cases, the ranges 1 .. 13 bytes apart in an output of 0xA5: (the output on the
    host, the status words, the ranges' offsets); every byte outside the ranges is checked here."""
    from ccvs_amd import ops
    offsets, pos = [], 5
    for i, c in enumerate(cases):
        offsets.append(pos)
        pos += c[2] + 1 + (7 * i) % 13
    out = torch.full((pos,), FILL, dtype=torch.uint8, device="cuda")
    got, status = ops.zlib_inflate([c[1] for c in cases], [c[2] for c in cases], check=False, out=out, offsets=offsets)
    assert got is out
    host, inside = out.cpu().numpy(), np.zeros(pos, bool)
    for o, c in zip(offsets, cases):
        inside[o:o + c[2]] = True
    assert (host[~inside] == FILL).all()
    return host, status.cpu().numpy(), offsets


# ------------------------------------------------------------------ 1
def test_inflate_equals_zlib_on_plain_streams():
    plain = D.plain_streams()
    assert sum(len(raw) > 4 * 32768 for _, _, raw in plain) >= 10
    host, status, offsets = inflate_poisoned([(n, s, len(raw)) for n, s, raw in plain])
    assert not status.any(), [(plain[i][0], D.NAMES[status[i]]) for i in status.nonzero()[0][:5]]
    for o, (name, stream, raw) in zip(offsets, plain):
        assert host[o:o + len(raw)].tobytes() == raw, name


def test_inflate_through_ops_checks_and_raises():
    from ccvs_amd import ops
    raws = [b"", b"a", bytes(range(256)) * 40]
    out = ops.zlib_inflate([zlib.compress(r, 9) for r in raws], [len(r) for r in raws])
    assert out.is_cuda and out.cpu().numpy().tobytes() == b"".join(raws)
    with pytest.raises(ValueError, match=r"zlib_inflate: stream 1 failed with status 9 \(TOO_SHORT: .*\); 2 of 3 failed"):
        ops.zlib_inflate([zlib.compress(r) for r in raws], [0, 2, 5])


# ------------------------------------------------------------------ 2
def test_status_words_equal_the_mirror():
    good = [c for c in D.judged("plain") if len(c[1]) < 3000][:40]
    cases = D.judged("hand") + good + D.judged("mutations")
    assert len(cases) >= 2070
    host, status, offsets = inflate_poisoned(cases)
    wrong = [(c[0], D.NAMES[s], D.NAMES[c[3]]) for c, s in zip(cases, status) if s != c[3]]
    assert not wrong, (len(wrong), wrong[:8])
    for o, (name, stream, expect, want, out) in zip(offsets, cases):
        if want == D.OK:
            assert host[o:o + expect].tobytes() == out, name
    assert (status[len(D.judged("hand")):][:len(good)] == 0).all()


# ------------------------------------------------------------------ 3
SIZES = ((1, 1), (1, 70), (65, 1), (2, 2), (63, 63), (64, 64), (65, 67), (129, 33), (256, 256))


def filtered_frames(h, w, seed):
    """{name: the filtered bytes [h, 3 w + 1]}: random residuals under a random type per row and under each type forced, flat and ramp
    residuals under Paeth and under random types (a = b = c and pa = pb ties)."""
    rng = np.random.default_rng(seed)
    out = {}

    def add(name, res, types):
        out[name] = np.concatenate([np.asarray(types, np.uint8).reshape(h, 1), np.asarray(res, np.uint8).reshape(h, 3 * w)], 1)
    add("random", rng.integers(0, 256, (h, 3 * w)), rng.integers(0, 5, h))
    for t in range(5):
        add(f"type{t}", rng.integers(0, 256, (h, 3 * w)), np.full(h, t))
    add("flat_paeth", np.full((h, 3 * w), 3), np.full(h, 4))
    add("zero_random", np.zeros((h, 3 * w)), rng.integers(0, 5, h))
    add("ramp_paeth", (np.arange(3 * w)[None, :] // 3 + np.arange(h)[:, None]) % 7, np.full(h, 4))
    add("ramp_random", (np.arange(3 * w)[None, :] * 5 + np.arange(h)[:, None] * 3) % 256, rng.integers(1, 5, h))
    return out


@pytest.mark.parametrize("h,w", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_unfilter_equals_the_host(h, w):
    from ccvs_amd import ops
    from ccvs_amd.tools import apng
    frames = filtered_frames(h, w, 100 * h + w)
    if (h, w) == (256, 256):
        frames = {k: frames[k] for k in ("random", "type3", "type4", "ramp_paeth")}
    raws = [f.tobytes() for f in frames.values()]
    want = apng.unfilter(raws, h, w)
    got = ops.png_decode([zlib.compress(r, 1) for r in raws], h, w)
    assert got.shape == want.shape and got.dtype == torch.uint8
    for i, name in enumerate(frames):
        assert np.array_equal(got[i].cpu().numpy(), want[i]), name


def test_bad_filter_type_on_its_frame_only():
    from ccvs_amd import ops
    from ccvs_amd.tools import apng
    h, w = 65, 67
    frames = list(filtered_frames(h, w, 9).values())[:5]
    bad = frames[2].copy()
    bad[64, 0] = 5                                                      # the second pass of the frame: its one row
    raws = [f.tobytes() for f in frames[:2]] + [bad.tobytes()] + [f.tobytes() for f in frames[3:]]
    streams = [zlib.compress(r, 6) for r in raws]
    out = torch.full((5, h, w, 3), FILL, dtype=torch.uint8, device="cuda")
    got, status = ops.png_decode(streams, h, w, out=out, check=False)
    assert status.tolist() == [0, 0, D.BAD_FILTER, 0, 0]
    want = apng.unfilter([r for i, r in enumerate(raws) if i != 2], h, w)
    assert np.array_equal(got[[0, 1, 3, 4]].cpu().numpy(), want)
    with pytest.raises(ValueError, match=r"png_decode: frame 2 failed with status 11 \(BAD_FILTER: .*\); 1 of 5 failed"):
        ops.png_decode(streams, h, w)
    # a stream that does not inflate: its status word, the other frames whole
    streams[4] = streams[4][:-9]
    got, status = ops.png_decode(streams, h, w, check=False)
    cut = D.inflate(streams[4], h * (3 * w + 1))[0]
    assert cut != D.OK and status.tolist() == [0, 0, D.BAD_FILTER, 0, cut] and np.array_equal(got[[0, 1, 3]].cpu().numpy(), want[:3])


def test_five_frames_equal_their_single_launches_and_a_frame_stride():
    from ccvs_amd import ops
    from ccvs_amd.tools import apng
    h, w = 129, 33
    raws = [f.tobytes() for f in list(filtered_frames(h, w, 4).values())[:5]]
    streams = [zlib.compress(r, 9 if i % 2 else 0) for i, r in enumerate(raws)]
    want = apng.unfilter(raws, h, w)
    for i in (0, 3):
        assert np.array_equal(ops.png_decode(streams[i:i + 1], h, w).cpu().numpy(), want[i:i + 1])
    for lim in (0, 1):                                                  # 1: at most 8 workgroups
        runs = [budgeted(lim, lambda: ops.png_decode(streams * 4, h, w, check=False)) for _ in range(2)]
        assert not runs[0][1].any() and torch.equal(runs[0][0], runs[1][0])
        assert np.array_equal(runs[0][0].cpu().numpy(), np.concatenate([want] * 4)), lim
    per = h * w * 3
    stride = per + 61
    buf = torch.full((5 * stride,), FILL, dtype=torch.uint8, device="cuda")
    view = buf.view(5, stride)[:, :per].view(5, h, w, 3)
    assert view.stride(0) == stride
    got = ops.png_decode(streams, h, w, out=view)
    assert got is view and np.array_equal(view.cpu().numpy(), want)
    assert (buf.view(5, stride)[:, per:] == FILL).all()


# ------------------------------------------------------------------ 4
def test_files(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from ccvs_amd import ops
    from ccvs_amd.helpers.generator import save_video_batch
    from ccvs_amd.tools import apng
    vid = torch.rand(3, 4, 3, 24, 40, generator=torch.Generator().manual_seed(5)) * 2.4 - 1.2
    u8 = save_video_batch(vid.cuda(), 3, 0, str(tmp_path / "own"), 4, True, False, [-1, 1], "kinetics600", video_format="apng")
    own = [str(tmp_path / "own" / f"vid_{i:05d}.png") for i in range(3)]
    got = ops.read_apng_clips(own)
    assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), u8)
    os.makedirs(tmp_path / "pil")
    pil, pil_anim = [], []
    for i in range(3):
        pil_anim.append(str(tmp_path / "pil" / f"anim_{i}.png"))
        ims = [Image.fromarray(f) for f in u8[i].numpy()]
        ims[0].save(pil_anim[-1], save_all=True, append_images=ims[1:], default_image=False, disposal=0, blend=0)
        pil.append(str(tmp_path / "pil" / f"one_{i}.png"))
        ims[i].save(pil[-1])
    got = ops.read_apng_clips(pil)
    assert torch.equal(got.cpu(), torch.stack([u8[i, i:i + 1] for i in range(3)]))
    want = np.stack([apng.read_apng(p) for p in pil_anim])             # (noise frames: Pillow finds no smaller box to write, every frame is whole)
    assert np.array_equal(want, u8.numpy()) and np.array_equal(ops.read_apng_clips(pil_anim).cpu().numpy(), want)
    with pytest.raises(ValueError, match="read_apng_clips: .* holds 1 frames of 24 x 40"):
        ops.read_apng_clips([own[0], pil[0]])
    # the encoder's streams of a 256 x 256 clip, back
    clip = torch.from_numpy(np.stack([R.images()["smooth_256x256"], R.images()["smooth_256x256"][::-1], R.images()["smooth_256x256"][:, ::-1],
                                      np.random.default_rng(1).integers(0, 256, (256, 256, 3), dtype=np.uint8)]).copy()).cuda()
    stream, off = ops.png_encode_to_host(clip)
    back = ops.png_decode([stream[off[i]:off[i + 1]] for i in range(4)], 256, 256)
    assert torch.equal(back, clip)


# ------------------------------------------------------------------ 5
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """results/0001_pd/{real,fake}: 16 apng clips each, and the clips."""
    from ccvs_amd.helpers.generator import save_video_batch
    top = tmp_path_factory.mktemp("pd_tree")
    g = torch.Generator().manual_seed(3)
    real = torch.rand(16, 9, 3, 32, 32, generator=g) * 2 - 1
    fake = (real * 0.8 + 0.1 * torch.randn(real.shape, generator=g)).clamp(-1, 1)
    clips = {}
    for kind, vid in (("real", real), ("fake", fake)):
        d = top / "results" / "0001_pd" / kind
        os.makedirs(d)
        clips[kind] = save_video_batch(vid.cuda(), 16, 0, str(d), 4, True, False, [-1, 1], "kinetics600", video_format="apng")
    return top, clips


def test_commands_print_the_same_lines(tree, monkeypatch, capsys):
    from ccvs_amd import ops
    from ccvs_amd.tools.pytorch_metrics import metrics as M
    from ccvs_amd.tools.tf_fvd import fvd
    top, clips = tree
    monkeypatch.chdir(top)
    calls = []
    real_clips = ops.read_apng_clips
    monkeypatch.setattr(ops, "read_apng_clips", lambda paths: calls.append(len(paths)) or real_clips(paths))
    for kind in ("real", "fake"):
        files = M.get_video_files(os.path.join("results", "0001_pd", kind))
        assert len(files) == 16 and files[0].endswith(".png")
        got = {mode: fvd.load_videos(files, None, 1, png_decode=mode) for mode in ("host", "gpu")}
        assert got["gpu"].is_cuda and torch.equal(got["gpu"], got["host"]) and torch.equal(got["gpu"].cpu(), clips[kind])
    assert calls == [16, 16]
    lines = {}
    for mode in ("host", "gpu"):
        capsys.readouterr()
        M.main(M.parse_args(["--exp_tag", "pd", "--png_decode", mode]))
        lines[mode] = capsys.readouterr().out
    assert "Mean/std of PSNR across 1 runs" in lines["gpu"] and lines["gpu"] == lines["host"] and calls == [16] * 4
    # the fvd command: the loader and the printing are under test, so a fixed projection of the clips stands in for the I3D network
    proj = torch.randn(9 * 32 * 32 * 3, 400, generator=torch.Generator().manual_seed(1), dtype=torch.float64)

    def embed(total, real_batch, fake_batch, channel_order):
        e = lambda b: (b.reshape(len(b), -1).cpu().double() / 255 @ proj).numpy()
        return e(real_batch(slice(0, 16))), e(fake_batch(slice(0, 16)))
    monkeypatch.setattr(fvd, "_embed_batches", embed)
    for mode in ("host", "gpu"):
        capsys.readouterr()
        fvd.main(fvd.parse_args(["--exp_tag", "pd", "--mode", "full", "--png_decode", mode]))
        lines[mode] = capsys.readouterr().out
    assert "FVD score: " in lines["gpu"] and lines["gpu"] == lines["host"] and calls == [16] * 6


# ------------------------------------------------------------------ 6
def write_folders(root, shape=(40, 56), frames=4, videos=("a_png", "b_npy", "c_palette", "d_png")):
    from PIL import Image
    rng = np.random.RandomState(11)
    for v in videos:
        d = os.path.join(root, "original_frames_256", "test", v)
        os.makedirs(d)
        vid = rng.randint(0, 256, size=(frames, *shape, 3)).astype(np.uint8)
        vid[:, 5:20, 3:30] = vid[:, 5:6, 3:4]                             # a flat patch: matches for Pillow's deflate
        for k in range(frames):
            if v.endswith("npy"):
                np.save(os.path.join(d, f"{k:02d}.npy"), vid[k])
            elif v.endswith("palette"):
                Image.fromarray(vid[k]).quantize(16).save(os.path.join(d, f"{k:02d}.png"))
            else:
                Image.fromarray(vid[k]).save(os.path.join(d, f"{k:02d}.png"))


def batches(root, extra):
    from ccvs_amd.tools.options import Options
    from ccvs_amd.helpers.generator import Generator
    import random
    opt = Options().parse(load_qvid_generator=True, load_transformer=True, argv=TINY_ARGV + ["--dataroot", root] + extra)
    gen = Generator(opt)
    info = gen.get_data_info("valid", "vid")
    random.seed(5)
    return [gen.next_batch(info)["vid"] for _ in range(len(info["dataloader"]))]


def test_frame_folders_equal_the_host_path(tmp_path, monkeypatch):
    pytest.importorskip("PIL")
    from ccvs_amd import ops
    write_folders(str(tmp_path))
    calls = []
    real_decode = ops.png_decode_uploaded
    monkeypatch.setattr(ops, "png_decode_uploaded", lambda up, *a, **k: calls.append(up["n"]) or real_decode(up, *a, **k))
    for extra in (["--num_workers", "0", "--true_dim", "32"], ["--num_workers", "2", "--resize_center_crop_img", "36", "--true_dim", "36"]):
        del calls[:]
        host = batches(str(tmp_path), extra + ["--png_decode", "host"])
        assert not calls
        gpu = batches(str(tmp_path), extra + ["--png_decode", "gpu"])
        assert calls == [4, 4]                                          # per batch of two videos: the 4 frames of its one all-RGB PNG video
        assert len(host) == len(gpu) == 2
        for a, b in zip(host, gpu):
            assert a.shape[:3] == (2, 4, 3) and a.dtype == torch.float32 and torch.equal(a, b), extra


def test_a_broken_frame_is_named(tmp_path):
    pytest.importorskip("PIL")
    write_folders(str(tmp_path), videos=("a_png", "b_png"))
    path = os.path.join(str(tmp_path), "original_frames_256", "test", "b_png", "02.png")
    from ccvs_amd.tools import apng
    cs = apng.chunks(open(path, "rb").read())
    at = next(i for i, (tag, _) in enumerate(cs) if tag == b"IDAT")
    payload = bytearray(cs[at][1])
    payload[40] ^= 0x10                                                 # inside the zlib stream; the chunk's CRC is made right again
    cs[at] = (b"IDAT", bytes(payload))
    open(path, "wb").write(apng.SIGNATURE + b"".join(apng._chunk(tag, body) for tag, body in cs))
    with pytest.raises(ValueError, match=r"b_png.02\.png: the PNG decoder failed with status \d+ \([A-Z_]+: .*\); 1 of 8 frames of the batch failed"):
        batches(str(tmp_path), ["--num_workers", "0", "--true_dim", "32", "--png_decode", "gpu"])


def test_run_writes_the_same_real_files(tmp_path):
    pytest.importorskip("PIL")
    from ccvs_amd.tools.options import Options
    from ccvs_amd.helpers.generator import Generator
    root = tmp_path / "data"
    write_folders(str(root), shape=(32, 32), videos=("a_png", "b_npy", "c_palette", "d_png", "e_png", "f_png"))
    files = {}
    for mode in ("host", "gpu"):
        opt = Options().parse(load_qvid_generator=True, load_transformer=True,
                              argv=TINY_ARGV + ["--true_dim", "32", "--n_iter", "3", "--dataroot", str(root), "--save_path", str(tmp_path / mode), "--num_workers", "2",
                                                "--video_format", "npy", "--png_decode", mode])
        torch.manual_seed(0)
        Generator(opt).run()
        real = os.path.join(opt["transformer"].result_path, "real")
        files[mode] = {n: open(os.path.join(real, n), "rb").read() for n in sorted(os.listdir(real))}
    assert len(files["gpu"]) == 6 and files["gpu"] == files["host"]
