"""The mirror of `ccvs_ingest_f32` (include/ccvs_hip_video.h) in numpy float32: every line is ONE fp32 operation,
so nothing can contract into a fused multiply-add.  tests/test_video_dataset_host.py holds it against the literal torch chain of the
reference (`x.float() / 255 -> permute -> F.interpolate(bilinear, align_corners=False) per Resize -> crop -> sub / div`),
tests/test_video_ingest_gpu.py holds the kernel against it bit for bit."""
import numpy as np

F = np.float32
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
HALF = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))


def axis_taps(n_in, n_out):
    """(i0, i1, l0, l1) of every output index of an axis: torch's area_pixel_compute_source_index, align_corners=False."""
    scale = F(n_in) / F(n_out)
    dst = np.arange(n_out, dtype=F)
    s = dst + F(0.5)
    s = scale * s
    s = s - F(0.5)
    s = np.maximum(s, F(0))
    i0 = s.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = s - i0.astype(F)
    l0 = F(1) - l1
    assert s.dtype == l0.dtype == l1.dtype == F and int(i1.max()) <= n_in - 1
    return i0, i1, l0, l1


def stage(x, box, size):
    """One stage on fp32 planes x [..., H, W]: crop to `box` (top, left, h, w; None: all), bilinear resize to `size` (None: the box's)."""
    assert x.dtype == F
    if box is not None:
        top, left, h, w = box
        assert 0 <= top and 0 <= left and top + h <= x.shape[-2] and left + w <= x.shape[-1]
        x = x[..., top:top + h, left:left + w]
    ho, wo = x.shape[-2:] if size is None else size
    y0, y1, ly0, ly1 = axis_taps(x.shape[-2], ho)
    x0, x1, lx0, lx1 = axis_taps(x.shape[-1], wo)
    ly0, ly1 = ly0[:, None], ly1[:, None]
    a, b = x[..., y0, :][..., :, x0], x[..., y0, :][..., :, x1]
    c, d = x[..., y1, :][..., :, x0], x[..., y1, :][..., :, x1]
    ta = lx0 * a
    tb = lx1 * b
    r0 = ta + tb
    tc = lx0 * c
    td = lx1 * d
    r1 = tc + td
    u0 = ly0 * r0
    u1 = ly1 * r1
    out = u0 + u1
    assert out.dtype == F
    return out


def pre_op(src, pre):
    """uint8 [N, H, W, 3] or fp32 [N, C, H, W] -> fp32 planes [N, C, H, W] after the pre-op."""
    x = np.ascontiguousarray(src.transpose(0, 3, 1, 2)).astype(F) if src.dtype == np.uint8 else src.astype(F, copy=False)
    if pre == "div255":
        x = x / F(255)
    elif pre == "x2m1":
        x = x * F(2)
        x = x - F(1)
    else:
        assert pre is None, pre
    return x


def chain(src, stages, pre="div255", mean=None, std=None):
    """The whole op: pre-op, the stages through fp32 values, the post-op."""
    x = pre_op(src, pre)
    for box, size in stages:
        x = stage(x, box, size)
    if mean is not None:
        x = x - np.asarray(mean, dtype=F)[:, None, None]
        x = x / np.asarray(std, dtype=F)[:, None, None]
    assert x.dtype == F
    return np.ascontiguousarray(x)


# ------------------------------------------------------------------ the rows both test files walk
# (name, source kind, (N, C, Hs, Ws), stages, pre); kind "u8": uint8 [N, Hs, Ws, 3], "f32": fp32 [N, C, Hs, Ws]
ROWS = [
    ("5x7_to_8x8", "u8", (3, 3, 5, 7), [(None, (8, 8))], "div255"),
    ("24x32_rcc16_dim8", "u8", (2, 3, 24, 32), [(None, (16, 21)), ((0, 2, 16, 16), (8, 8))], "div255"),          # Resize(16) -> CenterCrop(16) -> Resize(8)
    ("8x8_up32_down8", "u8", (5, 3, 8, 8), [(None, (32, 32)), (None, (8, 8))], "div255"),                           # the Kinetics pattern
    ("30x40_rcc32", "u8", (2, 3, 30, 40), [(None, (32, 42)), ((0, 5, 32, 32), None)], "div255"),                    # UCF: a crop after a resize
    ("identity_rows", "u8", (1, 3, 9, 12), [(None, (9, 20))], "div255"),                                            # an identity axis
    ("identity_both", "u8", (2, 3, 9, 12), [((1, 2, 7, 8), None)], "div255"),                                       # a crop alone
    ("one_pixel_source_axis", "u8", (2, 3, 1, 6), [(None, (4, 9))], "div255"),
    ("one_pixel_output", "u8", (2, 3, 7, 5), [(None, (1, 1))], "div255"),
    ("stft_20x6", "f32", (4, 1, 20, 6), [(None, (64, 16))], "x2m1"),
    ("f32_c3_boxes", "f32", (2, 3, 13, 17), [((0, 0, 13, 9), (11, 14)), ((2, 3, 9, 11), (10, 10))], None),          # boxes at the top / left edge
    ("box_bottom_right", "u8", (2, 3, 14, 18), [((5, 7, 9, 11), (12, 13))], "div255"),                              # ... at the bottom / right edge
    ("wide_row", "u8", (1, 3, 3, 300), [(None, (2, 517))], "div255"),                                               # past one block's width, Wo % 4 == 1
    ("three_stages", "u8", (2, 3, 12, 16), [(None, (20, 26)), ((1, 1, 18, 24), (9, 12)), ((0, 2, 9, 8), (16, 16))], "div255"),
]


def row_source(row):
    name, kind, (n, c, h, w), _, _ = row
    rng = np.random.RandomState(sum(name.encode()) + 1000 * h + w)
    if kind == "u8":
        return rng.randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)
    return rng.rand(n, c, h, w).astype(F)


def torch_chain(src, stages, pre="div255", mean=None, std=None):
    """The reference's own arithmetic with torch on the CPU: what the mirror is held against."""
    import torch
    import torch.nn.functional as TF
    x = torch.from_numpy(src)
    if src.dtype == np.uint8:
        x = (x.float() / 255).permute(0, 3, 1, 2) if pre == "div255" else x.float().permute(0, 3, 1, 2)
    elif pre == "x2m1":
        x = x * 2 - 1
    for box, size in stages:
        if box is not None:
            x = x[..., box[0]:box[0] + box[2], box[1]:box[1] + box[3]]
        if size is not None and tuple(size) != tuple(x.shape[-2:]):
            x = TF.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False)
    if mean is not None:
        x = x.clone().sub_(torch.tensor(mean, dtype=torch.float32)[:, None, None]).div_(torch.tensor(std, dtype=torch.float32)[:, None, None])
    return x.contiguous()


# ------------------------------------------------------------------ tiny dataset trees (host and gpu tests)
# the tiny configuration of tests/test_e2e_gpu.py, per video dataset
def tiny_argv(dataset):
    return ["--name", "tiny", "--dataset", dataset, "--max_dim", "32", "--vid_len", "4", "--q_z_num", "32", "--q_z_size", "16",
            "--q_z_shape", "8", "8", "--q_use_enc", "--q_use_dec", "--q_necf", "8", "--q_necf_mult", "1", "2", "2",
            "--q_enc_model", "skipgan", "--q_dec_model", "skipgan", "--q_use_inter", "--q_inter_p", "0.75",
            "--q_skip_context", "1", "2", "3", "--q_skip_memory", "3", "--x_z_num", "32", "--x_z_len", "256", "--x_n_layer", "2",
            "--x_n_head", "2", "--x_n_embd", "32", "--x_z_chunk", "64", "--x_cond_len", "64", "--x_emb_mode", "temporal",
            "--x_num_blocks", "4", "--batch_size_vid", "2"]


VIDEO_FOLDERS = {"ucf101": "videos", "drums": "AudioSet_Dataset/test/mp4", "kinetics600": "clips"}


def write_video_tree(root, dataset, clips, fps=4):
    """`clips`: {name relative to the dataset's video folder: (list of JPEG files, h, w)} written with `write_avi`; for kinetics600 also
    the serialised lists the reference reads (valid_data.pkl: vid_paths in REVERSED name order, labels 0, 1, ...).  Returns the paths."""
    import os
    import pickle
    from ccvs_amd.tools import mjpeg
    paths = {}
    for name, (frames, h, w) in clips.items():
        path = os.path.join(root, VIDEO_FOLDERS[dataset], name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        mjpeg.write_avi(path, frames, fps, h, w)
        paths[name] = path
    if dataset == "kinetics600":
        order = sorted(paths, reverse=True)
        with open(os.path.join(root, "valid_data.pkl"), "wb") as fh:
            pickle.dump({"vid_paths": [os.path.join(VIDEO_FOLDERS[dataset], n) for n in order], "vid_labels": list(range(len(order)))}, fh)
    return paths
