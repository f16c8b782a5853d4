"""The transform geometry the reference's datasets share (data/base_dataset.py:74-75, 120-165, 341-357), validation phase: the crop
parameters, torchvision 0.8.1's size rules and the folding of the chain Resize / Resize + CenterCrop / Resize / crop / Resize(dim) into
stages (box, size).  `FrameDataset` runs the stages with Pillow's resampler (`ops.ingest_u8`), `VideoDataset` with torch's bilinear
interpolation in fp32 (`ops.ingest_f32`): the geometry is the same, the pixel arithmetic is not."""
import random

import numpy as np

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def resize_target(h, w, size):
    """Output (h, w) of torchvision 0.8.1's `Resize(size)` on an h x w frame: an int or a one-element list sizes the smaller edge, the
    other edge is int(size * long / short), a frame whose smaller edge already has that size is returned untouched; a two-element
    list is exactly (h, w)."""
    if isinstance(size, (list, tuple)) and len(size) == 1:
        size = size[0]
    if isinstance(size, (list, tuple)):
        assert len(size) == 2, size
        return int(size[0]), int(size[1])
    size = int(size)
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


class _Chain:
    """Folds the reference's chain into stages (box, size): a crop that follows a resize waits for the next resize and becomes its
    box; steps that change nothing are dropped."""

    def __init__(self, h, w):
        self.h, self.w, self.box, self.stages = h, w, None, []

    def resize(self, size):
        th, tw = resize_target(self.h, self.w, size)
        if (th, tw) != (self.h, self.w):
            self.stages.append((self.box, (th, tw)))
            self.box, self.h, self.w = None, th, tw

    def crop(self, top, left, h, w, what):
        if not (0 <= top and 0 <= left and h > 0 and w > 0 and top + h <= self.h and left + w <= self.w):
            raise ValueError(f"{what}: the crop (top {top}, left {left}, {h} x {w}) leaves the {self.h} x {self.w} image -- PIL would pad "
                             f"it with black; --true_dim / --true_ratio do not describe these frames")
        if (top, left, h, w) == (0, 0, self.h, self.w):
            return
        base = self.box or (0, 0, self.h, self.w)
        self.box, self.h, self.w = (base[0] + top, base[1] + left, h, w), h, w

    def done(self):
        if self.box is not None:
            self.stages.append((self.box, (self.h, self.w)))
            self.box = None
        return self.stages


class ChainGeometry:
    """What a dataset with `self.opt` needs to plan the chain: `init_geometry()` once, then `crop_offsets`, `augmentation`, `plan`."""

    def init_geometry(self):
        opt = self.opt
        dims = [2 ** k for k in range(2, int(np.log2(opt.max_dim)) + 1)]  # base_dataset.py:74-75
        self.dim = dims[int(np.log2(opt.dim)) - 2]
        self.out_size = (self.dim, int(self.dim * opt.aspect_ratio))    # the clip the reference allocates (:265)
        self.norm = (IMAGENET_MEAN, IMAGENET_STD) if getattr(opt, "imagenet_norm", False) else ((0.5,) * 3, (0.5,) * 3)

    # ---- geometry
    def crop_offsets(self):
        """The draws of `get_augmentation_parameters` in validation (:141): two `random.random()` for `fixed_crop` without
        `centered_crop`, none otherwise."""
        o = self.opt
        if not o.fixed_top_centered_zoom and o.fixed_crop and not o.centered_crop:
            return random.random(), random.random()
        return 0.5, 0.5

    def augmentation(self, offsets=(0.5, 0.5)):
        """(top, left, h_crop, w_crop, scale) of `get_augmentation_parameters` in validation (:120-165)."""
        o = self.opt
        h, w = int(o.true_dim), int(o.true_dim * o.true_ratio)
        if o.fixed_top_centered_zoom:
            h_crop = int(h / o.fixed_top_centered_zoom)
            w_crop = int(h_crop * o.aspect_ratio)
            assert w >= w_crop, (w, w_crop)
            return 0, int((w - w_crop) / 2), h_crop, w_crop, None
        if o.fixed_crop:
            h_crop, w_crop = o.fixed_crop[0], o.fixed_crop[1]
            h_scaled, w_scaled = int(h * 1.), int(w * 1.)
            assert h_scaled - h_crop >= 0 and w_scaled - w_crop >= 0, (h_scaled, w_scaled, o.fixed_crop)
            return int(offsets[0] * (h_scaled - h_crop)), int(offsets[1] * (w_scaled - w_crop)), h_crop, w_crop, (h_scaled, w_scaled)
        zoom = max(1., o.aspect_ratio / o.true_ratio)
        h_crop = int(h / zoom)
        w_crop = int(h_crop * o.aspect_ratio)
        assert h >= h_crop and w >= w_crop, (h, w, h_crop, w_crop)
        return 0, 0, h_crop, w_crop, None

    def plan(self, src_h, src_w, offsets=(0.5, 0.5)):
        """The stages [(box, size), ...] the reference's chain (`get_transform`, :348-357) amounts to for a src_h x src_w frame: each
        is a crop to `box` = (top, left, h, w) (None: the whole image) followed by a bilinear resize to `size` = (h, w).  [] when the
        frame already is the clip's frame.  Raises when a crop leaves the image or the result is not the clip's frame size."""
        o = self.opt
        top, left, h_crop, w_crop, scale = self.augmentation(offsets)
        c = _Chain(int(src_h), int(src_w))
        if o.resize_img is not None:
            c.resize(list(o.resize_img))
        if o.resize_center_crop_img is not None:
            s = int(o.resize_center_crop_img)
            c.resize(s)
            c.crop(int(round((c.h - s) / 2.)), int(round((c.w - s) / 2.)), s, s, "--resize_center_crop_img")
        if scale is not None:
            c.resize(list(scale))
        c.crop(top, left, h_crop, w_crop, "the crop of --true_dim / --fixed_crop / --fixed_top_centered_zoom")
        c.resize(self.dim)
        if (c.h, c.w) != self.out_size:
            raise ValueError(f"the transform chain turns a {src_h} x {src_w} frame into {c.h} x {c.w}, not the clip's {self.out_size[0]} x "
                             f"{self.out_size[1]} (--dim {self.dim}, --aspect_ratio {o.aspect_ratio})")
        return c.done()
