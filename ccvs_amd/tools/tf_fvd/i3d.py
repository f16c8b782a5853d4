"""The embedding network of the Frechet Video Distance: the Kinetics-400 RGB Inception-I3D the reference loads from TF-Hub
(tools/tf_fvd/fvd.py:63-122, `RGB/inception_i3d/Mean:0`), on the GPU from a weight file the user names.  The weights are not in this
repository and are never downloaded; `load_i3d_weights` reads the file the converter at the bottom writes.

The network (a restatement; parity with the TF-Hub module itself is not pinned -- TensorFlow is not installed where the tests run --
the float64 mirror tests/fvd_ref.py of this text is what the kernels are held to):
  * every unit is Conv3d without bias, BatchNorm (eps 1e-3), ReLU; the file holds the BatchNorm folded into weight and offset;
  * every convolution and pool pads as TensorFlow's SAME does, per axis: out = ceil(n / s), total = max((out - 1) s + k - n, 0),
    before = total // 2, after = total - before (`ops.same_pad`); a max pool's padding never wins;
  * Conv3d_1a_7x7 (3 -> 64, 7^3, stride 2^3), MaxPool3d_2a_3x3 ((1,3,3) / (1,2,2)), Conv3d_2b_1x1 (64 -> 64), Conv3d_2c_3x3 (64 -> 192, 3^3),
    MaxPool3d_3a_3x3 ((1,3,3) / (1,2,2)), Mixed_3b, Mixed_3c, MaxPool3d_4a_3x3 (3^3 / 2^3), Mixed_4b .. Mixed_4f, MaxPool3d_5a_2x2
    (2^3 / 2^3), Mixed_5b, Mixed_5c (-> 1024), then the head: average pool (2,7,7) stride 1 VALID, `logits` (1^3 convolution 1024 -> 400
    with bias, no BatchNorm, no ReLU), spatial squeeze, mean over time -> [N, 400];
  * a Mixed block [o0, o1,o2, o3,o4, o5] is the concatenation of b0 = 1^3(in -> o0); b1b = 3^3(o1 -> o2) of b1a = 1^3(in -> o1);
    b2b = 3^3(o3 -> o4) of b2a = 1^3(in -> o3); b3b = 1^3(in -> o5) of a 3^3 stride-1 max pool of the input.  57 units and the logits.

On the GPU the activations live as [N T, C, H, W] fp32 -- frames are the batch -- so the 1^3 convolutions are `ops.conv2d` as it stands,
and a k_t-tap convolution is `ops.conv2d` over the k_t Cin channels of time-stacked frames (`ops.time_unfold`, weight
w.permute(0, 2, 1, 3, 4).reshape(Cout, k_t Cin, k, k): `ops.stack_conv3d_weight`); the folded BatchNorm offset is the bias.  The stem's
spatial stride 2 goes into the channels as well (the four pixel phases, a 4 x 4 stride-1 convolution over 84 channels), because a
7 x 7 window at stride 2 is more than the convolution kernels' input tile holds.  A branch's last convolution writes into
its channel slice of the block's output.  ReLU is applied by whoever reads a map (`time_unfold`, `maxpool3d_same`, `i3d_head`) or once
per block (`ops.relu_`).  A clip needs T >= 9 frames (9 -> 5 -> 5 -> 3 -> 2, one average-pool window) and sides in 193 .. 224 (7 x 7 in
front of the head).

No CPU fallback: the kernels live in libccvs_hip.so.  The converter is host code:
  python -m ccvs_amd.tools.tf_fvd.i3d --state_dict rgb_imagenet.pt --out i3d_kinetics400.pt
"""
import argparse
import os

import torch

from ccvs_amd import ops

BN_EPS = 1e-3
# the widths of the Kinetics-400 network: the three stem convolutions, each Mixed block's [o0, o1,o2, o3,o4, o5], the logits
I3D_WIDTHS = {
    "stem": (64, 64, 192),
    "mixed": {
        "Mixed_3b": (64, 96, 128, 16, 32, 32), "Mixed_3c": (128, 128, 192, 32, 96, 64),
        "Mixed_4b": (192, 96, 208, 16, 48, 64), "Mixed_4c": (160, 112, 224, 24, 64, 64), "Mixed_4d": (128, 128, 256, 24, 64, 64),
        "Mixed_4e": (112, 144, 288, 32, 64, 64), "Mixed_4f": (256, 160, 320, 32, 128, 128),
        "Mixed_5b": (256, 160, 320, 32, 128, 128), "Mixed_5c": (384, 192, 384, 48, 128, 128),
    },
    "classes": 400,
}
STEM_NAMES = ("Conv3d_1a_7x7", "Conv3d_2b_1x1", "Conv3d_2c_3x3")
STEM_KERNELS = (7, 1, 3)
MIN_FRAMES, MIN_SIDE, MAX_SIDE = 9, 193, 224


def divided_widths(div):
    """The same graph with every width divided by `div` (the number of classes kept): what the tests run the whole mirror on."""
    return {"stem": tuple(c // div for c in I3D_WIDTHS["stem"]), "mixed": {k: tuple(c // div for c in v) for k, v in I3D_WIDTHS["mixed"].items()},
            "classes": I3D_WIDTHS["classes"]}


def block_out(o):
    return o[0] + o[2] + o[4] + o[5]


def units(widths=None):
    """[(unit name, Cin, Cout, k)] of the 57 convolution units in network order, and the logits' (Cin, classes)."""
    widths = widths or I3D_WIDTHS
    out, cin = [], 3
    for name, cout, k in zip(STEM_NAMES, widths["stem"], STEM_KERNELS):
        out.append((name, cin, cout, k))
        cin = cout
    for name, o in widths["mixed"].items():
        out += [(f"{name}.b0", cin, o[0], 1), (f"{name}.b1a", cin, o[1], 1), (f"{name}.b1b", o[1], o[2], 3),
                (f"{name}.b2a", cin, o[3], 1), (f"{name}.b2b", o[3], o[4], 3), (f"{name}.b3b", cin, o[5], 1)]
        cin = block_out(o)
    return out, (cin, widths["classes"])


def _tensor(sd, key, shape, who):
    if key not in sd:
        raise ValueError(f"{who}: no {key} (expected {shape})")
    v = sd[key]
    if not isinstance(v, torch.Tensor):
        raise ValueError(f"{who}: {key} is a {type(v).__name__}, not a tensor")
    if tuple(v.shape) != tuple(shape):
        raise ValueError(f"{who}: {key} is {tuple(v.shape)}, not {tuple(shape)}")
    return v.detach().cpu()


def fold_state_dict(sd, widths=None):
    """The state dict of the PyTorch port of this network -- `<unit>.conv3d.weight` [Cout, Cin, k, k, k], `<unit>.bn.weight / .bias /
    .running_mean / .running_var` [Cout], `logits.conv3d.weight` [classes, 1024, 1, 1, 1], `logits.conv3d.bias` -- with every BatchNorm
    folded in float64: weight * g / sqrt(var + 1e-3), bias = beta - mean * g / sqrt(var + 1e-3).  Returns the dict `load_i3d_weights`
    takes.  Other entries (num_batches_tracked) are ignored; a missing or misshapen one raises ValueError naming it."""
    who = "fold_state_dict"
    convs, (cin, classes) = units(widths)
    out = {}
    for name, ci, co, k in convs:
        w = _tensor(sd, f"{name}.conv3d.weight", (co, ci, k, k, k), who).double()
        g, beta, mean, var = (_tensor(sd, f"{name}.bn.{p}", (co,), who).double() for p in ("weight", "bias", "running_mean", "running_var"))
        s = g / torch.sqrt(var + BN_EPS)
        out[f"{name}.weight"] = (w * s.view(-1, 1, 1, 1, 1)).float().contiguous()
        out[f"{name}.bias"] = (beta - mean * s).float().contiguous()
    out["logits.weight"] = _tensor(sd, "logits.conv3d.weight", (classes, cin, 1, 1, 1), who).float().reshape(classes, cin).contiguous()
    out["logits.bias"] = _tensor(sd, "logits.conv3d.bias", (classes,), who).float().contiguous()
    return out


def load_i3d_weights(path_or_dict, widths=None):
    """Read and validate I3D weights: a file written with torch.save (read with weights_only=True) or the dict itself, holding per unit
    `<unit>.weight` [Cout, Cin, k, k, k] and `<unit>.bias` [Cout] with the BatchNorm folded in, `logits.weight` [classes, 1024] and
    `logits.bias` -- what the converter writes.  Only shapes can be judged: a missing or misshapen entry raises ValueError naming it.
    Returns fp32 host tensors."""
    who = "load_i3d_weights"
    src = path_or_dict
    if not isinstance(src, dict):
        src = torch.load(os.fspath(src), map_location="cpu", weights_only=True)
    if not isinstance(src, dict):
        raise ValueError(f"{who}: the weights are a dict of tensors (write one with python -m ccvs_amd.tools.tf_fvd.i3d)")
    if any(".conv3d." in str(k) for k in src):
        raise ValueError(f"{who}: this is the port's own state dict (BatchNorm not folded); convert it with python -m ccvs_amd.tools.tf_fvd.i3d")
    convs, (cin, classes) = units(widths)
    out = {}
    for name, ci, co, k in convs:
        out[f"{name}.weight"] = _tensor(src, f"{name}.weight", (co, ci, k, k, k), who).float().contiguous()
        out[f"{name}.bias"] = _tensor(src, f"{name}.bias", (co,), who).float().contiguous()
    out["logits.weight"] = _tensor(src, "logits.weight", (classes, cin), who).float().contiguous()
    out["logits.bias"] = _tensor(src, "logits.bias", (classes,), who).float().contiguous()
    return out


class I3D:
    """The I3D embedding on the GPU from user-supplied weights (a path or dict `load_i3d_weights` takes).

    precision: None follows `ops.CONV_PRECISION` (split-bf16 by default), "f32" is the exact-fp32 convolution; the 57 convolutions are
    packed once, here.  widths: another width table (`divided_widths`), for tests.  `features(x)` takes fp32 [N, T, 3, H, W] in [-1, 1]
    and `embed(u8, channel_order)` uint8 [N, T, H, W, 3] clips (through `ops.fvd_prep`); both return float64 [N, classes] on the device,
    the time-averaged logits, and synchronise nothing.  The clips run in chunks of `chunk_clips(T, H, W)`, sized so that the largest
    maps alive at a time stay under `max_workspace_bytes`."""

    def __init__(self, weights, precision=None, widths=None, max_workspace_bytes=2 << 30):
        if precision not in (None, "f32"):
            raise ValueError(f"I3D: precision is None (ops.CONV_PRECISION) or 'f32', not {precision!r}")
        if not torch.cuda.is_available():
            raise ops._lib.CcvsError("I3D needs a GPU: the HIP path has no CPU fallback")
        self.widths = widths or I3D_WIDTHS
        w = load_i3d_weights(weights, self.widths)
        self.precision = precision
        self.max_workspace_bytes = int(max_workspace_bytes)
        self.convs = {}
        for name, cin, cout, k in units(self.widths)[0]:
            # time taps stacked into the channels, tap-major; the stride-2 stem over the four pixel phases as a stride-1 4 x 4 convolution
            w4 = ops.stack_conv3d_weight(w[f"{name}.weight"].cuda(), phases=2 if name == STEM_NAMES[0] else 1)
            self.convs[name] = (ops.pack_conv_weight(w4, precision, scale=1.0), w[f"{name}.bias"].cuda(), cout, w4.shape[-1])
        self.logits_w, self.logits_b = w["logits.weight"].cuda(), w["logits.bias"].cuda()

    # -- geometry
    @staticmethod
    def check_clip(t, h, w):
        if t < MIN_FRAMES:
            raise ValueError(f"I3D: a clip of {t} frames; the network needs at least {MIN_FRAMES} (9 -> 5 -> 5 -> 3 -> 2: one (2, 7, 7) average-pool window)")
        if not (MIN_SIDE <= h <= MAX_SIDE and MIN_SIDE <= w <= MAX_SIDE):
            raise ValueError(f"I3D: frames of {h} x {w}; both sides must be in {MIN_SIDE} .. {MAX_SIDE} (a 7 x 7 map in front of the head)")

    def chunk_clips(self, t, h, w):
        """Clips per chunk: the largest count whose biggest stage -- the stem (stacked input, output, pooled output) or Conv3d_2c_3x3
        (input, stacked input, output) -- fits max_workspace_bytes."""
        c1, c2, c3 = self.widths["stem"]
        t1 = ops.same_pad(t, 7, 2)[0]
        (h1, hb, ha), (w1, wb, wa) = ops.same_pad(h, 7, 2), ops.same_pad(w, 7, 2)
        h2, w2 = ops.same_pad(h1, 3, 2)[0], ops.same_pad(w1, 3, 2)[0]
        stem = t1 * (21 * (h + hb + ha + 1) * (w + wb + wa + 1) + c1 * h1 * w1 + c1 * h2 * w2)
        conv2c = t1 * h2 * w2 * (c2 + 3 * c2 + c3)
        return max(1, self.max_workspace_bytes // (4 * max(stem, conv2c)))

    # -- the network
    def _conv(self, x, name, stride=1, pad=0, out=None):
        packed, bias, cout, k = self.convs[name]
        return ops.conv2d(x, packed, bias, cout, k, stride=stride, pad=pad, out=out)

    def _mixed(self, x, t, name, relu_out):
        """x: the block's input behind its ReLU.  Returns the concatenated branches; relu_out=False leaves them as pre-activations for
        a reader that applies the ReLU itself."""
        o = self.widths["mixed"][name]
        nt, _, h, w = x.shape
        out = torch.empty(nt, block_out(o), h, w, dtype=torch.float32, device=x.device)
        at = 0
        self._conv(x, f"{name}.b0", out=out[:, at:at + o[0]])
        at += o[0]
        for a, b, ob in (("b1a", "b1b", o[2]), ("b2a", "b2b", o[4])):
            y = self._conv(x, f"{name}.{a}")
            self._conv(ops.time_unfold(y, t, 3, 1, relu=True), f"{name}.{b}", pad=1, out=out[:, at:at + ob])
            at += ob
        p = ops.maxpool3d_same(x, t, (3, 3, 3), (1, 1, 1))
        self._conv(p, f"{name}.b3b", out=out[:, at:at + o[5]])
        return ops.relu_(out) if relu_out else out

    def _forward(self, x, t):
        """x: [n t, 3, H, W] fp32 -> float64 [n, classes]."""
        h, w = x.shape[2:]
        # The stem.  Its asymmetric SAME border is written into the stacked input.  The convolution kernels stage at most a 1280-pixel
        # input tile per channel, which a 7 x 7 window at stride 2 exceeds (21 x 69), so the stride goes into the channels: one more
        # zero row / column where a bordered side is odd (it meets the kernel's zero eighth tap only), the four pixel phases as
        # channels, and a 4 x 4 stride-1 convolution over them -- the same products.
        (_, hb, ha), (_, wb, wa) = ops.same_pad(h, 7, 2), ops.same_pad(w, 7, 2)
        ha, wa = ha + (h + hb + ha) % 2, wa + (w + wb + wa) % 2
        y = self._conv(ops.time_unfold(x, t, 7, 2, pad=(hb, ha, wb, wa), phases=2), "Conv3d_1a_7x7")
        t = ops.same_pad(t, 7, 2)[0]
        y = ops.maxpool3d_same(y, t, (1, 3, 3), (1, 2, 2), relu=True)
        y = self._conv(y, "Conv3d_2b_1x1")
        y = self._conv(ops.time_unfold(y, t, 3, 1, relu=True), "Conv3d_2c_3x3", pad=1)
        y = ops.maxpool3d_same(y, t, (1, 3, 3), (1, 2, 2), relu=True)
        y = self._mixed(y, t, "Mixed_3b", True)
        y = self._mixed(y, t, "Mixed_3c", False)
        y = ops.maxpool3d_same(y, t, (3, 3, 3), (2, 2, 2), relu=True)
        t = ops.same_pad(t, 3, 2)[0]
        for name in ("Mixed_4b", "Mixed_4c", "Mixed_4d", "Mixed_4e"):
            y = self._mixed(y, t, name, True)
        y = self._mixed(y, t, "Mixed_4f", False)
        y = ops.maxpool3d_same(y, t, (2, 2, 2), (2, 2, 2), relu=True)
        t = ops.same_pad(t, 2, 2)[0]
        y = self._mixed(y, t, "Mixed_5b", True)
        y = self._mixed(y, t, "Mixed_5c", False)
        return ops.i3d_head(y, t, self.logits_w, self.logits_b, relu=True)

    def features(self, x):
        """x: fp32 [N, T, 3, H, W] device tensor in [-1, 1] (what `preprocess` returns) -> float64 [N, classes]."""
        ops._need_gpu(x)
        if x.dim() != 5 or x.shape[2] != 3 or x.dtype != torch.float32 or x.shape[0] == 0:
            raise ValueError(f"I3D: clips are fp32 [N, T, 3, H, W], got {tuple(x.shape)} {x.dtype}")
        n, t, _, h, w = x.shape
        self.check_clip(t, h, w)
        x = x.contiguous()
        step = self.chunk_clips(t, h, w)
        out = [self._forward(x[i:i + step].reshape(-1, 3, h, w), t) for i in range(0, n, step)]
        return out[0] if len(out) == 1 else torch.cat(out)

    def embed(self, u8_clips, channel_order="bgr"):
        """uint8 clips [N, T, H, W, 3] (numpy or torch, in the RGB order this project's readers give) -> float64 [N, classes]: the
        reference's preprocess (resize to 224 x 224, 2 v / 255 - 1) and the network.  channel_order "bgr" feeds the channels reversed, as
        the reference does (it reads frames with OpenCV and never converts them); "rgb" is the canonical order."""
        if channel_order not in ("bgr", "rgb"):
            raise ValueError(f"I3D: channel_order is 'bgr' or 'rgb', not {channel_order!r}")
        u8 = torch.as_tensor(u8_clips)
        if u8.dim() != 5 or u8.shape[-1] != 3 or u8.dtype != torch.uint8 or u8.shape[0] == 0:
            raise ValueError(f"I3D: clips are uint8 [N, T, H, W, 3], got {tuple(u8.shape)} {u8.dtype}")
        n, t = u8.shape[:2]
        self.check_clip(t, 224, 224)
        step = self.chunk_clips(t, 224, 224)
        out = []
        for i in range(0, n, step):
            x = ops.fvd_prep(u8[i:i + step].cuda(), (224, 224), flip=channel_order == "bgr")
            out.append(self._forward(x.view(-1, 3, 224, 224), t))
        return out[0] if len(out) == 1 else torch.cat(out)


def convert(state_dict_path, out_path, widths=None):
    """The one file `load_i3d_weights` reads, from the state dict of the PyTorch port of the Kinetics-400 RGB I3D (rgb_imagenet.pt of the
    pytorch-i3d repository): every BatchNorm folded in float64, every shape validated.  Host only."""
    sd = torch.load(state_dict_path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError("convert: the file does not hold a state dict")
    w = load_i3d_weights(fold_state_dict(sd, widths), widths)
    torch.save(w, out_path)
    return w


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="write the I3D weight file the FVD command reads (--fvd_weights)")
    parser.add_argument("--state_dict", type=str, required=True, help="the PyTorch port's state dict (rgb_imagenet.pt)")
    parser.add_argument("--out", type=str, required=True)
    return parser.parse_args(argv)


if __name__ == "__main__":
    _args = parse_args()
    convert(_args.state_dict, _args.out)
    print(f"wrote {_args.out}")
