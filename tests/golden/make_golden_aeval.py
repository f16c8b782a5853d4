"""Generate tests/golden/tiny_aeval.npz: the reference's own frame autoencoder validation -- `QVidModel.forward(mode=
'eval_img_to_img_generator')` (quantized_video_model.py:53-55, 460-480) and its quantiser's loss and perplexity (quantize.py:59-68) --
on the CPU through `ref_harness`.

    CCVS_REFERENCE_ROOT=<reference checkout> python tests/golden/make_golden_aeval.py

Two launch lines (`aeval_ref.LINES`): TINY_ARGV and TINY_ARGV + ["--q_normalize_out"], both with the `e` / `q` / `g` weights of
tiny_e2e.npz; a line whose codebook differs stores its own under `<line>/w/q/`.  The input is `aeval_ref.frames(seed)`: 8 frames of flat
8 x 8 patches under a little noise, under the first seed from `aeval_ref.CLIP_SEED` on at which both lines meet the conditions below
(recorded as `clip`).  Per line the fixture holds the reference's eval value, `net_q(z)`'s loss, perplexity and
indices, the encoder's z and the decoded frames, max|z_q - z|, the smallest top-2 gap in squared distance, and the loss and
perplexity evaluated in float64 from the reference's z and indices.  The fixture is DATA; no reference source travels.

The maker asserts `aeval_ref.conditions` per line (well separated codes, at least 4 of them, a perplexity and an L1 that say
something); the host test re-asserts them on the file."""
import contextlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_harness as rh  # noqa: E402
import aeval_ref as A  # noqa: E402

ARGV = {"plain": rh.TINY_ARGV, "norm": rh.TINY_ARGV + ["--q_normalize_out"]}


def build(ns, e2e, line):
    qopt = rh.parse_reference_options(ARGV[line])["qvid_generator"]
    assert bool(qopt.normalize_out) == (line == "norm")
    torch.manual_seed(0)
    with open(os.devnull, "w") as devnull, contextlib.redirect_stdout(devnull):
        qv = ns.qvm.QVidModel(qopt, is_train=False, is_main=True).eval()
    for pre, net in (("e", qv.net_e), ("q", qv.net_q), ("g", qv.net_g)):
        sd = {k[len(pre) + 1:]: torch.from_numpy(e2e[k]) for k in e2e.files if k.startswith(pre + "/")}
        missing, unexpected = net.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.endswith(".kernel") for k in missing), (line, pre, missing, unexpected)
    return qv, qopt


def run(qv, line, img):
    """The reference's eval mode on `img`, with what its three networks returned on the way."""
    seen = {}
    hooks = [qv.net_e.register_forward_hook(lambda m, a, out: seen.__setitem__("z", out[0].detach().clone())),
             qv.net_q.register_forward_hook(lambda m, a, out: seen.__setitem__("q", out)),
             qv.net_g.register_forward_hook(lambda m, a, out: seen.__setitem__("fake", out[0].detach().clone()))]
    with torch.no_grad():
        l1 = qv({"img": img.clone()}, mode="eval_img_to_img_generator")
    for h in hooks:
        h.remove()
    z = seen["z"]
    _, loss, (ppl, _, idx) = seen["q"]
    cb = qv.net_q.embedding.weight.detach()
    scale = A.row_scale64(cb.numpy()) if line == "norm" else None
    m64, counts = A.vq_stats64(z.numpy(), idx.numpy(), cb.numpy(), scale)
    rows = cb.double()[idx.view(-1)] * (1.0 if scale is None else torch.from_numpy(scale)[idx.view(-1)][:, None])
    zq64 = rows.view(z.shape[0], -1, z.shape[1]).transpose(1, 2).reshape(z.shape)
    assert abs(A.l1_mean64(img.numpy(), seen["fake"].numpy()) - float(l1)) <= 1e-6 * float(l1)
    return {"l1": l1.numpy(), "q_loss": loss.detach().numpy(), "perplexity": ppl.numpy(), "code": idx.view(-1).numpy().astype(np.int16),
            "z": z.numpy(), "fake_img": seen["fake"].numpy(), "max_dz": np.float64((zq64 - z.double()).abs().max().item()),
            "min_gap": np.float64(A.top2_gap64(z.numpy(), cb.numpy())), "q_loss64": np.float64((1.0 + A.BETA) * m64),
            "perplexity64": np.float64(A.perplexity64(counts, idx.numel()))}


def main():
    ns = rh.load_reference()
    e2e = np.load(os.path.join(HERE, "tiny_e2e.npz"))
    models = {line: build(ns, e2e, line) for line in A.LINES}
    # the clip: `aeval_ref.frames` under the first seed from CLIP_SEED on at which BOTH lines meet `aeval_ref.conditions`
    for seed in range(A.CLIP_SEED, A.CLIP_SEED + 400):
        img = A.frames(seed)
        arrays = {"lines": np.array(json.dumps({k: list(v) for k, v in ARGV.items()})), "img": img.numpy(),
                  "clip": np.array([seed, A.CLIP_SCALE], dtype=np.float64)}
        try:
            for line in A.LINES:
                arrays.update({f"{line}/{k}": v for k, v in run(models[line][0], line, img).items()})
                A.conditions(arrays, line, models[line][1].z_num)
        except AssertionError as miss:
            print(f"  seed {seed}: {miss}")
            continue
        break
    else:
        raise SystemExit("no seed meets the conditions")
    for line in A.LINES:
        o = {k[len(line) + 1:]: v for k, v in arrays.items() if k.startswith(line + "/")}
        print(f"  {line:5s} l1 {float(o['l1']):.6f}  q_loss {float(o['q_loss']):.6f} (f64 {float(o['q_loss64']):.6f})  perplexity "
              f"{float(o['perplexity']):.5f} (f64 {float(o['perplexity64']):.5f})  codes used {np.unique(o['code']).size}  "
              f"min gap {float(o['min_gap']):.2e}  max|zq - z| {float(o['max_dz']):.3f}")
    path = os.path.join(HERE, "tiny_aeval.npz")
    np.savez_compressed(path, **arrays)
    print(f"  clip seed {seed}; wrote tiny_aeval.npz", sum(a.nbytes for a in arrays.values()) / 1e3, "KB raw,", os.path.getsize(path) / 1e3, "KB on disk")


if __name__ == "__main__":
    main()
