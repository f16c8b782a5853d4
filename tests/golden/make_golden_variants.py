"""Golden fixtures of the flow-decoder variants of Matching (--q_use_masked_flow, --q_use_deformed_conv, --q_use_tradeoff,
--q_no_corr and all four together) from the imported reference:

    CCVS_REFERENCE_ROOT=<reference checkout> python tests/golden/make_golden_variants.py

Runs the reference's own SkipGANDecoder (Matching / Subpixel / InterBlock, the toff threading, the offset layout as the
reference writes it) on CPU through `ref_harness`, with `deform_ref.DeformConv2d` standing in for torchvision.ops.DeformConv2d.
Writes tests/golden/tiny_variants.json (per config: launch line, seeded weight spec, the reference's state_dict keys and
shapes) and tests/golden/tiny_variants.npz (per config: the decoded frames, flows and occlusions of every level).  The
decoder input and the context features are drawn from seeded generators named in the JSON (`variant_inputs`).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import ref_harness as rh  # noqa: E402
import deform_ref  # noqa: E402

# feat_size a multiple of 32 at every level (the trade-off up-sampling is grouped by 32): inter sizes 64, 64, 32
VARIANT_ARGV = [
    "--name", "tiny_variants", "--dataset", "bairhd", "--max_dim", "32", "--vid_len", "4",
    "--q_z_num", "32", "--q_z_size", "16", "--q_z_shape", "8", "8",
    "--q_use_enc", "--q_use_dec", "--q_necf", "64", "--q_necf_mult", "1", "2", "2",
    "--q_enc_model", "skipgan", "--q_dec_model", "skipgan", "--q_use_inter", "--q_inter_p", "0.5",
    "--q_skip_context", "1", "2", "--q_skip_memory", "2",
    "--x_z_num", "32", "--x_z_len", "256", "--x_n_layer", "2", "--x_n_head", "2", "--x_n_embd", "32",
    "--x_z_chunk", "64", "--x_cond_len", "64", "--x_emb_mode", "temporal", "--x_num_blocks", "4",
    "--batch_size_vid", "2",
]
CONFIGS = {
    "masked": ["--q_use_masked_flow"],
    "deform": ["--q_use_deformed_conv"],
    "tradeoff": ["--q_use_tradeoff"],
    "nocorr": ["--q_no_corr"],
    "all": ["--q_use_masked_flow", "--q_use_deformed_conv", "--q_use_tradeoff", "--q_no_corr"],
}
WEIGHT_SEED = 1000
# decoder input z [1, 2 frames, 16, 8, 8] and k = 2 contexts, per level fine -> coarse (32, 64, 64 channels)
INPUTS = {"z": [[1, 2, 16, 8, 8], 11], "ctx": [[[1, 2, 32, 32, 32], [1, 2, 64, 16, 16], [1, 2, 64, 8, 8]], 21], "k": 2}


def variant_inputs(spec):
    g = torch.Generator().manual_seed(spec["z"][1])
    z = torch.randn(spec["z"][0], generator=g)
    ctx = []
    for j in range(spec["k"]):
        g = torch.Generator().manual_seed(spec["ctx"][1] + j)
        ctx.append([torch.randn(s, generator=g) for s in spec["ctx"][0]])
    return z, ctx


def variant_weight_spec(dec):
    """The decoder's own initialisers, with non-zero biases: the flow heads get large ones, so that every level's flow has
    x and y components that differ clearly (an offset read with the axes swapped fails)."""
    spec = rh.weight_spec(dec)
    for e in spec:
        name = e[0]
        if name.endswith("flow_head.0.bias"):
            e[3] = 1.0 if ".matching." in name else 0.3
        elif name.endswith("bias") and e[3] == 0.0:
            e[3] = 0.05
    return spec


def main():
    ns = rh.load_reference()
    sys.modules["torchvision.ops"].DeformConv2d = deform_ref.DeformConv2d
    meta = {"argv": VARIANT_ARGV, "configs": {}, "variant_inputs": INPUTS, "weight_seed": WEIGHT_SEED}
    arrays = {}
    z, ctx = variant_inputs(INPUTS)
    for name, flags in CONFIGS.items():
        opt = rh.parse_reference_options(VARIANT_ARGV + flags)
        qopt = opt["qvid_generator"]
        torch.manual_seed(0)
        dec = ns.sae.SkipGANDecoder(qopt).eval()
        spec = variant_weight_spec(dec)
        missing, unexpected = dec.load_state_dict(rh.seeded_weights(spec, WEIGHT_SEED), strict=False)
        assert not unexpected and all(k.endswith(".kernel") for k in missing)
        with torch.no_grad():
            rgb, _, flows, occs, _ = dec(z, [[t.clone() for t in c] for c in ctx], return_all=True)
        arrays[f"{name}/rgb"] = rgb.numpy()
        for i, (f, o) in enumerate(zip(flows, occs)):
            arrays[f"{name}/flow{i}"] = f.numpy()
            arrays[f"{name}/occ{i}"] = o.numpy()
        sd = [[k, list(v.shape)] for k, v in dec.state_dict().items() if not k.endswith(".kernel")]
        meta["configs"][name] = {"flags": flags, "weight_spec": spec, "state_dict": sd}
        fl = flows[-1]
        print(f"  {name:9s} rgb |max| {rgb.abs().max().item():.3f}  last flow x {fl[:, 0].mean().item():+.3f} y {fl[:, 1].mean().item():+.3f}"
              f"  occ {occs[-1].mean().item():+.3f}")
        if "--q_use_deformed_conv" in flags:   # the axis order matters: the same run with (dx, dy) read as (x, y) is far off
            orig = deform_ref.deform_conv2d

            def swapped(x, offset, *a, **k):
                b, t2, h, w = offset.shape
                return orig(x, offset.view(b, t2 // 2, 2, h, w).flip(2).reshape(b, t2, h, w), *a, **k)
            deform_ref.deform_conv2d = swapped
            try:
                with torch.no_grad():
                    rgb_s = dec(z, [[t.clone() for t in c] for c in ctx], return_all=True)[0]
            finally:
                deform_ref.deform_conv2d = orig
            print(f"            un-swapped offsets: max|rgb diff| {(rgb_s - rgb).abs().max().item():.3e}")
    np.savez_compressed(os.path.join(HERE, "tiny_variants.npz"), **arrays)
    with open(os.path.join(HERE, "tiny_variants.json"), "w") as f:
        json.dump(meta, f)
    print("  wrote tiny_variants.npz / .json", sum(a.nbytes for a in arrays.values()) / 1e6, "MB raw")


if __name__ == "__main__":
    main()
