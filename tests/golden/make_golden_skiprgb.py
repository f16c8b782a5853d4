"""Generate tests/golden/tiny_skiprgb.{npz,json}: the reference's skip_rgb output head (--q_skip_rgb, with and without --q_skip_tanh)
and its quantiser's --q_normalize_out, on CPU through `ref_harness`.

    CCVS_REFERENCE_ROOT=<reference checkout> python tests/golden/make_golden_skiprgb.py

Stored, from the reference's own modules:
  - decoder/<cfg>: SkipGANDecoder on the tiny 3-level geometry with k = 2 contexts and `return_all` (frames, flows and occlusions of
    every level) and one `has_ctx=False` call (the 8 x 8 RGB of level 0); the JSON keeps the state-dict keys and shapes;
  - gen/*: Generator.generate_vid with --q_skip_rgb, greedy: the clip's codes, the synthesized tokens, the fake and rec clips
    (the uint8 files it writes are the reference's pack of those; their SHA-256 digests go into the JSON);
  - torgb/*: one ToRGB(8) call with a skip input of odd width (x [2, 8, 6, 10], skip [2, 3, 3, 5]), inputs and output;
  - norm/*: QVidModel.encode with --q_normalize_out: the codes and the normalised quantised z;
  - state/*: the same encoder and quantiser in an --x_state run (StateModel reads the normalised z): the estimated state codes,
    and Generator.generate_vid greedy -- the synthesized frame and state tokens and the fake clip.
Weights are seeded (`rh.seeded_weights` of the modules' own specs); the inputs are drawn from the seeded generators named in the JSON."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_harness as rh  # noqa: E402

DEC_CONFIGS = {"rgb": ["--q_skip_rgb"], "tanh": ["--q_skip_rgb", "--q_skip_tanh"]}
WEIGHT_SEEDS = {"g": 2000, "e": 1000, "t": 3000, "s": 4000}
# decoder input z [1, 2 frames, 16, 8, 8] and k = 2 contexts, per level fine -> coarse (inter sizes 6, 12, 12)
INPUTS = {"z": [[1, 2, 16, 8, 8], 11], "ctx": [[[1, 2, 6, 32, 32], [1, 2, 12, 16, 16], [1, 2, 12, 8, 8]], 21], "k": 2}
GEN_SEED = 21


def decoder_inputs(spec):
    g = torch.Generator().manual_seed(spec["z"][1])
    z = torch.randn(spec["z"][0], generator=g)
    ctx = []
    for j in range(spec["k"]):
        g = torch.Generator().manual_seed(spec["ctx"][1] + j)
        ctx.append([torch.randn(s, generator=g) for s in spec["ctx"][0]])
    return z, ctx


def input_clip():
    """rand(2, 4, 3, 32, 32) * 2 - 1 from a CPU generator seeded with 1."""
    return torch.rand(2, 4, 3, 32, 32, generator=torch.Generator().manual_seed(1)) * 2 - 1


def digest(t):
    return hashlib.sha256(np.ascontiguousarray(t).tobytes()).hexdigest()


def pack_u8_reference(vid):
    """helpers/generator.py:306-309 for normalize=True, span [-1, 1]: [B, T, 3, H, W] -> [B, T, H, W, 3] uint8."""
    vid = (vid.clamp(-1, 1) + 1) / 2
    return (vid.permute(0, 1, 3, 4, 2) * 255).to(dtype=torch.uint8)


def decoder_weight_spec(dec):
    """The decoder's own initialisers, with non-zero biases (ToRGB's bias and the convolutions' start at zero)."""
    spec = rh.weight_spec(dec)
    for e in spec:
        if e[0].endswith("bias") and e[3] == 0.0:
            e[3] = 0.05
    return spec


def seed_module(module, spec, seed):
    missing, unexpected = module.load_state_dict(rh.seeded_weights(spec, seed), strict=False)
    assert not unexpected and all(k.endswith((".kernel", ".mask")) for k in missing), (missing, unexpected)


def main():
    ns = rh.load_reference()
    arrays = {}
    meta = {"argv": rh.TINY_ARGV, "decoder": {}, "decoder_inputs": INPUTS, "weight_seeds": WEIGHT_SEEDS}
    z, ctx = decoder_inputs(INPUTS)
    for name, flags in DEC_CONFIGS.items():
        qopt = rh.parse_reference_options(rh.TINY_ARGV + flags)["qvid_generator"]
        torch.manual_seed(0)
        dec = ns.sae.SkipGANDecoder(qopt).eval()
        spec = decoder_weight_spec(dec)
        seed_module(dec, spec, WEIGHT_SEEDS["g"])
        with torch.no_grad():
            rgb, _, flows, occs, _ = dec(z, [[t.clone() for t in c] for c in ctx], return_all=True)
            rgb0 = dec(z, [[t.clone() for t in c] for c in ctx], has_ctx=False)[0]
        assert rgb.shape[-1] == 32 and rgb0.shape[-1] == 8
        arrays[f"decoder/{name}/rgb"] = rgb.numpy()
        arrays[f"decoder/{name}/rgb_noctx"] = rgb0.numpy()
        for i, (f, o) in enumerate(zip(flows, occs)):
            arrays[f"decoder/{name}/flow{i}"] = f.numpy()
            arrays[f"decoder/{name}/occ{i}"] = o.numpy()
        meta["decoder"][name] = {"flags": flags, "weight_spec": spec,
                                 "state_dict": [[k, list(v.shape)] for k, v in dec.state_dict().items()]}
        print(f"  decoder {name}: rgb |max| {rgb.abs().max().item():.3f}, no-context rgb {tuple(rgb0.shape)}")

    # one ToRGB with the reference's own Upsample (its CPU upfirdn2d), inputs and weights stored
    g = torch.Generator().manual_seed(41)
    t = ns.sae.ToRGB(8).eval()
    with torch.no_grad():
        for p in t.parameters():
            p.copy_(torch.randn(p.shape, generator=g))
        x, skip = torch.randn(2, 8, 6, 10, generator=g), torch.randn(2, 3, 3, 5, generator=g)
        arrays["torgb/x"], arrays["torgb/skip"], arrays["torgb/out"] = x.numpy(), skip.numpy(), t(x, skip).numpy()
    for k, v in t.state_dict().items():
        arrays[f"torgb/{k}"] = v.numpy()

    # generate_vid with --q_skip_rgb (helpers/generator.py:57-230), greedy; write_video keeps the packed clips
    written, floats = {}, {}
    sys.modules["torchvision.io"].write_video = lambda filename, vid, fps: written.__setitem__(filename, vid.clone())
    from helpers import generator as ref_gen
    ref_gen.mkdir = lambda path: None
    orig_save = ref_gen.save_video_batch

    def save_video_batch(vid, bs, global_iter, path, *a, **k):
        floats[os.path.basename(path)] = vid.detach().clone()
        if k.get("state") is not None:   # the state marker assumes 256^2 frames; the float clip is all the fixture keeps
            return None
        return orig_save(vid, bs, global_iter, path, *a, **k)

    ref_gen.save_video_batch = save_video_batch
    gen_argv = rh.TINY_ARGV + ["--q_skip_rgb", "--x_top_k", "10"]
    opt = rh.parse_reference_options(gen_argv)
    qopt, xopt = opt["qvid_generator"], opt["transformer"]
    vid = input_clip()
    torch.manual_seed(0)
    qv = ns.qvm.QVidModel(qopt, is_train=False, is_main=True).eval()
    meta["gen"] = {"argv": gen_argv, "spec_e": rh.weight_spec(qv.net_e), "spec_g": decoder_weight_spec(qv.net_g), "seed": GEN_SEED,
                   "vid_sha256": digest(vid.numpy())}
    seed_module(qv.net_e, meta["gen"]["spec_e"], WEIGHT_SEEDS["e"])
    seed_module(qv.net_g, meta["gen"]["spec_g"], WEIGHT_SEEDS["g"])
    with torch.no_grad():
        z_e, _ = qv.net_e(vid)
        torch.manual_seed(4)
        qv.net_q.embedding.weight.copy_(torch.randn_like(qv.net_q.embedding.weight) * z_e.std())
    arrays["gen/q/embedding.weight"] = qv.net_q.embedding.weight.detach().numpy()
    torch.manual_seed(10)
    tr = ns.tm.Transformer(xopt, is_train=False, is_main=True).eval()
    g = torch.Generator().manual_seed(30)
    with torch.no_grad():
        for n, p in tr.net_t.named_parameters():
            if n.endswith("_emb"):
                p.normal_(0, 0.02, generator=g)
    meta["gen"]["spec_t"] = rh.weight_spec(tr.net_t)
    seed_module(tr.net_t, meta["gen"]["spec_t"], WEIGHT_SEEDS["t"])
    gen = object.__new__(ref_gen.Generator)
    gen.opt, gen.qvid_opt, gen.state_opt, gen.stft_ae_opt = xopt, qopt, opt["state_estimator"], opt["stft_ae"]
    gen.vid_model, gen.transformer_model, gen.state_model, gen.stft_model = qv, tr, None, None
    gen.valid_data_info = {"batch_size_per_gpu": vid.shape[0]}
    xopt.result_path = "golden"
    xopt.sample = False
    torch.manual_seed(GEN_SEED)
    with torch.no_grad(), rh.patched_overlapping_shift():
        gen.generate_vid({"vid": vid.clone()}, 0)
        enc = qv({"vid": vid.clone()}, mode="vid_encoder")
        out = tr({"code": enc["code"][:, :int(xopt.cond_len)].clone()}, mode="inference", total_len=xopt.vid_len * 64)
        fake = qv({"code": out["code"].clone(), "inter": [f[:, :1] for f in enc["inter"]]}, mode="vid_decoder")["vid"]
    assert torch.equal(floats["real"], vid)
    d = (fake - floats["fake"]).abs().max().item()
    print(f"  gen: tokens {tuple(out['code'].shape)}, fake {tuple(floats['fake'].shape)}, re-decoded vs generate_vid max|diff| = {d:.3e}")
    assert d == 0.0
    arrays["gen/enc_code"] = enc["code"].to(torch.int16).numpy()
    arrays["gen/code"] = out["code"].to(torch.int16).numpy()
    arrays["gen/fake"] = floats["fake"].numpy()
    arrays["gen/rec"] = floats["rec"].numpy()
    files = {}
    for fname, u8 in written.items():
        sub, base = fname.split(os.sep)[-2:]
        i = int(base[len("vid_"):-len(".mp4")])
        assert torch.equal(u8, pack_u8_reference(floats[sub])[i]), fname
        files[f"{sub}/{base}"] = digest(u8.numpy())
    meta["gen"]["files"] = dict(sorted(files.items()))

    # --q_normalize_out: the reference's encode (quantize.py:56-57 normalises the quantised z)
    norm_argv = rh.TINY_ARGV + ["--q_normalize_out"]
    qopt = rh.parse_reference_options(norm_argv)["qvid_generator"]
    torch.manual_seed(0)
    qn = ns.qvm.QVidModel(qopt, is_train=False, is_main=True).eval()
    meta["norm"] = {"argv": norm_argv, "spec_e": rh.weight_spec(qn.net_e)}
    seed_module(qn.net_e, meta["norm"]["spec_e"], WEIGHT_SEEDS["e"])
    with torch.no_grad():
        z_e, _ = qn.net_e(vid)
        torch.manual_seed(5)
        # unit rows near the clip's own normalised latents (the normalised z lies on the unit sphere), so that many codes are used
        zf = z_e.transpose(-3, -1).reshape(-1, z_e.shape[-3])
        zf = zf / zf.norm(dim=1, keepdim=True)
        cb = zf[torch.randperm(zf.shape[0])[:qn.net_q.embedding.weight.shape[0]]] + 0.05 * torch.randn_like(qn.net_q.embedding.weight)
        qn.net_q.embedding.weight.copy_(cb / cb.norm(dim=1, keepdim=True))
        enc = qn({"vid": vid.clone()}, mode="vid_encoder")
    arrays["norm/q/embedding.weight"] = qn.net_q.embedding.weight.detach().numpy()
    arrays["norm/code"] = enc["code"].to(torch.int16).numpy()
    arrays["norm/z"] = enc["z"].numpy()
    print(f"  norm: codes {tuple(enc['code'].shape)} ({len(torch.unique(enc['code']))} distinct), |z| per position "
          f"{enc['z'].norm(dim=2).min().item():.6f} .. {enc['z'].norm(dim=2).max().item():.6f}")

    # --x_state with --q_normalize_out: the state is estimated from the normalised z (state_model.py:110-116)
    state_argv = rh.TINY_STATEMODEL_ARGV + ["--x_z_len", "264", "--q_normalize_out", "--x_top_k", "10"]
    opt = rh.parse_reference_options(state_argv)
    qopt, xopt, sopt = opt["qvid_generator"], opt["transformer"], opt["state_estimator"]
    assert xopt.state and qopt.normalize_out
    torch.manual_seed(0)
    sm = ns.state_model.StateModel(sopt, is_train=False, is_main=True).eval()
    meta["state"] = {"argv": state_argv, "spec_s": decoder_weight_spec(sm.net_s), "spec_g": decoder_weight_spec(qn.net_g)}
    seed_module(qn.net_g, meta["state"]["spec_g"], WEIGHT_SEEDS["g"])
    seed_module(sm.net_s, meta["state"]["spec_s"], WEIGHT_SEEDS["s"])
    arrays["state/sq/embedding.weight"] = sm.net_q.embedding.weight.detach().numpy()
    torch.manual_seed(11)
    tr = ns.tm.Transformer(xopt, is_train=False, is_main=True).eval()
    g = torch.Generator().manual_seed(31)
    with torch.no_grad():
        for n, p in tr.net_t.named_parameters():
            if n.endswith("_emb"):
                p.normal_(0, 0.02, generator=g)
    meta["state"]["spec_t"] = rh.weight_spec(tr.net_t)
    seed_module(tr.net_t, meta["state"]["spec_t"], WEIGHT_SEEDS["t"] + 100)
    gen = object.__new__(ref_gen.Generator)
    gen.opt, gen.qvid_opt, gen.state_opt, gen.stft_ae_opt = xopt, qopt, sopt, opt["stft_ae"]
    gen.vid_model, gen.transformer_model, gen.state_model, gen.stft_model = qn, tr, sm, None
    gen.valid_data_info = {"batch_size_per_gpu": vid.shape[0]}
    xopt.result_path = "golden"
    xopt.sample, xopt.sample_state = False, False
    floats.clear()
    torch.manual_seed(GEN_SEED)
    with torch.no_grad(), rh.patched_overlapping_shift():
        gen.generate_vid({"vid": vid.clone()}, 0)
        enc = qn({"vid": vid.clone()}, mode="vid_encoder")
        st = sm(enc, mode="vid_encoder")["state_code"]
        ss = sopt.state_size
        out = tr({"code": enc["code"][:, :64].clone(), "state_code": st[:, :ss].clone()}, mode="inference",
                 total_len=xopt.vid_len * (64 + ss))
        fake = qn({"code": out["code"].clone(), "inter": [f[:, :1] for f in enc["inter"]]}, mode="vid_decoder")["vid"]
    d = (fake - floats["fake"]).abs().max().item()
    print(f"  state: state codes {tuple(st.shape)} ({len(torch.unique(st))} distinct), tokens {tuple(out['code'].shape)} / "
          f"{tuple(out['state_code'].shape)}, re-decoded vs generate_vid max|diff| = {d:.3e}")
    assert d == 0.0
    arrays["state/enc_code"] = enc["code"].to(torch.int16).numpy()
    arrays["state/state_code"] = st.to(torch.int16).numpy()
    arrays["state/code"] = out["code"].to(torch.int16).numpy()
    arrays["state/gen_state_code"] = out["state_code"].to(torch.int16).numpy()
    arrays["state/fake"] = floats["fake"].numpy()

    np.savez_compressed(os.path.join(HERE, "tiny_skiprgb.npz"), **arrays)
    meta["npz_sha256"] = {k: digest(v) for k, v in sorted(arrays.items())}
    json.dump(meta, open(os.path.join(HERE, "tiny_skiprgb.json"), "w"), indent=1)
    print("  wrote tiny_skiprgb.npz", sum(a.nbytes for a in arrays.values()) / 1e6, "MB raw")


if __name__ == "__main__":
    main()
