"""Generate tests/golden/tiny_deblur.{npz,json}: the reference's own `Generator.generate_vid` (helpers/generator.py:57-230) in the
deblurring mode (`--x_deblurring`), on CPU through `ref_harness`.

    CCVS_REFERENCE_ROOT=<reference checkout> python tests/golden/make_golden_deblur.py

torchvision is stubbed by the harness: `blur_ref.GaussianBlur` (pinned by tests/test_deblur_host.py) stands in for
`transforms.GaussianBlur`, and `torchvision.io.write_video` is replaced by a function that keeps the uint8 clips the reference's
`save_video_batch` packed.  Two configurations: the whole interleaved sequence (64 blurred-clip tokens + 64 frame tokens per frame,
4 frames) in one window, and the same with a window of two frames that slides.  Each runs greedy and with seeded multinomial
sampling; the tests reproduce the sampled run from the same process-generator seed (the blur's sigma draw comes first).

Stored: the codebook, every run's clip codes, blurred-clip codes and synthesized tokens; the decoded clips (fake of both
runs, rec) of the whole-sequence case -- the sliding case decodes along the same path and is there for its token windows.  NOT stored,
because the script checks here that they follow from what is: the input clip (`input_clip`, its SHA-256 in the JSON), the blurred clip (`blur_ref.blur` of the input, bit for bit) and the
uint8 packs (`pack_u8_reference` of the float clips, bit for bit; their SHA-256 digests go into the JSON)."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import blur_ref  # noqa: E402
import ref_harness as rh  # noqa: E402

DEBLUR_ARGV = rh.TINY_ARGV + ["--x_deblurring", "--x_state_size", "64", "--x_state_num", "32", "--x_top_k", "10"]
CASES = {
    "whole": {"flags": ["--x_z_len", "512", "--x_z_chunk", "128", "--x_num_blocks", "4", "--x_blur_sigma", "2"]},
    "slide": {"flags": ["--x_z_len", "256", "--x_z_chunk", "128", "--x_num_blocks", "2", "--x_blur_sigma", "10"]},
}
SEEDS = {"greedy": 21, "sampled": 23}


def pack_u8_reference(vid):
    """helpers/generator.py:306-309 for normalize=True, imagenet_norm=False, span [-1, 1]: [B, T, 3, H, W] -> [B, T, H, W, 3] uint8."""
    vid = vid.clamp(-1, 1)
    vid = (vid - (-1)) / (1 - (-1))
    return (vid.permute(0, 1, 3, 4, 2) * 255).to(dtype=torch.uint8)


def input_clip():
    """The fixture's input: rand(2, 4, 3, 32, 32) * 2 - 1 from a CPU generator seeded with 1."""
    return torch.rand(2, 4, 3, 32, 32, generator=torch.Generator().manual_seed(1)) * 2 - 1


def digest(t):
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def blur_sigma_of(flags):
    return int(flags[flags.index("--x_blur_sigma") + 1])


def seed_module(module, seed):
    """Replace the module's weights by `rh.seeded_weights` of its own spec; returns the spec (the fixture stores it, not the weights)."""
    spec = rh.weight_spec(module)
    missing, unexpected = module.load_state_dict(rh.seeded_weights(spec, seed), strict=False)
    assert not unexpected and all(k.endswith((".kernel", ".mask")) for k in missing), (missing, unexpected)
    return spec


def main():
    ns = rh.load_reference()
    sys.modules["torchvision.transforms"].GaussianBlur = blur_ref.GaussianBlur
    written = {}

    def write_video(filename, vid, fps):
        written[filename] = vid.clone()

    sys.modules["torchvision.io"].write_video = write_video
    from helpers import generator as ref_gen
    ref_gen.mkdir = lambda path: None
    floats = {}
    orig_save = ref_gen.save_video_batch

    def save_video_batch(vid, bs, global_iter, path, *a, **k):
        floats[os.path.basename(path)] = vid.detach().clone()
        return orig_save(vid, bs, global_iter, path, *a, **k)

    ref_gen.save_video_batch = save_video_batch

    vid = input_clip()
    arrays = {}
    meta = {"argv": DEBLUR_ARGV, "cases": {}, "seeds": SEEDS, "weight_seeds": {"e": 1000, "g": 2000, "t": 3000}, "vid_sha256": digest(vid)}
    qv = None
    for ci, (name, case) in enumerate(CASES.items()):
        opt = rh.parse_reference_options(DEBLUR_ARGV + case["flags"])
        qopt, xopt = opt["qvid_generator"], opt["transformer"]
        assert xopt.deblurring and xopt.state_size == 64 and xopt.state_num == 32
        if qv is None:
            torch.manual_seed(0)
            qv = ns.qvm.QVidModel(qopt, is_train=False, is_main=True).eval()
            meta["spec_e"] = seed_module(qv.net_e, meta["weight_seeds"]["e"])
            meta["spec_g"] = seed_module(qv.net_g, meta["weight_seeds"]["g"])
            with torch.no_grad():
                z_e, _ = qv.net_e(vid)
                torch.manual_seed(4)
                qv.net_q.embedding.weight.copy_(torch.randn_like(qv.net_q.embedding.weight) * z_e.std())
            arrays["q/embedding.weight"] = qv.net_q.embedding.weight.detach().numpy()
        torch.manual_seed(10 + ci)
        tr = ns.tm.Transformer(xopt, is_train=False, is_main=True).eval()
        meta["cases"][name] = {"flags": case["flags"]}
        g = torch.Generator().manual_seed(30 + ci)
        with torch.no_grad():
            for n, p in tr.net_t.named_parameters():       # the zero-initialised positional tables (s_emb, t_emb, state_s_emb)
                if n.endswith("_emb"):
                    p.normal_(0, 0.02, generator=g)
        meta["cases"][name]["spec_t"] = seed_module(tr.net_t, meta["weight_seeds"]["t"] + 100 * ci)

        gen = object.__new__(ref_gen.Generator)
        gen.opt, gen.qvid_opt, gen.state_opt, gen.stft_ae_opt = xopt, qopt, opt["state_estimator"], opt["stft_ae"]
        gen.vid_model, gen.transformer_model, gen.state_model, gen.stft_model = qv, tr, None, None
        gen.valid_data_info = {"batch_size_per_gpu": vid.shape[0]}
        xopt.result_path = "golden"
        meta["cases"][name]["files"] = {}
        blurred = blur_ref.blur(vid, blur_sigma_of(case["flags"]))
        fake_of = {}
        for mode, seed in SEEDS.items():
            xopt.sample = mode == "sampled"
            floats.clear()
            written.clear()
            torch.manual_seed(seed)
            with torch.no_grad(), rh.patched_overlapping_shift():
                gen.generate_vid({"vid": vid.clone()}, 0)
            # what generate_vid computed on the way: the blurred clip and its codes, the clip's codes, the synthesized tokens
            with torch.no_grad():
                enc = qv({"vid": vid.clone()}, mode="vid_encoder")
                benc = qv({"vid": floats["blur"].clone()}, mode="vid_encoder")
            pre = f"{name}/{mode}"
            arrays[f"{pre}/enc_code"] = enc["code"].to(torch.int16).numpy()
            arrays[f"{pre}/blur_code"] = benc["code"].to(torch.int16).numpy()
            assert torch.equal(floats["real"], vid) and torch.equal(floats["blur"], blurred)
            fake_of[mode] = floats["fake"]
            if name == "whole":
                arrays[f"{pre}/fake"] = floats["fake"].numpy()
                if "whole/rec" in arrays:       # the rec pass reads the clip's codes and the blurred features only: the same for both runs
                    assert np.array_equal(arrays["whole/rec"], floats["rec"].numpy())
                arrays["whole/rec"] = floats["rec"].numpy()
            digests = {}
            for fname, u8 in written.items():
                sub, base = fname.split(os.sep)[-2:]
                i = int(base[len("vid_"):-len(".mp4")])
                assert torch.equal(u8, pack_u8_reference(floats[sub])[i]), fname
                digests[f"{sub}/{base}"] = digest(u8)
            meta["cases"][name]["files"][mode] = dict(sorted(digests.items()))
        # the synthesized tokens: the transformer's own pass on the blurred-clip stream, from the same generator position as inside
        # generate_vid (the blur draws once, then the token loop; greedy draws nothing)
        cond = int(xopt.cond_len)
        total_len = xopt.vid_len * 64 + xopt.vid_len * 64
        for mode, seed in SEEDS.items():
            xopt.sample = mode == "sampled"
            pre = f"{name}/{mode}"
            code = torch.from_numpy(arrays[f"{pre}/enc_code"]).long()[:, :cond]
            state = torch.from_numpy(arrays[f"{pre}/blur_code"]).long()
            torch.manual_seed(seed)
            torch.empty(1).uniform_(xopt.blur_sigma, xopt.blur_sigma)
            with torch.no_grad():
                out = tr({"code": code.clone(), "state_code": state.clone()}, mode="inference", total_len=total_len)
            arrays[f"{pre}/code"] = out["code"].to(torch.int16).numpy()
            # the fake clip decoded from these tokens must be the one generate_vid wrote
            with torch.no_grad(), rh.patched_overlapping_shift():
                fake = qv({"code": out["code"].clone(), "inter": qv({"vid": blurred.clone()}, mode="vid_encoder")["inter"]},
                          mode="vid_decoder")["vid"]
            want = fake_of[mode]
            d = (fake - want).abs().max().item()
            print(f"  {pre}: tokens {tuple(out['code'].shape)}, fake re-decoded vs generate_vid max|diff| = {d:.3e}")
            assert d == 0.0
        xopt.sample = False

    np.savez_compressed(os.path.join(HERE, "tiny_deblur.npz"), **arrays)
    json.dump(meta, open(os.path.join(HERE, "tiny_deblur.json"), "w"), indent=1)
    print("  wrote tiny_deblur.npz", sum(a.nbytes for a in arrays.values()) / 1e6, "MB raw")


if __name__ == "__main__":
    main()
