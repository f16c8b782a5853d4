"""Generate tests/golden/tiny_stft_decoder.npz from the imported reference.

    CCVS_REFERENCE_ROOT=<reference checkout> python tests/golden/make_stft_decoder_golden.py

The reference's own `StftModel` (encoder, decoder, quantiser) on the CPU with `ref_harness.TINY_STATE_ARGV`: the three state
dicts, a [2, 5, 1, 16, 8] input, its codes, the `vid_decoder` / `img_decoder` outputs, the `eval_stft_reconstruction` value; and
from the reference's `StateModel` on the networks and inputs of tiny_statemodel.npz one `eval_state_estimator` value.  The fixture
is DATA; no reference source travels.

With the default initialiser the decoded spectrogram has max |x| = 1e-3: the weights are conditioned
(`stft_decoder_ref.condition_weights`: codebook ~ N(0, s^2), decoder biases ~ N(0, 0.1^2), the last convolution times a recorded
factor that doubles until the reference output has max |x| >= 0.5 and 1 % of its values beyond 0.5).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import ref_harness as rh  # noqa: E402
import stft_decoder_ref as R  # noqa: E402

S, SEED = 4.0, 41


def report(name, a, b):
    d = (a.float() - b.float()).abs().max().item()
    print(f"  composition vs reference  {name:32s} max|diff| = {d:.3e}")
    return d


def main():
    ns = rh.load_reference()
    opt = rh.parse_reference_options(rh.TINY_STATE_ARGV)
    aopt = opt["stft_ae"]
    out = {}
    torch.manual_seed(0)
    seeded = ns.sae.StftDecoder(aopt)            # the initialiser stream of a decoder built alone under seed 0
    out["seed0/convs.0.0.weight"] = seeded.state_dict()["convs.0.0.weight"].clone()
    out["seed0/convs.4.0.weight"] = seeded.state_dict()["convs.4.0.weight"].clone()
    torch.manual_seed(0)
    sm = ns.stft_model.StftModel(aopt, is_train=False, is_main=True).eval()
    sds = {"ae": sm.net_e.state_dict(), "ad": sm.net_d.state_dict(), "aq": sm.net_q.state_dict()}
    # what the model's own constructor drew under seed 0 (net_e, net_d, net_q in that order), before the conditioning below
    for pre, key in (("ae", "convs.4.0.weight"), ("ad", "convs.0.0.weight"), ("ad", "convs.4.0.weight"), ("aq", "embedding.weight")):
        out[f"model_seed0/{pre}/{key}"] = sds[pre][key].clone()
    torch.manual_seed(11)
    # a level per token position and frame under a little noise: plain uniform noise is averaged away by the encoder's three blurred
    # stride-2 layers and every position would get the same code
    level = (torch.rand(2, 5, 1, 2, 1) * 2 - 1).repeat_interleave(8, dim=-2).repeat_interleave(8, dim=-1)
    stft = (0.8 * level + 0.2 * (torch.rand(2, 5, 1, 16, 8) * 2 - 1)).clamp(-1, 1)
    factor = 1.0
    with torch.no_grad():
        R.condition_weights(sds["ae"], sds["ad"], sds["aq"], S, SEED)
        while True:
            codes = sm({"stft": stft.clone()}, mode="vid_encoder")["state_code"]
            vid = sm({"state_code": codes.clone()}, mode="vid_decoder")["stft"]
            if R.well_conditioned(vid):
                break
            sds["ad"]["convs.4.0.weight"].mul_(2.0)
            factor *= 2.0
            assert factor <= 1024.0
        img = sm({"state_code": codes[:, :2].clone()}, mode="img_decoder")["stft"]
        loss = sm({"stft": stft.clone()}, mode="eval_stft_reconstruction")
        pred = sm.net_d(sm.net_q(sm.net_e(stft))[0])
    print(f"  last-layer factor {factor}, codes used {codes.unique().numel()} of {aopt.stft_num}, max|vid| {vid.abs().max():.3f}, "
          f"beyond 0.5: {(vid.abs() > 0.5).float().mean():.3f}, loss {loss.item():.6f}")
    out.update(stft=stft, state_code=codes, vid_decoder=vid, img_decoder=img, eval_stft_reconstruction=loss, eval_stft_pred=pred,
               last_factor=torch.tensor(factor), codebook_std=torch.tensor(S))
    for pre, sd in sds.items():
        out.update({f"{pre}/{k}": v.clone() for k, v in sd.items() if not k.endswith(".kernel")})
    with torch.no_grad():
        report("vid_decoder", R.stft_decode(sds, aopt.stft_shape, codes, "vid"), vid)
        report("img_decoder", R.stft_decode(sds, aopt.stft_shape, codes[:, :2], "img"), img)
        l2, p2, _ = R.eval_stft_reconstruction(sds, stft)
        report("eval_stft_reconstruction", l2, loss)
        report("eval prediction", p2, pred)

    # eval_state_estimator on the networks and inputs of tiny_statemodel.npz
    sopt = rh.parse_reference_options(rh.TINY_STATEMODEL_ARGV)["state_estimator"]
    base = np.load(os.path.join(HERE, "tiny_statemodel.npz"))
    torch.manual_seed(0)
    st = ns.state_model.StateModel(sopt, is_train=False, is_main=True).eval()
    st.net_s.load_state_dict({k[2:]: torch.from_numpy(base[k]) for k in base.files if k.startswith("s/")}, strict=False)
    st.net_q.load_state_dict({k[3:]: torch.from_numpy(base[k]) for k in base.files if k.startswith("sq/")})
    z, given = torch.from_numpy(base["z"]), torch.from_numpy(base["given"])
    with torch.no_grad():
        assert torch.equal(st({"z": z.clone()}, mode="vid_encoder")["state_code"], torch.from_numpy(base["state_code"]))
        s_loss = st({"z": z.clone(), "state": given.clone()}, mode="eval_state_estimator")
        s_q = st.net_q(st.net_s(z))[0]
        nets = {"s": st.net_s.state_dict(), "sq": st.net_q.state_dict()}
        l3, q3, _ = R.eval_state_estimator(nets, sopt, z, given)
        report("eval_state_estimator", l3, s_loss)
        report("quantised state", q3, s_q)
    out.update(eval_state_estimator=s_loss, eval_state_q=s_q)
    arrays = {k: v.detach().cpu().numpy() for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, "tiny_stft_decoder.npz"), **arrays)
    print("  wrote tiny_stft_decoder.npz", sum(a.nbytes for a in arrays.values()) / 1e3, "KB raw")


if __name__ == "__main__":
    main()
