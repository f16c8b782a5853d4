"""Generate tests/golden/tiny_tloss.npz: the reference's own `Transformer.compute_transformer_loss` (transformer_model.py:142-253)
on the CPU through `ref_harness`.

    CCVS_REFERENCE_ROOT=<reference checkout> python tests/golden/make_golden_tloss.py

One tiny GPT (2 layers, the `TINY_*` option lines) per case of `CASES`; per case the fixture holds the launch line, the network's
weights (once per distinct network: `w/<net>/...`), the inputs, the reference's `t_loss` and the per-token values behind it --
`F.cross_entropy(..., reduction='none')` on the logits the reference's own call produced (captured at `net_t`'s output) and the
reference's row lists.  The fixture is DATA; no reference source travels.

With the default initialiser (std 0.02) every logit is ~0 and every loss is log V whatever the code under test does: `head.weight`
is multiplied by one recorded factor (`head_factor`), doubled until in EVERY case the reference's per-token frame NLLs have a
standard deviation of at least 1 and at least one value below 0.5 log V (`well_conditioned`; the tests assert it on the fixture).
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_harness as rh  # noqa: E402
from tloss_ref import reference_rows, well_conditioned  # noqa: E402  (the row lists and the conditioning rule: one copy, with the tests)

DEBLUR = ["--x_deblurring", "--x_state_size", "64", "--x_state_num", "32", "--x_z_len", "512", "--x_z_chunk", "128"]
# case -> (network, launch line, frame tokens per clip, ancillary tokens per clip, conditioning-prefix tokens, label)
CASES = {
    "plain":       ("base",  rh.TINY_ARGV, 192, 0, 0, False),
    "crop":        ("base",  rh.TINY_ARGV, 300, 0, 0, False),                      # longer than z_len = 256: cropped
    "p2p":         ("base",  rh.TINY_ARGV + ["--x_p2p"], 128, 0, 64, False),
    "start":       ("start", rh.TINY_ARGV + ["--x_use_start_token"], 130, 0, 0, False),
    "label":       ("label", rh.TINY_ARGV + ["--x_cat", "--categories", "a", "b", "c"], 130, 0, 0, True),
    "state2":      ("state", rh.TINY_STATE_ARGV, 128, 4, 0, False),                # two whole frames, 2 + 64 tokens each
    "state3":      ("state", rh.TINY_STATE_ARGV, 192, 6, 0, False),
    "state_front": ("state", rh.TINY_STATE_ARGV + ["--x_state_front"], 128, 8, 0, False),
    "deblur":      ("deblur", rh.TINY_ARGV + DEBLUR, 128, 128, 0, False),          # state_size = h * w, state_num = z_num
}
BATCH = 2


def per_token(xopt, logits, code, state_code):
    """The values `F.cross_entropy` averages in transformer_model.py:229,239: (frame [B, n], ancillary [B, n] or [B, 0])."""
    code = code[:, :xopt.z_len]
    b = code.shape[0]
    if 0 not in state_code.size():
        size = xopt.z_shape[0] * xopt.z_shape[1]
        state_i, frame_i = reference_rows(logits.size(1), xopt.state_size, size + xopt.state_size, xopt.num_blocks, xopt.state_front)
        state_logits = logits[:, state_i, :xopt.state_num]
        s = F.cross_entropy(state_logits.reshape(-1, state_logits.size(-1)), state_code[:, 1:].reshape(-1), reduction="none").view(b, -1)
        logits, target = logits[:, frame_i], code
    else:
        target = code if (xopt.use_start_token or xopt.cat) else code[:, 1:]
        s = torch.zeros(b, 0)
    f = F.cross_entropy(logits.reshape(-1, logits.size(-1)), target.reshape(-1), reduction="none").view(b, -1)
    return f, s


def inputs_of(name, xopt, n_code, n_state, n_cond, label, seed):
    g = torch.Generator().manual_seed(seed)
    empty = torch.tensor([])
    d = {"code": torch.randint(0, xopt.z_num, (BATCH, n_code), generator=g)}
    d["state_code"] = torch.randint(0, xopt.state_num, (BATCH, n_state), generator=g) if n_state else empty
    d["cond_code"] = torch.randint(0, xopt.z_num, (BATCH, n_cond), generator=g) if n_cond else empty
    d["delta_length_cond"] = torch.tensor([3, 2]) if n_cond else empty
    d["vid_lbl"] = torch.tensor([2, 0]) if label else empty
    return d


def main():
    ns = rh.load_reference()
    nets, runs = {}, {}
    for ci, (name, (net, argv, n_code, n_state, n_cond, label)) in enumerate(CASES.items()):
        xopt = rh.parse_reference_options(argv)["transformer"]
        torch.manual_seed(100 + list(dict.fromkeys(v[0] for v in CASES.values())).index(net))
        tr = ns.tm.Transformer(xopt, is_train=False, is_main=True).eval()
        if net in nets:
            tr.net_t.load_state_dict(nets[net], strict=False)
        else:
            g = torch.Generator().manual_seed(7)
            with torch.no_grad():
                for n, p in tr.net_t.named_parameters():   # the zero-initialised positional / start tables
                    if n.endswith("_emb"):
                        p.normal_(0, 0.02, generator=g)
            nets[net] = {k: v.clone() for k, v in tr.net_t.state_dict().items() if not k.endswith(".mask")}
        runs[name] = (tr, xopt, inputs_of(name, xopt, n_code, n_state, n_cond, label, 50 + ci))

    def run(name):
        tr, xopt, d = runs[name]
        seen = []
        hook = tr.net_t.register_forward_hook(lambda mod, args, out: seen.append(out.detach().clone()))
        with torch.no_grad():
            t_loss = tr.compute_transformer_loss(d["code"].clone(), d["state_code"].clone(), d["cond_code"].clone(),
                                                 d["delta_length_cond"].clone(), d["vid_lbl"].clone(), "", False, None)
        hook.remove()
        f, s = per_token(xopt, seen[0], d["code"], d["state_code"])
        want = f.mean() + (s.mean() if s.numel() else 0.0)
        assert abs(float(want) - float(t_loss)) <= 1e-6 * max(1.0, abs(float(t_loss))), (name, float(want), float(t_loss))
        return t_loss.clone(), f, s

    factor = 1.0
    while True:
        out = {name: run(name) for name in CASES}
        if all(well_conditioned(f.numpy(), runs[name][1].z_num) for name, (_, f, _) in out.items()):
            break
        factor *= 2.0
        assert factor <= 4096.0
        for name, (tr, _, _) in runs.items():
            with torch.no_grad():
                tr.net_t.head.weight.mul_(2.0)
    arrays = {"head_factor": np.float32(factor),
              "cases": np.array(json.dumps({name: {"net": v[0], "argv": list(v[1])} for name, v in CASES.items()}))}
    for net, sd in nets.items():
        sd = dict(sd)
        sd["head.weight"] = sd["head.weight"] * factor
        arrays.update({f"w/{net}/{k}": v.numpy() for k, v in sd.items()})
    for name, (t_loss, f, s) in out.items():
        tr, xopt, d = runs[name]
        assert torch.equal(tr.net_t.head.weight, torch.from_numpy(arrays[f"w/{CASES[name][0]}/head.weight"]))
        for k, v in d.items():
            arrays[f"{name}/{k}"] = v.numpy().astype(np.int16) if v.numel() else np.zeros(0, np.float32)
        arrays[f"{name}/t_loss"], arrays[f"{name}/nll"], arrays[f"{name}/state_nll"] = t_loss.numpy(), f.numpy(), s.numpy()
        print(f"  {name:12s} t_loss {float(t_loss):9.5f}  frame nll [{tuple(f.shape)}] std {f.std():.3f} min {f.min():.3f}"
              + (f"  state nll [{tuple(s.shape)}] mean {s.mean():.3f}" if s.numel() else ""))
    np.savez_compressed(os.path.join(HERE, "tiny_tloss.npz"), **arrays)
    print(f"  head factor {factor}; wrote tiny_tloss.npz", sum(a.nbytes for a in arrays.values()) / 1e3, "KB raw,",
          os.path.getsize(os.path.join(HERE, "tiny_tloss.npz")) / 1e3, "KB on disk")


if __name__ == "__main__":
    main()
