"""Test-side yardstick of the transformer's teacher-forced loss: the composition `oracle.gpt_forward` -> the reference's row lists ->
`F.cross_entropy`, and the readers of tests/golden/tiny_tloss.npz (tests/golden/make_golden_tloss.py).  Never imported by the
product."""
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import ccvs_oracle as O  # noqa: E402

INPUT_KEYS = ("code", "state_code", "cond_code", "delta_length_cond", "vid_lbl")


def reference_rows(n_logits, state_size, tot_size, num_blocks, state_front):
    """transformer_model.py:215-220 of the reference, restated."""
    if state_front:
        state_i = [i for i in range(n_logits) if (i + 1) < state_size * num_blocks]
        frame_i = [i for i in range(n_logits) if (i + 1) >= state_size * num_blocks]
    else:
        state_i = [i for i in range(n_logits) if (i + 1) % tot_size < state_size]
        frame_i = [i for i in range(n_logits) if (i + 1) % tot_size >= state_size]
    return state_i, frame_i


def well_conditioned(nll, vocab):
    """The fixture's condition: per-token NLLs that spread (std >= 1) and at least one confident prediction (< 0.5 log V)."""
    nll = np.asarray(nll, dtype=np.float64)
    return bool(nll.std() >= 1.0 and nll.min() < 0.5 * math.log(vocab))


def load_gold(golden_dir):
    gold = np.load(os.path.join(golden_dir, "tiny_tloss.npz"))
    return gold, json.loads(str(gold["cases"]))


def weights_of(gold, net):
    pre = f"w/{net}/"
    return {k[len(pre):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(pre)}


def inputs_of(gold, name):
    """The case's inputs as the reference saw them: int64 codes, an empty tensor where a stream is absent."""
    return {k: (torch.from_numpy(gold[f"{name}/{k}"]).long() if gold[f"{name}/{k}"].size else torch.tensor([])) for k in INPUT_KEYS}


def transformer_options(argv):
    from ccvs_amd.tools.options import Options
    return Options().parse(load_qvid_generator=True, load_transformer=True, load_state_estimator=True, load_stft_ae=True, argv=list(argv))["transformer"]


def oracle_loss(sd, xopt, d):
    """compute_transformer_loss (transformer_model.py:142-253, discrete branch) on the CPU oracle: (t_loss, frame NLL [B, n],
    ancillary NLL [B, n] or [B, 0])."""
    cfg = O.namespace(**vars(xopt))
    code = d["code"][:, :xopt.z_len]
    state = d["state_code"]
    has_state = 0 not in state.size()
    b = code.shape[0]
    with torch.no_grad():
        logits = O.gpt_forward(sd, cfg, code[:, :-1], d["cond_code"] if d["cond_code"].numel() else None,
                               d["delta_length_cond"] if d["cond_code"].numel() else None, state if has_state else None,
                               d["vid_lbl"] if d["vid_lbl"].numel() else None)
        if has_state:
            size = xopt.z_shape[0] * xopt.z_shape[1]
            state_i, frame_i = reference_rows(logits.size(1), xopt.state_size, size + xopt.state_size, xopt.num_blocks, xopt.state_front)
            sl = logits[:, state_i, :xopt.state_num]
            s = F.cross_entropy(sl.reshape(-1, sl.size(-1)), state[:, 1:].reshape(-1), reduction="none").view(b, -1)
            logits, target = logits[:, frame_i], code
        else:
            target = code if (xopt.use_start_token or xopt.cat) else code[:, 1:]
            s = torch.zeros(b, 0)
        f = F.cross_entropy(logits.reshape(-1, logits.size(-1)), target.reshape(-1), reduction="none").view(b, -1)
        t_loss = F.cross_entropy(logits.reshape(-1, logits.size(-1)), target.reshape(-1))
        if has_state:
            t_loss = t_loss + F.cross_entropy(sl.reshape(-1, sl.size(-1)), state[:, 1:].reshape(-1))
    return t_loss, f, s
