"""CPU reference of the STFT decoder and the two evaluation figures, composed from functions the oracle already has
(`oracle.ccvs_oracle.conv_layer`, the VQ helpers) plus `torch.tanh`, an embedding lookup and `F.mse_loss`.  Shared by
tests/test_stft_decoder_host.py (which pins this composition to the reference through tests/golden/tiny_stft_decoder.npz),
tests/test_stft_decoder_gpu.py and tests/golden/make_stft_decoder_golden.py.

Also holds the conditioning of the decoder weights both the fixture script and the Drums-size GPU test apply: with the default
initialiser the decoded spectrogram stays below 1e-3 in magnitude, and an all-zero output would pass a 1e-3 bar.
"""
import torch
import torch.nn.functional as F

from oracle import ccvs_oracle as O


def stft_decoder_forward(sd, z):
    """`StftDecoder.forward` (skip_autoencoder.py:544-556) on z [N, C, h, w] or [B, T, C, h, w]: a 3x3 ConvLayer, three up-sampling
    3x3 ConvLayers, a 1x1 ConvLayer to one channel (all with bias + LeakyReLU(0.1)), tanh."""
    lead = z.shape[:-3]
    x = z.reshape(-1, *z.shape[-3:])
    x = O.conv_layer(sd, "convs.0", x)
    for i in range(1, 4):
        x = O.conv_layer(sd, f"convs.{i}", x, upsample=True)
    x = O.conv_layer(sd, "convs.4", x)
    x = torch.tanh(x)
    return x.view(*lead, *x.shape[1:])


def stft_decode(nets, stft_shape, state_code, dtype="vid"):
    """`StftModel.decode` (stft_model.py:127-133): nets["aq"] the codebook, nets["ad"] the decoder.  state_code [B, (T *) h * w]."""
    cb = nets["aq"]["embedding.weight"]
    shape = list(stft_shape) if dtype == "img" else [-1] + list(stft_shape)
    z = O.embed_code(state_code.view(-1, *stft_shape), cb)
    z = z.view(state_code.size(0), *shape, cb.shape[1]).transpose(-2, -1).transpose(-3, -2).contiguous()
    return stft_decoder_forward(nets["ad"], z)


def stft_encoder_forward(sd, stft):
    """`StftEncoder.forward` (skip_autoencoder.py:530-542), the layers of `O.stft_encode`: [B, T, 1, H, W] -> [B, T, C, h, w]."""
    b, t = stft.shape[:2]
    x = stft.reshape(b * t, *stft.shape[2:])
    x = O.conv_layer(sd, "convs.0", x)
    for i in range(1, 4):
        x = O.conv_layer(sd, f"convs.{i}", x, downsample=True)
    x = O.conv_layer(sd, "convs.4", x)
    return x.view(b, t, *x.shape[1:])


def eval_stft_reconstruction(nets, stft):
    """`compute_eval_stft_reconstruction_loss` (stft_model.py:112-118).  Returns (loss, stft_pred, indices).  The quantiser's
    forward value is z + (z_q - z) (quantize.py:64, the straight-through form), not z_q itself: kept."""
    z = stft_encoder_forward(nets["ae"], stft)
    zq, idx = O.vq_quantize(z, nets["aq"]["embedding.weight"])
    zq = z + (zq - z)
    pred = stft_decoder_forward(nets["ad"], zq)
    return F.mse_loss(stft, pred), pred, idx


def eval_state_estimator(nets, sopt, z, state):
    """`compute_eval_state_estimator_loss` (state_model.py:99-107) with a StateEstimator.  Returns (loss, quantised state, indices)."""
    pred = O.state_estimator_forward(nets["s"], sopt, z)
    cb = nets["sq"]["embedding.weight"]
    idx = O.vq_indices(pred, cb)
    zq = cb[idx].view(pred.shape)
    zq = pred + (zq - pred)
    return F.mse_loss(zq, state), zq, idx


def condition_weights(ae, ad, aq, s, seed, last_factor=1.0):
    """In place on the three state dicts: codebook ~ N(0, s^2), every decoder bias ~ N(0, 0.1^2), the decoder's last convolution
    times `last_factor`, and the encoder's last convolution rescaled so that its output has the codebook's spread (else every
    position would pick the code nearest to zero).  Drawn on the CPU from generators seeded by `seed`."""
    g = torch.Generator().manual_seed(seed)
    aq["embedding.weight"].copy_(torch.randn(aq["embedding.weight"].shape, generator=g) * s)
    for k in sorted(ad):
        if k.endswith(".bias"):
            ad[k].copy_(torch.randn(ad[k].shape, generator=g) * 0.1)
    ad["convs.4.0.weight"].mul_(last_factor)
    if ae is not None:
        g2 = torch.Generator().manual_seed(seed + 1)
        probe = torch.rand(1, 2, 1, 8 * 2, 8 * 1, generator=g2) * 2 - 1
        z = stft_encoder_forward(ae, probe)
        ae["convs.4.0.weight"].mul_(s / float(z.std()))


def well_conditioned(x):
    """The condition a reference output must meet before a 1e-3 comparison against it means anything: max |x| >= 0.5 and at
    least 1 % of the values beyond 0.5 in magnitude."""
    a = x.abs()
    return float(a.max()) >= 0.5 and float((a > 0.5).float().mean()) >= 0.01
