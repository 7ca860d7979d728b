"""Golden fixtures for LSTM hidden sizes outside {16, 32, 48, 64}, from the
reference code (CPU).

    python tests/golden/make_golden_hsizes.py

gen_fwd_h40.npz   the committed GAT generator with --noise_dim 16: the decoder's
                  hidden size is the GAT encoder's 24 outputs + 16 = 40.
gen_fwd_h128.npz  the gcn family (the commented call at models.py:902,
                  make_golden._gen_forward) with --decoder_h_dim_g 128, upstream
                  Social-GAN's default.

Each holds the generator's weights (w/*), a 3-scene batch of {1, 5, 20}
pedestrians, the noise, the forward output, the output gradient and every
parameter gradient (dw/*).  The reference's constructors take both sizes as
they are, so nothing is generated from the oracle.
"""
import copy

import torch

import make_golden as MG

SIZES = [1, 5, 20]
SEED = 31


def fixture(name, mode, noise_dim, decoder_h_dim):
    saved = copy.copy(MG.ARGS)
    try:
        MG.ARGS.noise_dim = (noise_dim,)
        MG.ARGS.decoder_h_dim_g = decoder_h_dim
        g, _ = MG.build_models(0)
    finally:
        MG.ARGS.__dict__.update(saved.__dict__)
    b = MG.synth_batch(SIZES, seed=SEED)
    torch.manual_seed(SEED)
    noise = torch.randn(len(SIZES), noise_dim)
    g.zero_grad()
    y = MG._gen_forward(g, b, noise, mode)
    dy = torch.randn_like(y)
    (y * dy).sum().backward()
    out = {k: b[k].numpy() for k in ("obs_traj", "obs_traj_rel", "obs_traj_g", "seq_start_end")}
    out.update(noise=noise.numpy(), out=y.detach().numpy(), dout=dy.numpy())
    out.update(MG.sd_arrays(g, "w/"))
    out.update(MG.grad_arrays(g, "dw/"))
    MG.save(name, out)


if __name__ == "__main__":
    fixture("gen_fwd_h40.npz", "gat", 16, 40)
    fixture("gen_fwd_h128.npz", "gcn", 8, 128)
