"""Golden fixture for the pooling net with batch norm, from the reference code.

    python tests/golden/make_golden_pool_norm.py

pool_norm.npz  the reference's PoolHiddenNet with batch_norm=True (embedding_dim
               8, h_dim 32, bottleneck_dim 24) on scenes of 2, 5 and 20 peds:
               train() forward and backward (out, dout, dh, dpos, dw/*), the
               BatchNorm buffers after that forward (buf/*: one momentum update
               per scene and layer, three in all), then the eval() forward on
               those buffers (out_eval).  w/* holds the parameters and the
               initial buffers.

The net is the reference's under scripts/train.py's init_weights; the BatchNorm
weights are then drawn around 1 with every fifth entry negated and the biases
non-zero, so the affine map matters and a max taken before it would be wrong.
"""
import os

import numpy as np
import torch

from make_golden import HERE, M, TR, save

SIZES = [2, 5, 20]
E_DIM, H_DIM, BN = 8, 32, 24


def fx_pool_norm():
    torch.manual_seed(41)
    net = M.PoolHiddenNet(embedding_dim=E_DIM, h_dim=H_DIM, mlp_dim=64, bottleneck_dim=BN, activation="relu",
                          batch_norm=True)
    net.apply(TR.init_weights)
    with torch.no_grad():
        for m in net.mlp_pre_pool:
            if isinstance(m, torch.nn.BatchNorm1d):
                g = 1.0 + 0.3 * torch.randn(m.num_features)
                g[::5] = -g[::5]
                m.weight.copy_(g)
                m.bias.copy_(0.3 * torch.randn(m.num_features))
    net.train()
    arrs = {"w/" + k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
    B = sum(SIZES)
    off = np.concatenate([[0], np.cumsum(SIZES)])
    sse = torch.from_numpy(np.stack([off[:-1], off[1:]], 1).astype(np.int64))
    h = torch.randn(1, B, H_DIM, requires_grad=True)
    pos = (torch.rand(B, 2) * 15).requires_grad_(True)
    dout = torch.randn(B, BN)
    out = net(h, sse, pos)
    (out * dout).sum().backward()
    arrs.update(h=h.detach()[0].numpy(), pos=pos.detach().numpy(), sse=sse.numpy(), out=out.detach().numpy(),
                dout=dout.numpy(), dh=h.grad[0].numpy(), dpos=pos.grad.numpy())
    for k, p in net.named_parameters():
        arrs["dw/" + k] = p.grad.numpy()
    for k, b in net.named_buffers():
        arrs["buf/" + k] = b.detach().numpy().copy()
    net.eval()
    with torch.no_grad():
        arrs["out_eval"] = net(h, sse, pos).numpy()
    save("pool_norm.npz", arrs)
    assert os.path.getsize(os.path.join(HERE, "pool_norm.npz")) <= 1 << 20


if __name__ == "__main__":
    fx_pool_norm()
