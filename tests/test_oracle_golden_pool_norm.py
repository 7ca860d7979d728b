"""Pin the CPU oracle's PoolHiddenNet with batch_norm=True against the
reference's run (tests/golden/make_golden_pool_norm.py -> pool_norm.npz):
train() forward, backward and running statistics, then the eval() forward.
CPU only."""
import os

import numpy as np
import torch

from oracle import sgan_oracle as O

from test_oracle_golden import GOLDEN, T, close, grad_floor, npz

ZERO_BIASES = ("spatial_embedding.bias", "mlp_pre_pool.0.bias", "mlp_pre_pool.3.bias")


def test_pool_norm_fixture():
    assert os.path.getsize(os.path.join(GOLDEN, "pool_norm.npz")) <= 1 << 20
    f = npz("pool_norm.npz")
    E, hd, bn = f["w/spatial_embedding.weight"].shape[0], f["h"].shape[1], f["out"].shape[1]
    assert (E, hd, bn) == (8, 32, 24)
    assert np.diff(f["sse"], axis=1).ravel().tolist() == [2, 5, 20]
    net = O.PoolHiddenNet(E, hd, 64, bn, "relu", True)
    net.load_state_dict({k[2:]: T(f[k]) for k in f.files if k.startswith("w/")})
    assert float(net.mlp_pre_pool[4].weight.detach().min()) < 0 < float(net.mlp_pre_pool[4].bias.detach().abs().max())
    net.train()
    h = T(f["h"]).unsqueeze(0).requires_grad_(True)
    pos = T(f["pos"]).requires_grad_(True)
    y = net(h, T(f["sse"]), pos)
    close(y.detach(), f["out"])
    (y * T(f["dout"])).sum().backward()
    close(h.grad[0], f["dh"])
    close(pos.grad, f["dpos"])
    fl = grad_floor(f, "dw/")
    n = 0
    for k, p in net.named_parameters():
        if k in ZERO_BIASES:
            # mathematically zero: the reference's float32 value and the oracle's are both the rounding noise
            # of a sum that cancels (it moves with the summation order, e.g. the thread count), about 1e-6
            # against weight gradients of order 10
            assert float(np.abs(f["dw/" + k]).max()) <= 1e-3 * fl and float(p.grad.abs().max()) <= 1e-3 * fl, k
        else:
            close(p.grad, f["dw/" + k], floor=fl)
        n += 1
    assert n == 10
    for k, b in net.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(b) == int(f["buf/" + k]) == 3
        else:
            close(b, f["buf/" + k])
    net.eval()
    with torch.no_grad():
        close(net(h, T(f["sse"]), pos), f["out_eval"])
