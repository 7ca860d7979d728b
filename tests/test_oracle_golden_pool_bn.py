"""Pin the CPU oracle's PoolHiddenNet at bottleneck widths outside 8 / 16 / 32 /
48 / 64 against the reference's run (tests/golden/make_golden_pool_bn.py ->
pool_bn.npz), as test_oracle_golden.py does for pool.npz.  CPU only."""
import numpy as np
import pytest
import torch

from oracle import sgan_oracle as O

from test_oracle_golden import T, close, grad_floor, npz

NETS = {"a": (32, 72), "b": (48, 136)}


def pool_bn_net(f, tag, cls):
    """The fixture's net (weights stored as float16, exactly) as `cls`."""
    hd, bn = f[tag + "/h"].shape[1], f[tag + "/out"].shape[1]
    E = f[tag + "/w/spatial_embedding.weight"].shape[0]
    net = cls(E, hd, 64, bn, "relu", False)
    net.load_state_dict({k[len(tag) + 3:]: T(f[k].astype(np.float32)) for k in f.files if k.startswith(tag + "/w/")})
    return net


@pytest.mark.parametrize("tag", sorted(NETS))
def test_pool_bn_fixture(tag):
    f = npz("pool_bn.npz")
    assert (f[tag + "/h"].shape[1], f[tag + "/out"].shape[1]) == NETS[tag]
    assert np.diff(f[tag + "/sse"], axis=1).ravel().tolist() == [1, 2, 5, 20, 37]
    net = pool_bn_net(f, tag, O.PoolHiddenNet)
    h = T(f[tag + "/h"]).unsqueeze(0).requires_grad_(True)
    y = net(h, T(f[tag + "/sse"]), T(f[tag + "/pos"]))
    close(y.detach(), f[tag + "/out"])
    (y * T(f[tag + "/dout"])).sum().backward()
    close(h.grad[0], f[tag + "/dh"])
    n = 0
    for k, p in net.named_parameters():
        close(p.grad, f[tag + "/dw/" + k], floor=grad_floor(f, tag + "/dw/"))
        n += 1
    assert n == 6
