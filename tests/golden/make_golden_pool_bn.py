"""Golden fixture for pooling widths outside 8 / 16 / 32 / 48 / 64, from the
reference code.

    python tests/golden/make_golden_pool_bn.py

pool_bn.npz   PoolHiddenNet forward + backward of two stand-alone nets,
              tag a: (h_dim 32, bottleneck_dim 72), tag b: (h_dim 48,
              bottleneck_dim 136) -- two and three column tiles of 64, the
              last one partial -- embedding_dim 8, on scenes of 1 .. 37
              peds; pool.npz's keys (h, pos, sse, out, dout, dh, w/*, dw/*).

The nets are the reference's PoolHiddenNet under scripts/train.py's
init_weights.  Their weights are then rounded to the nearest float16 value and
stored as float16 (exactly: the reference ran on the rounded weights), which
is what keeps the file within the size limit of a committed file, 1 MiB =
1,048,576 bytes (it is 1,021,530 bytes; fx_pool_bn asserts the limit); a
reader converts them to float32.  The inputs meet make_golden_wide.pool_case's margin
check (no near tie of the maximum, no selected hidden unit at its ReLU's zero).
"""
import os

import numpy as np
import torch

import make_golden_wide as W
from make_golden import HERE, M, TR, save

POOL_BN_SIZES = [1, 2, 5, 20, 37]
# tag -> (h_dim, bottleneck_dim, weight seed, input seed).  pool_case redraws positions only, which cannot move
# a self pair (i, i) or the one-ped scene off a ReLU's zero: the input seed is the first of weight seed + 100,
# + 200, .. whose draw of h passes the check
POOL_BN_NETS = {"a": (32, 72, 21, 121), "b": (48, 136, 22, 222)}
EMBEDDING_DIM = 8    # (16 elsewhere: the narrower first layer keeps the file within the size limit)


def fx_pool_bn():
    W.POOL_WIDE_SIZES = POOL_BN_SIZES    # pool_case draws and checks the scenes of this list
    arrs = {}
    for tag, (hd, bn, seed, case_seed) in POOL_BN_NETS.items():
        torch.manual_seed(seed)
        net = M.PoolHiddenNet(embedding_dim=EMBEDDING_DIM, h_dim=hd, mlp_dim=64, bottleneck_dim=bn, activation="relu",
                              batch_norm=False)
        net.apply(TR.init_weights)
        net.train()
        with torch.no_grad():
            for p in net.parameters():
                p.copy_(p.half().float())
        for k, v in W.pool_case(net, hd, case_seed).items():
            arrs[tag + "/" + k] = v
        for k, p in net.named_parameters():
            w16 = p.detach().numpy().astype(np.float16)
            assert np.array_equal(w16.astype(np.float32), p.detach().numpy()), k
            arrs[tag + "/w/" + k] = w16
    save("pool_bn.npz", arrs)
    assert os.path.getsize(os.path.join(HERE, "pool_bn.npz")) <= 1 << 20


if __name__ == "__main__":
    fx_pool_bn()
