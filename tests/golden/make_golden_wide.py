"""Golden fixtures for scenes above 64 pedestrians, from the reference code.

    python tests/golden/make_golden_wide.py

pool_wide.npz     PoolHiddenNet forward + backward (the pooling nets of
                  build_models(0), tags g and d) on scenes of up to 200 peds;
                  pool.npz's keys but w/*, which are pool.npz's own.
gen_fwd_wide.npz  generator forward + every parameter gradient, gat and gcn
                  families, on a synthetic batch with 70- and 128-ped scenes
                  (weights: weights.npz, not stored again).

Max-pooling is discontinuous where the best and the second-best j nearly tie
and where the maximum sits near the ReLU's zero, so the pooling inputs are
accepted only when, on the reference's own pair values, no (i, c) has a
runner-up within MARGIN of the output range of its winner and no positive
maximum lies within MARGIN of the range from 0; and, for the same reason one
layer down, no hidden unit of a selected pair lies within KINK_MARGIN of its
ReLU's zero (pool_case).
"""
import copy
import os

import numpy as np
import torch

from make_golden import HERE, build_models, grad_arrays, label_patterns, save, sse_of, synth_batch, _gen_forward

POOL_WIDE_SIZES = [65, 1, 128, 20, 129, 64, 200, 2]
POOL_SEEDS = {"g": 11, "d": 12}
MARGIN = 1e-4
# |pre-activation| of every hidden unit of a selected pair, in float64.  Two fp32 evaluations that each
# deviate from the float64 value by at most d can disagree about a sign only below d, so the margin is
# (asserted in pool_case) at least twice the largest deviation of the reference's own fp32
# pre-activations from their float64 values among the units within 1e-3 of zero
KINK_MARGIN = 1e-5
GEN_WIDE_SIZES = [70, 3, 128, 20]
GEN_SEED = 9


def pool_case(net, hd, seed):
    """Inputs of one pooling case that satisfy the margin check, with one
    forward + backward of the reference's PoolHiddenNet on them.

    h and the positions are drawn from `seed`.  With some 30,000 (i, c)
    maxima per case, no seed passes the check outright (a margin of 1e-4
    expects a handful of near ties among that many), so the condition is met
    on the inputs directly: while some (i, c) fails, or a hidden unit of its
    selected pair sits within KINK_MARGIN of zero, the positions of exactly
    those peds i are drawn again (round r from seed + 1000 r) and everything
    is re-evaluated.  A deterministic function of `seed`."""
    torch.manual_seed(seed)
    B = sum(POOL_WIDE_SIZES)
    h = torch.randn(1, B, hd, requires_grad=True)
    pos = torch.rand(B, 2) * 15.0
    sse = sse_of(POOL_WIDE_SIZES)
    off = np.concatenate([[0], np.cumsum(POOL_WIDE_SIZES)])
    net64 = copy.deepcopy(net).double()
    for rnd in range(1, 400):
        pairs, pre, pre64 = [], [], []   # per scene: the (n^2, bn) pair values and the (n^2, 512) hidden pre-activations
        hooks = [net.mlp_pre_pool.register_forward_hook(lambda m, i, o: pairs.append(o.detach())),
                 net.mlp_pre_pool[0].register_forward_hook(lambda m, i, o: pre.append(o.detach())),
                 net64.mlp_pre_pool[0].register_forward_hook(lambda m, i, o: pre64.append(o.detach()))]
        y = net(h, sse, pos)
        with torch.no_grad():
            net64(h.detach().double(), sse, pos.double())
        for hk in hooks:
            hk.remove()
        rng = float(y.max() - y.min())
        bad = torch.zeros(B, dtype=torch.bool)
        gap, low, kink, dev = np.inf, np.inf, np.inf, 0.0
        for s, (n, z) in enumerate(zip(POOL_WIDE_SIZES, pairs)):
            z = z.view(n, n, -1)
            topv, topj = z.topk(min(2, n), dim=1)
            top = topv
            win = top[:, 0]
            # the hidden units of the selected pairs (i, argmax_j): the gradient is discontinuous where
            # one sits at its ReLU's zero, and fp32 roundings decide the side
            rows = (torch.arange(n)[:, None] * n + topj[:, 0]).reshape(-1)           # (i, c) -> i n + j*
            p64 = pre64[s][rows].view(n, -1, 512)
            sel = (win > 0)[:, :, None]
            close0 = sel & (p64.abs() < 1e-3)   # (the roundings that can decide a sign: those of values near 0)
            dev = max(dev, float(((pre[s][rows].view(n, -1, 512).double() - p64).abs() * close0).max()))
            near = (p64.abs() < KINK_MARGIN) & sel
            kink = min(kink, float(p64.abs()[sel.expand_as(p64)].min())) if sel.any() else kink
            live = win > 0   # an all-zero maximum carries no value and no gradient
            fail = live & (win < MARGIN * rng)
            if live.any():
                low = min(low, float(win[live].min()) / rng)
            if n > 1:
                d = top[:, 0] - top[:, 1]
                fail |= live & (d < MARGIN * rng)
                if live.any():
                    gap = min(gap, float(d[live].min()) / rng)
            bad[off[s]:off[s + 1]] = fail.any(1) | near.any(2).any(1)
        print("  seed %d round %d: %d peds fail; smallest top-two gap %.3e, smallest positive maximum %.3e "
              "(of the range), selected hidden unit nearest to 0 %.3e (fp32 deviation %.1e)"
              % (seed, rnd, int(bad.sum()), gap, low, kink, dev), flush=True)
        assert KINK_MARGIN >= 2 * dev, (KINK_MARGIN, dev)
        if not bad.any():
            break
        gen = torch.Generator().manual_seed(seed + 1000 * rnd)
        pos = torch.where(bad[:, None], torch.rand(B, 2, generator=gen) * 15.0, pos)
    else:
        raise AssertionError("margin check not met")
    torch.manual_seed(seed + 1)
    dy = torch.randn_like(y)
    net.zero_grad()
    (y * dy).sum().backward()
    out = {"h": h.detach().numpy()[0], "pos": pos.numpy(), "sse": sse.numpy(), "out": y.detach().numpy(),
           "dout": dy.numpy(), "dh": h.grad.numpy()[0]}
    for k, p in net.named_parameters():
        out["dw/" + k] = p.grad.numpy()
    return out


def fx_pool_wide():
    g, d = build_models(0)
    arrs = {}
    small = np.load(os.path.join(HERE, "pool.npz"))
    for tag, net, hd in (("g", g.pool_net, 32), ("d", d.pool_net, 48)):
        # the weights are pool.npz's w/* (both from build_models(0)): stored there only,
        # the two fixtures together would not fit the size limit of a committed file
        for k, p in net.named_parameters():
            assert np.array_equal(small[tag + "/w/" + k], p.detach().numpy()), k
        for k, v in pool_case(net, hd, POOL_SEEDS[tag]).items():
            arrs[tag + "/" + k] = v
    save("pool_wide.npz", arrs)


def fx_gen_wide():
    g, _ = build_models(0)
    b = synth_batch(GEN_WIDE_SIZES, seed=GEN_SEED)
    lab = torch.from_numpy(label_patterns(GEN_WIDE_SIZES, GEN_SEED)).float()
    b["obs_traj_g"] = lab.view(1, -1, 1).expand(b["obs_traj_g"].shape).contiguous()
    out = {k: b[k].numpy() for k in ("obs_traj", "obs_traj_rel", "obs_traj_g", "seq_start_end")}
    torch.manual_seed(77)
    noise = torch.randn(len(GEN_WIDE_SIZES), 8)
    out["noise"] = noise.numpy()
    for mode in ("gat", "gcn"):
        g.zero_grad()
        y = _gen_forward(g, b, noise, mode)
        torch.manual_seed(78)
        dy = torch.randn_like(y)
        (y * dy).sum().backward()
        out[mode + "/out"] = y.detach().numpy()
        out[mode + "/dout"] = dy.numpy()
        for k, v in grad_arrays(g, mode + "/dw/").items():
            out[k] = v
    save("gen_fwd_wide.npz", out)


if __name__ == "__main__":
    fx_pool_wide()
    fx_gen_wide()
