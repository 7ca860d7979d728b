"""The yardstick of the pooling net with dropout: the oracle's own
PoolHiddenNet (its layer order, its pair rows i*n + j) with the two nn.Dropout
of mlp_pre_pool replaced by a module that multiplies by the explicit scaled
mask of the kernels' contract (sgan.kernels.pool_dropout_keep_host).  Shared
by test_pool_dropout_abi.py (CPU) and test_gpu_pool_dropout.py.  Not a test
module."""
import functools

import numpy as np
import torch
from torch import nn

E_DIM, H_DIM = 16, 32
SIZES = ([1, 2, 5, 20, 37], [3, 70])
BNS = (8, 24, 65, 136)
PS = (0.25, 0.5)
SEED, OFFSET = 0x5EEDC0DE12345, 7      # the (seed, offset) of every kernel-level case


class MaskDropout(nn.Module):
    """Stands in for one nn.Dropout of mlp_pre_pool.  The oracle calls the MLP
    once per scene with rows i*n + j, so the module counts its calls: call k is
    scene k % S of pooling forward k // S, whose offset is offset0 + k // S
    (one DropoutRng.next() per forward)."""

    def __init__(self, p, seed, offset0, site, sizes):
        super().__init__()
        self.p, self.seed, self.offset0, self.site = p, seed, offset0, site
        self.sizes = list(sizes)
        self.starts = np.concatenate([[0], np.cumsum(sizes)])
        self.calls = 0

    def forward(self, x):
        from sgan import kernels as K
        k, S = self.calls, len(self.sizes)
        self.calls += 1
        s, off = k % S, self.offset0 + k // S
        n, o = self.sizes[s], int(self.starts[s])
        assert x.shape[0] == n * n, (x.shape, n)
        keep = K.pool_dropout_keep_host(self.p, self.seed, off, self.site, np.arange(o, o + n), np.arange(n),
                                        np.arange(x.shape[1]))
        _, scale = K.dropout_thr_scale_host(self.p)      # the float32 scale the kernels multiply by
        m = torch.from_numpy(np.where(keep, np.float64(scale), 0.0)).reshape(n * n, -1)
        return x * m.to(device=x.device, dtype=x.dtype)


def install_masks(net, p, seed, offset0, sizes):
    """Replace the nn.Dropout modules of net.mlp_pre_pool (an oracle
    PoolHiddenNet built with dropout=p) by MaskDropout -> the two modules."""
    from sgan import kernels as K
    idx = [i for i, m in enumerate(net.mlp_pre_pool) if isinstance(m, nn.Dropout)]
    assert len(idx) == 2 and isinstance(net.mlp_pre_pool[idx[0] + 1], nn.Linear), idx
    mods = []
    for i, site in zip(idx, (K.POOL_DROP_SITE_HIDDEN, K.POOL_DROP_SITE_OUT)):
        net.mlp_pre_pool[i] = MaskDropout(p, seed, offset0, site, sizes)
        mods.append(net.mlp_pre_pool[i])
    return mods


def sse_of(sizes):
    off = np.concatenate([[0], np.cumsum(sizes)])
    return torch.from_numpy(np.stack([off[:-1], off[1:]], 1).astype(np.int64))


@functools.lru_cache(maxsize=None)
def case(bn, sizes_id, p):
    """One kernel-level case, computed once: the float64 yardstick's forward
    (out, the per-scene pair values), its argmax statistics and its autograd
    gradients for a fixed dout.  Nothing in the returned dict is modified by
    the tests."""
    # the seed: the first of a fixed sequence at which the yardstick ALONE has no undecided argmax (no entry
    # with out > 0 and a top-two gap within 1e-5 of the range) -- a float32 forward that picks the other ped
    # of such a pair is right about out and still routes that entry's gradient elsewhere, which the backward
    # comparison at rtol 1e-4 would read as an error.  A property of the float64 numbers only.
    c = None
    for attempt in range(16):
        c = _case(bn, sizes_id, p, 1000 * bn + 10 * sizes_id + int(p * 100) + 7919 * attempt)
        if c["excluded"] == 0:
            break
    return c


def _case(bn, sizes_id, p, seed):
    from oracle import sgan_oracle as O
    sizes = list(SIZES[sizes_id])
    torch.manual_seed(seed)
    net = O.PoolHiddenNet(E_DIM, H_DIM, 64, bn, "relu", False, dropout=p).double()
    install_masks(net, p, SEED, OFFSET, sizes)
    B = sum(sizes)
    h = torch.randn(1, B, H_DIM, dtype=torch.float64, requires_grad=True)
    pos = (torch.rand(B, 2, dtype=torch.float64) * 15).requires_grad_(True)
    dout = torch.randn(B, bn, dtype=torch.float64)
    zs = []
    hook = net.mlp_pre_pool.register_forward_hook(lambda m, i, o: zs.append(o.detach()))
    ref = net(h, sse_of(sizes), pos)
    hook.remove()
    (ref * dout).sum().backward()
    ref = ref.detach()
    off = np.concatenate([[0], np.cumsum(sizes)])
    rng = float(ref.max() - ref.min())
    best, sure = [], []
    for n, z in zip(sizes, zs):
        z = z.view(n, n, bn)
        if n > 1:
            top = z.topk(2, dim=1)
            sure.append((top[0][:, 0] - top[0][:, 1]) > 1e-5 * rng)
            best.append(top[1][:, 0])
        else:
            sure.append(torch.ones(1, bn, dtype=torch.bool))
            best.append(torch.zeros(1, bn, dtype=torch.long))
    best = torch.cat([b + int(o) for b, o in zip(best, off[:-1])], 0)
    sure = torch.cat(sure, 0)
    live = ref > 0
    return dict(sizes=sizes, bn=bn, p=p, seed=seed, net=net, h=h.detach(), pos=pos.detach(), dout=dout, ref=ref,
                best=best, compare=live & sure, excluded=int((live & ~sure).sum()), total=B * bn, live=int(live.sum()),
                dh=h.grad[0].clone(), dpos=pos.grad.clone(),
                dw={k: v.grad.clone() for k, v in net.named_parameters()})


def float32_net(c, cls, dropout):
    """sgan.models.PoolHiddenNet (cls) with the case's weights; dropout=0: the
    keys of the second Linear move from .3. to .2."""
    net = cls(E_DIM, H_DIM, 64, c["bn"], "relu", False, dropout=dropout)
    sd = {k: v.float() for k, v in c["net"].state_dict().items()}
    if not dropout:
        sd = {k.replace("mlp_pre_pool.3.", "mlp_pre_pool.2."): v for k, v in sd.items()}
    net.load_state_dict(sd)
    return net


class _TakeLink(torch.autograd.Function):
    """Identity on h whose backward adds the gradient a GradLink carries (what
    the pooling op's backward does with the generator's link)."""

    @staticmethod
    def forward(ctx, h, link):
        ctx.link = link
        return h.view_as(h)

    @staticmethod
    def backward(ctx, g):
        base = ctx.link.take()
        return (g if base is None else g + base.view_as(g)), None


def torch_pool_net(src, p, seed, offset0, sizes):
    """A float32 torch restatement of a sgan.models.PoolHiddenNet built with
    dropout=p (the oracle's module, the explicit masks installed), with the
    same parameter names and values, callable the way the generator and the
    decoder call their pool_net."""
    from oracle import sgan_oracle as O

    class TorchPool(O.PoolHiddenNet):
        dropout = p

        def fused_ok(self):
            return False

        def forward(self, h_states, seq_start_end, end_pos, scenes=None, link=None, U=None, dh_in_lstm=False,
                    pos_grad=False):
            assert U is None
            if link is not None:
                h_states = _TakeLink.apply(h_states, link)
            return super().forward(h_states, seq_start_end, end_pos)

    net = TorchPool(src.embedding_dim, src.h_dim, 64, src.bottleneck_dim, "relu", False, dropout=p)
    net.load_state_dict(src.state_dict())
    net = net.to(next(src.parameters()).device)
    net.masks = install_masks(net, p, seed, offset0, sizes)
    return net
