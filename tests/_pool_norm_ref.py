"""The yardstick of the pooling net with batch norm: the oracle's own
PoolHiddenNet(E 16, H 32, 64, bn, "relu", True) -- its layer order, its pair
rows i*n + j, nn.BatchNorm1d per scene -- with gamma drawn around 1 (some
entries negative) and beta non-zero.  Computed once per case in float64 (the
reference) and in float32 on the CPU (the measured float32 error the
tolerances are built from).  Shared by test_pool_norm_abi.py (CPU) and
test_gpu_pool_norm.py.  Not a test module."""
import contextlib
import functools

import numpy as np
import torch

E_DIM, H_DIM = 16, 32
# 2, 3: more scenes than any kernel has workgroups, so every workgroup walks several scenes (its slab row, its LDS
# and its running sums carried from scene to scene).  The dense backward has 8 .. 128 workgroups (128 at bn 8, 31
# at bn 1024), the finish 32, the forward at most min(4 CUs / column tiles, S) per column tile: 1024 at bn 8 on
# 256 CUs, 64 at bn 1024.  1100 scenes of 3 .. 5 peds at bn 8 (every kernel's scene loop); 40 scenes of 2 peds at
# bn 1024 (the backward's and the finish's: the largest batch of that width that is decided early in the seed
# sequence -- 45 K live entries -- so its forward's loop, which starts at 65 scenes, is covered by the first case).
SIZES = ([2, 3, 5, 20, 37], [3, 70], [3, 4, 5, 3, 4] * 220, [2] * 40)
MANY_CASES = ((8, 2), (1024, 3))
BNS = (8, 24, 65, 136)
# (136, [3, 70]): no decided seed within the sequence's first attempts (CPU probe) -- not used
CASES = tuple((bn, sid) for bn in BNS for sid in (0, 1) if not (bn == 136 and sid == 1))
MAX_SEEDS = 16
FLOOR = 16 * 2.0 ** -23


@contextlib.contextmanager
def one_thread():
    """Every float32 CPU run that a tolerance is measured from runs on one
    thread: torch's float32 sums depend on how the host splits them over
    threads, and e32 with them (seen: 4 e32 = 6.6e-6 at 4 or 16 threads
    against 8.1e-6 at one for (136, [2, 3, 5, 20, 37])'s first-layer weight
    gradient) -- a tolerance must not depend on the host's thread count."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(threads)


def sse_of(sizes):
    off = np.concatenate([[0], np.cumsum(sizes)])
    return torch.from_numpy(np.stack([off[:-1], off[1:]], 1).astype(np.int64))


def build_net(bn, seed, dtype=torch.float64):
    """The oracle's net with the case's weights (gamma around 1 with negative
    entries, beta non-zero)."""
    from oracle import sgan_oracle as O
    torch.manual_seed(seed)
    net = O.PoolHiddenNet(E_DIM, H_DIM, 64, bn, "relu", True).double()
    with torch.no_grad():
        for m in net.mlp_pre_pool:
            if isinstance(m, torch.nn.BatchNorm1d):
                g = 1.0 + 0.3 * torch.randn(m.num_features, dtype=torch.float64)
                g[::5] = -g[::5]
                m.weight.copy_(g)
                m.bias.copy_(0.3 * torch.randn(m.num_features, dtype=torch.float64))
    return net.to(dtype)


def norms_of(net):
    return [m for m in net.mlp_pre_pool if isinstance(m, torch.nn.BatchNorm1d)]


def _run(net, h, pos, dout, sizes):
    """train() forward, backward, a second forward; -> dict of arrays (the
    model's dtype) plus the per-scene outputs of mlp_pre_pool."""
    net.train()
    h = h.clone().requires_grad_(True)
    pos = pos.clone().requires_grad_(True)
    zs = []
    hook = net.mlp_pre_pool.register_forward_hook(lambda m, i, o: zs.append(o.detach()))
    out = net(h, sse_of(sizes), pos)
    hook.remove()
    n1, n2 = norms_of(net)
    r = {"out": out.detach().clone()}
    for tag, m in (("1", n1), ("2", n2)):
        r["rm%s_a" % tag], r["rv%s_a" % tag] = m.running_mean.clone(), m.running_var.clone()
    r["nbt_a"] = int(n1.num_batches_tracked)
    (out * dout).sum().backward()
    with torch.no_grad():
        net(h, sse_of(sizes), pos)
    for tag, m in (("1", n1), ("2", n2)):
        r["rm%s_b" % tag], r["rv%s_b" % tag] = m.running_mean.clone(), m.running_var.clone()
    r["nbt_b"] = int(n1.num_batches_tracked)
    r["dh"], r["dpos"] = h.grad[0].clone(), pos.grad.clone()
    for k, v in net.named_parameters():
        r["dw." + k] = v.grad.clone()
    net.eval()
    with torch.no_grad():
        r["out_eval"] = net(h, sse_of(sizes), pos).clone()
    return r, zs


ZERO_BIASES = ("spatial_embedding.bias", "mlp_pre_pool.0.bias", "mlp_pre_pool.3.bias")


def _case(bn, sizes_id, seed):
    sizes = list(SIZES[sizes_id])
    net64 = build_net(bn, seed)
    state0 = {k: v.clone() for k, v in net64.state_dict().items()}
    B = sum(sizes)
    h = torch.randn(1, B, H_DIM, dtype=torch.float64)
    pos = torch.rand(B, 2, dtype=torch.float64) * 15
    dout = torch.randn(B, bn, dtype=torch.float64)
    r64, zs = _run(net64, h, pos, dout, sizes)
    ref = r64["out"]
    off = np.concatenate([[0], np.cumsum(sizes)])
    rng = float(ref.max() - ref.min())
    best, sure = [], []
    for n, z in zip(sizes, zs):
        top = z.view(n, n, bn).topk(2, dim=1)
        sure.append((top[0][:, 0] - top[0][:, 1]) > 1e-5 * rng)
        best.append(top[1][:, 0])
    best = torch.cat([b + int(o) for b, o in zip(best, off[:-1])], 0)
    sure = torch.cat(sure, 0)
    live = ref > 0
    excluded = int((live & ~sure).sum())
    c = dict(sizes=sizes, bn=bn, seed=seed, state0=state0, h=h, pos=pos, dout=dout, r64=r64, best=best,
             compare=live & sure, excluded=excluded, live=int(live.sum()))
    if excluded:
        return c       # not used: the float32 oracle is not run for it
    net32 = build_net(bn, seed, torch.float32)
    net32.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in state0.items()})
    with one_thread():
        r32, _ = _run(net32, h.float(), pos.float(), dout.float(), sizes)
    e32, tol = {}, {}
    for k, v in r64.items():
        if not torch.is_tensor(v):
            continue
        scale = float(v.abs().max())
        e32[k] = float((r32[k].double() - v).abs().max()) / scale if scale > 0 else 0.0
        tol[k] = max(4.0 * e32[k], FLOOR)
    c.update(e32=e32, tol=tol)
    return c


@functools.lru_cache(maxsize=None)
def case(bn, sizes_id):
    """One kernel-level case, computed once and never modified by the tests:
    the first seed of a fixed sequence (at most MAX_SEEDS) at which the
    float64 numbers ALONE have no live entry whose top-two gap is within 1e-5
    of the range (such an entry may pick the other ped in float32, rightly,
    and route its gradient elsewhere)."""
    c = None
    for attempt in range(MAX_SEEDS):
        c = _case(bn, sizes_id, 1000 * bn + 10 * sizes_id + 7919 * attempt)
        if c["excluded"] == 0:
            break
    return c


def rel_err(got, ref):
    """max |got - ref| relative to max |ref| (float64)."""
    ref = ref.double()
    scale = float(ref.abs().max())
    d = float((got.detach().double().cpu() - ref).abs().max())
    return d / scale if scale > 0 else d


def float32_net(c, cls, **kw):
    """sgan.models.PoolHiddenNet (cls) with the case's initial state."""
    net = cls(E_DIM, H_DIM, 64, c["bn"], "relu", True, **kw)
    net.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in c["state0"].items()})
    return net
