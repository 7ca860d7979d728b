"""Social pooling for scenes above 64 pedestrians (sgg_pool_fwd_wide /
sgg_pool_bwd_wide): against the LDS-resident kernels where both apply, the
reference's fixtures, the float64 oracle, and through the generators, a
training step and evaluation."""
import random

import numpy as np
import pytest
import torch

from conftest import RecordingAdam
from test_gpu_parity import DEV, T, build_models, close, grad_floor, npz

pytestmark = pytest.mark.gpu


def _scene_index(sizes):
    from sgan.scene import SceneIndex
    return SceneIndex(np.concatenate([[0], np.cumsum(sizes)]), DEV)


def _pool_operands(B, bn, seed):
    gen = torch.Generator().manual_seed(seed)
    U = torch.randn(B, 512, generator=gen) * 0.3
    pos = torch.rand(B, 2, generator=gen) * 15
    A = torch.randn(512, 2, generator=gen) * 0.3
    W2 = torch.randn(bn, 512, generator=gen) * 0.05
    b2 = torch.randn(bn, generator=gen) * 0.1
    return U, pos, A, W2, b2


def _fwd(lib, N, sc, ops, bn, wide, target=None):
    """target: the wide plan's chunk target; a small one gives chunks of up to
    64 rows, which a workgroup walks in several passes per j-tile."""
    U, pos, A, W2, b2 = ops
    B = U.shape[0]
    out = torch.empty(B, bn, device=DEV)
    am = torch.empty(B, bn, device=DEV, dtype=torch.int32)
    if wide:
        chunks, nchunks, max_rows, gpw = sc.pool_plan(bn, target_chunks=target, wide=True)
        if target is not None:   # the plan under test has chunks of several passes per j-tile
            assert max_rows * min(sc.max_n, 64) > 64 * gpw, (max_rows, gpw)
        N.check(lib.sgg_pool_fwd_wide(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2), N.ptr(b2), N.ptr(sc.scene_off),
                                      N.ptr(chunks), nchunks, max_rows, gpw, B, bn, sc.max_n, N.ptr(out), N.ptr(am),
                                      N.stream_ptr()), "sgg_pool_fwd_wide")
    else:
        chunks, nchunks, max_rows, gpw = sc.pool_plan(bn)
        N.check(lib.sgg_pool_fwd(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2), N.ptr(b2), N.ptr(sc.scene_off),
                                 N.ptr(chunks), nchunks, max_rows, gpw, B, bn, sc.max_n, N.ptr(out), N.ptr(am),
                                 None, N.stream_ptr()), "sgg_pool_fwd")
    return out, am


def _bwd(lib, N, sc, ops, bn, out, am, dout, wide):
    """-> dU, (dW2, dA, db2) summed over the slab rows in float64."""
    U, pos, A, W2, _ = ops
    B = U.shape[0]
    P = bn * 512 + 1024 + bn
    dU = torch.empty(B, 512, device=DEV)
    if wide:
        part = torch.empty(lib.sgg_pool_bwd_wide_grid(sc.S, sc.max_n), P, device=DEV)
        N.check(lib.sgg_pool_bwd_wide(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2), N.ptr(out), N.ptr(am), N.ptr(dout),
                                      N.ptr(sc.scene_off), sc.S, B, bn, sc.max_n, N.ptr(dU), N.ptr(part),
                                      N.stream_ptr()), "sgg_pool_bwd_wide")
    else:
        part = torch.empty(lib.sgg_pool_bwd_grid(sc.S), P, device=DEV)
        N.check(lib.sgg_pool_bwd(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2), N.ptr(out), N.ptr(am), N.ptr(dout),
                                 N.ptr(sc.scene_off), sc.S, B, bn, sc.max_n, N.ptr(dU), N.ptr(part),
                                 N.stream_ptr()), "sgg_pool_bwd")
    tot = part.double().sum(0).cpu()
    return dU, (tot[:bn * 512], tot[bn * 512:bn * 512 + 1024], tot[bn * 512 + 1024:])


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("target", [None, 16, 1])
@pytest.mark.parametrize("bn", [8, 48])
def test_wide_equals_resident_on_small_scenes(bn, target, monkeypatch):
    """Tiling does not change a pair's value: on scenes of <= 64 peds the wide
    forward's out and argmax and the wide backward's dU are bitwise the
    resident kernels' (fp32 MFMA forms: the split-bf16 forward, the default
    for bn 32 / 48, is off here); the reduced [dW2 | dA | db2] agree to 1e-5
    of each tensor's max (another slab partition, so another summation
    order).  target: the default plan (chunks of gpw rows, one pass per
    j-tile) and plans with chunks of up to 16 and up to 64 rows, which run
    in up to 8 / 32 passes (bn 8) or 4 / 16 passes (bn 48)."""
    from sgan import _native as N
    monkeypatch.setenv("SGG_POOL_X3", "0")
    lib = N.load()
    sizes = [1, 2, 5, 20, 57, 64, 3, 20]
    sc = _scene_index(sizes)
    ops = tuple(t.to(DEV) for t in _pool_operands(sum(sizes), bn, 100 + bn))
    out_r, am_r = _fwd(lib, N, sc, ops, bn, wide=False)
    out_w, am_w = _fwd(lib, N, sc, ops, bn, wide=True, target=target)
    assert torch.equal(out_r, out_w) and torch.equal(am_r, am_w)
    dout = torch.randn(sum(sizes), bn, generator=torch.Generator().manual_seed(5)).to(DEV)
    dU_r, sums_r = _bwd(lib, N, sc, ops, bn, out_r, am_r, dout, wide=False)
    dU_w, sums_w = _bwd(lib, N, sc, ops, bn, out_r, am_r, dout, wide=True)
    assert torch.equal(dU_r, dU_w)
    for name, a, b in zip(("dW2", "dA", "db2"), sums_w, sums_r):
        close(a, b.numpy(), rtol=1e-5, what="wide " + name)


# 2, 5 ------------------------------------------------------------------------
def _pool_net(tag):
    from sgan.models import PoolHiddenNet
    f, w = npz("pool_wide.npz"), npz("pool.npz")   # the weights are pool.npz's (the same nets)
    hd, bn = f[tag + "/h"].shape[1], f[tag + "/out"].shape[1]
    net = PoolHiddenNet(16, hd, 64, bn, "relu", False).to(DEV)
    net.load_state_dict({k[len(tag) + 3:]: torch.from_numpy(w[k]) for k in w.files if k.startswith(tag + "/w/")})
    return f, net


@pytest.mark.parametrize("target", [None, 1])
@pytest.mark.parametrize("tag", ["g", "d"])
def test_pool_wide_vs_reference_fixture(tag, target):
    """The reference's PoolHiddenNet on scenes of 65 .. 200 peds (and small
    ones in the same batch), test_pool_vs_reference_fixture's tolerances.
    target 1: the forward on chunks of up to 64 rows (several passes per
    j-tile, several j-tiles)."""
    from sgan.models import scene_index
    f, net = _pool_net(tag)
    h = T(f[tag + "/h"]).unsqueeze(0).requires_grad_(True)
    sse = T(f[tag + "/sse"])
    sc = scene_index(sse, h.device)
    if target is not None:
        sc.POOL_WIDE_TARGET_CHUNKS = target
        assert sc.pool_plan(f[tag + "/out"].shape[1], wide=True)[2] == 64
    y = net(h, sse, T(f[tag + "/pos"]), scenes=sc)
    close(y, f[tag + "/out"], rtol=1e-5, what="pool out")
    (y * T(f[tag + "/dout"])).sum().backward()
    close(h.grad[0], f[tag + "/dh"], rtol=1e-4, what="pool dh")
    fl = grad_floor(f, tag + "/dw/")
    for k, p in net.named_parameters():
        close(p.grad, f[tag + "/dw/" + k], rtol=1e-4, floor=fl, what="pool d" + k)


@pytest.mark.parametrize("tag", ["g", "d"])
def test_pool_wide_frozen_weights_same_dh(tag):
    """part = NULL (frozen weights): the same dh, bitwise, as with weight gradients."""
    f, net = _pool_net(tag)
    res = []
    for frozen in (False, True):
        net.requires_grad_(not frozen)
        h = T(f[tag + "/h"]).unsqueeze(0).requires_grad_(True)
        y = net(h, T(f[tag + "/sse"]), T(f[tag + "/pos"]))
        (y * T(f[tag + "/dout"])).sum().backward()
        res.append(h.grad.clone())
    assert all(p.grad is not None for p in net.parameters())   # (from the first pass)
    assert torch.equal(res[0], res[1])


# 3 ---------------------------------------------------------------------------
# checked on the CPU: with this seed the float64 oracle has at most 0.2 % of its entries within the
# 1e-5 top-two gap at every size below (31 and 32 leave all-zero columns at 193 / 65 peds)
_EDGE_SEED = 33


def _edge_case(n):
    """Single scene of n peds through the oracle's PoolHiddenNet in float64:
    (net64, h, pos, sse, z) with z the (n, n, bn) pair values."""
    from oracle import sgan_oracle as O
    torch.manual_seed(_EDGE_SEED + n)
    net = O.PoolHiddenNet(16, 32, 64, 8, "relu", False).double()
    h = torch.randn(1, n, 32, dtype=torch.float64)
    pos = torch.rand(n, 2, dtype=torch.float64) * 15
    sse = torch.tensor([[0, n]])
    zs = []
    hook = net.mlp_pre_pool.register_forward_hook(lambda m, i, o: zs.append(o.detach()))
    with torch.no_grad():
        out = net(h, sse, pos)
    hook.remove()
    return net, h, pos, sse, out, zs[0].view(n, n, -1)


@pytest.mark.parametrize("target", [None, 16, 1])
@pytest.mark.parametrize("n", [65, 127, 128, 129, 193])
def test_pool_wide_tile_edges_vs_float64_oracle(n, target):
    """One scene around the 64-ped j-tile edges, bn 8, forward, against the
    oracle in float64: out within 1e-5 of its max; argmax equal to the
    float64 argmax wherever the float64 top-two gap exceeds 1e-5 of the range
    (at most 1 % of the entries may be excluded that way).  target: the
    default plan (one pass per j-tile) and plans with chunks of 4 .. 16 and
    of up to 64 rows (several passes per tile, the last tile a partial one)."""
    from sgan.models import PoolHiddenNet
    net64, h, pos, sse, ref, z = _edge_case(n)
    net = PoolHiddenNet(16, 32, 64, 8, "relu", False)
    net.load_state_dict({k: v.float() for k, v in net64.state_dict().items()})
    net = net.to(DEV)
    from sgan import kernels as K
    sc = _scene_index([n])
    if target is not None:
        sc.POOL_WIDE_TARGET_CHUNKS = target
        assert sc.pool_plan(8, wide=True)[2] > 2    # more than gpw rows: several passes per full j-tile
    l1, l2, emb = net.mlp_pre_pool[0], net.mlp_pre_pool[2], net.spatial_embedding
    with torch.no_grad():
        out, am = K._Pool.apply(h.float().to(DEV).view(n, 32), pos.float().to(DEV), l1.weight, emb.weight, emb.bias,
                                l1.bias, l2.weight, l2.bias, sc, None, None)
    close(out, ref.numpy(), rtol=1e-5, what="wide out n=%d" % n)
    top = z.topk(2, dim=1)
    rng = float(ref.max() - ref.min())
    sure = (top[0][:, 0] - top[0][:, 1]) > 1e-5 * rng
    assert float((~sure).float().mean()) <= 0.01, float((~sure).float().mean())
    assert torch.equal(am.cpu().long()[sure], top[1][:, 0][sure])


# 4 ---------------------------------------------------------------------------
def test_pool_wide_upper_bound():
    """A 1024-ped scene (the bound) next to a 3-ped one, bn 8, forward,
    against a torch CPU evaluation in row blocks of 64 i; one more ped raises
    a ValueError from Python before any launch."""
    from sgan import _native as N
    from sgan import kernels as K
    from sgan.models import PoolHiddenNet
    lib = N.load()
    sizes = [1024, 3]
    sc = _scene_index(sizes)
    U, pos, A, W2, b2 = _pool_operands(sum(sizes), 8, 1024)
    out, _ = _fwd(lib, N, sc, tuple(t.to(DEV) for t in (U, pos, A, W2, b2)), 8, wide=True)
    ref = torch.empty(sum(sizes), 8, dtype=torch.float64)
    Ud, pd, Ad, Wd, bd = (t.double() for t in (U, pos, A, W2, b2))
    for s0, s1 in zip(sc.host_off[:-1], sc.host_off[1:]):
        for i0 in range(int(s0), int(s1), 64):
            i1 = min(i0 + 64, int(s1))
            r = pd[s0:s1].unsqueeze(0) - pd[i0:i1].unsqueeze(1)            # [i, j] = p_j - p_i
            hid = torch.relu(Ud[s0:s1].unsqueeze(0) + r @ Ad.t())          # (i, j, 512)
            ref[i0:i1] = torch.relu(hid @ Wd.t() + bd).max(1)[0]
    close(out, ref.numpy(), rtol=1e-5, what="wide out at 1024 peds")

    net = PoolHiddenNet(16, 32, 64, 8, "relu", False).to(DEV)
    big = _scene_index([1025])
    with pytest.raises(ValueError, match="1024"):
        net(torch.zeros(1, 1025, 32, device=DEV), None, torch.zeros(1025, 2, device=DEV), scenes=big)
    with pytest.raises(ValueError, match="1024"):
        K.pool_is_wide(big)


def test_pool_wide_bn64_full_chunks():
    """The largest LDS plan of the forward: bn 64 with chunks of 64 rows (keys
    64 x 64 x 8 B, 77 KiB in all) on scenes of 64, 130 and 3 peds, against a
    torch CPU evaluation in float64; the backward's largest too (96 KiB)."""
    from sgan import _native as N
    lib = N.load()
    sizes = [64, 130, 3]
    sc = _scene_index(sizes)
    ops = _pool_operands(sum(sizes), 64, 64)
    dev_ops = tuple(t.to(DEV) for t in ops)
    out, am = _fwd(lib, N, sc, dev_ops, 64, wide=True, target=1)
    assert sc.pool_plan(64, target_chunks=1, wide=True)[2] == 64
    Ud, pd, Ad, Wd, bd = (t.double() for t in ops)
    ref = torch.empty(sum(sizes), 64, dtype=torch.float64)
    for s0, s1 in zip(sc.host_off[:-1], sc.host_off[1:]):
        r = pd[s0:s1].unsqueeze(0) - pd[s0:s1].unsqueeze(1)            # [i, j] = p_j - p_i
        ref[s0:s1] = torch.relu(torch.relu(Ud[s0:s1].unsqueeze(0) + r @ Ad.t()) @ Wd.t() + bd).max(1)[0]
    close(out, ref.numpy(), rtol=1e-5, what="wide out bn 64")
    # backward at the forward's own argmax: dU against the same sum in float64
    dout = torch.randn(sum(sizes), 64, generator=torch.Generator().manual_seed(6))
    dU, _ = _bwd(lib, N, sc, dev_ops, 64, out, am, dout.to(DEV), wide=True)
    amc, outc = am.cpu().long(), out.cpu()
    dref = torch.zeros(sum(sizes), 512, dtype=torch.float64)
    g = torch.where(outc > 0, dout, torch.zeros_like(dout)).double()
    ii = torch.arange(sum(sizes))[:, None].expand(-1, 64)
    pre = Ud[amc] + (pd[amc] - pd[ii]) @ Ad.t()                          # (i, c, 512)
    dref.index_put_((amc.reshape(-1),), ((pre > 0) * g[:, :, None] * Wd[None]).reshape(-1, 512), accumulate=True)
    # (a hidden unit within fp32 rounding of its ReLU's zero may fall on either side: the dU cells such a
    # unit feeds are left out -- a handful of the 100,000)
    edge = torch.zeros(sum(sizes), 512, dtype=torch.float64)
    edge.index_put_((amc.reshape(-1),), ((pre.abs() < 1e-5) & (g != 0)[:, :, None]).double().reshape(-1, 512),
                    accumulate=True)
    keep = edge == 0
    assert float((~keep).double().mean()) < 1e-3
    scale = float(dref.abs().max())
    err = float(((dU.cpu().double() - dref).abs() * keep).max()) / scale
    assert err <= 1e-4, err


# 6 ---------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["gat", "gcn"])
def test_generator_wide_vs_reference_fixture(graph):
    """The gat and gcn generators on a batch with 70- and 128-ped scenes,
    test_generator_vs_reference_fixture's tolerances."""
    g, _ = build_models(graph)
    f = npz("gen_fwd_wide.npz")
    y = g(T(f["obs_traj"]), T(f["obs_traj_rel"]), T(f["seq_start_end"]), T(f["obs_traj_g"]), user_noise=T(f["noise"]))
    close(y, f[graph + "/out"], rtol=1e-4, what="G out")
    (y * T(f[graph + "/dout"])).sum().backward()
    fl = grad_floor(f, graph + "/dw/")
    for k, p in g.named_parameters():
        key = graph + "/dw/" + k
        if key in f.files:
            close(p.grad, f[key], rtol=1e-3, floor=fl, what="G d" + k)


# 7 ---------------------------------------------------------------------------
def test_gcn_wide_train_step_vs_oracle():
    """One GanTrainer iteration (D-step + G-step, best_k 20) of the gcn
    family on scenes of 70 and 100 peds against the oracle's
    reference-formulation steps from the same seeds: losses, the gradients
    each optimizer step consumed, weights."""
    from oracle import sgan_oracle as O
    from sgan.data.synthetic import synthetic_batch
    from sgan.scene import SceneIndex
    from sgan.train_step import GanTrainer
    from test_gpu_configs import reference_gd
    g, d = reference_gd("gcn")
    og, od = O.build_default("gcn")
    og.load_state_dict({k: v.detach().cpu() for k, v in g.state_dict().items()})
    od.load_state_dict({k: v.detach().cpu() for k, v in d.state_dict().items()})
    oog = RecordingAdam.make(og.named_parameters(), lr=1e-4)
    ood = RecordingAdam.make(od.named_parameters(), lr=1e-3)
    tr = GanTrainer(g, d)
    b = synthetic_batch([70, 5, 100, 20], seed=700)
    torch.manual_seed(21)
    random.seed(21)
    rld = O.discriminator_step(O.Args, b, og, od, ood)
    rlg = O.generator_step(O.Args, b, og, od, oog)
    rgd, rgg = dict(ood.rec[-1]), dict(oog.rec[-1])
    torch.manual_seed(21)
    random.seed(21)
    bd = [t.to(DEV) for t in b]
    sc = SceneIndex.from_seq_start_end(b[-1], DEV)
    ld, lg = tr.step(bd, sc)
    for k, v in list(ld.items()) + list(lg.items()):
        r = (rld if k.startswith("D") else rlg)[k]
        assert abs(float(v) - r) <= 1e-4 * max(1.0, abs(r)), (k, float(v), r)
    for mod, rg in ((d, rgd), (g, rgg)):
        mine = {k: p.grad for k, p in mod.named_parameters() if p.grad is not None}
        assert sorted(mine) == sorted(k for k in rg), (sorted(set(mine) ^ set(rg)))
        fl = 1e-2 * max(float(v.abs().max()) for v in rg.values())
        for k in rg:
            close(mine[k], rg[k], rtol=1e-3, floor=fl, what="grad %s" % k)
    for mod, omod, lr in ((g, og, 1e-4), (d, od, 1e-3)):
        rw = omod.state_dict()
        for k, v in mod.state_dict().items():
            err = (v.detach().cpu().double() - rw[k].double()).abs().max().item()
            assert err <= 2 * lr + 1e-5 * rw[k].abs().max().item(), (k, err)


# 8 ---------------------------------------------------------------------------
def test_sample_k_wide_equals_separate_calls():
    """evaluate.sample_k (context once, k rollouts) on a batch with a 70-ped
    scene equals k separate generator calls fed the same noise rows."""
    from sgan import evaluate
    from sgan.data.synthetic import synthetic_batch
    g, _ = build_models("gat")
    batch = synthetic_batch([70, 20], seed=8, device=DEV)
    k, S = 3, 2
    with torch.no_grad():
        torch.manual_seed(4)
        out, _ = evaluate.sample_k(g, batch, k)
        torch.manual_seed(4)
        sc = _scene_index([70, 20])
        z = evaluate.draw_sample_noise(g, sc, 90, k)
        for r in range(k):
            y = g(batch[0], batch[2], batch[-1], batch[6], user_noise=z[r * S:(r + 1) * S])
            close(out[:, r], y.cpu().numpy(), rtol=1e-6, what="sample %d" % r)


# dispatch ----------------------------------------------------------------------
def _pool_call(sc, ops, h, W1, We, be, b1):
    from sgan import kernels as K
    U, pos, _, W2, b2 = ops
    with torch.no_grad():
        return K._Pool.apply(h, pos, W1, We, be, b1, W2, b2, sc, None, U)


def test_wide_batch_runs_fp32_alone_under_bf16_and_pairing():
    """A batch with one 70-ped scene: the same out and argmax, bitwise, under
    set_precision("bf16") (no bf16 wide forward) and inside a pool_pair()
    block, where it never joins the paired launch -- a forward held before it
    is issued on its own and keeps its values."""
    from sgan import kernels as K
    gen = torch.Generator().manual_seed(3)
    W1 = (torch.randn(512, 48, generator=gen) * 0.1).to(DEV)
    We, be = (torch.randn(16, 2, generator=gen) * 0.3).to(DEV), (torch.randn(16, generator=gen) * 0.1).to(DEV)
    b1 = (torch.randn(512, generator=gen) * 0.1).to(DEV)
    wide_sc, small_sc = _scene_index([70, 5, 20]), _scene_index([20, 7])
    ops_w = tuple(t.to(DEV) for t in _pool_operands(95, 8, 70))
    ops_s = tuple(t.to(DEV) for t in _pool_operands(27, 8, 71))
    ops_s = (ops_s[0], ops_s[1], None, ops_w[3], ops_w[4])   # the same net
    h_w, h_s = torch.randn(95, 32, generator=gen).to(DEV), torch.randn(27, 32, generator=gen).to(DEV)
    args_w, args_s = (wide_sc, ops_w, h_w, W1, We, be, b1), (small_sc, ops_s, h_s, W1, We, be, b1)
    assert K.pool_is_wide(wide_sc) and not K.pool_is_wide(small_sc)
    ref_w, ref_s = _pool_call(*args_w), _pool_call(*args_s)
    K.set_precision("bf16")
    try:
        got = _pool_call(*args_w)
    finally:
        K.set_precision("fp32")
    assert torch.equal(got[0], ref_w[0]) and torch.equal(got[1], ref_w[1])
    with K.pool_pair() as rider:
        held = _pool_call(*args_s)
        assert rider.held is not None and not rider.fits((None, None, None), 8, False, 2, wide=True)
        got = _pool_call(*args_w)
        assert rider.held is None and not rider.carried
    torch.cuda.synchronize()
    assert torch.equal(held[0], ref_s[0]) and torch.equal(held[1], ref_s[1])
    assert torch.equal(got[0], ref_w[0]) and torch.equal(got[1], ref_w[1])
