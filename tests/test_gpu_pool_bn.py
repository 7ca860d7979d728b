"""Social pooling at any bottleneck_dim up to 1024 (sgg_pool_fwd_bn /
sgg_pool_bwd_bn, column tiles of 64): against the wide kernels where both
apply, the reference's fixture, the float64 oracle at the column-tile edges,
and through the generators, a training step and the refusals that remain."""
import random

import numpy as np
import pytest
import torch

from conftest import RecordingAdam
from test_gpu_lstm_gen import _Args3
from test_gpu_parity import DEV, T, close, grad_floor, npz
from test_gpu_pool_wide import _bwd, _fwd, _pool_operands, _scene_index

pytestmark = pytest.mark.gpu


def _fwd_bn(lib, N, sc, ops, bn):
    U, pos, A, W2, b2 = ops
    B = U.shape[0]
    out = torch.empty(B, bn, device=DEV)
    am = torch.empty(B, bn, device=DEV, dtype=torch.int32)
    chunks, nchunks, max_rows, gpw = sc.pool_plan(bn, family_bn=True)
    N.check(lib.sgg_pool_fwd_bn(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2), N.ptr(b2), N.ptr(sc.scene_off),
                                N.ptr(chunks), nchunks, max_rows, gpw, B, bn, sc.max_n, N.ptr(out), N.ptr(am),
                                N.stream_ptr()), "sgg_pool_fwd_bn")
    return out, am


def _bwd_bn(lib, N, sc, ops, bn, out, am, dout, wgrad=True):
    """-> dU, (dW2, dA, db2) summed over the slab rows in float64 (None when frozen), the raw slab."""
    U, pos, A, W2, _ = ops
    B = U.shape[0]
    P = bn * 512 + 1024 + bn
    dU = torch.empty(B, 512, device=DEV)
    rows = lib.sgg_pool_bwd_bn_grid(sc.S, bn, sc.max_n)
    nws = lib.sgg_pool_bwd_bn_ws_floats(sc.S, B, bn, sc.max_n)
    assert rows >= 1 and rows * P <= nws <= 16 * P
    part = torch.full((nws,), float("nan"), device=DEV) if wgrad else None
    N.check(lib.sgg_pool_bwd_bn(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2), N.ptr(out), N.ptr(am), N.ptr(dout),
                                N.ptr(sc.scene_off), sc.S, B, bn, sc.max_n, N.ptr(dU), N.ptr(part), nws if wgrad else 0,
                                N.stream_ptr()), "sgg_pool_bwd_bn")
    if not wgrad:
        return dU, None, None
    slab = part[:rows * P].view(rows, P)
    tot = slab.double().sum(0).cpu()
    return dU, (tot[:bn * 512], tot[bn * 512:bn * 512 + 1024], tot[bn * 512 + 1024:]), slab


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[1, 2, 5, 20, 57, 64, 3, 20], [3, 70]])
@pytest.mark.parametrize("bn", [8, 48, 64])
def test_bn_family_equals_wide_on_built_widths(bn, sizes, monkeypatch):
    """Tiling the columns does not change a pair's value: at the built widths
    out and argmax are bitwise sgg_pool_fwd_wide's and dU is bitwise
    sgg_pool_bwd_wide's; the reduced [dW2 | dA | db2] agree to 1e-5 of each
    tensor's max (another slab partition, so another summation order)."""
    from sgan import _native as N
    monkeypatch.setenv("SGG_POOL_X3", "0")
    lib = N.load()
    sc = _scene_index(sizes)
    ops = tuple(t.to(DEV) for t in _pool_operands(sum(sizes), bn, 100 + bn))
    out_w, am_w = _fwd(lib, N, sc, ops, bn, wide=True)
    out_b, am_b = _fwd_bn(lib, N, sc, ops, bn)
    assert torch.equal(out_w, out_b) and torch.equal(am_w, am_b)
    dout = torch.randn(sum(sizes), bn, generator=torch.Generator().manual_seed(5)).to(DEV)
    dU_w, sums_w = _bwd(lib, N, sc, ops, bn, out_w, am_w, dout, wide=True)
    dU_b, sums_b, slab = _bwd_bn(lib, N, sc, ops, bn, out_w, am_w, dout)
    assert torch.equal(dU_w, dU_b)
    assert not torch.isnan(slab).any()      # every slab cell is written
    for name, a, b in zip(("dW2", "dA", "db2"), sums_b, sums_w):
        close(a, b.numpy(), rtol=1e-5, what="bn family " + name)


# 2, 4 ------------------------------------------------------------------------
def _fixture_net(tag):
    from sgan.models import PoolHiddenNet
    from test_oracle_golden_pool_bn import pool_bn_net
    f = npz("pool_bn.npz")
    return f, pool_bn_net(f, tag, PoolHiddenNet).to(DEV)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_pool_bn_vs_reference_fixture(tag):
    """The reference's PoolHiddenNet at bottleneck_dim 72 and 136,
    test_pool_vs_reference_fixture's tolerances."""
    f, net = _fixture_net(tag)
    h = T(f[tag + "/h"]).unsqueeze(0).requires_grad_(True)
    y = net(h, T(f[tag + "/sse"]), T(f[tag + "/pos"]))
    close(y, f[tag + "/out"], rtol=1e-5, what="pool out")
    (y * T(f[tag + "/dout"])).sum().backward()
    close(h.grad[0], f[tag + "/dh"], rtol=1e-4, what="pool dh")
    fl = grad_floor(f, tag + "/dw/")
    for k, p in net.named_parameters():
        close(p.grad, f[tag + "/dw/" + k], rtol=1e-4, floor=fl, what="pool d" + k)


def test_pool_bn_frozen_weights_same_dh():
    """part = NULL (frozen weights): the same dh, bitwise, as with weight gradients (bn 136)."""
    f, net = _fixture_net("b")
    res = []
    for frozen in (False, True):
        net.requires_grad_(not frozen)
        h = T(f["b/h"]).unsqueeze(0).requires_grad_(True)
        y = net(h, T(f["b/sse"]), T(f["b/pos"]))
        (y * T(f["b/dout"])).sum().backward()
        res.append(h.grad.clone())
    assert all(p.grad is not None for p in net.parameters())   # (from the first pass)
    assert torch.equal(res[0], res[1])


# 3 ---------------------------------------------------------------------------
_EDGE_SIZES = [1, 2, 5, 20, 37]


@pytest.mark.parametrize("h_dim", [32, 128])
@pytest.mark.parametrize("bn,sizes", [(bn, s) for bn in (1, 24, 65, 72, 128, 136, 1024)
                                      for s in ([_EDGE_SIZES] + ([[3, 70]] if bn in (72, 136, 1024) else []))],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_pool_bn_column_tile_edges_vs_float64_oracle(bn, sizes, h_dim):
    """Widths around the 64-column tile edges (one column, a partial single
    tile, one column into the second tile, partial last tiles, full tiles, the
    bound) against the oracle's PoolHiddenNet in float64: out within 1e-5 of
    its max; argmax equal to the float64 argmax wherever out > 0 and the
    float64 top-two gap exceeds 1e-5 of the range of out (at most 1 % of the
    entries may be excluded that way; entries with out == 0 carry no gradient
    and are not compared)."""
    from oracle import sgan_oracle as O
    from sgan import kernels as K
    from sgan.models import PoolHiddenNet
    torch.manual_seed(41 + bn)
    net64 = O.PoolHiddenNet(16, h_dim, 64, bn, "relu", False).double()
    B = sum(sizes)
    h = torch.randn(1, B, h_dim, dtype=torch.float64)
    pos = torch.rand(B, 2, dtype=torch.float64) * 15
    off = np.concatenate([[0], np.cumsum(sizes)])
    sse = torch.from_numpy(np.stack([off[:-1], off[1:]], 1).astype(np.int64))
    zs = []
    hook = net64.mlp_pre_pool.register_forward_hook(lambda m, i, o: zs.append(o.detach()))
    with torch.no_grad():
        ref = net64(h, sse, pos)
    hook.remove()
    net = PoolHiddenNet(16, h_dim, 64, bn, "relu", False)
    net.load_state_dict({k: v.float() for k, v in net64.state_dict().items()})
    net = net.to(DEV)
    sc = _scene_index(sizes)
    l1, l2, emb = net.mlp_pre_pool[0], net.mlp_pre_pool[2], net.spatial_embedding
    with torch.no_grad():
        out, am = K._Pool.apply(h.float().to(DEV).view(B, h_dim), pos.float().to(DEV), l1.weight, emb.weight, emb.bias,
                                l1.bias, l2.weight, l2.bias, sc, None, None)
    close(out, ref.numpy(), rtol=1e-5, what="out bn=%d" % bn)
    rng = float(ref.max() - ref.min())
    am = am.cpu().long()
    excluded, total = 0, 0
    for s, (n, z) in enumerate(zip(sizes, zs)):
        z = z.view(n, n, bn)
        r = ref[off[s]:off[s + 1]]
        if n > 1:
            top = z.topk(2, dim=1)
            sure = (top[0][:, 0] - top[0][:, 1]) > 1e-5 * rng
            best = top[1][:, 0]
        else:
            sure, best = torch.ones(1, bn, dtype=torch.bool), torch.zeros(1, bn, dtype=torch.long)
        live = r > 0
        excluded += int((live & ~sure).sum())
        total += n * bn
        keep = live & sure
        assert torch.equal(am[off[s]:off[s + 1]][keep], (best + int(off[s]))[keep]), (s, n)
    assert excluded <= 0.01 * total, (excluded, total)


# 5 ---------------------------------------------------------------------------
def test_pool_bn_backward_deterministic_at_1024():
    """Two backward runs at bn 1024 (16 column tiles, scenes on both sides of
    the 64-ped i tile): bitwise equal dU and reduced gradients."""
    from sgan import _native as N
    from sgan import kernels as K
    lib = N.load()
    sizes, bn = [3, 70, 20], 1024
    sc = _scene_index(sizes)
    ops = tuple(t.to(DEV) for t in _pool_operands(sum(sizes), bn, 7))
    out, am = _fwd_bn(lib, N, sc, ops, bn)
    dout = torch.randn(sum(sizes), bn, generator=torch.Generator().manual_seed(8)).to(DEV)
    runs = []
    for _ in range(2):
        dU, _, slab = _bwd_bn(lib, N, sc, ops, bn, out, am, dout)
        P = bn * 512 + 1024 + bn
        dW2 = torch.empty(bn, 512, device=DEV)
        dA = torch.empty(1024, device=DEV)
        db2 = torch.empty(bn, device=DEV)
        gf = K.GradFinish()
        gf.rowsum(slab, slab.shape[0], P, 0, bn * 512, dW2)
        gf.rowsum(slab, slab.shape[0], P, bn * 512, 1024, dA)
        gf.rowsum(slab, slab.shape[0], P, bn * 512 + 1024, bn, db2)
        gf.run()
        torch.cuda.synchronize()
        runs.append((dU.clone(), dW2, dA, db2))
    for a, b in zip(*runs):
        assert not torch.isnan(a).any() and torch.equal(a, b)
    assert float(runs[0][0].abs().max()) > 0 and float(runs[0][1].abs().max()) > 0


# 6 ---------------------------------------------------------------------------
_UPSTREAM = dict(embedding_dim=64, encoder_h_dim=64, decoder_h_dim=128, mlp_dim=1024, bottleneck_dim=1024,
                 n_units=[32, 16, 32], graph="vanilla")
# (decoder H = 32: sgg_dec_step_ok takes the decoder, so per-step pooling runs on the fused step kernels
# with the column-tiled pooling launches between them; at H = 128 above the per-op loop runs)
_STEP72 = dict(embedding_dim=16, encoder_h_dim=32, decoder_h_dim=32, mlp_dim=64, bottleneck_dim=72,
               n_units=[40, 16, 40], graph="vanilla")
_GCN24 = dict(embedding_dim=16, encoder_h_dim=32, decoder_h_dim=32, mlp_dim=64, bottleneck_dim=24,
              n_units=[56, 16, 40], graph="gcn")


def _gen_kw(sizes, pool_every_timestep):
    kw = dict(num_layers=1, noise_dim=(8,), noise_type="gaussian", noise_mix_type="global", pooling_type="pool_net",
              pool_every_timestep=pool_every_timestep, dropout=0.0, batch_norm=False, n_heads=1, dropout1=0.0,
              alpha=0.2)
    kw.update(sizes)
    return kw


def _oracle_generator(kw):
    """The oracle's generator.  Its Decoder restates the rollout without
    per-step pooling only; for pool_every_timestep=1 the decoder gets, from the
    oracle's own PoolHiddenNet and mlp, the step the reference's Decoder.forward
    (models.py:157-175) adds after hidden2pos: pool the new hidden state at the
    new positions, then h <- mlp([h | pooled]); the cell state is kept."""
    from oracle import sgan_oracle as O
    if not kw["pool_every_timestep"]:
        return O.TrajectoryGenerator(8, 12, **kw)
    og = O.TrajectoryGenerator(8, 12, **dict(kw, pool_every_timestep=False))
    dec, H, bn = og.decoder, kw["decoder_h_dim"], kw["bottleneck_dim"]
    dec.pool_net = O.PoolHiddenNet(kw["embedding_dim"], H, kw["mlp_dim"], bn, "relu", False)
    dec.mlp = O.mlp([H + bn, kw["mlp_dim"], H], "relu", False, 0.0)

    def forward(last_pos, last_pos_rel, state, seq_start_end):
        B = last_pos.shape[0]
        x = dec.spatial_embedding(last_pos_rel).view(1, B, dec.embedding_dim)
        outs = []
        for _ in range(dec.seq_len):
            y, state = dec.decoder(x, state)
            rel = dec.hidden2pos(y.view(-1, H))
            last_pos = rel + last_pos
            pooled = dec.pool_net(state[0], seq_start_end, last_pos)
            state = (dec.mlp(torch.cat([state[0].view(-1, H), pooled], 1)).unsqueeze(0), state[1])
            x = dec.spatial_embedding(rel).view(1, B, dec.embedding_dim)
            outs.append(rel.view(B, -1))
        return torch.stack(outs, 0), state[0]
    dec.forward = forward
    return og


@pytest.mark.parametrize("sizes,pet", [(_UPSTREAM, False), (_UPSTREAM, True), (_STEP72, True), (_GCN24, False)],
                         ids=["upstream-1024", "upstream-1024-pool-every-step", "step-kernels-72-pool-every-step",
                              "gcn-24"])
def test_generators_vs_oracle(sizes, pet):
    """A vanilla generator at upstream Social-GAN's sizes (bottleneck_dim
    1024, with and without per-step pooling) and a gcn generator at
    bottleneck_dim 24 against the oracle's modules: output and every
    parameter gradient, test_gpu_lstm_gen.py's generator tolerances."""
    from sgan.data.synthetic import synthetic_batch
    from sgan.models import TrajectoryGenerator
    from sgan import kernels as K
    kw = _gen_kw(sizes, pet)
    torch.manual_seed(17)
    og = _oracle_generator(kw)
    g = TrajectoryGenerator(8, 12, **kw)
    g.load_state_dict(og.state_dict())
    g = g.to(DEV)
    if pet:   # the route under test: the fused step kernels at H = 32, the per-op loop at H = 128
        assert K.dec_step_enabled() and bool(g.decoder.step_ok()) == (sizes is _STEP72), g.decoder.step_ok()
    b = synthetic_batch([1, 5, 20], seed=23)
    obs, obs_rel, obs_g, sse = b[0], b[2], b[6], b[10]
    z = torch.randn(3, 8)
    y_ref = og(obs, obs_rel, sse, obs_g, user_noise=z)
    dy = torch.randn_like(y_ref)
    (y_ref * dy).sum().backward()
    y = g(obs.to(DEV), obs_rel.to(DEV), sse.to(DEV), obs_g.to(DEV), user_noise=z.to(DEV))
    (y * dy.to(DEV)).sum().backward()
    close(y, y_ref.detach().numpy(), rtol=1e-4, what="G out")
    ref = {k: p.grad for k, p in og.named_parameters() if p.grad is not None}
    assert any(k.startswith("pool_net.") for k in ref) and (not pet or any(".pool_net." in k for k in ref))
    fl = 1e-2 * max(float(v.abs().max()) for v in ref.values())
    mine = dict(g.named_parameters())
    for k, v in ref.items():
        close(mine[k].grad, v.numpy(), rtol=1e-3, floor=fl, what="G d" + k)


# 7 ---------------------------------------------------------------------------
def _gd72():
    """(oracle G, oracle D, G, D): a vanilla generator at bottleneck_dim 72, a local discriminator."""
    from oracle import sgan_oracle as O
    from sgan.models import TrajectoryDiscriminator, TrajectoryGenerator
    kw = _gen_kw(dict(embedding_dim=16, encoder_h_dim=32, decoder_h_dim=32, mlp_dim=64, bottleneck_dim=72,
                      n_units=[40, 16, 40], graph="vanilla"), False)
    dkw = dict(embedding_dim=16, h_dim=48, mlp_dim=64, num_layers=1, batch_norm=False, dropout=0.0, d_type="local")
    torch.manual_seed(5)
    og, od = O.TrajectoryGenerator(8, 12, **kw), O.TrajectoryDiscriminator(8, 12, **dkw)
    g, d = TrajectoryGenerator(8, 12, **kw), TrajectoryDiscriminator(8, 12, **dkw)
    g.load_state_dict(og.state_dict())
    d.load_state_dict(od.state_dict())
    return og, od, g.to(DEV), d.to(DEV)


def test_train_step_bn72_vs_oracle():
    """One GanTrainer iteration (best_k 3) against the oracle's restatement of
    the reference's steps from the same seeds: losses, the gradients each
    optimizer step consumed, weights."""
    from oracle import sgan_oracle as O
    from sgan.data.synthetic import synthetic_batch
    from sgan.scene import SceneIndex
    from sgan.train_step import GanTrainer, TrainArgs
    og, od, g, d = _gd72()
    oog = RecordingAdam.make(og.named_parameters(), lr=1e-4)
    ood = RecordingAdam.make(od.named_parameters(), lr=1e-3)
    tr = GanTrainer(g, d, TrainArgs(best_k=3))
    b = synthetic_batch([20, 7, 13], seed=70)
    bd = [t.to(DEV) for t in b]
    sc = SceneIndex.from_seq_start_end(b[-1], DEV)
    torch.manual_seed(21)
    random.seed(21)
    rld = O.discriminator_step(_Args3, b, og, od, ood)
    rlg = O.generator_step(_Args3, b, og, od, oog)
    rgd, rgg = dict(ood.rec[-1]), dict(oog.rec[-1])
    torch.manual_seed(21)
    random.seed(21)
    ld, lg = tr.step(bd, sc)
    for k, v in list(ld.items()) + list(lg.items()):
        r = (rld if k.startswith("D") else rlg)[k]
        assert abs(float(v) - r) <= 1e-4 * max(1.0, abs(r)), (k, float(v), r)
    for mod, rg in ((d, rgd), (g, rgg)):
        mine = {k: p.grad for k, p in mod.named_parameters() if p.grad is not None}
        assert sorted(mine) == sorted(rg), sorted(set(mine) ^ set(rg))
        fl = 1e-2 * max(float(v.abs().max()) for v in rg.values())
        assert fl > 0
        for k in rg:
            close(mine[k], rg[k], rtol=1e-3, floor=fl, what="grad %s" % k)
    for mod, omod, lr in ((g, og, 1e-4), (d, od, 1e-3)):
        rw = omod.state_dict()
        for k, v in mod.state_dict().items():
            err = (v.detach().cpu().double() - rw[k].double()).abs().max().item()
            assert err <= 2 * lr + 1e-5 * rw[k].abs().max().item(), (k, err)


def test_graphed_trainer_bn72_replays_bitwise():
    """GraphedTrainer (one warm-up iteration + two replays) == three eager
    iterations of the same step, bit for bit: weights and losses."""
    from sgan.data.synthetic import synthetic_batch
    from sgan.scene import SceneIndex
    from sgan.train_step import GanTrainer, GraphedTrainer, TrainArgs
    batch = synthetic_batch([20, 7, 13], seed=70, device=DEV)
    res = []
    for graphed in (False, True):
        _, _, g, d = _gd72()
        tr = GanTrainer(g, d, TrainArgs(best_k=3), capturable=True)
        sc = SceneIndex.from_seq_start_end(batch[-1], DEV)
        torch.manual_seed(11)
        random.seed(11)
        if graphed:
            gt = GraphedTrainer(tr, batch, sc, warmup=1)
            for _ in range(2):
                ld, lg = gt.step()
        else:
            for _ in range(3):
                ld, lg = tr.step(batch, sc)
        torch.cuda.synchronize()
        ws = {"g." + k: v.detach().cpu().clone() for k, v in g.state_dict().items()}
        ws.update({"d." + k: v.detach().cpu().clone() for k, v in d.state_dict().items()})
        res.append(({k: float(v) for k, v in list(ld.items()) + list(lg.items())}, ws))
    (la, wa), (lb, wb) = res
    assert la == lb, (la, lb)
    for k in wa:
        assert torch.equal(wa[k], wb[k]), (k, (wa[k] - wb[k]).abs().max().item())


# 8 ---------------------------------------------------------------------------
def test_bottleneck_1025_refused_before_any_launch(monkeypatch):
    from sgan import _native as N
    from sgan.models import PoolHiddenNet
    net = PoolHiddenNet(16, 32, 64, 1025, "relu", False).to(DEV)
    sc = _scene_index([5, 20])
    calls = []
    real = N.check
    monkeypatch.setattr(N, "check", lambda rc, name: (calls.append(name), real(rc, name))[1])
    with pytest.raises(N.NativeError, match="1024"):
        net(torch.zeros(1, 25, 32, device=DEV), None, torch.zeros(25, 2, device=DEV), scenes=sc)
    assert calls == [], calls


@pytest.mark.parametrize("repeated", [False, True])
def test_padded_scenes_refuse_bn72_before_any_launch(repeated, monkeypatch):
    """A fixed-capacity batch (PaddedScenes, and its repeat view) through a
    pooling net at bottleneck_dim 72: NotImplementedError naming
    bottleneck_dim from the pooling op itself, nothing launched (not the fold,
    not the U product)."""
    from sgan import _native as N
    from sgan.models import PoolHiddenNet
    from sgan.scene import PaddedScenes
    ps = PaddedScenes(4, 32, DEV, 20, reps=(2,))
    ps.load(np.array([0, 5, 12], np.int32), np.arange(12, dtype=np.int32))
    sc = ps.repeat(2) if repeated else ps
    net = PoolHiddenNet(16, 32, 64, 72, "relu", False).to(DEV)
    h, pos = torch.zeros(1, sc.B, 32, device=DEV), torch.zeros(sc.B, 2, device=DEV)
    torch.cuda.synchronize()
    calls = []
    real = N.check
    monkeypatch.setattr(N, "check", lambda rc, name: (calls.append(name), real(rc, name))[1])
    with pytest.raises(NotImplementedError, match="bottleneck_dim"):
        net(h, None, pos, scenes=sc)
    assert calls == [], calls


def test_bucketed_trainer_refuses_bn72_by_name(monkeypatch):
    from sgan import _native as N
    from sgan.train_step import BucketedGraphTrainer, GanTrainer, TrainArgs
    _, _, g, d = _gd72()
    tr = GanTrainer(g, d, TrainArgs(best_k=3), capturable=True)
    calls = []
    real = N.check
    monkeypatch.setattr(N, "check", lambda rc, name: (calls.append(name), real(rc, name))[1])
    with pytest.raises(NotImplementedError, match="bottleneck_dim"):
        BucketedGraphTrainer(tr, None)
    assert calls == [], calls
