"""Social pooling with batch norm on the GPU (sgg_pool_norm_fwd /
sgg_pool_norm_bwd / sgg_pool_norm_running in train(), the fold in eval()):
against the float64 yardstick of _pool_norm_ref.py with tolerances measured
from its float32 CPU run, and through the generators and the discriminator.

Measured max(error / tolerance) per case is printed by
test_kernels_vs_yardstick before it asserts."""
import functools

import numpy as np
import pytest
import torch

import _pool_norm_ref as R
from test_gpu_parity import DEV, close

pytestmark = pytest.mark.gpu


def _sc(sizes):
    from sgan.scene import SceneIndex
    return SceneIndex(np.concatenate([[0], np.cumsum(sizes)]), DEV)


def _apply(net, h, pos, sc, pos_grad=True):
    """The train() op on the module's parameters -> (out, argmax)."""
    from sgan import kernels as K
    l1, l2 = K.pool_linears(net)
    n1, n2 = K.pool_norms(net)
    emb = net.spatial_embedding
    min_n = K.pool_norm_check(sc, l2.weight.shape[0], (n1, n2), dropout=net.dropout)
    stats = tuple((float(m.eps), float(m.momentum), m.running_mean, m.running_var, m.num_batches_tracked)
                  for m in (n1, n2))
    op = K._PoolNorm
    return op.apply(h, pos, l1.weight, emb.weight, emb.bias, l1.bias, n1.weight, n1.bias, l2.weight, l2.bias,
                    n2.weight, n2.bias, sc, None, stats, min_n, pos_grad)


@functools.lru_cache(maxsize=None)
def _gpu_run(bn, sizes_id):
    """The case on the GPU, once: train() forward, backward, second forward, eval() forward."""
    from sgan.models import PoolHiddenNet
    c = R.case(bn, sizes_id)
    net = R.float32_net(c, PoolHiddenNet).to(DEV).train()
    sc = _sc(c["sizes"])
    h = c["h"][0].float().to(DEV).requires_grad_(True)
    pos = c["pos"].float().to(DEV).requires_grad_(True)
    out, am = _apply(net, h, pos, sc)
    n1, n2 = [m for m in net.mlp_pre_pool if isinstance(m, torch.nn.BatchNorm1d)]
    g = {"out": out.detach().clone(), "am": am.clone()}
    for tag, m in (("1", n1), ("2", n2)):
        g["rm%s_a" % tag], g["rv%s_a" % tag] = m.running_mean.clone(), m.running_var.clone()
    g["nbt_a"] = (int(n1.num_batches_tracked), int(n2.num_batches_tracked))
    (out * c["dout"].float().to(DEV)).sum().backward()
    with torch.no_grad():
        net(h.view(1, -1, R.H_DIM), None, pos, scenes=sc)
    for tag, m in (("1", n1), ("2", n2)):
        g["rm%s_b" % tag], g["rv%s_b" % tag] = m.running_mean.clone(), m.running_var.clone()
    g["nbt_b"] = (int(n1.num_batches_tracked), int(n2.num_batches_tracked))
    g["dh"], g["dpos"] = h.grad.clone(), pos.grad.clone()
    for k, v in net.named_parameters():
        g["dw." + k] = v.grad.clone()
    net.eval()
    with torch.no_grad():
        g["out_eval"] = net(h.view(1, -1, R.H_DIM), None, pos, scenes=sc).clone()
    torch.cuda.synchronize()
    return g


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("bn,sizes_id", R.CASES + R.MANY_CASES)
def test_kernels_vs_yardstick(bn, sizes_id):
    """(The last two cases have more scenes than the kernels have workgroups:
    1100 scenes of 3 .. 5 peds at bn 8, 40 scenes of 2 peds at bn 1024 -- every
    workgroup walks several scenes and sums them into its slab row.)  out, the argmax where decided, dh, dpos, every parameter gradient and
    the running statistics after one and two forwards against the float64
    yardstick: each within max(4 e32, 16 * 2^-23) of the array's max, e32 the
    float32 CPU oracle's own error on that array; the three biases in front
    of a BatchNorm get exact zeros."""
    c = R.case(bn, sizes_id)
    assert c["excluded"] == 0
    g = _gpu_run(bn, sizes_id)
    worst = {}
    for k, ref in c["r64"].items():
        if not torch.is_tensor(ref) or k[3:] in R.ZERO_BIASES:
            continue
        worst[k] = R.rel_err(g[k], ref) / c["tol"][k]
    print("bn %d sizes %s: max err/tol %.3f at %s" % (bn, c["sizes"], max(worst.values()), max(worst, key=worst.get)))
    print("   " + ", ".join("%s %.2f" % kv for kv in sorted(worst.items())))
    S = len(c["sizes"])
    assert g["nbt_a"] == (S, S) and g["nbt_b"] == (2 * S, 2 * S)
    assert c["r64"]["nbt_a"] == S and c["r64"]["nbt_b"] == 2 * S
    for k in R.ZERO_BIASES:
        z = g["dw." + k]
        assert z is not None and z.shape == c["r64"]["dw." + k].shape and not z.any(), k
    am = g["am"].cpu().long()
    assert torch.equal(am[c["compare"]], c["best"][c["compare"]])
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


# 2 ---------------------------------------------------------------------------
def test_frozen_weights_du_only():
    """Weights frozen: the same dh and dpos, bitwise, and no parameter gradient."""
    from sgan.models import PoolHiddenNet
    c = R.case(24, 0)
    g = _gpu_run(24, 0)
    net = R.float32_net(c, PoolHiddenNet).to(DEV).train()
    for p in net.parameters():
        p.requires_grad_(False)
    h = c["h"][0].float().to(DEV).requires_grad_(True)
    pos = c["pos"].float().to(DEV).requires_grad_(True)
    out, _ = _apply(net, h, pos, _sc(c["sizes"]))
    (out * c["dout"].float().to(DEV)).sum().backward()
    assert torch.equal(out, g["out"]) and torch.equal(h.grad, g["dh"]) and torch.equal(pos.grad, g["dpos"])
    assert all(p.grad is None for p in net.parameters())


# 3 ---------------------------------------------------------------------------
def test_two_runs_bitwise_equal_at_1024():
    from sgan.models import PoolHiddenNet
    sizes = [2, 20]
    torch.manual_seed(3)
    src = PoolHiddenNet(R.E_DIM, R.H_DIM, 64, 1024, "relu", True)
    h0, pos0, dout = torch.randn(22, R.H_DIM), torch.rand(22, 2) * 15, torch.randn(22, 1024)
    runs = []
    for _ in range(2):
        net = PoolHiddenNet(R.E_DIM, R.H_DIM, 64, 1024, "relu", True)
        net.load_state_dict(src.state_dict())
        net = net.to(DEV).train()
        h, pos = h0.to(DEV).requires_grad_(True), pos0.to(DEV).requires_grad_(True)
        out = net(h.view(1, 22, -1), None, pos, scenes=_sc(sizes), pos_grad=True)
        (out * dout.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        runs.append([out.detach(), h.grad, pos.grad] + [p.grad for p in net.parameters()]
                    + [b for b in net.buffers()])
    for a, b in zip(*runs):
        assert not torch.isnan(a.float()).any() and torch.equal(a, b)
    assert float(runs[0][1].abs().max()) > 0


# 4 ---------------------------------------------------------------------------
def test_one_scene_of_130_peds():
    """A scene above 64 peds (more pair tiles, several blocks of the position
    gradient's reduction): against the float32 / float64 oracle at bn 8."""
    from sgan.models import PoolHiddenNet
    torch.manual_seed(11)
    sizes, bn = [130], 8
    o64 = R.build_net(bn, 4242)
    h, pos, dout = torch.randn(1, 130, R.H_DIM).double(), torch.rand(130, 2).double() * 15, torch.randn(130, bn).double()
    state0 = {k: v.clone() for k, v in o64.state_dict().items()}
    r64, _ = R._run(o64, h, pos, dout, sizes)
    o32 = R.build_net(bn, 4242, torch.float32)
    o32.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in state0.items()})
    with R.one_thread():
        r32, _ = R._run(o32, h.float(), pos.float(), dout.float(), sizes)
    net = PoolHiddenNet(R.E_DIM, R.H_DIM, 64, bn, "relu", True)
    net.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in state0.items()})
    net = net.to(DEV).train()
    hg, pg = h[0].float().to(DEV).requires_grad_(True), pos.float().to(DEV).requires_grad_(True)
    out = net(hg.view(1, 130, -1), None, pg, scenes=_sc(sizes), pos_grad=True)
    (out * dout.float().to(DEV)).sum().backward()
    got = {"out": out, "dh": hg.grad, "dpos": pg.grad}
    got.update({"dw." + k: v.grad for k, v in net.named_parameters()})
    for k, v in got.items():
        if k[3:] in R.ZERO_BIASES:
            assert not v.any()
            continue
        tol = max(4 * R.rel_err(r32[k], r64[k]), R.FLOOR)
        e = R.rel_err(v, r64[k])
        print("%s err %.2e tol %.2e" % (k, e, tol))
        assert e <= tol, (k, e, tol)


# 5 ---------------------------------------------------------------------------
@pytest.mark.parametrize("bn", [8, 72])
def test_eval_is_the_folded_net_bitwise(bn):
    """eval(): bitwise the batch_norm=0 net carrying the folded tensors, and
    the oracle in eval() within the float32 tolerance; gradients reach the raw
    parameters through the fold."""
    from sgan import kernels as K
    from sgan.models import PoolHiddenNet
    sizes = [2, 3, 5, 20, 37]
    B = sum(sizes)
    o64 = R.build_net(bn, 99 + bn)
    with torch.no_grad():
        for m in R.norms_of(o64):
            m.running_mean.copy_(0.5 * torch.randn(m.num_features).double())
            m.running_var.copy_((0.5 + torch.rand(m.num_features)).double())
    o64.eval()
    h, pos = torch.randn(1, B, R.H_DIM).double(), torch.rand(B, 2).double() * 15
    ref = o64(h, R.sse_of(sizes), pos).detach()
    o32 = R.build_net(bn, 99 + bn, torch.float32)
    o32.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in o64.state_dict().items()})
    o32.eval()
    with R.one_thread():
        e32 = R.rel_err(o32(h.float(), R.sse_of(sizes), pos.float()), ref)
    net = PoolHiddenNet(R.E_DIM, R.H_DIM, 64, bn, "relu", True)
    net.load_state_dict(o32.state_dict())
    net = net.to(DEV).eval()
    sc = _sc(sizes)
    hg, pg = h.float().to(DEV).requires_grad_(True), pos.float().to(DEV)
    out = net(hg, None, pg, scenes=sc)
    plain = PoolHiddenNet(R.E_DIM, R.H_DIM, 64, bn, "relu", False).to(DEV)
    with torch.no_grad():
        (l1, l2), (n1, n2) = K.pool_linears(net), K.pool_norms(net)
        W1, b1 = K.pool_norm_fold(l1, n1)
        W2, b2 = K.pool_norm_fold(l2, n2)
        plain.load_state_dict({"spatial_embedding.weight": net.spatial_embedding.weight,
                               "spatial_embedding.bias": net.spatial_embedding.bias, "mlp_pre_pool.0.weight": W1,
                               "mlp_pre_pool.0.bias": b1, "mlp_pre_pool.2.weight": W2, "mlp_pre_pool.2.bias": b2})
        out_plain = plain(hg.detach(), None, pg, scenes=sc)
    assert torch.equal(out.detach(), out_plain)
    e = R.rel_err(out, ref)
    print("bn %d eval err %.2e, e32 %.2e" % (bn, e, e32))
    assert e <= max(4 * e32, R.FLOOR)
    out.sum().backward()
    for k, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert float(net.mlp_pre_pool[1].weight.grad.abs().max()) > 0 and float(hg.grad.abs().max()) > 0
    assert int(net.mlp_pre_pool[1].num_batches_tracked) == 0      # eval() leaves the statistics alone


# 6 ---------------------------------------------------------------------------
_SMALL = dict(embedding_dim=16, encoder_h_dim=32, decoder_h_dim=32, mlp_dim=64, bottleneck_dim=8, n_units=[40, 16, 40])


def _gen_kw(graph, pet):
    kw = dict(num_layers=1, noise_dim=(8,), noise_type="gaussian", noise_mix_type="global", pooling_type="pool_net",
              pool_every_timestep=pet, dropout=0.0, batch_norm=True, n_heads=1, dropout1=0.0, alpha=0.2, graph=graph)
    kw.update(_SMALL)
    return kw


def _oracle_generator(kw):
    """test_gpu_pool_bn._oracle_generator with batch_norm=True in the decoder's
    pooling net and mlp (the oracle's Decoder restates the rollout without
    per-step pooling only)."""
    from oracle import sgan_oracle as O
    if not kw["pool_every_timestep"]:
        return O.TrajectoryGenerator(8, 12, **kw)
    og = O.TrajectoryGenerator(8, 12, **dict(kw, pool_every_timestep=False))
    dec, H, bn = og.decoder, kw["decoder_h_dim"], kw["bottleneck_dim"]
    dec.pool_net = O.PoolHiddenNet(kw["embedding_dim"], H, kw["mlp_dim"], bn, "relu", True)
    dec.mlp = O.mlp([H + bn, kw["mlp_dim"], H], "relu", True, 0.0)

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


def _randomise_norms(net, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.copy_(1.0 + 0.3 * torch.randn(m.num_features, generator=gen))
                m.bias.copy_(0.3 * torch.randn(m.num_features, generator=gen))


def _compare_grads(ref_named, mine_named):
    ref = {k: p.grad for k, p in ref_named if p.grad is not None}
    fl = 1e-2 * max(float(v.abs().max()) for v in ref.values())
    mine = dict(mine_named)
    for k, v in ref.items():
        assert mine[k].grad is not None, k
        close(mine[k].grad, v.numpy(), rtol=1e-3, floor=fl, what="d" + k)


def _compare_buffers(oracle, mine):
    ob = dict(oracle.named_buffers())
    n = 0
    for k, b in mine.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(b) == int(ob[k]), k
            n += 1
        elif "running_" in k:
            close(b, ob[k].numpy(), rtol=1e-4, what=k)
    assert n > 0


@pytest.mark.parametrize("graph,pet", [("vanilla", False), ("vanilla", True), ("gat", False)],
                         ids=["vanilla", "vanilla-pool-every-step", "gat-bn8"])
def test_generators_train_then_eval_vs_oracle(graph, pet):
    """Generators built with batch_norm=True: train() forward and backward
    against the oracle's modules with test_gpu_pool_bn.py's tolerances, the
    running statistics, then eval() forward."""
    from sgan.data.synthetic import synthetic_batch
    from sgan.models import TrajectoryGenerator
    kw = _gen_kw(graph, pet)
    torch.manual_seed(17)
    og = _oracle_generator(kw)
    _randomise_norms(og, 5)
    g = TrajectoryGenerator(8, 12, **kw)
    g.load_state_dict(og.state_dict())
    g = g.to(DEV)
    og.train(), g.train()
    b = synthetic_batch([2, 5, 20], seed=23)
    obs, obs_rel, obs_g, sse = b[0], b[2], b[6], b[10]
    z = torch.randn(3, 8)
    y_ref = og(obs, obs_rel, sse, obs_g, user_noise=z)
    dy = torch.randn_like(y_ref)
    (y_ref * dy).sum().backward()
    y = g(obs.to(DEV), obs_rel.to(DEV), sse.to(DEV), obs_g.to(DEV), user_noise=z.to(DEV))
    (y * dy.to(DEV)).sum().backward()
    close(y, y_ref.detach().numpy(), rtol=1e-4, what="G out")
    assert any(k.startswith("pool_net.") for k, p in og.named_parameters() if p.grad is not None)
    _compare_grads(og.named_parameters(), g.named_parameters())
    _compare_buffers(og, g)
    og.eval(), g.eval()
    with torch.no_grad():
        y_ref = og(obs, obs_rel, sse, obs_g, user_noise=z)
        y = g(obs.to(DEV), obs_rel.to(DEV), sse.to(DEV), obs_g.to(DEV), user_noise=z.to(DEV))
    close(y, y_ref.numpy(), rtol=1e-4, what="G out, eval()")


def test_global_discriminator_train_then_eval_vs_oracle():
    from oracle import sgan_oracle as O
    from sgan.data.synthetic import synthetic_batch
    from sgan.models import TrajectoryDiscriminator
    dkw = dict(embedding_dim=16, h_dim=48, mlp_dim=64, num_layers=1, batch_norm=True, dropout=0.0, d_type="global")
    torch.manual_seed(29)
    od = O.TrajectoryDiscriminator(8, 12, **dkw)
    _randomise_norms(od, 6)
    d = TrajectoryDiscriminator(8, 12, **dkw)
    d.load_state_dict(od.state_dict())
    d = d.to(DEV)
    od.train(), d.train()
    b = synthetic_batch([2, 5, 20], seed=31)
    traj, traj_rel, sse = torch.cat([b[0], b[1]], 0), torch.cat([b[2], b[3]], 0), b[10]
    s_ref = od(traj, traj_rel, sse)
    ds = torch.randn_like(s_ref)
    (s_ref * ds).sum().backward()
    s = d(traj.to(DEV), traj_rel.to(DEV), sse.to(DEV))
    (s * ds.to(DEV)).sum().backward()
    close(s, s_ref.detach().numpy(), rtol=1e-4, what="D scores")
    _compare_grads(od.named_parameters(), d.named_parameters())
    _compare_buffers(od, d)
    od.eval(), d.eval()
    with torch.no_grad():
        close(d(traj.to(DEV), traj_rel.to(DEV), sse.to(DEV)), od(traj, traj_rel, sse).numpy(), rtol=1e-4,
              what="D scores, eval()")


# 7 ---------------------------------------------------------------------------
def _no_launch(monkeypatch):
    from sgan import _native as N
    calls = []
    real = N.check
    monkeypatch.setattr(N, "check", lambda rc, name: (calls.append(name), real(rc, name))[1])
    return calls


def test_refusals_before_any_launch(monkeypatch):
    from sgan.models import PoolHiddenNet
    from sgan.scene import PaddedScenes
    net = PoolHiddenNet(16, 32, 64, 24, "relu", True).to(DEV).train()
    z = lambda sc: (torch.zeros(1, sc.B, 32, device=DEV), None, torch.zeros(sc.B, 2, device=DEV))
    torch.cuda.synchronize()
    calls = _no_launch(monkeypatch)
    sc = _sc([1, 5])
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        net(*z(sc), scenes=sc)
    sc = _sc([3, 257])
    with pytest.raises(NotImplementedError, match="batch_norm.*256"):
        net(*z(sc), scenes=sc)
    ps = PaddedScenes(4, 32, DEV, 20, reps=(2,))
    ps.load(np.array([0, 5, 12], np.int32), np.arange(12, dtype=np.int32))
    for sc in (ps, ps.repeat(2)):
        for mode in (True, False):
            net.train(mode)
            with pytest.raises(NotImplementedError, match="batch_norm"):
                net(*z(sc), scenes=sc)
    net.train()
    sc = _sc([3, 5])
    net.mlp_pre_pool[1].momentum = None
    with pytest.raises(NotImplementedError, match="momentum"):
        net(*z(sc), scenes=sc)
    drop = PoolHiddenNet(16, 32, 64, 24, "relu", True, dropout=0.25).to(DEV).train()
    with pytest.raises(NotImplementedError, match="batch_norm.*dropout|dropout.*batch_norm"):
        drop(*z(sc), scenes=sc)
    assert calls == [], calls
