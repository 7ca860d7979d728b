"""Social pooling with dropout on the GPU (sgg_pool_fwd_bn_drop /
sgg_pool_bwd_bn_drop / sgg_pool_dpos_drop): against the float64 yardstick of
_pool_dropout_ref.py (the oracle's PoolHiddenNet with the explicit masks), the
plain column-tiled family at p = 0, the mask's behaviour, the module in
train() and eval(), a generator and the per-step pooling decoder."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _pool_dropout_ref as R
from test_gpu_parity import DEV, close
from test_gpu_pool_bn import _bwd_bn, _fwd_bn
from test_gpu_pool_wide import _pool_operands, _scene_index

pytestmark = pytest.mark.gpu

CASES = [(bn, s) for bn in R.BNS for s in range(len(R.SIZES))]
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, (list, tuple)) else str(v)


def _fwd_drop(lib, N, sc, ops, bn, p, seed=R.SEED, offset=R.OFFSET, rng=None):
    U, pos, A, W2, b2 = ops
    B = U.shape[0]
    out = torch.empty(B, bn, device=DEV)
    am = torch.empty(B, bn, device=DEV, dtype=torch.int32)
    chunks, nchunks, max_rows, gpw = sc.pool_plan(bn, family_bn=True, dropout=True)
    N.check(lib.sgg_pool_fwd_bn_drop(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2), N.ptr(b2), N.ptr(sc.scene_off),
                                     N.ptr(chunks), nchunks, max_rows, gpw, B, bn, sc.max_n, N.ptr(out), N.ptr(am),
                                     p, seed, offset, N.ptr(rng), N.stream_ptr()), "sgg_pool_fwd_bn_drop")
    return out, am


def _bwd_drop(lib, N, sc, ops, bn, out, am, dout, p, seed=R.SEED, offset=R.OFFSET, rng=None, wgrad=True):
    """-> dU, the raw slab rows (None when frozen)."""
    U, pos, A, W2, _ = ops
    B = U.shape[0]
    P = bn * 512 + 1024 + bn
    dU = torch.empty(B, 512, device=DEV)
    rows = lib.sgg_pool_bwd_bn_grid(sc.S, bn, sc.max_n)
    nws = lib.sgg_pool_bwd_bn_ws_floats(sc.S, B, bn, sc.max_n)
    part = torch.full((nws,), float("nan"), device=DEV) if wgrad else None
    N.check(lib.sgg_pool_bwd_bn_drop(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2), N.ptr(out), N.ptr(am), N.ptr(dout),
                                     N.ptr(sc.scene_off), sc.S, B, bn, sc.max_n, N.ptr(dU), N.ptr(part),
                                     nws if wgrad else 0, p, seed, offset, N.ptr(rng), N.stream_ptr()),
            "sgg_pool_bwd_bn_drop")
    return dU, (part[:rows * P].view(rows, P) if wgrad else None)


def _case_operands(c):
    """(U, pos, A, W2, b2) of the yardstick's net, formed in float64 and rounded once."""
    net, E = c["net"], R.E_DIM
    l1, l2 = net.mlp_pre_pool[0], net.mlp_pre_pool[3]
    W1 = l1.weight.detach()
    We, be = net.spatial_embedding.weight.detach(), net.spatial_embedding.bias.detach()
    A = W1[:, :E] @ We
    U = c["h"][0] @ W1[:, E:].t() + (W1[:, :E] @ be + l1.bias.detach())
    return tuple(t.float().contiguous().to(DEV) for t in (U, c["pos"], A, l2.weight.detach(), l2.bias.detach()))


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("p", R.PS)
@pytest.mark.parametrize("bn,sizes_id", CASES)
def test_kernel_forward_vs_float64_yardstick(bn, sizes_id, p):
    """out within 1e-5 of the yardstick's max (test_pool_bn_column_tile_edges_
    vs_float64_oracle's rule); argmax equal to the float64 argmax wherever out
    > 0 and the float64 top-two gap exceeds 1e-5 of the range (at most 1 % of
    the entries excluded: checked on the yardstick alone in
    test_pool_dropout_abi.py); entries with out == 0 are not compared."""
    from sgan import _native as N
    c = R.case(bn, sizes_id, p)
    assert c["excluded"] <= 0.01 * c["total"]
    out, am = _fwd_drop(N.load(), N, _scene_index(c["sizes"]), _case_operands(c), bn, p)
    err = float((out.cpu().double() - c["ref"]).abs().max() / c["ref"].abs().max())
    print("bn %d sizes %s p %g: out err %.3e, excluded %d of %d" % (bn, c["sizes"], p, err, c["excluded"], c["total"]))
    close(out, c["ref"].numpy(), rtol=1e-5, what="drop out bn=%d" % bn)
    keep = c["compare"]
    assert torch.equal(am.cpu().long()[keep], c["best"][keep])


# 2 ---------------------------------------------------------------------------
def _op_backward(c, frozen=False):
    from sgan import kernels as K
    from sgan.models import PoolHiddenNet
    net = R.float32_net(c, PoolHiddenNet, c["p"]).to(DEV).requires_grad_(not frozen)
    l1, l2 = K.pool_linears(net)
    emb = net.spatial_embedding
    h = c["h"][0].float().to(DEV).requires_grad_(True)
    pos = c["pos"].float().to(DEV).requires_grad_(True)
    y = K.social_pool_drop(h, pos, l1.weight, emb.weight, emb.bias, l1.bias, l2.weight, l2.bias,
                           _scene_index(c["sizes"]), (c["p"], R.SEED, R.OFFSET), pos_grad=True)
    (y * c["dout"].float().to(DEV)).sum().backward()
    return net, y, h.grad, pos.grad


@pytest.mark.parametrize("p", R.PS)
@pytest.mark.parametrize("bn,sizes_id", CASES)
def test_backward_vs_float64_autograd(bn, sizes_id, p):
    """dh, dpos and every parameter gradient of the autograd op against
    float64 autograd of the yardstick: rtol 1e-4, the parameters with the floor
    of test_pool_bn_vs_reference_fixture (1e-2 of the largest parameter
    gradient); frozen weights (part = NULL) give the same dh bitwise."""
    c = R.case(bn, sizes_id, p)
    net, y, dh, dpos = _op_backward(c)
    close(y, c["ref"].numpy(), rtol=1e-5, what="drop op out")
    close(dh, c["dh"].numpy(), rtol=1e-4, what="drop dh")
    close(dpos, c["dpos"].numpy(), rtol=1e-4, what="drop dpos")
    fl = 1e-2 * max(float(v.abs().max()) for v in c["dw"].values())
    assert fl > 0
    for k, prm in net.named_parameters():
        close(prm.grad, c["dw"][k].numpy(), rtol=1e-4, floor=fl, what="drop d" + k)
    net_f, _, dh_f, dpos_f = _op_backward(c, frozen=True)
    assert all(prm.grad is None for prm in net_f.parameters())
    assert torch.equal(dh, dh_f) and torch.equal(dpos, dpos_f)


# 3 ---------------------------------------------------------------------------
@pytest.mark.parametrize("bn,sizes_id", CASES)
def test_p0_is_bitwise_the_plain_family(bn, sizes_id):
    from sgan import _native as N
    lib = N.load()
    sizes = list(R.SIZES[sizes_id])
    sc = _scene_index(sizes)
    ops = tuple(t.to(DEV) for t in _pool_operands(sum(sizes), bn, 300 + bn))
    out, am = _fwd_bn(lib, N, sc, ops, bn)
    out_d, am_d = _fwd_drop(lib, N, sc, ops, bn, 0.0)
    assert torch.equal(out, out_d) and torch.equal(am, am_d)
    dout = torch.randn(sum(sizes), bn, generator=torch.Generator().manual_seed(6)).to(DEV)
    dU, _, slab = _bwd_bn(lib, N, sc, ops, bn, out, am, dout)
    dU_d, slab_d = _bwd_drop(lib, N, sc, ops, bn, out, am, dout, 0.0)
    assert torch.equal(dU, dU_d)
    assert not torch.isnan(slab_d).any() and torch.equal(slab, slab_d)
    dU_f, _ = _bwd_drop(lib, N, sc, ops, bn, out, am, dout, 0.0, wgrad=False)
    assert torch.equal(dU, dU_f)


# 4 ---------------------------------------------------------------------------
@pytest.mark.parametrize("bn,sizes_id", [(24, 0), (136, 1)])
def test_mask_behaviour(bn, sizes_id):
    """The same (seed, offset) twice: bitwise equal; another offset: another
    out; (seed, offset) read from rng_dev: the by-value result, bitwise."""
    from sgan import _native as N
    lib = N.load()
    sizes = list(R.SIZES[sizes_id])
    sc = _scene_index(sizes)
    ops = tuple(t.to(DEV) for t in _pool_operands(sum(sizes), bn, 400 + bn))
    dout = torch.randn(sum(sizes), bn, generator=torch.Generator().manual_seed(9)).to(DEV)
    p = 0.5

    def run(**kw):
        out, am = _fwd_drop(lib, N, sc, ops, bn, p, **kw)
        dU, slab = _bwd_drop(lib, N, sc, ops, bn, out, am, dout, p, **kw)
        return out, am, dU, slab
    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert float(a[2].abs().max()) > 0
    other = run(offset=R.OFFSET + 1)
    assert not torch.equal(a[0], other[0])
    plain, _ = _fwd_bn(lib, N, sc, ops, bn)
    assert not torch.equal(a[0], plain)      # the masks act
    rng = torch.tensor([R.SEED, R.OFFSET], dtype=torch.int64, device=DEV)
    dev = run(seed=1, offset=2, rng=rng)       # the by-value pair is ignored
    for x, y in zip(a, dev):
        assert torch.equal(x, y)


# 5, 6 ------------------------------------------------------------------------
def _module_run(net, c):
    h = c["h"].float().to(DEV).requires_grad_(True)
    y = net(h, R.sse_of(c["sizes"]).to(DEV), c["pos"].float().to(DEV))
    (y * c["dout"].float().to(DEV)).sum().backward()
    return y, h.grad


@pytest.mark.parametrize("bn,sizes_id", [(8, 0), (65, 1)])
def test_module_train_matches_yardstick(bn, sizes_id, monkeypatch):
    """PoolHiddenNet(dropout=0.5).train() draws one (seed, offset) from
    K.DROPOUT_RNG and matches the yardstick with that pair's masks."""
    from sgan import kernels as K
    from sgan.models import PoolHiddenNet
    c = R.case(bn, sizes_id, 0.5)
    rng = K.DropoutRng(seed=R.SEED, offset=R.OFFSET)
    monkeypatch.setattr(K, "DROPOUT_RNG", rng)
    net = R.float32_net(c, PoolHiddenNet, 0.5).to(DEV).train()
    y, dh = _module_run(net, c)
    assert rng.offset == R.OFFSET + 1
    close(y, c["ref"].numpy(), rtol=1e-5, what="module out")
    close(dh[0], c["dh"].numpy(), rtol=1e-4, what="module dh")
    fl = 1e-2 * max(float(v.abs().max()) for v in c["dw"].values())
    for k, prm in net.named_parameters():
        close(prm.grad, c["dw"][k].numpy(), rtol=1e-4, floor=fl, what="module d" + k)


@pytest.mark.parametrize("bn,sizes_id", [(8, 0), (65, 1)])
def test_module_eval_is_bitwise_the_dropout0_net(bn, sizes_id, monkeypatch):
    from sgan import kernels as K
    from sgan.models import PoolHiddenNet
    c = R.case(bn, sizes_id, 0.5)
    rng = K.DropoutRng(seed=R.SEED, offset=R.OFFSET)
    monkeypatch.setattr(K, "DROPOUT_RNG", rng)
    net_d = R.float32_net(c, PoolHiddenNet, 0.5).to(DEV).eval()
    net_0 = R.float32_net(c, PoolHiddenNet, 0.0).to(DEV).eval()
    (y_d, dh_d), (y_0, dh_0) = _module_run(net_d, c), _module_run(net_0, c)
    assert rng.offset == R.OFFSET      # nothing drawn
    assert torch.equal(y_d, y_0) and torch.equal(dh_d, dh_0)
    g0 = {k.replace(".2.", ".3."): v.grad for k, v in net_0.named_parameters()}
    for k, prm in net_d.named_parameters():
        assert torch.equal(prm.grad, g0[k]), k


# 7 ---------------------------------------------------------------------------
_GEN_SIZES = [2, 5, 20]


def _grads(mod):
    return {k: v.grad.detach().clone() for k, v in mod.named_parameters() if v.grad is not None}


def test_generator_with_pooling_dropout(monkeypatch):
    """A graph='gat' generator at train.py's sizes, dropout=0.25,
    pool_every_timestep=0, in train().  The reference builds the generator's
    own pool_net without the dropout argument (models.py:769-776) and so do we,
    so the test installs a PoolHiddenNet(dropout=0.25) there; the yardstick is
    the same generator with that pool_net swapped for the float32 torch
    restatement with the explicit masks.  Then eval() through sample_k."""
    from sgan import kernels as K
    from sgan.data.synthetic import synthetic_batch
    from sgan.evaluate import sample_k
    from sgan.models import PoolHiddenNet, TrajectoryGenerator
    p = 0.25
    torch.manual_seed(31)
    g = TrajectoryGenerator(8, 12, embedding_dim=16, encoder_h_dim=32, decoder_h_dim=32, mlp_dim=64, num_layers=1,
                            noise_dim=(8,), noise_type="gaussian", noise_mix_type="global", pooling_type="pool_net",
                            pool_every_timestep=False, dropout=p, bottleneck_dim=8, batch_norm=False,
                            n_units=[40, 16, 40], n_heads=1, dropout1=0.0, alpha=0.2, graph="gat")
    g.pool_net = PoolHiddenNet(16, 32, 64, 8, "relu", False, dropout=p)
    g = g.to(DEV).train()
    g_ref = copy.deepcopy(g)
    g_ref.pool_net = R.torch_pool_net(g.pool_net, p, R.SEED, R.OFFSET, _GEN_SIZES)
    g_ref.train()
    b = [t.to(DEV) for t in synthetic_batch(_GEN_SIZES, seed=29)]
    obs, obs_rel, obs_g, sse = b[0], b[2], b[6], b[10]
    z = torch.randn(len(_GEN_SIZES), 8).to(DEV)
    dy = None
    res = []
    for mod in (g_ref, g):
        monkeypatch.setattr(K, "DROPOUT_RNG", K.DropoutRng(seed=R.SEED, offset=R.OFFSET))
        torch.manual_seed(77)
        y = mod(obs, obs_rel, sse, obs_g, user_noise=z)
        dy = torch.randn_like(y) if dy is None else dy
        (y * dy).sum().backward()
        res.append((y.detach(), _grads(mod)))
    (y_ref, gr_ref), (y, gr) = res
    assert K.DROPOUT_RNG.offset == R.OFFSET + 1 and g_ref.pool_net.masks[0].calls == len(_GEN_SIZES)
    close(y, y_ref.cpu().numpy(), rtol=1e-4, what="G out")
    assert sorted(gr) == sorted(gr_ref) and any(k.startswith("pool_net.mlp_pre_pool.3.") for k in gr)
    fl = 1e-2 * max(float(v.abs().max()) for v in gr_ref.values())
    for k, v in gr_ref.items():
        close(gr[k], v.cpu().numpy(), rtol=1e-3, floor=fl, what="G d" + k)
    g.eval()
    with torch.no_grad():
        out, _ = sample_k(g, b, 3)
    assert out.shape[1:] == (3, sum(_GEN_SIZES), 2) and bool(torch.isfinite(out).all())


# 8 ---------------------------------------------------------------------------
def _loop_restated(dec, pool, last_pos, last_pos_rel, state, sse):
    """Decoder.forward's per-step pooling loop (reference models.py:157-175) in torch ops."""
    B, H, E = last_pos.size(0), dec.h_dim, dec.embedding_dim
    emb = lambda r: F.linear(r, dec.spatial_embedding.weight, dec.spatial_embedding.bias).view(1, B, E)
    x = emb(last_pos_rel)
    outs = []
    for _ in range(dec.seq_len):
        y, state = dec.decoder(x, state)
        rel = F.linear(y.view(-1, H), dec.hidden2pos.weight, dec.hidden2pos.bias)
        last_pos = rel + last_pos
        pooled = pool(state[0], sse, last_pos)
        state = (dec.mlp(torch.cat([state[0].view(-1, H), pooled], 1)).unsqueeze(0), state[1])
        x = emb(rel)
        outs.append(rel.view(B, -1))
    return torch.stack(outs, 0), state[0]


def test_per_step_pooling_decoder_with_dropout(monkeypatch):
    """Decoder(pool_every_timestep=1, dropout=0.25, pred_len=3) in train():
    the per-op loop (the step kernels decline a dropout net), one (seed,
    offset) per step, against the loop restated in torch with the explicit
    pooling masks; decoder.mlp's torch dropout draws the same masks after the
    same torch.manual_seed."""
    from sgan import kernels as K
    from sgan.models import Decoder
    p, T, H = 0.25, 3, 32
    torch.manual_seed(53)
    dec = Decoder(T, embedding_dim=16, h_dim=H, mlp_dim=64, num_layers=1, pool_every_timestep=True, dropout=p,
                  bottleneck_dim=8, activation="relu", batch_norm=False).to(DEV).train()
    assert dec.step_ok() == 0 and dec.pool_net.dropout == p
    pool_ref = R.torch_pool_net(dec.pool_net, p, R.SEED, R.OFFSET, _GEN_SIZES)
    B = sum(_GEN_SIZES)
    sse = R.sse_of(_GEN_SIZES).to(DEV)
    gen = torch.Generator().manual_seed(3)
    ins = [torch.rand(B, 2, generator=gen) * 15, torch.randn(B, 2, generator=gen) * 0.3,
           torch.randn(1, B, H, generator=gen) * 0.5, torch.randn(1, B, H, generator=gen) * 0.5]
    dys = [torch.randn(T, B, 2, generator=gen).to(DEV), torch.randn(1, B, H, generator=gen).to(DEV)]
    res = []
    for ours in (False, True):
        dec.zero_grad(set_to_none=True)
        lp, lpr, h0, c0 = [t.to(DEV).requires_grad_(True) for t in ins]
        monkeypatch.setattr(K, "DROPOUT_RNG", K.DropoutRng(seed=R.SEED, offset=R.OFFSET))
        torch.manual_seed(99)
        if ours:
            rel, hT = dec(lp, lpr, (h0, c0), sse, scenes=_scene_index(_GEN_SIZES))
        else:
            rel, hT = _loop_restated(dec, pool_ref, lp, lpr, (h0, c0), sse)
        ((rel * dys[0]).sum() + (hT * dys[1]).sum()).backward()
        grads = _grads(dec)
        if not ours:      # the restatement's pooling net holds its own copies of the parameters
            grads.update({"pool_net." + k: v for k, v in _grads(pool_ref).items()})
        grads.update({"in%d" % i: t.grad.detach().clone() for i, t in enumerate((lp, lpr, h0, c0))})
        res.append((rel.detach(), hT.detach(), grads))
    (rel_r, h_r, gr_r), (rel, hT, gr) = res
    assert K.DROPOUT_RNG.offset == R.OFFSET + T and pool_ref.masks[0].calls == T * len(_GEN_SIZES)
    close(rel, rel_r.cpu().numpy(), rtol=1e-4, what="decoder rel")
    close(hT, h_r.cpu().numpy(), rtol=1e-4, what="decoder h")
    assert sorted(gr) == sorted(gr_r), sorted(set(gr) ^ set(gr_r))
    fl = 1e-2 * max(float(v.abs().max()) for v in gr_r.values())
    for k, v in gr_r.items():
        close(gr[k], v.cpu().numpy(), rtol=1e-3, floor=fl, what="decoder d" + k)
