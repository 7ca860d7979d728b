"""Attention and feature dropout of the GAT families (sgg_dropout,
sgg_gat_fwd_drop / sgg_gat_bwd_drop, the modules in training with dropout1 >
0) against fp64 restatements that apply the host mirror of the mask contract
(sgan.kernels.dropout_keep_host, tests/_dropout_ref.py)."""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_family
from _dropout_ref import batch_gat_ref, close, gat_attention_ref, gat_encoder_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 0xC3A5C85C97CB3127      # (bit 63 set: the key's high word is used)


def _lib():
    from sgan import _native as N
    return N, N.load()


def _rng_dev(seed, offset):
    return torch.from_numpy(np.array([seed, offset], np.uint64).view(np.int64)).to(DEV)


# ---------------------------------------------------------------------------
# 1. sgg_dropout
# ---------------------------------------------------------------------------
def _dropout(x, rows, cols, p, seed, offset, site, y=None, rng_dev=None):
    N, lib = _lib()
    if y is None:
        y = torch.full((rows, cols), float("nan"), device=DEV)
    N.check(lib.sgg_dropout(N.ptr(x), x.stride(0), rows, cols, p, seed, offset, site, N.ptr(rng_dev), N.ptr(y),
                            y.stride(0), N.stream_ptr()), "sgg_dropout")
    return y


def _dropout_want(x, p, seed, offset, site):
    from sgan import kernels as K
    keep = K.dropout_keep_host(p, seed, offset, site, 0, np.arange(x.shape[0]), np.arange(x.shape[1]))
    _, scale = K.dropout_thr_scale_host(p)
    return np.where(keep, x * np.float32(scale), np.float32(0)).astype(np.float32)


@pytest.mark.parametrize("rows,cols,ld", [(37, 40, 40), (5, 3, 3), (37, 40, 44), (37, 38, 41), (130, 72, 72)])
def test_feature_dropout_is_the_host_mask(rows, cols, ld):
    """y is bitwise np.where(keep, x * scale, 0): ragged against the 4 x 4 work
    items and the block, a strided input (ldx > cols, vector and element
    paths), in place, the backward on dy (the same mask), p = 0 (a copy)."""
    torch.manual_seed(rows * 100 + cols)
    buf = torch.randn(rows, ld, device=DEV)
    x = buf[:, :cols]
    xh = x.cpu().numpy()
    p, off, site = 0.3, 5, 9
    y = _dropout(x, rows, cols, p, SEED, off, site)
    want = _dropout_want(xh, p, SEED, off, site)
    assert np.array_equal(y.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert 0.1 < (want == 0).mean() < 0.5
    # the pad columns of the strided input are not touched by an in-place run
    keep_pad = buf[:, cols:].clone()
    dy = torch.randn(rows, cols, device=DEV)
    dx = _dropout(dy, rows, cols, p, SEED, off, site)
    assert np.array_equal(dx.cpu().numpy(), _dropout_want(dy.cpu().numpy(), p, SEED, off, site))
    yd = _dropout(x, rows, cols, 0.9, 1, 2, 3, rng_dev=_rng_dev(SEED, off))     # by-value pair ignored
    assert np.array_equal(yd.cpu().numpy(), _dropout_want(xh, 0.9, SEED, off, 3))
    y0 = _dropout(x, rows, cols, 0.0, SEED, off, site)
    assert np.array_equal(y0.cpu().numpy().view(np.uint32), xh.view(np.uint32))
    _dropout(x, rows, cols, p, SEED, off, site, y=x)
    assert np.array_equal(x.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert torch.equal(buf[:, cols:], keep_pad)


def test_feature_dropout_autograd_and_bad_p():
    from sgan import kernels as K
    from sgan._native import NativeError
    x = torch.randn(9, 24, device=DEV, requires_grad=True)
    drop = (0.5, SEED, 3, 1, 0)
    y = K.feature_dropout(x, drop)
    dy = torch.randn(9, 24, device=DEV)
    (y * dy).sum().backward()
    assert np.array_equal(y.detach().cpu().numpy(), _dropout_want(x.detach().cpu().numpy(), 0.5, SEED, 3, 1))
    assert np.array_equal(x.grad.cpu().numpy(), _dropout_want(dy.cpu().numpy(), 0.5, SEED, 3, 1))
    N, lib = _lib()
    xd = x.detach()
    for bad in (1.0, -0.25, 1.5):
        with pytest.raises(ValueError):
            K.feature_dropout(xd, (bad, SEED, 0, 0, 0))
        assert lib.sgg_dropout(N.ptr(xd), 24, 9, 24, bad, SEED, 0, 0, None, N.ptr(xd), 24, N.stream_ptr()) == -1
    with pytest.raises(NativeError):
        N.check(lib.sgg_dropout(N.ptr(xd), 24, 9, 24, 0.5, SEED, 0, 1 << 24, None, N.ptr(xd), 24, N.stream_ptr()),
                "sgg_dropout")


# ---------------------------------------------------------------------------
# 2. attention forward / backward against the fp64 restatement
# ---------------------------------------------------------------------------
CASES = [
    # heads, F, sizes, mode, epi, bias, pad, p
    (1, 16, [1, 2, 5, 16, 17, 32], 0, 1, False, 0, 0.3),
    (1, 40, [33, 64, 3], 0, 2, False, 0, 0.5),
    (4, 16, [20, 1, 64, 7, 33], 1, 1, True, 3, 0.1),
    (2, 17, [65, 128, 9], 0, 1, False, 0, 0.5),
    (1, 72, [30, 2], 1, 0, True, 0, 0.3),
]


def _case(heads, F, sizes, mode, use_bias, pad):
    from sgan import kernels as K
    torch.manual_seed(heads * 100 + F)
    n_seg = sum(sizes)
    n = n_seg + pad
    seg_off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=DEV)
    labels = None
    if mode == 0:
        rs = np.random.RandomState(F)
        labels = torch.from_numpy(rs.randint(0, 4, n).astype(np.float32)).to(DEV).view(-1, 1)
    graph = K.SegmentGraph(seg_off, len(sizes), max(sizes), mode, labels)
    wh = torch.randn(n, heads * F, device=DEV)
    if pad:
        wh[n_seg:] = 0
    a = torch.randn(heads, 2 * F, device=DEV) * 0.5
    bias = torch.randn(F, device=DEV) * 0.1 if use_bias else None
    dy = torch.randn(n, heads * F, device=DEV)
    dy[n_seg:] = 0      # pad rows are read by no consumer
    return graph, seg_off, labels, wh, a, bias, dy, n_seg


@pytest.mark.parametrize("heads,F,sizes,mode,epi,use_bias,pad,p", CASES)
def test_gat_attention_dropout_vs_torch(heads, F, sizes, mode, epi, use_bias, pad, p):
    """sgg_gat_fwd_drop / sgg_gat_bwd_drop against the fp64 restatement with
    the host mask applied after the softmax, differentiated by autograd: y,
    dWh, da (both a-forms), dbias; pad rows stay exactly zero."""
    from sgan import kernels as K
    graph, seg_off, labels, wh, a, bias, dy, n_seg = _case(heads, F, sizes, mode, use_bias, pad)
    head0 = 2 if heads > 1 else 5
    drop = (p, SEED, 17, 3, head0)
    wr = wh.double().cpu().requires_grad_(True)
    ar = a.double().cpu().requires_grad_(True)
    br = bias.double().cpu().requires_grad_(True) if use_bias else None
    yr = gat_attention_ref(wr, ar, br, labels.cpu() if labels is not None else None, seg_off.cpu(), mode, epi, heads,
                           drop=drop)
    (yr * dy.double().cpu()).sum().backward()
    # the mask bites: the undropped layer is another function
    y_plain = gat_attention_ref(wr.detach(), ar.detach(), br.detach() if use_bias else None,
                                labels.cpu() if labels is not None else None, seg_off.cpu(), mode, epi, heads)
    assert (y_plain - yr.detach()).abs().max() > 1e-3
    for ex in (False, True):
        whg = wh.clone().requires_grad_(True)
        bg = bias.clone().requires_grad_(True) if use_bias else None
        if ex:
            asg = a[:, :F].clone().view(heads, F, 1).requires_grad_(True)
            adg = a[:, F:].clone().view(heads, F, 1).requires_grad_(True)
            y = K.gat_attention_ex(whg, asg, adg, 0.2, graph, epi, heads=heads, bias=bg, drop=drop)
        else:
            ag = a.clone().requires_grad_(True)
            y = K.gat_attention(whg, ag, 0.2, graph, epi, heads=heads, bias=bg, drop=drop)
        (y * dy).sum().backward()
        w = "ex " if ex else ""
        close(y, yr.detach().numpy(), rtol=2e-5, what=w + "y")
        if pad:
            assert torch.equal(y[n_seg:], torch.zeros_like(y[n_seg:]))
            assert torch.equal(whg.grad[n_seg:], torch.zeros_like(whg.grad[n_seg:]))
        close(whg.grad[:n_seg], wr.grad[:n_seg].numpy(), rtol=1e-4, what=w + "dWh")
        da = torch.cat([asg.grad.view(heads, F), adg.grad.view(heads, F)], 1) if ex else ag.grad
        close(da, ar.grad.numpy(), rtol=1e-4, what=w + "da")
        if use_bias:
            close(bg.grad, br.grad.numpy(), rtol=1e-4, what=w + "dbias")


# ---------------------------------------------------------------------------
# 3. bitwise checks of the entry points
# ---------------------------------------------------------------------------
def _raw(case, epi, p, seed, offset, site, head0, rng_dev=None, drop_entry=True):
    """One forward + backward through the C ABI (the `_ex` operand layout) ->
    dict of outputs.  drop_entry False: sgg_gat_fwd_ex / sgg_gat_bwd_ex."""
    N, lib = _lib()
    graph, seg_off, labels, wh, a, bias, dy, _ = case
    heads = a.shape[0]
    n, HF = wh.shape
    F = HF // heads
    a_s, a_d = a[:, :F].contiguous(), a[:, F:].contiguous()
    nseg, max_seg, mode = graph.nseg, graph.max_seg, graph.mode
    o = {k: torch.full((n, HF), float("nan"), device=DEV) for k in ("y", "hp", "dWh")}
    o["da_s"], o["da_d"] = torch.full_like(a_s, float("nan")), torch.full_like(a_d, float("nan"))
    o["dbias"] = torch.full((F,), float("nan"), device=DEV) if bias is not None else None
    work = torch.empty(max(16, int(lib.sgg_gat_bwd_ex_work_bytes(nseg, heads, F))), device=DEV, dtype=torch.uint8)
    st = N.stream_ptr()
    if drop_entry:
        N.check(lib.sgg_gat_fwd_drop(N.ptr(wh), heads, N.ptr(a_s), N.ptr(a_d), F, N.ptr(bias), N.ptr(labels),
                                     N.ptr(seg_off), nseg, n, F, 0.2, mode, epi, max_seg, N.ptr(o["hp"]),
                                     N.ptr(o["y"]), HF, p, seed, offset, site, head0, N.ptr(rng_dev), st),
                "sgg_gat_fwd_drop")
        N.check(lib.sgg_gat_bwd_drop(N.ptr(wh), heads, N.ptr(a_s), N.ptr(a_d), F, N.ptr(labels), N.ptr(seg_off),
                                     nseg, n, F, 0.2, mode, epi, max_seg, N.ptr(o["hp"]), N.ptr(o["y"]), N.ptr(dy),
                                     HF, N.ptr(o["dWh"]), None, None, N.ptr(o["da_s"]), N.ptr(o["da_d"]),
                                     N.ptr(o["dbias"]), N.ptr(work), p, seed, offset, site, head0, N.ptr(rng_dev),
                                     st), "sgg_gat_bwd_drop")
    else:
        N.check(lib.sgg_gat_fwd_ex(N.ptr(wh), heads, N.ptr(a_s), N.ptr(a_d), N.ptr(bias), N.ptr(labels),
                                   N.ptr(seg_off), nseg, n, F, 0.2, mode, epi, max_seg, N.ptr(o["hp"]), N.ptr(o["y"]),
                                   HF, st), "sgg_gat_fwd_ex")
        N.check(lib.sgg_gat_bwd_ex(N.ptr(wh), heads, N.ptr(a_s), N.ptr(a_d), N.ptr(labels), N.ptr(seg_off), nseg, n,
                                   F, 0.2, mode, epi, max_seg, N.ptr(o["hp"]), N.ptr(o["y"]), N.ptr(dy), HF,
                                   N.ptr(o["dWh"]), N.ptr(o["da_s"]), N.ptr(o["da_d"]), N.ptr(o["dbias"]),
                                   N.ptr(work), st), "sgg_gat_bwd_ex")
    torch.cuda.synchronize()
    return {k: v for k, v in o.items() if v is not None}


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("ci", [0, 2])
def test_drop_entry_points_bitwise(ci):
    """p = 0: bitwise sgg_gat_fwd_ex / sgg_gat_bwd_ex; rng_dev == the by-value
    pair; the same arguments twice give the same bits; another offset gives
    another y."""
    heads, F, sizes, mode, epi, use_bias, pad, p = CASES[ci]
    case = _case(heads, F, sizes, mode, use_bias, pad)
    plain = _raw(case, epi, 0.0, 0, 0, 0, 0, drop_entry=False)
    assert not any(bool(torch.isnan(v).any()) for v in plain.values())
    _same(_raw(case, epi, 0.0, SEED, 4, 2, 1), plain)
    one = _raw(case, epi, p, SEED, 4, 2, 1)
    assert not any(bool(torch.isnan(v).any()) for v in one.values())
    _same(_raw(case, epi, p, SEED, 4, 2, 1), one)
    _same(_raw(case, epi, p, 1, 2, 2, 1, rng_dev=_rng_dev(SEED, 4)), one)
    other = _raw(case, epi, p, SEED, 5, 2, 1)
    assert not torch.equal(other["y"], one["y"]) and not torch.equal(other["dWh"], one["dWh"])
    assert not torch.equal(one["y"], plain["y"])


def test_drop_entry_points_refuse_bad_arguments():
    N, lib = _lib()
    heads, F, sizes, mode, epi, use_bias, pad, p = CASES[4]
    graph, seg_off, labels, wh, a, bias, dy, _ = _case(heads, F, sizes, mode, use_bias, pad)
    n, HF = wh.shape
    y = torch.zeros_like(wh)

    def fwd(p, site=0, head0=0, max_seg=graph.max_seg):
        return lib.sgg_gat_fwd_drop(N.ptr(wh), heads, N.ptr(a), N.ptr(a[:, F:]), 2 * F, N.ptr(bias), None,
                                    N.ptr(seg_off), graph.nseg, n, F, 0.2, mode, epi, max_seg, None, N.ptr(y), HF,
                                    p, SEED, 0, site, head0, None, N.stream_ptr())
    assert fwd(0.3) == 0
    for bad in (1.0, -0.5, 2.0):
        assert fwd(bad) == -1
    assert fwd(0.3, site=1 << 24) == -1 and fwd(0.3, head0=256) == -1
    assert fwd(0.3, max_seg=129) == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# 4. modules in training
# ---------------------------------------------------------------------------
def _scene_batch(sizes, seed):
    rs = np.random.RandomState(seed)
    off = np.concatenate([[0], np.cumsum(sizes)])
    labels = rs.randint(0, 4, off[-1]).astype(np.float32)      # 0: a ped in no group
    sse = torch.tensor([[int(off[i]), int(off[i + 1])] for i in range(len(sizes))])
    return off, labels, sse


def _check_module(mod, run, ref_fn, x, rng_args):
    """run(mod, x) on the GPU in training against ref_fn(fp64 copy, x64, rng)."""
    torch.manual_seed(2)
    ref = copy.deepcopy(mod).cpu().double()
    xg = x.clone().to(DEV).requires_grad_(True)
    y = run(mod, xg)
    dy = torch.randn(y.shape)
    (y * dy.to(DEV)).sum().backward()
    xr = x.double().requires_grad_(True)
    yr = ref_fn(ref, xr, rng_args)
    (yr * dy.double()).sum().backward()
    close(y, yr.detach().numpy(), rtol=1e-4, what="out")
    grads = dict(ref.named_parameters())
    fl = 1e-2 * max(float(p.grad.abs().max()) for p in grads.values())
    close(xg.grad, xr.grad.numpy(), rtol=1e-3, floor=1e-2 * float(xr.grad.abs().max()), what="dx")
    for k, p in mod.named_parameters():
        assert p.grad is not None and grads[k].grad is not None, k
        close(p.grad, grads[k].grad.numpy(), rtol=1e-3, floor=fl, what="d" + k)
    return y.detach()


@pytest.mark.parametrize("n_heads", [1, 2])
def test_gat_encoder_training_dropout(n_heads, monkeypatch):
    from sgan import kernels as K
    from sgan import models as M
    torch.manual_seed(10 + n_heads)
    mod = M.GATEncoder([40, 16, 40], n_heads, 0.3, 0.2).to(DEV).train()
    off, labels, sse = _scene_batch([3, 7, 20], 5)
    assert (labels == 0).any() and len(set(labels[labels != 0])) > 1
    x = torch.randn(int(off[-1]), 40)
    lab = torch.from_numpy(labels).to(DEV)
    pos = torch.zeros(int(off[-1]), 2, device=DEV)
    monkeypatch.setattr(K, "DROPOUT_RNG", K.DropoutRng(seed=SEED, offset=11))
    run = lambda m, xx: m(xx, sse.to(DEV), pos, lab)   # noqa: E731
    y1 = _check_module(mod, run, lambda r, xr, rng: gat_encoder_ref(r, xr, labels, off, rng), x, (0.3, SEED, 11))
    # the next forward draws the next offset
    with torch.no_grad():
        y2 = run(mod, x.to(DEV))
        close(y2, gat_encoder_ref(copy.deepcopy(mod).cpu().double(), x.double(), labels, off, (0.3, SEED, 12)),
              rtol=1e-4, what="second forward")
    assert not torch.equal(y1, y2)
    # eval: bitwise the module without dropout
    plain = M.GATEncoder([40, 16, 40], n_heads, 0.0, 0.2).to(DEV).eval()
    plain.load_state_dict(mod.state_dict())
    with torch.no_grad():
        assert torch.equal(run(mod.eval(), x.to(DEV)), run(plain, x.to(DEV)))


def test_batch_gat_encoder_training_dropout(monkeypatch):
    from sgan import kernels as K
    from sgan import models as M
    torch.manual_seed(20)
    mod = M.BatchGATEncoder([40, 16, 40], [4, 1], 0.3, 0.2).to(DEV).train()
    with torch.no_grad():
        for l in mod.gat_net.layer_stack:
            l.bias.normal_(0, 0.1)
    off, _, sse = _scene_batch([5, 20, 33], 6)
    x = torch.randn(int(off[-1]), 40)
    monkeypatch.setattr(K, "DROPOUT_RNG", K.DropoutRng(seed=SEED, offset=40))
    run = lambda m, xx: m(xx, sse.to(DEV))   # noqa: E731
    y1 = _check_module(mod, run, lambda r, xr, rng: batch_gat_ref(r, xr, off, rng), x, (0.3, SEED, 40))
    with torch.no_grad():
        y2 = run(mod, x.to(DEV))
    assert not torch.equal(y1, y2)
    # forward_pair: separate offsets for its two batches (41 is y2's)
    from sgan.scene import SceneIndex
    sc = SceneIndex.from_seq_start_end(sse.to(DEV), DEV)
    with torch.no_grad():
        ya, yb = mod.forward_pair(x.to(DEV), sc, x.to(DEV), sc)
    ref = copy.deepcopy(mod).cpu().double()
    close(ya, batch_gat_ref(ref, x.double(), off, (0.3, SEED, 42)).detach().numpy(), rtol=1e-4, what="pair a")
    close(yb, batch_gat_ref(ref, x.double(), off, (0.3, SEED, 43)).detach().numpy(), rtol=1e-4, what="pair b")
    plain = M.BatchGATEncoder([40, 16, 40], [4, 1], 0.0, 0.2).to(DEV).eval()
    plain.load_state_dict(mod.state_dict())
    with torch.no_grad():
        assert torch.equal(run(mod.eval(), x.to(DEV)), run(plain, x.to(DEV)))


# ---------------------------------------------------------------------------
# 5. the generator
# ---------------------------------------------------------------------------
def _generator(dropout1):
    from sgan.models import TrajectoryGenerator
    g = TrajectoryGenerator(8, 12, embedding_dim=16, encoder_h_dim=32, decoder_h_dim=32, mlp_dim=64, num_layers=1,
                            noise_dim=(8,), noise_type="gaussian", noise_mix_type="global",
                            pooling_type="pool_net", pool_every_timestep=False, dropout=0.0, bottleneck_dim=8,
                            batch_norm=False, n_units=[40, 16, 40], n_heads=1, dropout1=dropout1, alpha=0.2,
                            graph="gat")
    w = np.load(os.path.join(GOLDEN, "weights.npz"))
    load_family(g, {k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("g/")})
    return g.to(DEV).train()


def test_generator_trains_with_dropout1(monkeypatch):
    from sgan import kernels as K
    f = np.load(os.path.join(GOLDEN, "train_step.npz"))
    b = {k: torch.from_numpy(f["b0/" + k]).to(DEV) for k in ("obs_traj", "obs_traj_rel", "seq_start_end", "obs_traj_g")}
    assert b["seq_start_end"].shape[0] == 6

    def step(dropout1):
        g = _generator(dropout1)
        torch.manual_seed(7)
        monkeypatch.setattr(K, "DROPOUT_RNG", K.DropoutRng())
        out = g(b["obs_traj"], b["obs_traj_rel"], b["seq_start_end"], b["obs_traj_g"])
        out.square().sum().backward()
        torch.cuda.synchronize()
        return out.detach(), {k: p.grad.clone() for k, p in g.named_parameters() if p.grad is not None}
    out0, g0 = step(0.0)
    out1, g1 = step(0.2)
    assert bool(torch.isfinite(out1).all()) and not torch.equal(out0, out1)
    for k in g0:
        assert k in g1 and bool(torch.isfinite(g1[k]).all()), k
    assert any(float(v.abs().max()) > 0 for k, v in g1.items() if k.startswith("gatencoder."))
    out2, g2 = step(0.2)
    assert torch.equal(out1, out2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


# ---------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------
def test_dropout_refuses_wide_segments_before_any_launch(monkeypatch):
    from sgan import _native as N
    from sgan import models as M
    launches = []
    real = N.check
    monkeypatch.setattr(N, "check", lambda rc, name: (launches.append(name), real(rc, name))[1])
    sse = torch.tensor([[0, 129], [129, 140]], device=DEV)
    x = torch.randn(140, 40, device=DEV)
    lab = torch.zeros(140, device=DEV)
    pos = torch.zeros(140, 2, device=DEV)
    enc = M.GATEncoder([40, 16, 40], 1, 0.3, 0.2).to(DEV).train()
    with pytest.raises(NotImplementedError, match="128"):
        enc(x, sse, pos, lab)
    bat = M.BatchGATEncoder([40, 16, 40], [4, 1], 0.3, 0.2).to(DEV).train()
    with pytest.raises(NotImplementedError, match="128"):
        bat(x, sse)
    assert launches == []
    with torch.no_grad():      # eval takes the wide kernels as before
        assert bool(torch.isfinite(bat.eval()(x, sse)).all())
    assert launches


def test_gan_trainer_refuses_dropout1():
    from sgan.models import TrajectoryDiscriminator
    from sgan.train_step import GanTrainer
    d = TrajectoryDiscriminator(8, 12, embedding_dim=16, h_dim=48, mlp_dim=64, num_layers=1, batch_norm=False,
                                dropout=0.0, d_type="global").to(DEV)
    with pytest.raises(NotImplementedError, match="dropout1"):
        GanTrainer(_generator(0.2), d)
    GanTrainer(_generator(0.0), d)
