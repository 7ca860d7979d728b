"""Graph attention for segments of 129 to 1024 nodes (sgg_gat_fwd_wide /
sgg_gat_bwd_wide): against the LDS-resident kernels where both apply, an
fp64 torch restatement above their bound, the reference's fixtures, and
through the modules, the gat generator, a training step and evaluation."""
import random

import numpy as np
import pytest
import torch

from conftest import RecordingAdam
from test_gpu_parity import DEV, T, _batch_gat_ref, _gat_attention_ref, build_models, close, grad_floor, npz

pytestmark = pytest.mark.gpu


def _seg_off(sizes):
    return torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=DEV)


def _labels(sizes, n, seed):
    """Mode-0 labels in {0 .. 3} with, where the largest segment allows it,
    one label (7) shared by 129 of its nodes; at least one node has label 0."""
    rs = np.random.RandomState(seed)
    lab = rs.randint(0, 4, n).astype(np.float32)
    g = int(np.argmax(sizes))
    o = int(np.sum(sizes[:g]))
    if sizes[g] >= 129:
        lab[o + rs.permutation(sizes[g])[:129]] = 7.0
    if not (lab[:sum(sizes)] == 0).any():
        lab[sum(sizes) - 1 if g + 1 < len(sizes) else 0] = 0.0
    return torch.from_numpy(lab).to(DEV).view(-1, 1)


# 1 ---------------------------------------------------------------------------
def _st_ref(wh, s, t, labels, so, mode, epi, heads, alpha=0.2):
    """_gat_attention_ref with the scores s, t (n x heads) as inputs of their
    own, so that autograd gives the kernel's ds, dt."""
    F = wh.shape[1] // heads
    rows = []
    for g in range(len(so) - 1):
        o, e = so[g], so[g + 1]
        cols = []
        for h in range(heads):
            W = wh[o:e, h * F:(h + 1) * F]
            z = torch.nn.functional.leaky_relu(s[o:e, h, None] + t[None, o:e, h], alpha)
            if mode == 0:
                lab = labels[o:e].view(-1)
                m = ((lab[:, None] == lab[None, :]) & (lab[:, None] != 0)) | torch.eye(e - o, dtype=torch.bool,
                                                                                      device=wh.device)
                z = z.masked_fill(~m, float("-inf"))
            out = torch.softmax(z, 1) @ W
            if epi:
                out = torch.nn.functional.elu(out)
            if epi == 2:
                out = torch.log_softmax(out, 1)
            cols.append(out)
        rows.append(torch.cat(cols, 1))
    return torch.cat(rows, 0)


@pytest.mark.parametrize("heads,F,epi", [(2, 17, 1), (1, 40, 2)])
def test_wide_equals_resident_where_both_apply(heads, F, epi):
    """Direct C-ABI calls on segments of <= 128 nodes (label mask): y and hp
    of the wide forward are bitwise the resident kernel's.  The wide backward
    sums in another order than the resident one (row statistics from the
    forward, i tiles of 64), so dWh, ds and dt of both are measured against an
    fp64 restatement: the wide kernel's max error is at most twice the
    resident kernel's plus 1e-6 of the tensor's scale (test_pool_x3_vs_fp32's
    rule for two fp32 forms with different summation orders)."""
    from sgan import _native as N
    lib = N.load()
    sizes = [100, 128, 9, 1, 64, 65]
    n, HF = sum(sizes), heads * F
    off = _seg_off(sizes)
    torch.manual_seed(heads * 100 + F)
    labels = _labels(sizes, n, F)
    wh = torch.randn(n, HF, device=DEV)
    a = torch.randn(heads, 2 * F, device=DEV) * 0.5
    dy = torch.randn(n, HF, device=DEV)
    af = a.view(-1)
    res = {}
    for wide in (False, True):
        y, hp = torch.full((n, HF), 7.0, device=DEV), torch.full((n, HF), 7.0, device=DEV)
        dWh = torch.full((n, HF), 7.0, device=DEV)
        ds, dt = torch.full((n, heads), 7.0, device=DEV), torch.full((n, heads), 7.0, device=DEV)
        if wide:
            work = torch.empty(int(lib.sgg_gat_wide_work_floats(n, len(sizes), heads, F, 128)), device=DEV)
            N.check(lib.sgg_gat_fwd_wide(N.ptr(wh), heads, N.ptr(af), N.ptr(af[F:]), 2 * F, None, N.ptr(labels),
                                         N.ptr(off), len(sizes), n, F, 0.2, 0, epi, 128, N.ptr(hp), N.ptr(y), HF,
                                         N.ptr(work), N.stream_ptr()), "sgg_gat_fwd_wide")
            N.check(lib.sgg_gat_bwd_wide(N.ptr(wh), heads, N.ptr(af), N.ptr(af[F:]), 2 * F, N.ptr(labels), N.ptr(off),
                                         len(sizes), n, F, 0.2, 0, epi, 128, N.ptr(hp), N.ptr(y), N.ptr(dy), HF,
                                         N.ptr(dWh), N.ptr(ds), N.ptr(dt), None, None, None, N.ptr(work),
                                         N.stream_ptr()), "sgg_gat_bwd_wide")
        else:
            N.check(lib.sgg_gat_fwd(N.ptr(wh), heads, N.ptr(af), None, N.ptr(labels), N.ptr(off), len(sizes), n, F,
                                    0.2, 0, epi, 128, N.ptr(hp), N.ptr(y), HF, N.stream_ptr()), "sgg_gat_fwd")
            N.check(lib.sgg_gat_bwd(N.ptr(wh), heads, N.ptr(af), N.ptr(labels), N.ptr(off), len(sizes), n, F, 0.2, 0,
                                    epi, 128, N.ptr(hp), N.ptr(y), N.ptr(dy), HF, N.ptr(dWh), N.ptr(ds), N.ptr(dt),
                                    N.stream_ptr()), "sgg_gat_bwd")
        res[wide] = dict(y=y, hp=hp, dWh=dWh, ds=ds, dt=dt)
    assert torch.equal(res[True]["y"], res[False]["y"])
    assert torch.equal(res[True]["hp"], res[False]["hp"])
    # fp64: dWh through the whole layer; ds, dt with the scores as inputs
    wr = wh.double().requires_grad_(True)
    yr = _gat_attention_ref(wr, a.double(), None, labels, off, 0, epi, heads)
    (yr * dy.double()).sum().backward()
    w64, a64 = wh.double(), a.double().view(heads, 2, F)
    s = torch.einsum("nhf,hf->nh", w64.view(n, heads, F), a64[:, 0]).requires_grad_(True)
    t = torch.einsum("nhf,hf->nh", w64.view(n, heads, F), a64[:, 1]).requires_grad_(True)
    (_st_ref(w64, s, t, labels, off.tolist(), 0, epi, heads) * dy.double()).sum().backward()
    for name, ref in (("dWh", wr.grad), ("ds", s.grad), ("dt", t.grad)):
        scale = float(ref.abs().max())
        er = float((res[False][name].double() - ref).abs().max())
        ew = float((res[True][name].double() - ref).abs().max())
        print("%s: resident err %.3e, wide err %.3e (scale %.3e)" % (name, er, ew, scale))
        assert ew <= 2 * er + 1e-6 * scale, "%s: wide err %.3e vs resident %.3e (scale %.3e)" % (name, ew, er, scale)


# 2, 3 ------------------------------------------------------------------------
def _check_vs_fp64(heads, F, sizes, mode, epi, use_bias, pad):
    """test_gat_attention_vs_torch's comparison and tolerances (y 2e-5, dWh /
    da / dbias 1e-4) through K.gat_attention and K.gat_attention_ex."""
    from sgan import kernels as K
    torch.manual_seed(heads * 100 + F + len(sizes))
    n_seg = sum(sizes)
    n = n_seg + pad
    seg_off = _seg_off(sizes)
    labels = _labels(sizes, n, F) if mode == 0 else None
    if mode == 0:
        lab = labels[:n_seg].view(-1)
        assert bool((lab == 0).any()) and (max(sizes) < 129 or int((lab == 7).sum()) > 128)
    graph = K.SegmentGraph(seg_off, len(sizes), max(sizes), mode, labels)
    assert K.gat_is_wide(graph)
    wh = torch.randn(n, heads * F, device=DEV)
    if pad:
        wh[n_seg:] = 0
    a = torch.randn(heads, 2 * F, device=DEV) * 0.5
    bias = torch.randn(F, device=DEV) * 0.1 if use_bias else None
    dy = torch.randn(n, heads * F, device=DEV)
    dy[n_seg:] = 0      # pad rows are read by no consumer
    wr = wh.double().requires_grad_(True)
    ar = a.double().requires_grad_(True)
    br = bias.double().requires_grad_(True) if use_bias else None
    yr = _gat_attention_ref(wr, ar, br, labels, seg_off, mode, epi, heads)
    (yr * dy.double()).sum().backward()
    for ex in (False, True):
        whg = wh.clone().requires_grad_(True)
        bg = bias.clone().requires_grad_(True) if use_bias else None
        if ex:
            asg = a[:, :F].clone().view(heads, F, 1).requires_grad_(True)
            adg = a[:, F:].clone().view(heads, F, 1).requires_grad_(True)
            y = K.gat_attention_ex(whg, asg, adg, 0.2, graph, epi, heads=heads, bias=bg)
        else:
            ag = a.clone().requires_grad_(True)
            y = K.gat_attention(whg, ag, 0.2, graph, epi, heads=heads, bias=bg)
        (y * dy).sum().backward()
        w = "ex " if ex else ""
        close(y, yr.detach().cpu().numpy(), rtol=2e-5, what=w + "y")
        if pad:
            assert torch.equal(y[n_seg:], torch.zeros_like(y[n_seg:]))
            assert torch.equal(whg.grad[n_seg:], torch.zeros_like(whg.grad[n_seg:]))
        close(whg.grad[:n_seg], wr.grad[:n_seg].cpu().numpy(), rtol=1e-4, what=w + "dWh")
        da = torch.cat([asg.grad.view(heads, F), adg.grad.view(heads, F)], 1) if ex else ag.grad
        close(da, ar.grad.cpu().numpy(), rtol=1e-4, what=w + "da")
        if use_bias:
            close(bg.grad, br.grad.cpu().numpy(), rtol=1e-4, what=w + "dbias")


@pytest.mark.parametrize("sizes,pad", [([129, 1], 0), ([191, 192, 193, 2], 0), ([257, 64], 3)])
@pytest.mark.parametrize("heads,F,mode,epi,use_bias", [
    (1, 72, 0, 1, False),    # the GAT family's hidden layer
    (1, 16, 0, 2, False),    # its output layer: log_softmax epilogue
    (4, 16, 1, 1, True),     # configs[4] batched GAT, layer 1
    (1, 128, 1, 0, True),    # widest F
    (2, 17, 0, 1, False),    # F not a multiple of 4
])
def test_gat_wide_vs_fp64(heads, F, mode, epi, use_bias, sizes, pad):
    """Segments around the 64-node tile edges above the resident bound (one
    and several tiles, a partial last tile, a 1- / 2- / 64-node segment in the
    same graph, pad rows past the last segment) against the fp64 torch
    restatement, forward and backward, both autograd functions."""
    _check_vs_fp64(heads, F, sizes, mode, epi, use_bias, pad)


def test_gat_wide_upper_bound():
    """A 1024-node segment (the bound) beside a 3-node one; one more node
    raises a ValueError from Python before any launch."""
    from sgan import kernels as K
    from sgan.models import BatchGATEncoder, GATEncoder
    from sgan.scene import SceneIndex
    _check_vs_fp64(1, 16, [1024, 3], 1, 1, False, 0)
    big = SceneIndex(np.array([0, 1025]), DEV)
    with pytest.raises(ValueError, match="1024"):
        K.gat_is_wide(K.SegmentGraph(big.scene_off, 1, 1025, 1, None))
    x = torch.zeros(1025, 40, device=DEV)
    with pytest.raises(ValueError, match="1024"):
        GATEncoder([40, 16, 40], 1, 0.0, 0.2).to(DEV)(x, None, None, torch.zeros(1025, 1, device=DEV), scenes=big)
    with pytest.raises(ValueError, match="1024"):
        BatchGATEncoder([40, 16, 40], [4, 1], 0.0, 0.2).to(DEV)(x, None, scenes=big)


# 4 ---------------------------------------------------------------------------
def test_gat_encoder_wide_vs_reference_fixture():
    """The reference's GATEncoder (two heads) on scenes of 200 (everybody
    ungrouped: a 200-node inter-group segment), 130 (one group), 150 and 20
    peds; test_graph_module_vs_reference_fixture's tolerances."""
    from sgan.models import GATEncoder
    f = npz("gat_encoder_wide.npz")
    mod = GATEncoder([40, 16, 40], 2, 0.0, 0.2)
    mod.load_state_dict({k[2:]: torch.from_numpy(f[k]) for k in f.files if k.startswith("w/")})
    mod = mod.to(DEV)
    x = T(f["x"]).requires_grad_(True)
    y = mod(x, T(f["sse"]), None, T(f["labels"]).view(-1, 1))
    close(y, f["out"], rtol=1e-5, what="out")
    (y * T(f["dout"])).sum().backward()
    close(x.grad, f["dx"], rtol=1e-4, what="dx")
    fl = grad_floor(f, "dw/")
    for k, p in mod.named_parameters():
        if "dw/" + k in f.files:
            close(p.grad, f["dw/" + k], rtol=2e-4, floor=fl, what="d" + k)


def test_batch_gat_encoder_wide_vs_fp64():
    """The sgangat batched GAT (configs[4]: units 40-16-40, heads 4, 1) on
    scenes of 130, 200 and 2 peds -- the per-op path, sgg_gat_layer_fwd stops
    at 128 -- against _batch_gat_ref in fp64, at the sgangat module test's
    tolerances (out 1e-5, dx 1e-4, parameters 2e-4, layer 0's near-cancelling
    bias gradient 1e-3, on grad_floor's scale)."""
    from sgan.models import BatchGATEncoder
    from sgan.scene import SceneIndex
    sizes = [130, 200, 2]
    torch.manual_seed(len(sizes))
    mod = BatchGATEncoder([40, 16, 40], [4, 1], 0.0, 0.2).to(DEV)
    with torch.no_grad():
        for l in mod.gat_net.layer_stack:
            l.bias.normal_(0, 0.1)
    off = np.concatenate([[0], np.cumsum(sizes)])
    sc = SceneIndex(off, DEV)
    x = torch.randn(sum(sizes), 40, device=DEV)
    dy = torch.randn(sum(sizes), 40, device=DEV)
    xi = x.clone().requires_grad_(True)
    y = mod(xi, None, scenes=sc)
    (y * dy).sum().backward()
    ref = BatchGATEncoder([40, 16, 40], [4, 1], 0.0, 0.2).to(DEV).double()
    ref.load_state_dict({k: v.double() for k, v in mod.state_dict().items()})
    xr = x.double().requires_grad_(True)
    yr = _batch_gat_ref(xr, ref, torch.from_numpy(off))
    (yr * dy.double()).sum().backward()
    close(y, yr.detach().cpu().numpy(), rtol=1e-5, what="out")
    close(xi.grad, xr.grad.cpu().numpy(), rtol=1e-4, what="dx")
    rg = {k: p.grad.cpu().numpy() for k, p in ref.named_parameters()}
    fl = 1e-2 * max(float(np.abs(v).max()) for v in rg.values())
    for k, p in mod.named_parameters():
        close(p.grad, rg[k], rtol=1e-3 if k.endswith("0.bias") else 2e-4, floor=fl, what="d" + k)


# 5 ---------------------------------------------------------------------------
def test_generator_gat_wide_vs_reference_fixture():
    """The gat generator on a batch with 129- and 200-ped scenes,
    test_generator_vs_reference_fixture's tolerances."""
    g, _ = build_models("gat")
    f = npz("gen_fwd_gat_wide.npz")
    y = g(T(f["obs_traj"]), T(f["obs_traj_rel"]), T(f["seq_start_end"]), T(f["obs_traj_g"]), user_noise=T(f["noise"]))
    close(y, f["gat/out"], rtol=1e-4, what="G out")
    (y * T(f["gat/dout"])).sum().backward()
    fl = grad_floor(f, "gat/dw/")
    for k, p in g.named_parameters():
        key = "gat/dw/" + k
        if key in f.files:
            close(p.grad, f[key], rtol=1e-3, floor=fl, what="G d" + k)


# 6 ---------------------------------------------------------------------------
def test_gat_wide_train_step_vs_oracle():
    """One GanTrainer iteration (D-step + G-step, best_k 20) of the gat
    family on scenes of 130, 5 and 20 peds against the oracle's
    reference-formulation steps from the same seeds: losses, the gradients
    each optimizer step consumed, weights (test_gcn_wide_train_step_vs_oracle's
    assertions and tolerances)."""
    from oracle import sgan_oracle as O
    from sgan.data.synthetic import synthetic_batch
    from sgan.scene import SceneIndex
    from sgan.train_step import GanTrainer
    from test_gpu_configs import reference_gd
    g, d = reference_gd("gat")
    og, od = O.build_default("gat")
    og.load_state_dict({k: v.detach().cpu() for k, v in g.state_dict().items()})
    od.load_state_dict({k: v.detach().cpu() for k, v in d.state_dict().items()})
    oog = RecordingAdam.make(og.named_parameters(), lr=1e-4)
    ood = RecordingAdam.make(od.named_parameters(), lr=1e-3)
    tr = GanTrainer(g, d)
    b = synthetic_batch([130, 5, 20], seed=700)
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


# 7 ---------------------------------------------------------------------------
def test_sample_k_gat_wide_equals_separate_calls():
    """evaluate.sample_k (context once, k rollouts) on a batch with a 130-ped
    scene equals k separate generator calls fed the same noise rows."""
    from sgan import evaluate
    from sgan.data.synthetic import synthetic_batch
    from sgan.scene import SceneIndex
    g, _ = build_models("gat")
    batch = synthetic_batch([130, 20], seed=8, device=DEV)
    k, S = 3, 2
    with torch.no_grad():
        torch.manual_seed(4)
        out, _ = evaluate.sample_k(g, batch, k)
        torch.manual_seed(4)
        sc = SceneIndex(np.array([0, 130, 150]), DEV)
        z = evaluate.draw_sample_noise(g, sc, 150, k)
        for r in range(k):
            y = g(batch[0], batch[2], batch[-1], batch[6], user_noise=z[r * S:(r + 1) * S])
            close(out[:, r], y.cpu().numpy(), rtol=1e-6, what="sample %d" % r)
