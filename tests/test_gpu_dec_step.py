"""Per-step pooling (pool_every_timestep=1) on the row-local step kernels
(csrc/dec_step.hip): the kernels alone against a float64 restatement, the
modules against the reference's fixtures (tests/golden/make_golden_pets.py),
and the host paths around them."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda"
E = 16


def npz(name):
    return np.load(os.path.join(GOLDEN, name))


def T(a, dev=DEV):
    return torch.from_numpy(np.asarray(a)).clone().to(dev)


def close(a, b, rtol, floor=1e-6, what=""):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(np.abs(b).max(), floor)
    err = np.abs(a - b).max() / scale
    assert err <= rtol, "%s max rel err %.3e (scale %.3e)" % (what, err, scale)


def grad_floor(f, prefix, frac=1e-2):
    return frac * max(np.abs(f[k]).max() for k in f.files if k.startswith(prefix))


# ---------------------------------------------------------------------------
# the kernels alone
# ---------------------------------------------------------------------------
STEPS = 3


def _ref_rollout(P, h0, c0, r0, pos0, pools, want_u):
    """float64 restatement of models.py:157-178 around given pool vectors:
    nn.LSTMCell arithmetic on the embedded input, the linear layers."""
    sig = torch.sigmoid
    mlp = lambda x: torch.relu(torch.relu(x @ P["W1"].t() + P["b1"]) @ P["W2"].t() + P["b2"])
    h, c, r, pos = h0, (c0 if c0 is not None else torch.zeros_like(h0)), r0, pos0
    hs, rels, poss, us = [], [], [], []
    for t in range(STEPS):
        hm = h if t == 0 else mlp(torch.cat([h, pools[t - 1]], 1))
        x = r @ P["We"].t() + P["be"]
        gates = x @ P["W_ih"].t() + P["b_ih"] + hm @ P["W_hh"].t() + P["b_hh"]
        i, f, g, o = gates.chunk(4, 1)
        c = sig(f) * c + sig(i) * torch.tanh(g)
        h = sig(o) * torch.tanh(c)
        r = h @ P["Wp"].t() + P["bp"]
        pos = pos + r
        hs.append(h), rels.append(r), poss.append(pos)
        if want_u:
            us.append(h @ P["Wu"].t() + P["cu"])
    return hs, c, rels, poss, us, mlp(torch.cat([h, pools[STEPS - 1]], 1))


def _loss(hs, c, rels, poss, tail, W):
    s = (c * W["c"]).sum() + (tail * W["tail"]).sum()
    for t in range(STEPS):
        s = s + (hs[t] * W["h"][t]).sum() + (rels[t] * W["rel"][t]).sum() + (poss[t] * W["pos"][t]).sum()
    return s


def _ref_run(dtype, P, ins, pools, Wu, cu, W, want_u):
    """The restatement in `dtype` on copies of the operands -> (outputs, {name: gradient})."""
    d = lambda t: t.detach().to(dtype).cpu()
    P2 = {k: d(v).requires_grad_(True) for k, v in P.items()}
    P2["Wu"], P2["cu"] = d(Wu), d(cu)
    ins2 = {k: d(v).requires_grad_(True) for k, v in ins.items()}
    pools2 = [d(p).requires_grad_(True) for p in pools]
    outs = _ref_rollout(P2, ins2["h0"], ins2.get("c0"), ins2["r0"], ins2["pos0"], pools2, want_u)
    hs, c, rels, poss, us, tail = outs
    _loss(hs, c, rels, poss, tail, {k: d(v) for k, v in W.items()}).backward()
    grads = {"d" + k: v.grad for k, v in ins2.items()}
    grads.update({"dpool[%d]" % t: p.grad for t, p in enumerate(pools2)})
    grads.update({"d" + k: P2[k].grad for k in P})
    return outs, grads


def _err(a, b, floor=1e-6):
    a, b = np.asarray(a.detach().cpu(), np.float64), np.asarray(b.detach().cpu(), np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), floor)


@pytest.mark.parametrize("bn,mlp_dim", [(8, 64), (16, 32)])
@pytest.mark.parametrize("H", [16, 32, 48, 64])
@pytest.mark.parametrize("B", [1, 16, 17, 33])
def test_step_kernels_vs_float64(B, H, bn, mlp_dim):
    """Three chained steps (step 0: no mlp; B in {1, 17}: c_prev NULL, else a
    given c0) and the cell-off tail, with U (B in {16, 17}) and without:
    every output, every input gradient (dh_prev, dpool_prev, dc_prev, dr_in,
    dpos_prev) and every parameter gradient through the stacked products.
    Tolerances of test_fused_lstm_vs_oracle: 1e-5 / 1e-4, floor 1e-6.
    The inputs are checked for conditioning as the fixtures are: the same
    restatement in float32 must agree with the float64 one to a tenth of the
    gradient tolerance, else the next seed is taken (a ReLU unit within
    rounding of zero flips between any two float32 implementations)."""
    from sgan import kernels as K
    from sgan.models import make_mlp
    assert K.dec_step_ok(H, bn, mlp_dim) == 3
    want_u, with_c0 = B in (16, 17), B in (16, 33)
    leaf = lambda *s: torch.randn(*s, device=DEV).requires_grad_(True)
    for attempt in range(8):
        torch.manual_seed(100000 * attempt + 1000 * B + 10 * H + bn)
        lstm, emb, proj = nn.LSTM(E, H).to(DEV), nn.Linear(2, E).to(DEV), nn.Linear(H, 2).to(DEV)
        mlp = make_mlp([H + bn, mlp_dim, H], batch_norm=False).to(DEV)
        W1u = (0.3 * torch.randn(512, E + H, device=DEV))
        Wu, cu = W1u[:, E:], 0.3 * torch.randn(512, device=DEV)     # a column block: ldwu != H
        ins = {"h0": leaf(B, H), "r0": leaf(B, 2), "pos0": leaf(B, 2)}
        if with_c0:
            ins["c0"] = leaf(B, H)
        pools = [leaf(B, bn) for _ in range(STEPS)]
        W = {"c": torch.randn(B, H, device=DEV), "tail": torch.randn(B, H, device=DEV),
             "h": torch.randn(STEPS, B, H, device=DEV), "rel": torch.randn(STEPS, B, 2, device=DEV),
             "pos": torch.randn(STEPS, B, 2, device=DEV)}
        P = {"W_ih": lstm.weight_ih_l0, "W_hh": lstm.weight_hh_l0, "b_ih": lstm.bias_ih_l0, "b_hh": lstm.bias_hh_l0,
             "We": emb.weight, "be": emb.bias, "Wp": proj.weight, "bp": proj.bias, "W1": mlp[0].weight,
             "b1": mlp[0].bias, "W2": mlp[2].weight, "b2": mlp[2].bias}
        (rhs, rc, rrels, rposs, rus, rtail), rg = _ref_run(torch.float64, P, ins, pools, Wu, cu, W, want_u)
        _, rg32 = _ref_run(torch.float32, P, ins, pools, Wu, cu, W, want_u)
        cond = max(_err(rg32[k], rg[k]) for k in rg)
        print("B %d H %d bn %d mlp %d attempt %d: float32 vs float64 restatement, worst gradient %.2e"
              % (B, H, bn, mlp_dim, attempt, cond))
        if cond < 1e-5:
            break
    else:
        raise AssertionError("no well-conditioned inputs")
    h0, c0, r0, pos0 = ins["h0"], ins.get("c0"), ins["r0"], ins["pos0"]

    ro = K.dec_rollout(STEPS, B, lstm, emb, proj, mlp, (Wu, cu), True, (h0, c0, r0, pos0), DEV)
    ro.want_u = want_u
    h, c, rel, pos = h0, c0, r0, pos0
    hs, rels, poss, us = [], [], [], []
    for t in range(STEPS):
        h, c, rel, pos, U = K.dec_step(ro, t, h, pools[t - 1] if t else None, c, rel, pos)
        hs.append(h), rels.append(rel), poss.append(pos), us.append(U)
    tail = K.dec_step(ro, STEPS, h, pools[STEPS - 1], None, None, None)
    _loss(hs, c, rels, poss, tail, W).backward()

    for t in range(STEPS):
        close(hs[t], rhs[t], 1e-5, what="h[%d]" % t)
        close(rels[t], rrels[t], 1e-5, what="rel[%d]" % t)
        close(poss[t], rposs[t], 1e-5, what="pos[%d]" % t)
        if want_u:
            close(us[t], rus[t], 1e-5, what="U[%d]" % t)
        else:
            assert us[t] is None
    close(c, rc, 1e-5, what="c")
    close(tail, rtail, 1e-5, what="tail")
    got = {"d" + k: v.grad for k, v in ins.items()}
    got.update({"dpool[%d]" % t: p.grad for t, p in enumerate(pools)})
    got.update({"d" + k: v.grad for k, v in P.items()})
    errs = {k: _err(got[k], rg[k]) for k in rg}
    print("kernel vs float64, worst gradients:", sorted(errs.items(), key=lambda kv: -kv[1])[:4])
    for k in rg:
        close(got[k], rg[k], 1e-4, what=k)


def test_step_backward_that_never_ran_adds_nothing():
    """Gradient reaches step 0 only: the later steps' slices of the stacked
    operand gradients stay zero, so the weight gradients are step 0's."""
    from sgan import kernels as K
    from sgan.models import make_mlp
    torch.manual_seed(5)
    B, H, bn, D = 19, 32, 8, 64
    lstm, emb, proj = nn.LSTM(E, H).to(DEV), nn.Linear(2, E).to(DEV), nn.Linear(H, 2).to(DEV)
    mlp = make_mlp([H + bn, D, H], batch_norm=False).to(DEV)
    u = (torch.randn(512, H, device=DEV), torch.randn(512, device=DEV))
    h0, r0, pos0 = (torch.randn(B, n, device=DEV) for n in (H, 2, 2))
    w = torch.randn(B, 2, device=DEV)
    grads = []
    for steps in (1, 3):
        for p in list(lstm.parameters()) + list(proj.parameters()):
            p.grad = None
        ro = K.dec_rollout(steps, B, lstm, emb, proj, mlp, u, True, (h0,), DEV)
        h, c, rel, pos, rel0 = h0, None, r0, pos0, None
        for t in range(steps):
            h, c, rel, pos, _ = K.dec_step(ro, t, h, torch.randn(B, bn, device=DEV) if t else None, c, rel, pos)
            rel0 = rel if t == 0 else rel0
        (rel0 * w).sum().backward()
        grads.append([p.grad.clone() for p in list(lstm.parameters()) + list(proj.parameters())])
    for a, b in zip(*grads):
        close(b, a, 1e-6, what="weight gradient with idle slices")


# ---------------------------------------------------------------------------
# the modules against the reference's fixtures
# ---------------------------------------------------------------------------
def build_generator():
    from sgan.models import TrajectoryGenerator
    g = TrajectoryGenerator(8, 12, embedding_dim=16, encoder_h_dim=32, decoder_h_dim=32, mlp_dim=64, num_layers=1,
                            noise_dim=(8,), noise_type="gaussian", noise_mix_type="global",
                            pooling_type="pool_net", pool_every_timestep=True, dropout=0.0, bottleneck_dim=8,
                            batch_norm=False, n_units=[40, 16, 40], n_heads=1, dropout1=0.0, alpha=0.2, graph="gat")
    w = npz("weights_pets.npz")
    g.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("g/")})
    return g.to(DEV)


def build_decoder():
    from sgan.models import Decoder
    d = Decoder(12, embedding_dim=16, h_dim=48, mlp_dim=32, num_layers=1, pool_every_timestep=True, dropout=0.0,
                bottleneck_dim=16, activation="relu", batch_norm=False, pooling_type="pool_net")
    f = npz("gen_fwd_pets_dec.npz")
    d.load_state_dict({k[2:]: torch.from_numpy(f[k]) for k in f.files if k.startswith("w/")})
    return d.to(DEV)


def _check_generator(g):
    f = npz("gen_fwd_pets.npz")
    for b in ("synth", "wide"):
        g.zero_grad()
        y = g(T(f[b + "/obs_traj"]), T(f[b + "/obs_traj_rel"]), T(f[b + "/seq_start_end"]), T(f[b + "/obs_traj_g"]),
              user_noise=T(f[b + "/noise"]))
        close(y, f[b + "/out"], rtol=1e-4, what="G %s out" % b)
        (y * T(f[b + "/dout"])).sum().backward()
        fl = grad_floor(f, b + "/dw/")
        seen = 0
        for k, p in g.named_parameters():
            key = b + "/dw/" + k
            if key in f.files:
                assert p.grad is not None, k
                close(p.grad, f[key], rtol=1e-3, floor=fl, what="G %s d%s" % (b, k))
                seen += 1
        assert seen == sum(k.startswith(b + "/dw/") for k in f.files)


def _check_decoder(d):
    f = npz("gen_fwd_pets_dec.npz")
    for b in ("synth", "wide"):
        d.zero_grad()
        h0 = T(f[b + "/h0"]).requires_grad_(True)
        y, _ = d(T(f[b + "/obs_traj"])[-1], T(f[b + "/obs_traj_rel"])[-1], (h0.unsqueeze(0), None),
                 T(f[b + "/seq_start_end"]))
        close(y, f[b + "/out"], rtol=1e-4, what="decoder %s out" % b)
        (y * T(f[b + "/dout"])).sum().backward()
        fl = grad_floor(f, b + "/dw/")
        close(h0.grad, f[b + "/dh0"], rtol=1e-3, floor=1e-2 * np.abs(f[b + "/dh0"]).max(), what="decoder dh0")
        for k, p in d.named_parameters():
            close(p.grad, f[b + "/dw/" + k], rtol=1e-3, floor=fl, what="decoder %s d%s" % (b, k))


def test_generator_vs_reference_fixture():
    g = build_generator()
    assert g.decoder.step_ok() == 3
    _check_generator(g)


def test_decoder_48_32_16_vs_reference_fixture():
    d = build_decoder()
    assert d.step_ok() == 3
    _check_decoder(d)


def test_no_stock_lstm(monkeypatch):
    """The fused loop issues no nn.LSTM call (MIOpen), forward or backward."""
    def boom(self, *a, **k):
        raise AssertionError("nn.LSTM.forward called")
    monkeypatch.setattr(nn.LSTM, "forward", boom)
    _check_generator(build_generator())


def test_switch_off_reproduces_the_fixtures(monkeypatch):
    """SGG_DEC_STEP=0: the per-op loop (stock nn.LSTM, one launch per layer)
    is pinned to the same fixtures at the same tolerances."""
    monkeypatch.setenv("SGG_DEC_STEP", "0")
    calls = []
    orig = nn.LSTM.forward
    monkeypatch.setattr(nn.LSTM, "forward", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
    _check_generator(build_generator())
    assert len(calls) == 2 * 12     # the decoder's, per step and batch; the encoder is fused
    _check_decoder(build_decoder())


def test_mlp_out_of_bounds_runs_on_linear_launches(monkeypatch):
    """sgg_dec_step_ok = 1 (only the mlp out of bounds): decoder.mlp on its own
    Linear launches, the step with its mlp part off -- the same fixtures."""
    from sgan import kernels as K
    monkeypatch.setattr(K, "dec_step_ok", lambda *a, **k: 1)
    _check_decoder(build_decoder())


def test_decode_copies_equals_single_decodes():
    """decode(copies=3) on the replicated scene index = three decode(copies=1)
    calls with the matching noise rows (same math: 1e-4)."""
    g = build_generator()
    f = npz("gen_fwd_pets.npz")
    obs, rel, sse, og = (T(f["synth/" + k]) for k in ("obs_traj", "obs_traj_rel", "seq_start_end", "obs_traj_g"))
    S, B = sse.size(0), obs.size(1)
    torch.manual_seed(3)
    z = torch.randn(3 * S, 8)
    with torch.no_grad():
        ctx = g.context(obs, rel, sse, og)
        y3 = g.decode(ctx, obs, rel, sse, user_noise=z.to(DEV), copies=3)
        assert y3.shape == (12, 3 * B, 2)
        for r in range(3):
            y1 = g.decode(ctx, obs, rel, sse, user_noise=z[r * S:(r + 1) * S].to(DEV))
            close(y3[:, r * B:(r + 1) * B], y1, rtol=1e-4, what="copy %d" % r)


def test_sample_k_runs_the_context_once(monkeypatch):
    """evaluate.sample_k: one context, then decode(copies=k); equal to k
    single-sample generator calls with the same host noise stream."""
    from sgan.evaluate import sample_k
    g = build_generator()
    f = npz("gen_fwd_pets.npz")
    obs, rel, sse, og = (T(f["synth/" + k]) for k in ("obs_traj", "obs_traj_rel", "seq_start_end", "obs_traj_g"))
    batch = (obs, None, rel, None, None, None, og, None, None, None, sse)
    n = []
    orig = g.context
    monkeypatch.setattr(g, "context", lambda *a, **k: (n.append(1), orig(*a, **k))[1])
    with torch.no_grad():
        torch.manual_seed(11)
        out, _ = sample_k(g, batch, 4)
        assert len(n) == 1 and out.shape == (12, 4, obs.size(1), 2)
        torch.manual_seed(11)
        for r in range(4):
            close(out[:, r], g(obs, rel, sse, og), rtol=1e-4, what="sample %d" % r)


# ---------------------------------------------------------------------------
# trainers and evaluation
# ---------------------------------------------------------------------------
KEYS = ["obs_traj", "pred_traj", "obs_traj_rel", "pred_traj_rel", "obs_vel", "pred_vel", "obs_traj_g",
        "pred_traj_g", "non_linear_ped", "loss_mask", "seq_start_end"]


class _Merged:
    """The per-iteration, per-network train-step fixture files as one mapping."""

    def __init__(self):
        self.parts = [npz("train_step_pets_it%d_%s.npz" % (it, n)) for it in range(2) for n in "gd"]
        self.files = [k for p in self.parts for k in p.files]

    def __getitem__(self, k):
        for p in self.parts:
            if k in p.files:
                return p[k]
        raise KeyError(k)


def build_discriminator():
    from sgan.models import TrajectoryDiscriminator
    d = TrajectoryDiscriminator(8, 12, embedding_dim=16, h_dim=48, mlp_dim=64, num_layers=1, batch_norm=False,
                                dropout=0.0, d_type="global")
    w = npz("weights.npz")
    d.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("d/")})
    return d.to(DEV)


def _trainer(**kw):
    from sgan.train_step import GanTrainer, TrainArgs
    g, d = build_generator(), build_discriminator()
    return g, d, GanTrainer(g, d, args=TrainArgs(best_k=3), **kw)


@pytest.mark.parametrize("selective", [True, False])
def test_train_step_vs_reference_fixture(selective):
    """Two reference iterations (discriminator_step + generator_step,
    pool_every_timestep=1, best_k=3, fresh Adam, seeded host RNGs) reproduced
    by GanTrainer, with test_gpu_parity's assertions: losses 1e-4, the
    gradients each optimizer step consumed (check_step_grads), weights within
    2 lr (it + 1).  The second iteration starts from weights Adam moved by the
    sign of noise-level gradient elements; make_golden_pets.py picks the
    batches whose second-iteration gradients the reference itself reproduces
    best under such noise (2.1e-4, a fifth of the tolerance)."""
    import random
    from conftest import check_step_grads
    from sgan.scene import SceneIndex
    g, d, tr = _trainer(selective_backward=selective)
    f = _Merged()
    torch.manual_seed(1234)
    random.seed(1234)
    for it in range(2):
        b = [T(f["b%d/%s" % (it, k)]) for k in KEYS]
        sc = SceneIndex.from_seq_start_end(b[-1], DEV)
        ld, lg = tr.step(b, sc)
        for k, v in list(ld.items()) + list(lg.items()):
            tag = "D" if k.startswith("D") else "G"
            ref = float(f["it%d/%s/%s" % (it, tag, k)])
            assert abs(float(v) - ref) <= 1e-4 * max(1.0, abs(ref)), (it, k, float(v), ref)
        check_step_grads({k: p.grad for k, p in d.named_parameters() if p.grad is not None}, f, it, "D")
        check_step_grads({k: p.grad for k, p in g.named_parameters() if p.grad is not None}, f, it, "G")
        for mod, tag, lr in ((g, "g", 1e-4), (d, "d", 1e-3)):
            for k, v in mod.state_dict().items():
                ref = f["it%d/%s/%s" % (it, tag, k)]
                err = np.abs(v.detach().cpu().numpy().astype(np.float64) - ref).max()
                assert err <= 2 * lr * (it + 1) + 1e-5 * np.abs(ref).max(), (it, tag, k, err)


def _three_iterations(graphed):
    import random
    from sgan.scene import SceneIndex
    from sgan.train_step import GraphedTrainer
    g, d, tr = _trainer(capturable=True)
    f = _Merged()
    b = [T(f["b0/%s" % k]) for k in KEYS]
    sc = SceneIndex.from_seq_start_end(b[-1], DEV)
    torch.manual_seed(7)
    random.seed(7)
    if graphed:
        gt = GraphedTrainer(tr, b, sc, warmup=1)
        hist = [gt.step(), gt.step()]
    else:
        hist = [tr.step(b, sc) for _ in range(3)][1:]
    torch.cuda.synchronize()
    losses = [{k: float(v) for k, v in list(ld.items()) + list(lg.items())} for ld, lg in hist]
    w = {"g." + k: v.detach().cpu().clone() for k, v in g.state_dict().items()}
    w.update({"d." + k: v.detach().cpu().clone() for k, v in d.state_dict().items()})
    return losses, w


def test_graphed_trainer_replays_bit_identical_to_eager():
    """GraphedTrainer on the first fixture batch: a warm-up iteration and two
    replays == three eager iterations from the same state and seeds, bit for bit."""
    la, wa = _three_iterations(False)
    lb, wb = _three_iterations(True)
    assert la == lb, (la, lb)
    for k in wa:
        assert torch.equal(wa[k], wb[k]), (k, (wa[k] - wb[k]).abs().max().item())


def test_evaluate_ade_fde():
    """scripts/evaluate_model.py semantics, 20 samples, seeded host RNG, on the
    eth and hotel test splits: within 1e-3 relative of the reference on CPU."""
    import json
    from sgan.evaluate import evaluate_split
    ev = json.load(open(os.path.join(GOLDEN, "evaluate_pets.json")))
    g = build_generator()
    for split in ("eth", "hotel"):
        torch.manual_seed(0)
        ade, fde = evaluate_split(g, os.path.join(GOLDEN, "datasets_group", split, "test"), num_samples=20)
        ref = ev[split]
        assert abs(ade - ref["ade"]) <= 1e-3 * ref["ade"], (split, ade, ref)
        assert abs(fde - ref["fde"]) <= 1e-3 * ref["fde"], (split, fde, ref)


def test_bucketed_trainer_refuses_before_any_launch(monkeypatch):
    from sgan import _native
    from sgan.train_step import BucketedGraphTrainer
    _g, _d, tr = _trainer()
    lib = _native.load()

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError("launch before the refusal: " + name)
    monkeypatch.setattr(_native, "_lib", NoLaunch())
    try:
        with pytest.raises(NotImplementedError, match="pool_every_timestep"):
            BucketedGraphTrainer(tr, ddset=None)
    finally:
        monkeypatch.setattr(_native, "_lib", lib)
