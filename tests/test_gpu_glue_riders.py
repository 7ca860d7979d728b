"""The two per-scene L2 glue launches of a training iteration (sgg_l2_select,
sgg_l2_loss_bwd_scenes) riding as extra workgroups of an LSTM encoder launch
(sgg_lstm_fwd_seg_glue, kernels.GlueRider): bit-identical to the stand-alone
launches at the kernel level and over whole trainer steps, and flushed on
their own wherever no carrier comes."""
import random

import numpy as np
import pytest
import torch

from test_gpu_parity import DEV, build_models, close

pytestmark = pytest.mark.gpu

H, TL, T0 = 48, 20, 8                      # a 20-step H = 48 sequence continued from step 8
SIZES = [20, 7, 13, 20, 2, 1, 64]          # the glue body's scenes: a 1-ped scene, the largest mask stage
TP = TL - T0                               # prediction steps of the glue body (12)

_CACHE = {}


def _lstm(B):
    """Weights, input and the states after the first T0 steps (run once per B
    and never modified: every arm continues from a clone)."""
    if B in _CACHE:
        return _CACHE[B]
    from sgan import _native as N
    from sgan import kernels as K
    lib = K._lib()
    gen = torch.Generator(device="cpu").manual_seed(100 + B)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, generator=gen) * sc).to(DEV)
    rel, A, Whh, bias = rnd(TL, B, 2, sc=0.5), rnd(4 * H, 2, sc=0.3), rnd(4 * H, H, sc=0.1), rnd(4 * H, sc=0.1)
    h_all = torch.zeros(TL + 1, B, H, device=DEV)
    c_all = torch.zeros(int(lib.sgg_lstm_state_floats(TL, B, H, 1)), device=DEV)
    act = torch.zeros(int(lib.sgg_lstm_state_floats(TL, B, H, 0)), device=DEV)
    seg = N.LstmSeg(N.ptr(rel), N.ptr(A), N.ptr(Whh), N.ptr(bias), None, None, T0, B, B, 0, TL, B, N.ptr(h_all),
                    N.ptr(c_all), N.ptr(act), None, 0, None, 0, None)
    N.check(lib.sgg_lstm_fwd_seg(N.ctypes.byref(seg), H, N.stream_ptr()), "sgg_lstm_fwd_seg")
    torch.cuda.synchronize()
    _CACHE[B] = (rel, A, Whh, bias, h_all, c_all, act)
    return _CACHE[B]


def _glue_inputs():
    """gt, mask (some zero steps, scene 2 all zero), scene offsets of SIZES."""
    if "glue" in _CACHE:
        return _CACHE["glue"]
    Bg = sum(SIZES)
    off = np.concatenate([[0], np.cumsum(SIZES)])
    gen = torch.Generator(device="cpu").manual_seed(7)
    gt = torch.randn(TP, Bg, 2, generator=gen).to(DEV)
    lm = (torch.rand(Bg, T0 + TP, generator=gen) > 0.25).float()
    lm[off[2]:off[3]] = 0.0
    lm = lm.to(DEV)
    pred_k = torch.randn(TP, 20 * Bg, 2, generator=gen).to(DEV)     # up to 20 samples
    wide = torch.randn(TP, 2 * Bg, 2, generator=gen).to(DEV)        # the backward reads its first Bg columns
    so = torch.tensor(off, dtype=torch.int32, device=DEV)
    _CACHE["glue"] = (gt, lm[:, T0:], so, pred_k, wide)
    return _CACHE["glue"]


def _continue(B, glue):
    """Steps T0 .. TL - 1 on clones of the prefix states -> (h_all, c_all, act);
    glue: a SggGlueSeg for sgg_lstm_fwd_seg_glue, or None for sgg_lstm_fwd_seg."""
    from sgan import _native as N
    from sgan import kernels as K
    lib = K._lib()
    rel, A, Whh, bias, h0, c0, a0 = _lstm(B)
    h_all, c_all, act = h0.clone(), c0.clone(), a0.clone()
    seg = N.LstmSeg(N.ptr(rel), N.ptr(A), N.ptr(Whh), N.ptr(bias), None, None, TP, B, B, T0, TL, B, N.ptr(h_all),
                    N.ptr(c_all), N.ptr(act), None, 0, None, 0, None)
    if glue is None:
        N.check(lib.sgg_lstm_fwd_seg(N.ctypes.byref(seg), H, N.stream_ptr()), "sgg_lstm_fwd_seg")
    else:
        N.check(lib.sgg_lstm_fwd_seg_glue(N.ctypes.byref(seg), H, N.ctypes.byref(glue), N.stream_ptr()),
                "sgg_lstm_fwd_seg_glue")
    torch.cuda.synchronize()
    return h_all, c_all, act


def _plain(B):
    if ("plain", B) not in _CACHE:
        _CACHE[("plain", B)] = _continue(B, None)
    return _CACHE[("plain", B)]


def _same_states(got, B):
    for name, a, b in zip(("h_all", "cells", "activations"), got, _plain(B)):
        assert torch.equal(a, b), name
    assert float(got[0][TL].abs().max()) > 0     # (the continuation ran)


@pytest.mark.parametrize("B", [127, 16])
@pytest.mark.parametrize("k", [1, 3, 20])
def test_select_glue_segment_is_bit_identical(B, k):
    """sgg_lstm_fwd_seg_glue(select) == sgg_lstm_fwd_seg + sgg_l2_select:
    B = 127 is eight LSTM blocks with a partial last one, B = 16 one block;
    k = 1, 3 leave waves of the four-wave host without a sample, k = 20 takes
    two rounds of its sample loop (the stand-alone kernel has eight waves)."""
    from sgan import _native as N
    from sgan import kernels as K
    lib = K._lib()
    gt, mask, so, pred_k, _ = _glue_inputs()
    Bg, S = sum(SIZES), len(SIZES)
    pred = pred_k[:, :k * Bg].contiguous()
    ref = torch.full((S,), -1, dtype=torch.int64, device=DEV)
    N.check(lib.sgg_l2_select(N.ptr(pred), N.ptr(gt), N.ptr(mask), mask.stride(0), N.ptr(so), S, TP, Bg, k,
                              N.ptr(ref), N.stream_ptr()), "sgg_l2_select")
    best = torch.full((S,), -2, dtype=torch.int64, device=DEV)
    gl = N.GlueSeg(N.GLUE_SELECT, N.ptr(pred), 0, N.ptr(gt), N.ptr(mask), mask.stride(0), N.ptr(so), S, TP, Bg, k,
                   N.ptr(best), 0.0, None, None, 0, None)
    _same_states(_continue(B, gl), B)
    assert torch.equal(best, ref), (best.tolist(), ref.tolist())
    assert int(ref.min()) >= 0 and int(ref.max()) < k
    if k == 20:
        assert len(set(ref.tolist())) > 1        # (not a constant answer)


@pytest.mark.parametrize("B", [127, 16])
def test_l2_backward_glue_segment_is_bit_identical(B):
    """sgg_lstm_fwd_seg_glue(l2 backward) == sgg_lstm_fwd_seg +
    sgg_l2_loss_bwd_scenes: dpred and the scenes' terms, a strided pred, the
    all-zero-mask scene's 0 gradient and 0 term."""
    from sgan import _native as N
    from sgan import kernels as K
    lib = K._lib()
    gt, mask, so, _, wide = _glue_inputs()
    Bg, S, w = sum(SIZES), len(SIZES), 0.7
    pred = wide[:, :Bg]
    gout = torch.full((), 1.0, device=DEV)
    out = []
    for fill in (float("nan"), 3.0):
        out.append((torch.full((TP, Bg, 2), fill, device=DEV), torch.full((S,), fill, device=DEV)))
    (dref, tref), (dpred, term) = out
    N.check(lib.sgg_l2_loss_bwd_scenes(N.ptr(pred), pred.stride(0), N.ptr(gt), N.ptr(mask), mask.stride(0), N.ptr(so),
                                       S, TP, Bg, w, N.ptr(gout), N.ptr(dref), 2 * Bg, N.ptr(tref), N.stream_ptr()),
            "sgg_l2_loss_bwd_scenes")
    gl = N.GlueSeg(N.GLUE_L2BWD, N.ptr(pred), pred.stride(0), N.ptr(gt), N.ptr(mask), mask.stride(0), N.ptr(so), S,
                   TP, Bg, 0, None, w, N.ptr(gout), N.ptr(dpred), 2 * Bg, N.ptr(term))
    _same_states(_continue(B, gl), B)
    assert torch.equal(dpred, dref) and torch.equal(term, tref)
    assert torch.isfinite(dref).all() and torch.isfinite(tref).all()
    o = so.tolist()
    assert float(tref[2]) == 0.0 and float(dref[:, o[2]:o[3]].abs().max()) == 0.0   # the all-zero-mask scene
    assert float(tref[5]) != 0.0 or float(mask[o[5]].sum()) == 0.0                  # the 1-ped scene


def test_glue_segment_without_scenes_is_a_plain_launch():
    """S = 0 and kind none: no glue workgroups, the LSTM segment as ever; bad
    glue arguments are refused before the launch."""
    from sgan import _native as N
    from sgan import kernels as K
    gt, mask, so, pred_k, _ = _glue_inputs()
    Bg = sum(SIZES)
    best = torch.full((len(SIZES),), -2, dtype=torch.int64, device=DEV)
    for kind, S in ((N.GLUE_SELECT, 0), (N.GLUE_NONE, len(SIZES))):
        gl = N.GlueSeg(kind, N.ptr(pred_k), 0, N.ptr(gt), N.ptr(mask), mask.stride(0), N.ptr(so), S, TP, Bg, 3,
                       N.ptr(best), 0.0, None, None, 0, None)
        _same_states(_continue(127, gl), 127)
        assert int(best.max()) == -2
    for bad in (dict(k=257), dict(ldm=TP - 1), dict(best=None)):
        f = dict(kind=N.GLUE_SELECT, pred=N.ptr(pred_k), ldp=0, gt=N.ptr(gt), mask=N.ptr(mask), ldm=mask.stride(0),
                 scene_off=N.ptr(so), S=len(SIZES), T=TP, B=Bg, k=3, best=N.ptr(best), w=0.0, gout=None, dpred=None,
                 ldd=0, term=None)
        f.update(bad)
        with pytest.raises(N.NativeError):
            _continue(127, N.GlueSeg(**f))
    gout = torch.full((), 1.0, device=DEV)
    dpred = torch.empty(TP, Bg, 2, device=DEV)
    for bad in (dict(ldp=2 * Bg - 1), dict(ldd=2 * Bg - 1), dict(gout=None)):
        f = dict(kind=N.GLUE_L2BWD, pred=N.ptr(pred_k), ldp=2 * Bg, gt=N.ptr(gt), mask=N.ptr(mask),
                 ldm=mask.stride(0), scene_off=N.ptr(so), S=len(SIZES), T=TP, B=Bg, k=0, best=None, w=1.0,
                 gout=N.ptr(gout), dpred=N.ptr(dpred), ldd=2 * Bg, term=None)
        f.update(bad)
        with pytest.raises(N.NativeError):
            _continue(127, N.GlueSeg(**f))
    assert int(best.max()) == -2


def _count_alone(monkeypatch):
    """Count the stand-alone launches of the two glue wrappers."""
    from sgan import kernels as K
    calls = {"select": 0, "l2bwd": 0}
    sel, bwd = K._l2_select_alone, K._l2_bwd_scenes_alone

    def c_sel(*a):
        calls["select"] += 1
        return sel(*a)

    def c_bwd(*a):
        calls["l2bwd"] += 1
        return bwd(*a)
    monkeypatch.setattr(K, "_l2_select_alone", c_sel)
    monkeypatch.setattr(K, "_l2_bwd_scenes_alone", c_bwd)
    return calls


def _run_steps(monkeypatch, ride, graphed, iters, paired=True, **trainer_kw):
    from sgan import kernels as K
    from sgan import train_step as TS
    from sgan.data.synthetic import synthetic_batch
    from sgan.scene import SceneIndex
    monkeypatch.setattr(K, "GLUE_RIDE", ride)
    batch = synthetic_batch([20, 7, 13, 20, 2], seed=3, device=DEV)
    batch_g = synthetic_batch([20, 7, 13, 20, 2], seed=4, device=DEV)
    torch.manual_seed(0)
    g, d = build_models()
    tr = TS.GanTrainer(g, d, capturable=True, **trainer_kw)
    sc = SceneIndex.from_seq_start_end(batch[-1], DEV)
    scg = SceneIndex.from_seq_start_end(batch_g[-1], DEV)
    torch.manual_seed(5)
    random.seed(5)
    if graphed:
        gt = TS.GraphedTrainer(tr, batch, sc, warmup=1, batch_g=batch_g, sc_g=scg)
        for _ in range(iters):
            ld, lg = gt.step()
    else:
        for _ in range(iters):
            if paired:
                ld, lg = tr.step(batch, sc, batch_g, scg)
            else:                                   # the sequential steps (no launch shared between them)
                ld, lg = tr.d_step(batch, sc), tr.g_step(batch_g, scg)
    torch.cuda.synchronize()
    assert K._GRIDE[0] is None                      # (no scope left open, nothing held)
    ws = {"g." + k: v.detach().cpu().clone() for k, v in g.state_dict().items()}
    ws.update({"d." + k: v.detach().cpu().clone() for k, v in d.state_dict().items()})
    return {k: float(v) for k, v in list(ld.items()) + list(lg.items())}, ws


def _same_run(a, b):
    (la, wa), (lb, wb) = a, b
    assert la == lb, (la, lb)
    assert sorted(wa) == sorted(wb)
    for k in wa:
        assert torch.equal(wa[k], wb[k]), k


@pytest.mark.parametrize("graphed", [False, True])
def test_glue_ride_step_is_bit_identical(graphed, monkeypatch):
    """GanTrainer.step with the glue launches riding (SGG_GLUE_RIDE, the
    default) == on their own: losses and every state_dict entry, over three
    eager iterations and two replays of a GraphedTrainer.  Eager: riding issues
    no stand-alone glue launch at all, the switch off one of each per
    iteration."""
    calls = _count_alone(monkeypatch)
    res = []
    for ride in (True, False):
        calls.update(select=0, l2bwd=0)
        res.append(_run_steps(monkeypatch, ride, graphed, 2 if graphed else 3))
        if not graphed:
            assert calls == ({"select": 0, "l2bwd": 0} if ride else {"select": 3, "l2bwd": 3}), (ride, calls)
    _same_run(*res)


def test_glue_is_flushed_without_a_carrier(monkeypatch):
    """K.lstm_u_ok answering no (the one predicate for "this encoder launch can
    carry"): the encoders return no fused projection, the shared prefix is
    off and the D-encoder launch is no carrier, so nothing can carry; every
    held glue launch is issued on its own and the steps equal the switch-off
    run bitwise.  (The sequential d_step / g_step: step()'s paired plan shares
    encoder launches between the steps and does not run without carriers.)"""
    from sgan import kernels as K
    monkeypatch.setattr(K, "lstm_u_ok", lambda *a: False)
    calls = _count_alone(monkeypatch)
    res = []
    for ride in (True, False):
        calls.update(select=0, l2bwd=0)
        res.append(_run_steps(monkeypatch, ride, False, 2, paired=False))
        assert calls == {"select": 2, "l2bwd": 2}, (ride, calls)
    _same_run(*res)


def test_eager_losses_path_never_holds(monkeypatch):
    """GanTrainer(bce_pair=K.bce_pair) reads the loss values before the
    backward (eager_losses): its L2 loss is never queued, so its backward is
    never pre-formed -- the same steps with the switch on and off, and the L2
    backward keeps its own kernel (no sgg_l2_loss_bwd_scenes either way)."""
    from sgan import kernels as K
    calls = _count_alone(monkeypatch)
    res = []
    for ride in (True, False):
        calls.update(select=0, l2bwd=0)
        res.append(_run_steps(monkeypatch, ride, False, 2, bce_pair=K.bce_pair))
        assert calls == {"select": 0 if ride else 2, "l2bwd": 0}, (ride, calls)
    _same_run(*res)


def test_l2_loss_with_another_backward_seed(monkeypatch):
    """K.l2_loss inside a trainer scope pre-forms its backward for the seed
    1.0; a total back-propagated with another seed ((2 loss).backward()) must
    not take it: the held launch is flushed, the backward re-issues with the
    seed it received (the torch expression, at the tolerance of
    test_step_glue_kernels_match_torch), bitwise equal to the switch-off run."""
    from sgan import kernels as K
    from sgan.scene import SceneIndex
    sizes = [20, 1, 7, 13, 20, 2]
    B, S, T = sum(sizes), len(sizes), 12
    sc = SceneIndex(np.concatenate([[0], np.cumsum(sizes)]), DEV)
    seg = sc.ped_scene_long()
    torch.manual_seed(11)
    gt = torch.randn(T, B, 2, device=DEV)
    mask = (torch.rand(B, 8 + T, device=DEV) > 0.2).float()[:, 8:]
    p = torch.randn(T, 2 * B, 2, device=DEV)
    pv = p[:, :B].clone().requires_grad_(True)
    num = torch.zeros(S, device=DEV).index_add_(0, seg, (mask.t().unsqueeze(2) * (gt - pv) ** 2).sum((0, 2)))
    den = torch.zeros(S, device=DEV).index_add_(0, seg, mask.sum(1))
    (2 * (num / den).sum()).backward()
    calls = _count_alone(monkeypatch)
    grads = []
    for ride in (True, False):
        monkeypatch.setattr(K, "GLUE_RIDE", ride)
        calls.update(select=0, l2bwd=0)
        pk = p[:, :B].clone().requires_grad_(True)
        with K.defer_grad_finish(), K.glue_ride() as rider:
            loss = K.l2_loss(pk, gt, mask, sc, 1.0)
            assert (rider.held is not None) == ride
            (2 * loss).backward()
            assert rider.held is None
        # riding: the flushed pre-formed launch, then the re-issue with the real seed
        assert calls == {"select": 0, "l2bwd": 2 if ride else 1}, (ride, calls)
        close(pk.grad, pv.grad.cpu().numpy(), rtol=1e-5, what="l2 loss grad, seed 2")
        close(loss, ((num / den).sum()).detach().cpu().numpy(), rtol=1e-5, what="l2 loss (queued value)")
        grads.append(pk.grad.clone())
    assert torch.equal(grads[0], grads[1])
    # the seed 1.0 itself: the pre-formed gradient is taken, nothing re-issued
    monkeypatch.setattr(K, "GLUE_RIDE", True)
    calls.update(select=0, l2bwd=0)
    pk = p[:, :B].clone().requires_grad_(True)
    with K.defer_grad_finish(), K.glue_ride():
        torch.autograd.backward(K.l2_loss(pk, gt, mask, sc, 1.0), grad_tensors=K.const(1.0, pk.device))
    assert calls == {"select": 0, "l2bwd": 1}, calls       # (the flush: no carrier came)
    close(pk.grad, 0.5 * pv.grad.cpu().numpy(), rtol=1e-5, what="l2 loss grad, seed 1")


def test_plain_sequence_carries_a_held_glue_segment(monkeypatch):
    """A saved-state encoder sequence with no prefix and no projection (the
    trainer steps above reach the carrier through a continuation or a
    projection launch only) carries a held select segment through the segment
    entry == the switch off (sgg_l2_select, then sgg_lstm_fwd): best, h_T and
    every gradient bitwise.  21 peds (a partial tile), 4 + 4 steps, H = 48;
    riding issues no stand-alone select at all."""
    from sgan import kernels as K
    from sgan.scene import SceneIndex
    calls = _count_alone(monkeypatch)
    gt, mask, so, pred_k, _ = _glue_inputs()
    sc = SceneIndex(np.concatenate([[0], np.cumsum(SIZES)]), DEV)
    pred = pred_k[:, :3 * sum(SIZES)].contiguous()
    torch.manual_seed(21)
    emb, lstm = torch.nn.Linear(2, 16).to(DEV), torch.nn.LSTM(16, H).to(DEV)
    params = list(emb.parameters()) + list(lstm.parameters())
    rel, dh = torch.randn(8, 21, 2, device=DEV), torch.randn(21, H, device=DEV)
    res = []
    for ride in (True, False):
        monkeypatch.setattr(K, "GLUE_RIDE", ride)
        calls.update(select=0, l2bwd=0)
        for p in params:
            p.grad = None
        with K.glue_ride() as rider:
            best = K.l2_select(pred, gt, mask, sc, 3)
            assert (rider.held is not None) == ride
            h, _ = K.lstm_sequence(rel, lstm, emb)
            assert rider.held is None
        (h * dh).sum().backward()
        assert calls["select"] == (0 if ride else 1), (ride, calls)
        res.append([best, h.detach()] + [p.grad.clone() for p in params])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    best, h = res[0][:2]
    assert 0 <= int(best.min()) and int(best.max()) < 3 and float(h.abs().max()) > 0
    assert all(float(g.abs().max()) > 0 for g in res[0][2:])


def test_select_outside_a_scope_launches_at_once(monkeypatch):
    """Outside a trainer scope nothing is ever held."""
    from sgan import kernels as K
    from sgan.scene import SceneIndex
    calls = _count_alone(monkeypatch)
    gt, mask, so, pred_k, _ = _glue_inputs()
    sc = SceneIndex(np.concatenate([[0], np.cumsum(SIZES)]), DEV)
    Bg = sum(SIZES)
    pred = pred_k[:, :3 * Bg].contiguous()
    ref = K.l2_select(pred, gt, mask, sc, 3)
    assert calls["select"] == 1 and K._GRIDE[0] is None
    with K.glue_ride() as rider:                            # held, then issued when the scope closes
        best = K.l2_select(pred, gt, mask, sc, 3)
        assert rider.held is not None and calls["select"] == 1
    assert calls["select"] == 2 and torch.equal(best, ref)
