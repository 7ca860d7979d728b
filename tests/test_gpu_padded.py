"""The fixed-capacity (padded) batch contract, kernel by kernel.

Real-data training replays one captured graph per capacity bucket: every
batch is padded to S_cap scenes / B_cap peds (sgan.scene.PaddedScenes) and the
kernels take their true sizes from device memory.  Each padded operator is
held to three rules here, without a dataset and without graph capture:

1. real rows equal the unpadded call on the real batch alone (bitwise where
   the operator works per scene / per row with the same instruction sequence,
   else against an fp64 restatement at the tolerance of the operator's
   existing unpadded test);
2. padding rows: everything written is finite, and every gradient is exactly
   0.0 where the upstream gradient is zero;
3. parameter gradients equal those of the real rows alone.

Two shapes: SMALL = real scenes [20, 1, 7, 13, 2] (43 peds) in 8 scenes / 64
peds (three padding scenes of 7 peds), WIDE = [64, 20, 3] in 5 scenes / 128
peds.  np_cap is the largest real scene on purpose: the one-launch modules
then size their LDS plan alike for the padded and the unpadded launch.
"""
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN, check_step_grads

pytestmark = pytest.mark.gpu

DEV = "cuda"

# (real scene sizes, S_cap, B_cap, np_cap)
SMALL = ([20, 1, 7, 13, 2], 8, 64, 20)
WIDE = ([64, 20, 3], 5, 128, 64)
TINY = [2, 2]


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def make_scenes(shape, reps=(), device=DEV):
    """(PaddedScenes loaded with the shape's real batch, the real batch's own
    SceneIndex, number of real peds)."""
    from sgan.scene import PaddedScenes, SceneIndex
    real, S_cap, B_cap, np_cap = shape
    off = offsets(real)
    ps = PaddedScenes(S_cap, B_cap, device, np_cap, reps=reps)
    ps.load(off, np.arange(off[-1], dtype=np.int32))
    assert ps.host_off[-1] == B_cap and len(ps.host_off) == S_cap + 1
    return ps, SceneIndex(off, device), int(off[-1])


def pad(t, n, dim=0):
    """t with zero rows appended along dim up to n."""
    shp = list(t.shape)
    shp[dim] = n - t.shape[dim]
    return torch.cat([t, t.new_zeros(shp)], dim)


def close(a, b, rtol, floor=1e-30, what=""):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, np.float64)
    scale = max(np.abs(b).max(), floor)
    err = np.abs(a - b).max() / scale
    print("%s: max rel err %.3e (scale %.3e, bound %.1e)" % (what, err, scale, rtol))
    assert err <= rtol, "%s max rel err %.3e (scale %.3e)" % (what, err, scale)


def i32(v):
    return torch.tensor([int(v)], dtype=torch.int32, device=DEV)


def all_zero(t):
    return bool((t == 0).all())


# ---------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------
def _bce_ref(x, split, nv, ya, yb, w, g):
    """losses.bce_loss in float64 on the first nv scores of each range ->
    (loss, d loss * g / d x with zeros on the scores that are not live)."""
    from sgan.losses import bce_loss
    xr = x.detach().double().clone().requires_grad_(True)
    n = xr.shape[0]
    nv = n if nv is None else nv
    parts = [bce_loss(t, torch.ones_like(t) * y) for t, y in ((xr[:split][:nv], ya), (xr[split:][:nv], yb))
             if t.numel()]
    ref = w * sum(parts)
    (ref * g).backward()
    live = torch.zeros(n, dtype=torch.bool)
    live[:min(split, nv)] = True
    live[split:split + min(n - split, nv)] = True
    return ref.detach(), xr.grad, live


@pytest.mark.parametrize("n,split,nvalid", [(128, 64, 43), (64, 64, 43), (128, 64, 64), (128, 64, 1),
                                            (4200, 2100, 1500), (4200, 2100, None), (9000, 4500, 3000)])
def test_bce_nvalid_matches_reference(n, split, nvalid):
    """sgg_bce_fwd / sgg_bce_bwd with the device count `nvalid` (the
    bce_live(i, split, nv) comparison of both score ranges; n = 4200 gives a
    thread several scores, n = 9000 is past the 8,192 scores the value's
    workgroup loads ahead: its loop form; (64, 64) is the G-step's one-range
    form), K.bce_pair_total, and the same value formed by the loss
    workgroup of sgg_grad_finish_losses (SggBceJob, the value path of the
    training step): against sgan.losses.bce_loss in float64 on the first
    nvalid scores of each range, loss and gradient within 2e-6 (the bound of
    test_bce_pair_matches_reference_formula); dx of a score that is not live
    is exactly 0; the SggBceJob value is bit-identical to the stand-alone
    forward's, as include/sgg.h states."""
    from sgan import kernels as K
    torch.manual_seed(2)
    x = torch.randn(n, 1, device=DEV) * 3
    x[::3] = 0.0                      # the scores D's trailing ReLU pins at exactly 0
    ya, yb = 0.0, 0.93
    nv = None if nvalid is None else i32(nvalid)
    for w in (1.0, 0.25):
        ref, gref, live = _bce_ref(x, split, nvalid, ya, yb, w, 1.7)
        xa = x.clone().requires_grad_(True)
        loss = K.bce_pair(xa, split, ya, torch.tensor(yb, device=DEV), w, nvalid=nv)
        loss.backward(torch.tensor(1.7, device=DEV))
        close(loss, ref, rtol=2e-6, what="bce loss %s" % ((n, split, nvalid, w),))
        close(xa.grad, gref, rtol=2e-6, what="bce grad %s" % ((n, split, nvalid, w),))
        assert all_zero(xa.grad.view(-1)[~live.to(DEV)]), "dx of a score that is not live"
        assert bool(torch.isfinite(xa.grad).all())
        # (bce, bce + addend) from one launch
        xb = x.clone().requires_grad_(True)
        l2 = torch.tensor(0.37, device=DEV, requires_grad=True)
        adv, tot = K.bce_pair_total(xb, split, ya, torch.tensor(yb, device=DEV), w, l2 * 1.0, nvalid=nv)
        tot.backward(torch.tensor(1.7, device=DEV))
        assert torch.equal(adv, loss.detach()), "bce_pair_total loss"
        close(tot, float(ref) + 0.37, rtol=2e-6, what="bce total")
        assert torch.equal(xb.grad, xa.grad), "bce_pair_total grad"
        # the value path of the training step: queued, formed by sgg_grad_finish_losses
        with K.defer_grad_finish():
            queued = K._loss_deferrable("bce")
            lq = K.bce_pair(x.clone(), split, ya, torch.tensor(yb, device=DEV), w, nvalid=nv)
            assert K._loss_pending(lq) == queued
            aq, tq = K.bce_pair_total(x.clone(), split, ya, torch.tensor(yb, device=DEV), w, l2.detach() * 1.0,
                                      nvalid=nv)
        assert not K._loss_pending(lq)
        assert torch.equal(lq, loss.detach()), ("SggBceJob value", float(lq), float(loss.detach()))
        assert torch.equal(aq, adv) and torch.equal(tq, tot.detach()), "SggBceJob value + addend"


@pytest.mark.parametrize("M", [128, 130])
def test_head_bce_handoff_nvalid(M, monkeypatch):
    """The discriminator head with the BCE hand-off on a padded batch:
    sgg_head_fwdbwd (K.bce_handoff with the trainer's backward seed),
    sgg_head_bwd with bce_g (the hand-off without the fused forward) and
    sgg_bce_bwd + sgg_head_bwd apart, each with nvalid = 43 of split = M / 2
    rows per range; K = 48, N1 = 64, both ReLUs; M = 130 leaves the last
    64-row block partial.  Reference: float64 autograd of the head followed
    by the BCE over the live rows, at test_fused_head_matches_torch's bounds
    (y 2e-6, dx and weights 2e-5); dx of a row that is not live is exactly 0;
    the three forms are bit-identical."""
    from sgan import kernels as K
    from sgan.losses import bce_loss
    from sgan.models import make_mlp
    torch.manual_seed(M)
    Kd, N1, split, nvalid, w, yb = 48, 64, M // 2, 43, 0.5, 0.93
    seq = make_mlp([Kd, N1, 1], batch_norm=False).to(DEV)
    spec = K.head_ok(seq)
    assert spec is not None and spec[2] == 3
    x0 = torch.randn(M, Kd, device=DEV)
    ya_t, yb_t = torch.tensor(0.0, device=DEV), torch.tensor(yb, device=DEV)
    nv = i32(nvalid)
    calls = []
    real_fwd = K._head_fwd
    monkeypatch.setattr(K, "_head_fwd", lambda *a, **k: (calls.append(1), real_fwd(*a, **k))[1])
    res = {}
    for form, (bce, fuse) in (("fwdbwd", (True, True)), ("bwd_bce_g", (True, False)), ("apart", (False, False))):
        monkeypatch.setattr(K, "HEAD_BCE", bce)
        monkeypatch.setattr(K, "HEAD_FUSE", fuse)
        del calls[:]
        seq.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        with K.bce_handoff():
            scores = K.head(x, spec)
            assert (getattr(scores, "_sgg_bce_link", None) is not None) == bce
            loss = K.bce_pair(scores, split, ya_t, yb_t, w, nvalid=nv)
            loss.backward(K.const(1.0, x.device))  # the trainer's seed: the fused launch's result stands
        assert (len(calls) == 0) == (form == "fwdbwd"), (form, len(calls))   # (no separate forward launch)
        res[form] = [scores.detach().clone(), loss.detach().clone(), x.grad.clone()] + \
                    [p.grad.clone() for p in seq.parameters()]
    for form in ("bwd_bce_g", "apart"):
        for a, b in zip(res["fwdbwd"], res[form]):
            assert torch.equal(a, b), form
    # float64 autograd of head + BCE over the live rows
    ref = make_mlp([Kd, N1, 1], batch_norm=False).double().to(DEV)
    ref.load_state_dict({k: v.double() for k, v in seq.state_dict().items()})
    xd = x0.double().requires_grad_(True)
    yr = ref(xd)
    lr = w * (bce_loss(yr[:split][:nvalid], torch.zeros_like(yr[:split][:nvalid]))
              + bce_loss(yr[split:][:nvalid], torch.ones_like(yr[split:][:nvalid]) * yb))
    lr.backward()
    y, loss, dx = res["fwdbwd"][:3]
    close(y, yr.detach(), rtol=2e-6, what="head y M=%d" % M)
    # (a mean of 1-Lipschitz-in-the-score terms over scores within 2e-6: well inside 2e-5)
    close(loss, lr.detach(), rtol=2e-5, what="head bce loss M=%d" % M)
    close(dx, xd.grad, rtol=2e-5, what="head dx M=%d" % M)
    for (name, _), g, pr in zip(seq.named_parameters(), res["fwdbwd"][3:], ref.parameters()):
        close(g, pr.grad, rtol=2e-5, what="head d%s M=%d" % (name, M))
    live = torch.zeros(M, dtype=torch.bool, device=DEV)
    live[:nvalid] = True
    live[split:split + nvalid] = True
    assert all_zero(dx[~live]), "dx of a row that is not live"
    assert bool(dx[live].abs().sum() > 0)


def _l2_ref(pred, gt, mask, off, w):
    """float64 restatement of train.py:459-464 over the scenes of `off`:
    (per-sample per-scene masked squared errors (k, S), loss of sample 0 and
    its gradient w.r.t. pred[:, 0])."""
    S = len(off) - 1
    seg = torch.from_numpy(np.repeat(np.arange(S), np.diff(off))).to(pred.device)
    p = pred.double().clone().requires_grad_(True)              # (T, k, B, 2)
    se = ((gt.double().unsqueeze(1) - p) ** 2).sum(3) * mask.double().t().unsqueeze(1)   # (T, k, B)
    k = p.shape[1]
    per = torch.zeros(k, S, dtype=torch.float64, device=pred.device).index_add_(1, seg, se.sum(0))
    den = torch.zeros(S, dtype=torch.float64, device=pred.device).index_add_(0, seg, mask.double().sum(1))
    loss = (w * per[0] / den).sum()
    loss.backward()
    return per.detach(), loss.detach(), p.grad[:, 0]


def _l2_checks(pred, gt, mask, scenes, off_real, k, w, B_real, what):
    """l2_select, then l2_loss forward + backward (sgg_l2_loss_fwd / _bwd),
    then the same through sgg_l2_loss_bwd_scenes + SggL2Job, of a batch whose
    first len(off_real) - 1 scenes / B_real peds are real."""
    from sgan import kernels as K
    T, Bc = gt.shape[0], gt.shape[1]
    S = len(off_real) - 1
    per, loss_ref, g_ref = _l2_ref(pred[:, :, :B_real], gt[:, :B_real], mask[:B_real], off_real, w)
    srt = per.sort(0)[0]
    if k > 1:   # the seed leaves no near tie between the two best samples of a scene
        assert float(((srt[1] - srt[0]) / srt[0]).min()) > 1e-4
    best = K.l2_select(pred.view(T, k * Bc, 2), gt, mask, scenes, k)
    assert best.shape == (scenes.S,) and torch.equal(best[:S], per.argmin(0)), what + " l2_select real scenes"
    assert all_zero(best[S:]), what + " l2_select padding scenes"
    got = []
    for path in ("fwd+bwd", "bwd_scenes+job"):
        p = pred[:, 0].clone().requires_grad_(True)
        if path == "fwd+bwd":
            loss = K.l2_loss(p, gt, mask, scenes, w)
            loss.backward(torch.tensor(1.0, device=DEV))
        else:
            with K.defer_grad_finish():
                queued = K._loss_deferrable("l2")
                loss = K.l2_loss(p, gt, mask, scenes, w)
                assert K._loss_pending(loss) == queued
                loss.backward(torch.tensor(1.0, device=DEV))
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(p.grad).all()), what + " NaN " + path
        close(loss, loss_ref, rtol=1e-5, what="%s l2 loss (%s)" % (what, path))
        close(p.grad[:, :B_real], g_ref, rtol=1e-5, what="%s l2 grad (%s)" % (what, path))
        assert all_zero(p.grad[:, B_real:]), what + " l2 gradient on padding rows " + path
        got.append((loss.detach().clone(), p.grad.clone()))
    # the SggL2Job value is sgg_l2_loss_fwd's, and the scenes' backward writes l2_loss_bwd's expression (include/sgg.h)
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), what + " the two L2 paths"


@pytest.mark.parametrize("k", [1, 5])
def test_l2_on_padded_batch(k):
    """sgg_l2_select, sgg_l2_loss_fwd / _bwd and sgg_l2_loss_bwd_scenes +
    SggL2Job on the SMALL padded batch (T = 12, loss mask zero on padding
    rows): the msum == 0 branches.  l2_select returns 0 on padding scenes and
    the float64 argmin on real ones; loss and gradient match the float64
    restatement over the real scenes to 1e-5 (test_step_glue_kernels_match_torch's
    bound); the gradient on padding rows is exactly 0; nothing is NaN."""
    torch.manual_seed(11 + k)
    ps, _, B = make_scenes(SMALL)
    T, Bc = 12, ps.B
    gt = pad(torch.randn(T, B, 2, device=DEV), Bc, 1)
    pred = pad(torch.randn(T, k, B, 2, device=DEV), Bc, 2)
    lm = pad((torch.rand(B, 8 + T, device=DEV) > 0.2).float(), Bc, 0)
    _l2_checks(pred, gt, lm[:, 8:], ps, offsets(SMALL[0]), k, 0.7, B, "padded k=%d" % k)


def test_l2_unstaged_mask_path():
    """l2_body.h with n * T = 64 * 33 = 2112 > kL2MaxElems = 2048: the loss
    mask is read in place (row stride ldm = 40) instead of from LDS.
    l2_select, l2_loss forward and backward (both backward forms) against the
    same float64 expressions as the staged path, 1e-5."""
    from sgan.scene import SceneIndex
    torch.manual_seed(5)
    n, T, k = 64, 33, 5
    sc = SceneIndex(offsets([n]), DEV)
    gt = torch.randn(T, n, 2, device=DEV)
    pred = torch.randn(T, k, n, 2, device=DEV)
    lm = (torch.rand(n, 40, device=DEV) > 0.2).float()
    mask = lm[:, :T]
    assert mask.stride(0) == 40
    _l2_checks(pred, gt, mask, sc, offsets([n]), k, 1.0, n, "unstaged")


# ---------------------------------------------------------------------------
# pooling
# ---------------------------------------------------------------------------
def _pool_net(bn, seed):
    from sgan.models import PoolHiddenNet
    torch.manual_seed(seed)
    return PoolHiddenNet(embedding_dim=16, h_dim=32, mlp_dim=64, bottleneck_dim=bn, batch_norm=False)


def _pool_inputs(sizes, B_cap, seed):
    """(h, pos) of a batch, drawn on the host (the same numbers on every
    device), zero on the padding rows."""
    g = torch.Generator().manual_seed(seed)
    B = int(sum(sizes))
    return pad(torch.randn(B, 32, generator=g), B_cap), pad(torch.rand(B, 2, generator=g) * 15, B_cap)


def _pool_apply(net, h, pos, scenes, U=None):
    """K.social_pool's op with its argmax output -> (out, argmax)."""
    from sgan import kernels as K
    l1, l2, emb = net.mlp_pre_pool[0], net.mlp_pre_pool[2], net.spatial_embedding
    return K._Pool.apply(h, pos, l1.weight, emb.weight, emb.bias, l1.bias, l2.weight, l2.bias, scenes, None, U)


def _pool_ref(U, pos, A, W2, b2, off, bf16=False):
    """float64 pair MLP of test_pool_x3_vs_fp32 (bf16: the rounded operands of
    test_pool_bf16_kernel_matches_rounded_reference) over the scenes of off
    -> (max over j (B, bn), first argmax as a global ped index, per-scene z)."""
    Ud, pd, Ad, bd = (t.detach().cpu().double() for t in (U, pos, A, b2))
    Wd = (W2.detach().to(torch.bfloat16) if bf16 else W2.detach()).cpu().double()
    B, bn = U.shape[0], W2.shape[0]
    ref = torch.empty(B, bn, dtype=torch.float64)
    am = torch.empty(B, bn, dtype=torch.int64)
    zs = []
    for o, e in zip(off[:-1], off[1:]):
        o, e = int(o), int(e)
        r = pd[o:e].unsqueeze(0) - pd[o:e].unsqueeze(1)                 # [i, j] = p_j - p_i
        hid = torch.relu(Ud[o:e].unsqueeze(0) + r @ Ad.t())               # (i, j, 512)
        if bf16:
            hid = hid.float().to(torch.bfloat16).double()
        z = torch.relu(hid @ Wd.t() + bd)                                 # (i, j, bn)
        v, j = z.max(1)
        ref[o:e], am[o:e] = v, j + o
        zs.append(z)
    return ref, am, zs


def _near_ties(zs, scale, n_scenes, eps=1e-5):
    """Entries of the first n_scenes scenes whose two largest fp64 values over
    j are positive and within eps * scale."""
    n = 0
    for z in zs[:n_scenes]:
        if z.shape[1] < 2:
            continue
        top = z.topk(2, dim=1)[0]
        n += int(((top[:, 0] - top[:, 1] <= eps * scale) & (top[:, 0] > 0)).sum())
    return n


def _plan_counts(bn):
    """(grid basis, device chunk count of the tiny batch, of the SMALL batch)
    of a fixed-capacity plan registered with the tiny batch: host data."""
    from sgan.scene import PaddedScenes
    real, S_cap, B_cap, np_cap = SMALL
    ps = PaddedScenes(S_cap, B_cap, "cpu", np_cap, reps=())
    ps.load(offsets(TINY), np.arange(sum(TINY), dtype=np.int32))
    plan = ps.pool_plan(bn)
    n_tiny = int(plan[4])
    ps.load(offsets(real), np.arange(sum(real), dtype=np.int32))
    return plan[1], n_tiny, int(ps.pool_plan(bn)[4])


@pytest.mark.parametrize("bn", [8, 48])
def test_pool_forward_device_chunk_count(bn, monkeypatch):
    """sgg_pool_fwd / sgg_pool_fwd_bf16 walking the DEVICE chunk count
    (nchunks_dev) of a fixed-capacity plan, on both sides of the grid the
    first batch sized: the plan is registered with a tiny batch, then the
    SMALL batch (more chunks than that grid: every workgroup's XCD-aware
    walk takes a second chunk) and the tiny one again.  The fp32 forms
    (SGG_POOL_X3 0 / 1) against the fp64 pair MLP of test_pool_x3_vs_fp32:
    real rows within 1e-5 of the output scale, argmax the fp64 argmax or a
    near tie under that test's rule (the seed leaves no positive near tie on
    real rows); the bf16 form against the rounded-operand reference of
    test_pool_bf16_kernel_matches_rounded_reference (2e-3, argmax equal on
    >= 99 %).  Every row's argmax -- padding rows included: the backward
    scatters through it -- lies inside its own scene, and on padding rows,
    whose pairs all tie, it is the smallest j (include/sgg.h)."""
    from sgan import kernels as K
    real, S_cap, B_cap, np_cap = SMALL
    grid, n_tiny, n_small = _plan_counts(bn)
    assert n_small > grid >= n_tiny, (grid, n_tiny, n_small)    # the test covers both sides of the grid
    ps, _, _ = make_scenes((TINY, S_cap, B_cap, np_cap))
    plan = ps.pool_plan(bn)
    assert plan[1] == grid and int(plan[4]) == n_tiny
    net = _pool_net(bn, 3).to(DEV)
    l1, l2, emb = net.mlp_pre_pool[0], net.mlp_pre_pool[2], net.spatial_embedding
    for step, sizes in enumerate((TINY, real, TINY)):
        off_real = offsets(sizes)
        B = int(off_real[-1])
        ps.load(off_real, np.arange(B, dtype=np.int32))
        torch.cuda.synchronize()
        assert int(ps.pool_plan(bn)[4]) == (n_small if sizes is real else n_tiny) and ps.pool_plan(bn)[1] == grid
        off = ps.host_off
        scene_of = np.repeat(np.arange(S_cap), np.diff(off))
        lo, hi = torch.from_numpy(off[scene_of]).view(-1, 1), torch.from_numpy(off[scene_of + 1]).view(-1, 1)
        h, pos = (t.to(DEV) for t in _pool_inputs(sizes, B_cap, 100 * bn + step))
        with torch.no_grad():
            A, c = K.fold_fwd(l1.weight[:, :16], emb.weight, emb.bias, l1.bias)
            U = K.xw_raw(h, l1.weight[:, 16:], c, trans_w=True)
        ref, ref_am, zs = _pool_ref(U, pos, A, l2.weight, l2.bias, off)
        scale = float(ref[:B].abs().max())
        assert _near_ties(zs, scale, len(sizes)) == 0, "pick another seed: near tie in the fp64 reference"
        for form in ("x3=0", "x3=1", "bf16"):
            monkeypatch.setenv("SGG_POOL_X3", "0" if form == "x3=0" else "1")
            K.set_precision("bf16" if form == "bf16" else "fp32")
            try:
                with torch.no_grad():
                    out, am = _pool_apply(net, h, pos, ps, U)
            finally:
                K.set_precision("fp32")
            out, am = out.cpu().double(), am.cpu().long()
            what = "pool bn=%d %s step %d" % (bn, form, step)
            assert bool(torch.isfinite(out).all()), what
            assert bool(((am >= lo) & (am < hi)).all()), what + ": argmax outside its scene"
            assert bool((am[B:] == lo[B:]).all()), what + ": padding rows tie on every j -> the smallest j"
            if form == "bf16":
                rb, rb_am, _ = _pool_ref(U, pos, A, l2.weight, l2.bias, off, bf16=True)
                close(out[:B], rb[:B], rtol=2e-3, what=what)
                assert float((am[:B] == rb_am[:B]).double().mean()) >= 0.99, what
                continue
            err = float((out[:B] - ref[:B]).abs().max()) / scale
            print("%s: err %.3e of scale" % (what, err))
            assert err <= 1e-5, (what, err)
            for i, col in (am[:B] != ref_am[:B]).nonzero().tolist():
                s = int(scene_of[i])
                z, o = zs[s], int(off[s])
                a, b = int(am[i, col]) - o, int(ref_am[i, col]) - o
                assert abs(float(z[i - o, a, col] - z[i - o, b, col])) <= 1e-5 * scale, (what, i, col)


@pytest.mark.parametrize("bn", [8, 48])
def test_pool_fwd2_padded_and_unpadded(bn):
    """sgg_pool_fwd2 with one padded batch (device chunk count) and one
    unpadded batch (host count) in ONE launch (K.pool_pair): each batch's
    output and argmax are bitwise what its single launch writes."""
    from sgan import kernels as K
    from sgan.scene import SceneIndex
    ps, _, _ = make_scenes(SMALL)
    sc_b = SceneIndex(offsets([20, 20, 1, 9]), DEV)
    net = _pool_net(bn, 4).to(DEV)
    ha, pa = (t.to(DEV) for t in _pool_inputs(SMALL[0], ps.B, 7))
    hb, pb = (t.to(DEV) for t in _pool_inputs([20, 20, 1, 9], 50, 8))
    with torch.no_grad():
        single = [_pool_apply(net, ha, pa, ps), _pool_apply(net, hb, pb, sc_b)]
        for first, second in (((ha, pa, ps), (hb, pb, sc_b)), ((hb, pb, sc_b), (ha, pa, ps))):
            with K.pool_pair() as r:
                one = _pool_apply(net, *first)
                two = _pool_apply(net, *second)
            assert r.carried, "the second forward did not carry the first"
            pair = [one, two] if first[2] is ps else [two, one]
            for (o1, a1), (o2, a2) in zip(single, pair):
                assert torch.equal(o1, o2) and torch.equal(a1, a2)


@pytest.mark.parametrize("bn", [8, 48])
@pytest.mark.parametrize("shape", [SMALL, WIDE], ids=["small", "wide"])
def test_pool_backward_on_padded_batch(shape, bn):
    """sgg_pool_bwd (+ the dh / weight-gradient launches) on a padded batch
    with dout zero on padding rows: dU (and dh) on padding rows is exactly 0;
    out and dh on real rows and every parameter gradient match the unpadded
    launch within test_pool_vs_reference_fixture's bounds (out 1e-5, dh 1e-4,
    weights 1e-4 with the 1 % floor)."""
    from sgan import _native as N
    ps, sc, B = make_scenes(shape)
    net = _pool_net(bn, 5).to(DEV)
    h0, pos = (t.to(DEV) for t in _pool_inputs(shape[0], ps.B, 9 + bn))
    dout = pad(torch.randn(B, bn, device=DEV), ps.B)
    res = []
    for scenes, rows in ((ps, ps.B), (sc, B)):
        net.zero_grad(set_to_none=True)
        h = h0[:rows].clone().requires_grad_(True)
        out, am = _pool_apply(net, h, pos[:rows].contiguous(), scenes)
        (out * dout[:rows]).sum().backward()
        res.append((out.detach(), am, h.grad, {k: p.grad.clone() for k, p in net.named_parameters()}))
    (out_p, am_p, dh_p, g_p), (out_r, _, dh_r, g_r) = res
    close(out_p[:B], out_r, rtol=1e-5, what="pool out real rows")
    close(dh_p[:B], dh_r, rtol=1e-4, what="pool dh real rows")
    assert bool(torch.isfinite(out_p).all()) and all_zero(dh_p[B:]), "dh on padding rows"
    fl = 1e-2 * max(float(g.abs().max()) for g in g_r.values())
    for k in g_r:
        close(g_p[k], g_r[k], rtol=1e-4, floor=fl, what="pool d" + k)
    # dU itself: the backward kernel on the padded forward's state
    from sgan import kernels as K
    lib = N.load()
    l1, l2, emb = net.mlp_pre_pool[0], net.mlp_pre_pool[2], net.spatial_embedding
    with torch.no_grad():
        A, c = K.fold_fwd(l1.weight[:, :16], emb.weight, emb.bias, l1.bias)
        U = K.xw_raw(h0, l1.weight[:, 16:], c, trans_w=True)
    dU = torch.full((ps.B, 512), float("nan"), device=DEV)
    N.check(lib.sgg_pool_bwd(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(l2.weight), N.ptr(out_p), N.ptr(am_p),
                             N.ptr(dout), N.ptr(ps.scene_off), ps.S, ps.B, bn, ps.max_n, N.ptr(dU), None,
                             N.stream_ptr()), "sgg_pool_bwd")
    assert bool(torch.isfinite(dU).all()) and all_zero(dU[B:]), "dU on padding rows"
    assert bool(dU[:B].abs().sum() > 0)


# ---------------------------------------------------------------------------
# segment ops, group index, batch gather
# ---------------------------------------------------------------------------
def _segments():
    """The SMALL padded batch's scenes with random groups inside each scene:
    (scene_off (S + 1), ped -> scene, ped -> global group id, group -> scene
    padded to n rows, number of groups), int32 numpy."""
    rng = np.random.default_rng(0)
    sizes = list(SMALL[0]) + [7, 7, 7]
    off = offsets(sizes)
    ped_scene = np.repeat(np.arange(len(sizes)), sizes)
    gid, gscene, G = np.zeros(off[-1], np.int64), [], 0
    for s, n in enumerate(sizes):
        local = rng.integers(0, max(1, (n + 2) // 3), size=n)
        _, local = np.unique(local, return_inverse=True)
        gid[off[s]:off[s + 1]] = G + local
        gscene += [s] * (local.max() + 1)
        G += local.max() + 1
    gs = np.zeros(off[-1], np.int64)
    gs[:G] = gscene
    return off, ped_scene, gid, gs, G


def test_seg_reduce_and_gather_device_counts():
    """sgg_seg_reduce (the `k < *nseg_dev` branch, seg_range absent / present,
    row_scale, mean, row strides ldx / ldo > F, F in {1, 16, 72}) against a
    float64 index_add_: the kernel is a serial fp32 sum of cnt <= 64 terms,
    so |out - ref| <= (cnt + 2) 2^-24 sum |scale x| (over cnt for the mean);
    rows >= *nseg_dev are exactly 0 and the columns of `out` past F stay
    untouched.  sgg_seg_gather (`i < *nrow_dev`) does one multiply per
    element: bitwise the fp32 torch expression, rows >= *nrow_dev exactly 0."""
    from sgan import _native as N
    lib = N.load()
    off, ped_scene, gid, gscene, G = _segments()
    n = int(off[-1])
    S = len(off) - 1
    to_dev = lambda a: torch.from_numpy(np.asarray(a).astype(np.int32)).to(DEV)
    torch.manual_seed(1)
    for F in (1, 16, 72):
        xb = torch.randn(n, F + 3, device=DEV)
        x = xb[:, :F]
        scale = torch.rand(n, device=DEV) + 0.5
        for ranged in (False, True):
            # absent: segment k is range k (the scenes); present: the groups, each inside its scene's rows
            seg, cap, nreal = (gid, n, G) if ranged else (ped_scene, S, S)
            seg_d, range_off, seg_range = to_dev(seg), to_dev(off), (to_dev(gscene) if ranged else None)
            for mean in (0, 1):
                for rs in (None, scale):
                    for nseg in (None, cap, nreal, nreal - 2):
                        nd = i32(nseg) if nseg is not None else None
                        out = torch.full((cap, F + 2), 123.0, device=DEV)
                        N.check(lib.sgg_seg_reduce(N.ptr(x), xb.stride(0), F, N.ptr(seg_d), N.ptr(rs),
                                                   N.ptr(range_off), N.ptr(seg_range),
                                                   N.ptr(nd), cap, mean,
                                                   N.ptr(out), out.stride(0), N.stream_ptr()), "sgg_seg_reduce")
                        live = cap if nseg is None else nseg
                        v = (x.double() * (rs.double().unsqueeze(1) if rs is not None else 1.0)).cpu()
                        idx = torch.from_numpy(np.asarray(seg))
                        ref = torch.zeros(cap, F, dtype=torch.float64).index_add_(0, idx, v)
                        mag = torch.zeros(cap, F, dtype=torch.float64).index_add_(0, idx, v.abs())
                        cnt = torch.bincount(idx, minlength=cap).double().unsqueeze(1)
                        assert cnt.max() <= 64
                        if mean:
                            ref, mag = ref / cnt.clamp(min=1), mag / cnt.clamp(min=1)
                        got = out.cpu().double()
                        what = (F, ranged, mean, rs is not None, nseg)
                        assert bool((got[:, F:] == 123.0).all()), ("columns past F written", what)
                        assert all_zero(got[live:, :F]), ("rows past *nseg_dev", what)
                        bound = (cnt + 2) * 2.0 ** -24 * mag
                        assert bool(((got[:live, :F] - ref[:live]).abs() <= bound[:live]).all()), what
                        if live:
                            assert float(got[:live, :F].abs().sum()) > 0
        # gather: out[i] = scale_i * src[seg(i)]
        srcb = torch.randn(n, F + 5, device=DEV)
        src = srcb[:, :F]
        seg_d = to_dev(gid)
        for rs in (None, scale):
            for nrow in (None, n, 43, 1):
                nd = i32(nrow) if nrow is not None else None
                out = torch.full((n, F + 2), 123.0, device=DEV)
                N.check(lib.sgg_seg_gather(N.ptr(src), srcb.stride(0), F, N.ptr(seg_d), N.ptr(rs),
                                           N.ptr(nd), n, N.ptr(out),
                                           out.stride(0), N.stream_ptr()), "sgg_seg_gather")
                live = n if nrow is None else nrow
                ref = src.index_select(0, seg_d.long())
                if rs is not None:
                    ref = ref * rs.unsqueeze(1)
                assert torch.equal(out[:live, :F], ref[:live]), (F, rs is not None, nrow)
                assert all_zero(out[live:, :F]) and bool((out[:, F:] == 123.0).all()), (F, rs is not None, nrow)


@pytest.mark.parametrize("scale", [True, False])
def test_group_mean_unpool_on_padded_scenes(scale):
    """K.group_mean / K.group_unpool (sgg_seg_reduce with *nseg_dev = the
    device group count, sgg_seg_gather) under autograd on
    PaddedScenes.groups(labels), labels and inputs zero on padding rows (every
    padding ped a singleton group): the group rows of the real scenes, the
    real rows of the un-pooled output and of dx equal, bitwise, those on the
    real batch's own SceneIndex (the same serial per-group sums); dx on
    padding rows is exactly 0."""
    from sgan import kernels as K
    ps, sc, B = make_scenes(SMALL)
    rng = np.random.default_rng(4)
    lab_r = torch.from_numpy(rng.integers(0, 4, size=B).astype(np.float32)).to(DEV)
    torch.manual_seed(6)
    x0 = pad(torch.randn(B, 16, device=DEV), ps.B)
    dy = pad(torch.randn(B, 16, device=DEV), ps.B)
    res = []
    for scenes, lab, rows in ((ps, pad(lab_r, ps.B), ps.B), (sc, lab_r, B)):
        g = scenes.groups(lab)
        x = x0[:rows].clone().requires_grad_(True)
        gm = K.group_mean(x, g)
        y = K.group_unpool(gm, g, scale=scale)
        (y * dy[:rows]).sum().backward()
        res.append((gm.detach(), y.detach(), x.grad, int(g.n_groups_dev)))
    (gm_p, y_p, dx_p, G_p), (gm_r, y_r, dx_r, G_r) = res
    assert G_p == G_r + (ps.B - B)                      # one singleton group per padding ped
    assert torch.equal(gm_p[:G_r], gm_r[:G_r]) and all_zero(gm_r[G_r:]) and all_zero(gm_p[G_p:])
    assert torch.equal(y_p[:B], y_r) and torch.equal(dx_p[:B], dx_r)
    assert bool(torch.isfinite(y_p).all()) and all_zero(dx_p[B:])
    assert float(dx_r.abs().sum()) > 0


def test_group_index_more_scenes_than_scan_threads():
    """sgg_group_index with S = 1030 scenes of 1 to 3 peds: group_scan_kernel
    then gives two scenes to a thread (S > 1024).  The partition assertions
    of test_group_index_matches_oracle_partition (two peds share a group iff
    they share a scene and a non-zero label; groups per scene; each group's
    scene and member count), in vectorised numpy."""
    from sgan.scene import SceneIndex
    rng = np.random.default_rng(8)
    S = 1030
    sizes = rng.integers(1, 4, size=S)
    off = offsets(sizes)
    B = int(off[-1])
    lab = rng.integers(0, 3, size=B)
    scene = np.repeat(np.arange(S), sizes)
    g = SceneIndex(off, DEV).groups(torch.from_numpy(lab.astype(np.float32)).to(DEV))
    gid, goff = g.ped_gid.cpu().numpy().astype(np.int64), g.group_off.cpu().numpy().astype(np.int64)
    cnt, gs = g.group_count.cpu().numpy(), g.group_scene.cpu().numpy()

    def canon(key):   # classes numbered by first member
        _, first, inv = np.unique(key, return_index=True, return_inverse=True)
        rank = np.empty(len(first), np.int64)
        rank[np.argsort(first)] = np.arange(len(first))
        return rank[inv.reshape(-1)]
    # the distinct rows of M_intra: (scene, label) for a non-zero label, a singleton per label-0 ped
    want = canon(np.where(lab != 0, scene * 4 + lab, -(np.arange(B) + 1)))
    assert np.array_equal(canon(gid), want), "partition"
    G = int(want.max()) + 1
    assert goff[0] == 0 and goff[S] == G and int(g.n_groups_dev) == G
    first_of = np.zeros(G, np.int64)
    first_of[want[::-1]] = np.arange(B)[::-1]                      # first member of each class
    assert np.array_equal(np.diff(goff), np.bincount(scene[first_of], minlength=S)), "groups per scene"
    assert bool(((gid >= goff[scene]) & (gid < goff[scene + 1])).all()), "a ped's group lies in its scene's range"
    assert np.array_equal(gs[gid], scene), "group_scene"
    assert np.array_equal(cnt[:G], np.bincount(gid, minlength=G)), "group_count"


def test_gather_batch_padding_rows():
    """sgg_gather_batch with negative rows (`rows[b] < 0`: padding peds): on a
    synthetic table of 50 random records the real columns of all ten outputs
    are bitwise the numpy slicing of the table, the padding columns all zero,
    the loss mask included."""
    from sgan import _native as N
    from sgan.data.device import DeviceTrajectoryDataset
    lib = N.load()
    To, Tp = 8, 12
    T = To + Tp
    rec = 6 * T + 1
    rng = np.random.default_rng(2)
    table = rng.standard_normal((50, rec)).astype(np.float32)
    rows = np.array([3, 49, -1, 0, -1, 7, 7, -1, 21, -1, -1, 48, 1, -1, -1, -1, 30], dtype=np.int32)
    B = len(rows)
    dd = object.__new__(DeviceTrajectoryDataset)
    dd.table, dd.rec, dd.obs_len, dd.pred_len = torch.from_numpy(table).to(DEV), rec, To, Tp
    out = torch.full((int(lib.sgg_gather_batch_floats(B, To, Tp)),), float("nan"), device=DEV)
    dd.gather_into(torch.from_numpy(rows).to(DEV), B, out)
    got = [t.cpu().numpy() for t in dd.views(out, B, np.arange(B + 1))[:10]]
    r = table[np.maximum(rows, 0)] * (rows >= 0)[:, None].astype(np.float32)
    absx, rel = r[:, :2 * T].reshape(B, T, 2), r[:, 2 * T:4 * T].reshape(B, T, 2)
    grp, lm, nl = r[:, 4 * T:5 * T], r[:, 5 * T:6 * T], r[:, 6 * T]
    tm = lambda a: np.ascontiguousarray(np.swapaxes(a, 0, 1))       # time-major
    vel = rel * np.float32(2.5)
    want = [tm(absx)[:To], tm(absx)[To:], tm(rel)[:To], tm(rel)[To:], tm(vel)[:To], tm(vel)[To:],
            tm(grp)[:To, :, None], tm(grp)[To:, :, None], nl, lm]
    real = rows >= 0
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, (k, a.shape, b.shape)
        bdim = 0 if k >= 8 else 1
        ar, br = np.compress(real, a, bdim), np.compress(real, b, bdim)
        assert ar.tobytes() == br.tobytes(), ("real columns of output", k)
        assert not np.compress(~real, a, bdim).any(), ("padding columns of output", k)
        assert np.isfinite(a).all()


# ---------------------------------------------------------------------------
# one-launch graph modules
# ---------------------------------------------------------------------------
def _labels(sizes):
    """The label patterns of test_gat_encoder_fused_equals_per_layer: all
    singletons (0), one big group, mixed groups, scene by scene."""
    labs = []
    for k, n in enumerate(sizes):
        pat = k % 3
        labs.append(np.zeros(n) if pat == 0 else np.full(n, 3.0) if pat == 1
                    else np.random.RandomState(k).randint(0, 4, n))
    return torch.from_numpy(np.concatenate(labs).astype(np.float32)).to(DEV)


def _module_runs(mod, call, shape, fout):
    """The module on the padded batch (inputs, labels, dy zero on padding rows)
    and on the real batch alone -> [(y, dx, parameter gradients)] x 2, B."""
    ps, sc, B = make_scenes(shape)
    torch.manual_seed(len(shape[0]))
    x0 = pad(torch.randn(B, 40, device=DEV), ps.B)
    dy = pad(torch.randn(B, fout, device=DEV), ps.B)
    lab = pad(_labels(shape[0]), ps.B)
    res = []
    for scenes, rows in ((ps, ps.B), (sc, B)):
        mod.zero_grad(set_to_none=True)
        x = x0[:rows].clone().requires_grad_(True)
        y = call(x, lab[:rows].view(-1, 1), scenes)
        (y * dy[:rows]).sum().backward()
        res.append((y.detach(), x.grad, {k: p.grad.clone() for k, p in mod.named_parameters()}))
    (y_p, dx_p, _), (y_r, dx_r, _) = res
    assert torch.equal(y_p[:B], y_r), "y on real rows"
    assert torch.equal(dx_p[:B], dx_r), "dX on real rows"
    assert bool(torch.isfinite(y_p).all()), "y on padding rows"
    assert all_zero(dx_p[B:]), "dX on padding rows"
    assert float(dx_r.abs().sum()) > 0
    return res, (x0, dy, sc, B)


@pytest.mark.parametrize("nh,shape", [(1, SMALL), (1, WIDE), (2, SMALL)], ids=["nh1-small", "nh1-wide", "nh2-small"])
def test_gat_encoder_on_padded_batch(nh, shape):
    """sgg_gatenc_fwd / _bwd on a padded batch (padding scenes are whole
    scenes of zero rows with label 0; WIDE takes the compact 64-ped backward
    plan; two heads have no plan at 49 peds or more): y and dX on real rows
    bitwise the unpadded launch (one workgroup per scene, the same LDS plan
    as np_cap is the largest real scene), y finite and dX exactly 0 on
    padding rows, and every parameter gradient BITWISE the unpadded one: the
    kernel writes one slab row per scene, the padding scenes' rows are exact
    zeros and sgg_slab_reduce appends them at the end of each phase's sum."""
    from sgan.models import GATEncoder
    torch.manual_seed(nh)
    mod = GATEncoder([40, 16, 40], nh, 0.0, 0.2).to(DEV)
    ps, sc, _ = make_scenes(shape)
    assert mod.fused_ok(ps, True) and mod.fused_ok(sc, True)
    res, _ = _module_runs(mod, lambda x, lab, s: mod(x, None, None, lab, scenes=s), shape, 24)
    for k in res[1][2]:
        assert torch.equal(res[0][2][k], res[1][2][k]), "d" + k
    assert all(float(v.abs().sum()) > 0 for v in res[1][2].values())


@pytest.mark.parametrize("shape", [SMALL, WIDE], ids=["small", "wide"])
def test_gcn_module_on_padded_batch(shape):
    """sgg_gcnmod_fwd / _bwd on a padded batch: y and dX on real rows bitwise
    the unpadded launch, y finite and dX exactly 0 on padding rows, parameter
    gradients within test_gcn_module_fused_equals_per_op's fp32 bound (2e-4 of
    the tensor max, floor 1 % of the largest gradient): a backward workgroup
    accumulates several scenes, so the slab's summation order may move."""
    from sgan.models import GCNModule
    torch.manual_seed(3)
    mod = GCNModule(40, 72, 16, 2, 24).to(DEV)
    with torch.no_grad():   # (the reference's unscaled randn init makes ReLU-dead columns the rule: as that test)
        for p in mod.parameters():
            if p.dim() == 2 and p.shape[1] in (72, 16):
                p.mul_(0.2)
    ps, sc, _ = make_scenes(shape)
    assert mod.fused_ok(ps, 40) and mod.fused_ok(sc, 40)
    res, _ = _module_runs(mod, lambda x, lab, s: mod(x, None, None, lab, scenes=s), shape, 24)
    g_p, g_r = res[0][2], res[1][2]
    fl = 1e-2 * max(float(g.abs().max()) for g in g_r.values())
    for k in g_r:
        close(g_p[k], g_r[k], rtol=2e-4, floor=fl, what="gcn module d" + k)


@pytest.mark.parametrize("shape", [SMALL, WIDE], ids=["small", "wide"])
def test_batch_gat_on_padded_batch(shape):
    """The sgangat layers (BatchGATEncoder: sgg_gat_layer_fwd per layer, the
    instance norm of an all-zero padding scene is 0 / sqrt(eps)) on a padded
    batch: y and dX on real rows bitwise the unpadded launch, y finite and dX
    exactly 0 on padding rows.  Parameter gradients by the rule of
    test_gat_layer_fused_equals_per_op: against the fp64 restatement on the
    real batch, the padded launch's error is at most twice the unpadded
    launch's plus 1e-5 of scale, and within 1e-3."""
    from sgan.models import BatchGATEncoder
    from test_gpu_parity import _batch_gat_ref
    torch.manual_seed(2)
    mod = BatchGATEncoder([40, 16, 40], [4, 1], 0.0, 0.2).to(DEV)
    with torch.no_grad():
        for l in mod.gat_net.layer_stack:
            l.bias.normal_(0, 0.1)
    res, (x0, dy, sc, B) = _module_runs(mod, lambda x, lab, s: mod(x, None, scenes=s), shape, 40)
    ref = BatchGATEncoder([40, 16, 40], [4, 1], 0.0, 0.2).to(DEV).double()
    ref.load_state_dict({k: v.double() for k, v in mod.state_dict().items()})
    xr = x0[:B].double().requires_grad_(True)
    yr = _batch_gat_ref(xr, ref, torch.from_numpy(sc.host_off))
    (yr * dy[:B].double()).sum().backward()
    for k, p in ref.named_parameters():
        scale = float(p.grad.abs().max())
        e_p = float((res[0][2][k].double() - p.grad).abs().max()) / scale
        e_r = float((res[1][2][k].double() - p.grad).abs().max()) / scale
        print("sgangat d%s: padded err %.3e, unpadded %.3e" % (k, e_p, e_r))
        assert e_p <= 2 * e_r + 1e-5 and e_p <= 1e-3, (k, e_p, e_r)


# ---------------------------------------------------------------------------
# the padded training step against the reference's own iterations
# ---------------------------------------------------------------------------
KEYS = ["obs_traj", "pred_traj", "obs_traj_rel", "pred_traj_rel", "obs_vel", "pred_vel", "obs_traj_g",
        "pred_traj_g", "non_linear_ped", "loss_mask", "seq_start_end"]


@pytest.mark.parametrize("selective", [True])
def test_padded_train_step_vs_reference_fixture(selective):
    """The two reference iterations of tests/golden/train_step.npz replayed by
    an eager GanTrainer (no graph) on batches padded into PaddedScenes(9
    scenes, 128 peds, np_cap 20; reps=(2,) for the D-step's [fake | real]
    batch), the host draws made by BucketedGraphTrainer._draw (the real
    scenes' noise in the reference's order, zero-padded) and passed as
    StepInputs: every nvalid / nchunks_dev / msum == 0 branch of the step at
    once, with exactly the assertions and tolerances of
    test_train_step_vs_reference_fixture -- losses 1e-4, check_step_grads
    1e-3, the CPU-Adam twin, the weight bound.  The reference is the fixture,
    not the unpadded run.

    selective=False is left out: the non-selective G-step forms its per-scene
    L2 terms in torch through SceneIndex.ped_scene_long(), which PaddedScenes
    does not provide (NotImplementedError), and would divide by the padding
    scenes' zero mask sums; the capacity-bucket trainer only runs the
    selective step."""
    from sgan.scene import PaddedScenes
    from sgan.train_step import BucketedGraphTrainer, GanTrainer, StepInputs
    from test_gpu_parity import build_models
    g, d = build_models()
    tr = GanTrainer(g, d, selective_backward=selective)
    f = np.load(os.path.join(GOLDEN, "train_step.npz"))
    S_cap, B_cap = 9, 128
    ps = PaddedScenes(S_cap, B_cap, DEV, 20, reps=(2,))
    twins = {}
    for mod, tag, lr in ((g, "g", 1e-4), (d, "d", 1e-3)):
        cp = {k: p.detach().cpu().clone().requires_grad_(True) for k, p in mod.named_parameters()}
        twins[tag] = (cp, torch.optim.Adam(list(cp.values()), lr=lr))
    torch.manual_seed(1234)
    random.seed(1234)
    for it in range(2):
        b = [torch.from_numpy(f["b%d/%s" % (it, k)]).clone() for k in KEYS]
        sse = b[-1].numpy()
        off_real = np.concatenate([[0], sse[:, 1]]).astype(np.int64)
        S, B = len(off_real) - 1, int(off_real[-1])
        ps.load(off_real, np.arange(B, dtype=np.int32))
        off = ps.host_off
        batch = [pad(t.to(DEV), B_cap, 1) for t in b[:8]] + [pad(t.to(DEV), B_cap, 0) for t in b[8:10]]
        batch.append(torch.from_numpy(np.stack([off[:-1], off[1:]], 1).astype(np.int64)))
        z_d, z_g, y = BucketedGraphTrainer._draw(tr, S_cap, {"S_real": (S, S)})
        assert z_d.shape[0] == S_cap and all_zero(z_d[S:]) and all_zero(z_g[:, S:])
        ld, lg = tr.step(batch, ps, inputs=StepInputs(z_d.to(DEV), z_g.to(DEV), y.to(DEV)))
        for mod, tag, lr in ((g, "g", 1e-4), (d, "d", 1e-3)):
            cp, opt = twins[tag]
            for k, p in mod.named_parameters():
                cp[k].grad = p.grad.detach().cpu().clone() if p.grad is not None else None
            opt.step()
            for k, p in mod.named_parameters():
                err = (p.detach().cpu() - cp[k].detach()).abs().max().item()
                assert err <= 1e-2 * lr + 1e-6 * cp[k].abs().max().item(), ("Adam update", it, tag, k, err)
        for k, v in list(ld.items()) + list(lg.items()):
            tag = "D" if k.startswith("D") else "G"
            ref = float(f["it%d/%s/%s" % (it, tag, k)])
            print("it%d %s: %.7f (reference %.7f)" % (it, k, float(v), ref))
            assert abs(float(v) - ref) <= 1e-4 * max(1.0, abs(ref)), (it, k, float(v), ref)
        check_step_grads({k: p.grad for k, p in d.named_parameters() if p.grad is not None}, f, it, "D")
        check_step_grads({k: p.grad for k, p in g.named_parameters() if p.grad is not None}, f, it, "G")
        for mod, tag, lr in ((g, "g", 1e-4), (d, "d", 1e-3)):
            for k, v in mod.state_dict().items():
                ref = f["it%d/%s/%s" % (it, tag, k)]
                err = np.abs(v.detach().cpu().numpy().astype(np.float64) - ref).max()
                assert err <= 2 * lr * (it + 1) + 1e-5 * np.abs(ref).max(), (it, tag, k, err)
