"""The validation pass on the device: sgg_val_metrics (csrc/metrics.hip)
against a float64 restatement, its accumulation and determinism, and
sgan.validate.check_accuracy against the reference's own check_accuracy
(tests/golden/check_accuracy.json)."""
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda"
OBS = 8
KEYS = ("d_loss", "g_l2_loss_abs", "g_l2_loss_rel", "ade", "fde", "ade_l", "fde_l", "ade_nl", "fde_nl")


# ---------------------------------------------------------------------------
# 1. the kernel against fp64
# ---------------------------------------------------------------------------
def make_inputs(B, T, nl_mode, seed):
    """Random trajectories on a 1/256 m grid (the datasets' coordinates are on
    a centimetre grid): positions within +-16 m, so the cumulative sum, the
    start add and the differences are exact in fp32 whatever their order, and
    the two fp32 routes differ from fp64 by the roundings of the squares, the
    square roots, the BCE terms and the sums only -- what the bound is about."""
    rng = np.random.default_rng(seed)
    grid = lambda a: np.round(a * 256.0) / 256.0
    start = grid(rng.uniform(-8, 8, size=(B, 2)))
    gt_rel = grid(rng.normal(0, 0.3, size=(T, B, 2)))
    pred_rel = grid(gt_rel + rng.normal(0, 0.2, size=(T, B, 2)))
    gt = start[None] + np.cumsum(gt_rel, 0)
    mask20 = (rng.uniform(size=(B, 20)) < 0.8).astype(np.float64)
    nl = {"zeros": np.zeros(B), "ones": np.ones(B), "mixed": (rng.uniform(size=B) < 0.4).astype(np.float64)}[nl_mode]
    scores = rng.normal(0, 1.5, size=2 * B)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(DEV)
    return dict(pred_rel=f(pred_rel), gt=f(gt), gt_rel=f(gt_rel), start=f(start), mask20=f(mask20), nl=f(nl),
                scores=f(scores))


def ref64(x, T, y_real, with_scores):
    """numpy float64 on the same fp32 inputs -> the eleven slots."""
    d = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in x.items()}
    B = d["nl"].shape[0]
    mask = d["mask20"][:, OBS:OBS + T]                       # (B, T)
    fake = d["start"][None] + np.cumsum(d["pred_rel"], 0)    # (T, B, 2)
    m = mask.T[:, :, None]
    dist = np.sqrt(((d["gt"] - fake) ** 2).sum(2))           # (T, B)
    ade, fde = dist.sum(0), dist[-1]
    nl, lin = d["nl"], 1.0 - d["nl"]
    bce = lambda s, y: (np.maximum(s, 0) - s * y + np.log1p(np.exp(-np.abs(s)))).mean()
    out = [(m * (d["gt"] - fake) ** 2).sum(), (m * (d["gt_rel"] - d["pred_rel"]) ** 2).sum(),
           ade.sum(), (ade * lin).sum(), (ade * nl).sum(), fde.sum(), (fde * lin).sum(), (fde * nl).sum(),
           bce(d["scores"][B:], np.float64(np.float32(y_real))) + bce(d["scores"][:B], 0.0) if with_scores else 0.0,
           lin.sum(), nl.sum()]
    return np.array(out, np.float64)


def torch32(x, T, y_real, with_scores):
    """The fp32 torch route the kernel replaces, on the device."""
    from sgan.losses import bce_loss, displacement_error, final_displacement_error, l2_loss
    from sgan.utils import relative_to_abs
    B = x["nl"].shape[0]
    mask = x["mask20"][:, OBS:OBS + T]
    fake = relative_to_abs(x["pred_rel"], x["start"])
    nl, lin = x["nl"], 1 - x["nl"]
    sf, sr = x["scores"][:B].view(B, 1), x["scores"][B:].view(B, 1)
    out = [l2_loss(fake, x["gt"], mask, mode="sum"), l2_loss(x["pred_rel"], x["gt_rel"], mask, mode="sum"),
           displacement_error(fake, x["gt"]), displacement_error(fake, x["gt"], lin),
           displacement_error(fake, x["gt"], nl), final_displacement_error(fake[-1], x["gt"][-1]),
           final_displacement_error(fake[-1], x["gt"][-1], lin), final_displacement_error(fake[-1], x["gt"][-1], nl),
           (bce_loss(sr, torch.ones_like(sr) * y_real) + bce_loss(sf, torch.zeros_like(sf))) if with_scores
           else torch.zeros((), device=DEV), lin.sum(), nl.sum()]
    return np.array([float(v) for v in out], np.float64)


def launch(x, T, y_real, with_scores, acc=None, work=None):
    from sgan import _native as N
    lib = N.load()
    B = x["nl"].shape[0]
    acc = acc if acc is not None else torch.zeros(N.VAL_SLOTS, dtype=torch.float64, device=DEV)
    if work is None:
        work = torch.zeros(int(lib.sgg_val_metrics_work_floats(B)), dtype=torch.float32, device=DEV)
    mask = x["mask20"][:, OBS:OBS + T]   # the strided view: rows of 20 floats
    assert mask.stride(0) == 20 and mask.data_ptr() != x["mask20"].data_ptr()
    N.check(lib.sgg_val_metrics(N.ptr(x["pred_rel"]), N.ptr(x["gt"]), N.ptr(x["gt_rel"]), N.ptr(x["start"]),
                                N.ptr(mask), 20, N.ptr(x["nl"]), N.ptr(x["scores"]) if with_scores else None,
                                float(y_real), T, B, N.ptr(acc), N.ptr(work), N.stream_ptr()), "sgg_val_metrics")
    return acc, work


@pytest.mark.parametrize("T", [1, 12])
@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 256, 257, 1000])
def test_kernel_against_fp64(B, T):
    """One lane, both sides of a wave (64) and of a workgroup (256), several
    workgroups for the ticket; non_linear all 0 / all 1 / mixed; with scores
    and without.  Per slot the kernel's error against float64 is at most
    twice the fp32 torch route's plus 1e-6 of the slot's value
    (test_gpu_gat_wide.py test 1's rule); the ped counts are exact."""
    y_real = 0.9
    for i, nl_mode in enumerate(("zeros", "ones", "mixed")):
        x = make_inputs(B, T, nl_mode, seed=1000 * B + 10 * T + i)
        for with_scores in (True, False):
            ref = ref64(x, T, y_real, with_scores)
            t32 = torch32(x, T, y_real, with_scores)
            acc, work = launch(x, T, y_real, with_scores)
            got = acc.cpu().numpy()
            assert int(work.view(torch.int32)[0]) == 0, "ticket left non-zero"
            for s in range(11):
                ek, et, scale = abs(got[s] - ref[s]), abs(t32[s] - ref[s]), abs(ref[s])
                print("B %d T %d %s scores %d slot %2d: kernel err %.3e torch err %.3e (scale %.3e)"
                      % (B, T, nl_mode, with_scores, s, ek, et, scale))
                if s >= 9:
                    assert got[s] == ref[s], (s, got[s], ref[s])
                else:
                    assert ek <= 2 * et + 1e-6 * scale, (nl_mode, with_scores, s, got[s], ref[s], t32[s])
            if not with_scores:
                assert got[8] == 0.0


# ---------------------------------------------------------------------------
# 2. accumulation and determinism
# ---------------------------------------------------------------------------
def _batch_of(x, T):
    """An 11-tuple (only the members ValSums.add reads are real)."""
    B = x["nl"].shape[0]
    obs = x["start"].view(1, B, 2).expand(OBS, B, 2)
    return [obs, x["gt"], None, x["gt_rel"], None, None, None, None, x["nl"], x["mask20"], None]


def test_accumulation_and_determinism():
    from sgan import _native as N
    from sgan.validate import ValSums
    xa, xb = make_inputs(300, 12, "mixed", 5), make_inputs(77, 12, "mixed", 6)

    def run(batches):
        s = ValSums(DEV)
        for x in batches:
            s.add(x["pred_rel"], _batch_of(x, 12), OBS, x["scores"], 0.8)
        return s

    both, a, b = run([xa, xb]), run([xa]), run([xb])
    # (0 + a) + b against a + b: the fp64 add is the only difference, and 0 + a == a
    assert torch.equal(both.acc, a.acc + b.acc)
    assert torch.equal(run([xa, xb]).acc, both.acc), "two runs of the same sequence differ"
    r = both.read()
    assert (r["total_traj"], r["loss_mask_sum"], r["n_batches"]) == (377, 377 * 12, 2)
    assert r["n_l"] + r["n_nl"] == 377
    # a refused call leaves the accumulator alone
    lib = N.load()
    before = both.acc.clone()
    x = xa
    rc = lib.sgg_val_metrics(N.ptr(x["pred_rel"]), N.ptr(x["gt"]), N.ptr(x["gt_rel"]), N.ptr(x["start"]),
                             N.ptr(x["mask20"][:, OBS:]), 20, N.ptr(x["nl"]), None, 0.0, 0, 300, N.ptr(both.acc),
                             N.ptr(both.work), N.stream_ptr())
    assert rc == -1
    torch.cuda.synchronize()
    assert torch.equal(both.acc, before)


# ---------------------------------------------------------------------------
# 3. the module against the reference's own check_accuracy
# ---------------------------------------------------------------------------
def cases():
    return json.load(open(os.path.join(GOLDEN, "check_accuracy.json")))


class Args:
    def __init__(self, c):
        self.obs_len, self.pred_len, self.skip, self.delim = 8, 12, 1, "tab"
        self.loader_num_workers = 0
        self.batch_size = c["batch_size"]
        self.num_samples_check = c["num_samples_check"]


def seed(c):
    torch.manual_seed(c["seed"])
    random.seed(c["seed"])


def split_dir(c):
    return os.path.join(GOLDEN, "datasets_group", c["split"], c["dset_type"])


@pytest.mark.parametrize("name", sorted(cases()))
def test_check_accuracy_vs_reference_fixture(name):
    """Every value within 1e-3 relative (test_evaluate_ade_fde_all_splits'
    gate on the same kind of fixture), both host streams where the reference
    leaves them, the generator back in train mode."""
    from sgan.data.loader import data_loader
    from sgan.validate import check_accuracy
    from test_gpu_parity import build_models
    c = cases()[name]
    g, d = build_models(c["family"])
    g.train()
    a = Args(c)
    _, loader = data_loader(a, split_dir(c))
    seed(c)
    got = check_accuracy(a, loader, g, d, limit=c["limit"])
    after = (random.random(), float(torch.rand(1)))
    assert g.training
    ref = c["metrics"]
    assert sorted(got) == sorted(ref) == sorted(KEYS)
    for k in KEYS:
        print("%-14s got %.9g ref %.9g" % (k, got[k], ref[k]))
        assert abs(got[k] - ref[k]) <= 1e-3 * abs(ref[k]), (k, got[k], ref[k])
    assert after == (c["after"]["random"], c["after"]["torch"]), "host RNG streams"


# ---------------------------------------------------------------------------
# 4. loader forms and branches
# ---------------------------------------------------------------------------
def test_device_loader_equals_host_loader():
    """test_evaluate_with_device_data_path's tolerance: 1e-3."""
    from sgan.data.device import device_data_loader
    from sgan.data.loader import data_loader
    from sgan.validate import check_accuracy
    from test_gpu_parity import build_models
    c = cases()["gat/eth"]
    g, d = build_models("gat")
    a = Args(c)
    _, host = data_loader(a, split_dir(c))
    seed(c)
    mh = check_accuracy(a, host, g, d)
    _, dev = device_data_loader(a, split_dir(c), DEV)
    seed(c)
    md = check_accuracy(a, dev, g, d)
    after = (random.random(), float(torch.rand(1)))
    for k in KEYS:
        assert abs(md[k] - mh[k]) <= 1e-3 * abs(mh[k]), (k, md[k], mh[k])
        assert abs(md[k] - c["metrics"][k]) <= 1e-3 * abs(c["metrics"][k]), (k, md[k])
    assert after == (c["after"]["random"], c["after"]["torch"])


def _hand_batches():
    from sgan.data.synthetic import synthetic_batch
    out = []
    for i, sizes in enumerate(([5, 3, 9], [2, 20, 1, 4])):
        b = list(synthetic_batch(sizes, seed=30 + i))
        b[8] = torch.ones_like(b[8])   # every ped non-linear
        out.append(tuple(b))
    return out


def test_branches_raw_and_custom_loss():
    from sgan.losses import bce_loss
    from sgan.validate import check_accuracy, reference_metrics
    from test_gpu_parity import build_models
    g, d = build_models("gat")
    a = Args(dict(batch_size=64, num_samples_check=5000))
    batches = _hand_batches()

    def run(**kw):
        torch.manual_seed(3)
        random.seed(3)
        return check_accuracy(a, batches, g, d, **kw)

    m = run()
    # no linear ped: the reference's integer 0
    assert m["ade_l"] == 0 and m["fde_l"] == 0 and isinstance(m["ade_l"], int)
    assert m["ade_nl"] > 0 and m["ade_nl"] == m["ade"] and m["fde_nl"] == m["fde"]   # (every ped is non-linear)
    # raw: the separated sums, which recombine to the aliased dict
    raw = run(raw=True)
    assert (raw["total_traj"], raw["n_batches"], raw["loss_mask_sum"]) == (44, 2, 44 * 12)
    assert raw["n_l"] == 0 and raw["n_nl"] == 44 and raw["ade_l"] == 0 and raw["ade"] == raw["ade_nl"] > 0
    assert raw["l2_abs"] != raw["l2_rel"]
    assert reference_metrics(raw, 12) == m
    assert m["ade"] == (raw["ade"] + raw["ade_l"] + raw["ade_nl"]) / (44 * 12) == 2 * raw["ade"] / (44 * 12)
    # limit: the host-known ped count stops the loop after the first batch
    a.num_samples_check = 10
    assert run(limit=True, raw=True)["n_batches"] == 1
    a.num_samples_check = 5000
    # a custom loss callable is honoured, gets (scores_real, scores_fake), draws nothing itself here
    seen = []

    def const_loss(sr, sf):
        seen.append((tuple(sr.shape), tuple(sf.shape)))
        return sr.sum() * 0 + 2.5

    mc = run(d_loss_fn=const_loss)
    assert mc["d_loss"] == 2.5 and seen == [((17, 1), (17, 1)), ((27, 1), (27, 1))]
    assert random.random() == random.Random(3).random(), "the fused path's label draws were made for a custom loss"
    assert mc["ade"] == m["ade"]

    def torch_d_loss(sr, sf):   # gan_d_loss, restated: the fused path's value
        y = random.uniform(0.7, 1.2)
        random.uniform(0, 0.3)
        return bce_loss(sr, torch.ones_like(sr) * y) + bce_loss(sf, torch.zeros_like(sf))

    mt = run(d_loss_fn=torch_d_loss)
    assert abs(mt["d_loss"] - m["d_loss"]) <= 1e-5 * abs(m["d_loss"]), (mt["d_loss"], m["d_loss"])


# ---------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from sgan import _native as N
    lib = N.load()
    x = make_inputs(5, 12, "mixed", 9)
    acc = torch.full((N.VAL_SLOTS,), 7.0, dtype=torch.float64, device=DEV)
    work = torch.zeros(int(lib.sgg_val_metrics_work_floats(5)), dtype=torch.float32, device=DEV)
    mask = x["mask20"][:, OBS:]
    ok = dict(pred_rel=N.ptr(x["pred_rel"]), gt=N.ptr(x["gt"]), gt_rel=N.ptr(x["gt_rel"]), start=N.ptr(x["start"]),
              mask=N.ptr(mask), ld=20, nl=N.ptr(x["nl"]), T=12, B=5, acc=N.ptr(acc), work=N.ptr(work))

    def call(**kw):
        q = dict(ok, **kw)
        return lib.sgg_val_metrics(q["pred_rel"], q["gt"], q["gt_rel"], q["start"], q["mask"], q["ld"], q["nl"], None,
                                   0.0, q["T"], q["B"], q["acc"], q["work"], N.stream_ptr())

    bad = [dict([(k, None)]) for k in ("pred_rel", "gt", "gt_rel", "start", "mask", "nl", "acc", "work")]
    bad += [dict(B=0), dict(B=-1), dict(T=0), dict(T=-2), dict(ld=11)]
    for kw in bad:
        with pytest.raises(N.NativeError, match="sgg_val_metrics"):
            N.check(call(**kw), "sgg_val_metrics")
    torch.cuda.synchronize()
    assert torch.equal(acc, torch.full_like(acc, 7.0)) and int(work.view(torch.int32)[0]) == 0
    N.check(call(), "sgg_val_metrics")   # the same arguments unspoiled are accepted
    torch.cuda.synchronize()
    assert float(acc[2]) > 7.0 and float(acc[8]) == 7.0
