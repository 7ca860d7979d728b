"""The restatement of the validation loop (tests/_check_accuracy_ref.py) on
the float32 CPU oracle's models against the reference's own check_accuracy
(tests/golden/check_accuracy.json, make_golden_check_accuracy.py): every
value within HALF of the 1e-3 the GPU test (test_gpu_validate.py) applies to
the same fixture, and both host RNG streams left exactly where the reference
leaves them.  Also the argument refusals of sgg_val_metrics, which are made
before the device is touched.  CPU only."""
import ctypes
import json
import os
import random

import pytest
import torch

from conftest import GOLDEN

from _check_accuracy_ref import check_accuracy_ref
from test_oracle_golden import load_models

RTOL = 0.5e-3
KEYS = ("d_loss", "g_l2_loss_abs", "g_l2_loss_rel", "ade", "fde", "ade_l", "fde_l", "ade_nl", "fde_nl")


def cases():
    return json.load(open(os.path.join(GOLDEN, "check_accuracy.json")))


class Args:
    def __init__(self, c):
        self.obs_len, self.pred_len, self.skip, self.delim = 8, 12, 1, "tab"
        self.loader_num_workers = 0
        self.batch_size = c["batch_size"]
        self.num_samples_check = c["num_samples_check"]


def check_case(c, got, rtol):
    """got against the case's recorded dict, then the two stream positions
    (drawn here: call right after the pass)."""
    after = (random.random(), float(torch.rand(1)))
    ref = c["metrics"]
    assert sorted(got) == sorted(ref) == sorted(KEYS)
    for k in KEYS:
        print("%-14s got %.9g ref %.9g" % (k, got[k], ref[k]))
        if ref[k] == 0:
            assert got[k] == 0, k
        else:
            assert abs(got[k] - ref[k]) <= rtol * abs(ref[k]), (k, got[k], ref[k])
    assert after == (c["after"]["random"], c["after"]["torch"]), "host RNG streams"


def test_fixture_covers_the_cases():
    cs = cases()
    assert {c["family"] for c in cs.values()} >= {"gat", "gcn"}
    assert any(c["limit"] and c["n_batches"] == 3 for c in cs.values())
    assert any(not c["limit"] for c in cs.values())
    # the aliasing of train.py:490-492 is in the recorded numbers
    for c in cs.values():
        m = c["metrics"]
        assert m["g_l2_loss_abs"] == m["g_l2_loss_rel"]
        assert m["ade"] > 0 and m["fde"] > 0
        # one numerator for the three: ade_l / ade = total_traj / linear peds = fde_l / fde
        if m["ade_l"] != 0:
            assert m["ade_l"] / m["ade"] == pytest.approx(m["fde_l"] / m["fde"], rel=1e-12)


@pytest.mark.parametrize("name", sorted(cases()))
def test_restatement_reproduces_reference(name):
    from sgan.data.loader import data_loader
    c = cases()[name]
    g, d = load_models(graph=c["family"])
    g.train()
    a = Args(c)
    _, loader = data_loader(a, os.path.join(GOLDEN, "datasets_group", c["split"], c["dset_type"]))
    torch.manual_seed(c["seed"])
    random.seed(c["seed"])
    got = check_accuracy_ref(a, loader, g, d, limit=c["limit"])
    assert g.training
    check_case(c, got, RTOL)


def _lib():
    from sgan import _native
    if not os.path.exists(_native.lib_path()):
        pytest.skip("libsgg.so not built")
    return _native, _native.load(require_gpu=False)


def test_val_metrics_refuses_bad_arguments_without_a_device():
    """NULL operands, B < 1, T < 1, ld < T: SGG_E_ARG and a message, checked
    before anything touches the device (the pointers here are never read)."""
    N, lib = _lib()
    p = ctypes.c_void_p(4096)   # non-NULL, 8-byte aligned, never dereferenced
    ok = dict(pred_rel=p, gt=p, gt_rel=p, start=p, mask=p, ld=12, nl=p, scores=None, y=0.9, T=12, B=5, acc=p, work=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sgg_val_metrics(a["pred_rel"], a["gt"], a["gt_rel"], a["start"], a["mask"], a["ld"], a["nl"],
                                   a["scores"], a["y"], a["T"], a["B"], a["acc"], a["work"], None)

    for kw in ([dict([(k, None)]) for k in ("pred_rel", "gt", "gt_rel", "start", "mask", "nl", "acc", "work")]
               + [dict(B=0), dict(B=-3), dict(T=0), dict(ld=11), dict(acc=ctypes.c_void_p(4100))]):
        assert call(**kw) == -1, kw
        assert b"sgg_val_metrics" in lib.sgg_last_error(), kw
        with pytest.raises(N.NativeError, match="sgg_val_metrics"):
            N.check(call(**kw), "sgg_val_metrics")


def test_val_metrics_work_floats():
    """A ticket word, a pad word, then SGG_VAL_SLOTS + 1 doubles per
    workgroup of 256 peds."""
    N, lib = _lib()
    per = 2 * (N.VAL_SLOTS + 1)
    assert lib.sgg_val_metrics_work_floats(0) == 0 and lib.sgg_val_metrics_work_floats(-1) == 0
    for B, blocks in ((1, 1), (256, 1), (257, 2), (1000, 4), (20480, 80), (2 ** 31 - 1, 2 ** 23)):
        assert lib.sgg_val_metrics_work_floats(B) == 2 + per * blocks, B
