"""Social pooling with dropout (sgg_pool_fwd_bn_drop / sgg_pool_bwd_bn_drop /
sgg_pool_dpos_drop): symbols, argument checks, the mask contract on the host
(sgan.kernels.pool_dropout_keep_host against hand-built Philox counters), the
float64 yardstick's own argmax statistics, and the refusals that stay.  Host
code only, no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import _pool_dropout_ref as R

SYMBOLS = ("sgg_pool_fwd_bn_drop", "sgg_pool_bwd_bn_drop", "sgg_pool_dpos_drop")
E_ARG = -1
_P = ctypes.c_void_p(64)    # non-NULL, never dereferenced: every check below fails before any launch


@pytest.fixture(scope="module")
def lib():
    from sgan import _native
    return _native.load(require_gpu=False)


def test_symbols_declared_and_exported(lib):
    import os
    from sgan import _native, kernels as K
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sgg.h")).read()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None
        assert name in _native.SIGNATURES and ("int %s(" % name) in hdr
    assert "#define SGG_POOL_DROP_SITE_HIDDEN %d" % K.POOL_DROP_SITE_HIDDEN in hdr
    assert "#define SGG_POOL_DROP_SITE_OUT %d" % K.POOL_DROP_SITE_OUT in hdr
    assert K.POOL_DROP_SITE_HIDDEN > 7 and K.POOL_DROP_SITE_OUT > 7      # clear of the GAT families' sites
    assert K.POOL_DROP_SITE_HIDDEN != K.POOL_DROP_SITE_OUT


def _refused(lib, rc, *needles):
    assert rc == E_ARG, rc
    msg = lib.sgg_last_error()
    assert msg, "no message"
    for n in needles:
        assert n in msg, (n, msg)


def _fwd_args(**kw):
    a = dict(U=_P, pos=_P, A=_P, W2=_P, b2=_P, off=_P, chunks=_P, nchunks=1, max_rows=4, gpw=4, B=8, bn=72, max_n=8,
             out=_P, am=_P, p=0.5, seed=1, offset=0, rng=None)
    a.update(kw)
    return [a[k] for k in ("U", "pos", "A", "W2", "b2", "off", "chunks", "nchunks", "max_rows", "gpw", "B", "bn",
                           "max_n", "out", "am", "p", "seed", "offset", "rng")] + [None]


def _bwd_args(**kw):
    a = dict(U=_P, pos=_P, A=_P, W2=_P, out=_P, am=_P, dout=_P, off=_P, S=2, B=8, bn=72, max_n=8, dU=_P, part=_P,
             nws=1 << 40, p=0.5, seed=1, offset=0, rng=None)
    a.update(kw)
    return [a[k] for k in ("U", "pos", "A", "W2", "out", "am", "dout", "off", "S", "B", "bn", "max_n", "dU", "part",
                           "nws", "p", "seed", "offset", "rng")] + [None]


def _dpos_args(**kw):
    a = dict(U=_P, pos=_P, A=_P, W2=_P, out=_P, am=_P, dout=_P, off=_P, S=2, B=8, bn=72, dpos=_P, p=0.5, seed=1,
             offset=0, rng=None)
    a.update(kw)
    return [a[k] for k in ("U", "pos", "A", "W2", "out", "am", "dout", "off", "S", "B", "bn", "dpos", "p", "seed",
                           "offset", "rng")] + [None]


_CALLS = (("sgg_pool_fwd_bn_drop", _fwd_args), ("sgg_pool_bwd_bn_drop", _bwd_args), ("sgg_pool_dpos_drop", _dpos_args))


@pytest.mark.parametrize("p", [-0.25, 1.0, 1.5, float("nan")])
def test_bad_p(lib, p):
    for name, args in _CALLS:
        _refused(lib, getattr(lib, name)(*args(p=p)), name.encode(), b"[0, 1)")


@pytest.mark.parametrize("op", ["U", "pos", "A", "W2", "b2", "off", "chunks", "out", "am"])
def test_fwd_null_operand(lib, op):
    _refused(lib, lib.sgg_pool_fwd_bn_drop(*_fwd_args(**{op: None})), b"sgg_pool_fwd_bn_drop")


@pytest.mark.parametrize("op", ["U", "pos", "A", "W2", "out", "am", "dout", "off", "dU"])
def test_bwd_null_operand(lib, op):
    _refused(lib, lib.sgg_pool_bwd_bn_drop(*_bwd_args(**{op: None})), b"sgg_pool_bwd_bn_drop")


@pytest.mark.parametrize("op", ["U", "pos", "A", "W2", "out", "am", "dout", "off", "dpos"])
def test_dpos_null_operand(lib, op):
    _refused(lib, lib.sgg_pool_dpos_drop(*_dpos_args(**{op: None})), b"sgg_pool_dpos_drop")


@pytest.mark.parametrize("bn", [0, 1025])
def test_bad_bn(lib, bn):
    for name, args in _CALLS:
        _refused(lib, getattr(lib, name)(*args(bn=bn)), name.encode(), b"1024")


def test_bwd_workspace_too_small(lib):
    need = lib.sgg_pool_bwd_bn_ws_floats(2, 8, 72, 8)
    _refused(lib, lib.sgg_pool_bwd_bn_drop(*_bwd_args(nws=need - 1)), b"sgg_pool_bwd_bn_drop", b"workspace")


# ---- the mask on the host ------------------------------------------------------
def _by_hand(p, seed, offset, site, i, j, col):
    """One element through philox4x32_10_host with the counter of sgg.h spelled out."""
    from sgan import kernels as K
    c1 = (j << 8) | ((col >> 4) << 2) | (col & 3)
    w = K.philox4x32_10_host((i, c1, site << 8, offset), (seed & 0xFFFFFFFF, seed >> 32))
    thr = int(float(np.float32(p)) * 4294967296.0)
    return int(w[(col >> 2) & 3]) >= thr


@pytest.mark.parametrize("p", [0.25, 0.5])
def test_keep_host_against_hand_built_counters(p):
    from sgan import kernels as K
    seed, offset = 0x123456789ABCDEF, 0xFFFFFFF0
    rows, js, cols = [0, 5, 1023, 70000], [0, 1, 37, 1023], [0, 3, 4, 15, 16, 511, 1023]
    for site in (K.POOL_DROP_SITE_HIDDEN, K.POOL_DROP_SITE_OUT):
        got = K.pool_dropout_keep_host(p, seed, offset, site, rows, js, cols)
        assert got.shape == (len(rows), len(js), len(cols)) and got.dtype == np.bool_
        for a, i in enumerate(rows):
            for b, j in enumerate(js):
                for c, col in enumerate(cols):
                    assert bool(got[a, b, c]) == _by_hand(p, seed, offset, site, i, j, col), (site, i, j, col)


def test_four_words_of_one_call_cover_col_plus_4_8_12():
    """Columns col, col + 4, col + 8, col + 12 share one counter and take its words 0..3."""
    from sgan import kernels as K
    seed, offset, i, j = 99, 3, 41, 17
    for col in (0, 3, 16, 35, 496, 1008):
        c1 = (j << 8) | ((col >> 4) << 2) | (col & 3)
        w = K.philox4x32_10_host((i, c1, K.POOL_DROP_SITE_HIDDEN << 8, offset), (seed, 0))
        got = K.pool_dropout_keep_host(0.5, seed, offset, K.POOL_DROP_SITE_HIDDEN, [i], [j],
                                       [col, col + 4, col + 8, col + 12])
        assert [bool(v) for v in got[0, 0]] == [int(w[q]) >= 1 << 31 for q in range(4)]


def test_mask_changes_with_site_offset_i_j():
    from sgan import kernels as K
    base = dict(p=0.5, seed=7, offset=11, site=K.POOL_DROP_SITE_HIDDEN, i_rows=np.arange(40, 48), j_local=np.arange(8),
                cols=np.arange(512))
    m0 = K.pool_dropout_keep_host(**base)
    assert np.array_equal(m0, K.pool_dropout_keep_host(**base))
    for change in (dict(site=K.POOL_DROP_SITE_OUT), dict(offset=12), dict(seed=8), dict(i_rows=np.arange(41, 49)),
                   dict(j_local=np.arange(1, 9))):
        m1 = K.pool_dropout_keep_host(**dict(base, **change))
        assert 0.4 < float((m0 != m1).mean()) < 0.6, change
    # a pure function of (i, j, col): a sub-block is the block of the whole
    sub = K.pool_dropout_keep_host(**dict(base, i_rows=[43], j_local=[5], cols=np.arange(100, 200)))
    assert np.array_equal(sub[0, 0], m0[3, 5, 100:200])


@pytest.mark.parametrize("p", [0.0, 0.1, 0.25, 0.5, 0.9])
def test_keep_fraction(p):
    from sgan import kernels as K
    n = 1 << 16
    keep = K.pool_dropout_keep_host(p, 2024, 5, K.POOL_DROP_SITE_OUT, np.arange(16), np.arange(16), np.arange(256))
    assert keep.size == n
    sigma = np.sqrt(p * (1 - p) / n)
    assert abs(float(keep.mean()) - (1 - p)) <= 4 * sigma + 1e-12, (float(keep.mean()), 1 - p, sigma)
    with pytest.raises(ValueError):
        K.pool_dropout_keep_host(1.0, 1, 0, K.POOL_DROP_SITE_OUT, [0], [0], [0])


# ---- the yardstick itself ------------------------------------------------------
@pytest.mark.parametrize("p", R.PS)
@pytest.mark.parametrize("sizes_id", range(len(R.SIZES)))
@pytest.mark.parametrize("bn", R.BNS)
def test_yardstick_argmax_is_decided(bn, sizes_id, p):
    """The float64 yardstick alone, at the seeds the GPU tests use: at most 1 %
    of the entries have out > 0 and a top-two gap within 1e-5 of the range (the
    entries the GPU test may not compare), dropout really drops, and the
    yardstick at the masks' p differs from the net without dropout."""
    c = R.case(bn, sizes_id, p)
    assert c["excluded"] <= 0.01 * c["total"], (c["excluded"], c["total"])
    assert 0 < c["live"] < c["total"]
    assert int(c["compare"].sum()) >= 0.2 * c["total"]      # the comparison is not vacuous


def test_module_linears_found_by_type_and_state_dict_keys():
    from sgan import kernels as K
    from sgan.models import PoolHiddenNet
    net = PoolHiddenNet(16, 32, 64, 24, "relu", False, dropout=0.25)
    keys = set(net.state_dict())
    assert {"mlp_pre_pool.0.weight", "mlp_pre_pool.3.weight", "mlp_pre_pool.3.bias"} <= keys
    assert not any(".2." in k for k in keys)
    l1, l2 = K.pool_linears(net)
    assert l1 is net.mlp_pre_pool[0] and l2 is net.mlp_pre_pool[3] and l2.out_features == 24
    assert not net.fused_ok()
    plain = PoolHiddenNet(16, 32, 64, 24, "relu", False, dropout=0.0)
    assert K.pool_linears(plain)[1] is plain.mlp_pre_pool[2] and plain.fused_ok()
    assert K.pool_fold_spec(net)[3] is net.mlp_pre_pool[0].bias


# ---- refusals -------------------------------------------------------------------
@pytest.mark.parametrize("bn", [8, 72])
def test_padded_plans_refuse_dropout_by_name(bn):
    from sgan.scene import PaddedScenes
    ps = PaddedScenes(4, 32, "cpu", 20, reps=(2,))
    ps.load(np.array([0, 5, 12], np.int32), np.arange(12, dtype=np.int32))
    for sc in (ps, ps.repeat(2)):
        with pytest.raises(NotImplementedError, match="dropout"):
            sc.pool_plan(bn, family_bn=True, dropout=True)
    assert ps.pool_plan(8)[3] >= 1    # a built width without dropout still plans


def _generator(dropout, pool_every_timestep=False):
    from sgan.models import TrajectoryGenerator
    return TrajectoryGenerator(8, 12, embedding_dim=16, encoder_h_dim=32, decoder_h_dim=32, mlp_dim=64, num_layers=1,
                               noise_dim=(8,), noise_type="gaussian", noise_mix_type="global", pooling_type="pool_net",
                               pool_every_timestep=pool_every_timestep, dropout=dropout, bottleneck_dim=8,
                               batch_norm=False, n_units=[40, 16, 40], n_heads=1, dropout1=0.0, alpha=0.2, graph="gat")


@pytest.mark.parametrize("where", ["decoder", "generator"])
def test_gan_trainer_refuses_pooling_dropout(where):
    """The decoder's pooling net gets the constructor's dropout
    (pool_every_timestep=1, reference models.py:124-132); the generator's own
    is built without it (models.py:769-776), so the test installs one."""
    from sgan.models import PoolHiddenNet, TrajectoryDiscriminator
    from sgan.train_step import GanTrainer
    d = TrajectoryDiscriminator(8, 12, embedding_dim=16, h_dim=48, mlp_dim=64, num_layers=1, batch_norm=False,
                                dropout=0.0, d_type="local")
    if where == "decoder":
        g = _generator(0.25, True)
        assert g.decoder.pool_net.dropout == 0.25 and g.pool_net.dropout == 0
    else:
        g = _generator(0.0)
        g.pool_net = PoolHiddenNet(16, 32, 64, 8, "relu", False, dropout=0.25)
    with pytest.raises(NotImplementedError, match="dropout=0.25"):
        GanTrainer(g, d)
