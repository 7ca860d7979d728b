"""The C ABI of the column-tiled pooling family (sgg_pool_*_bn, any
bottleneck_dim up to SGG_POOL_BN_MAX): symbols, argument checks, the
workspace bound and the chunk plan.  Host code only, no GPU."""
import ctypes

import numpy as np
import pytest

SYMBOLS = ("sgg_pool_plan_bn", "sgg_pool_fwd_bn", "sgg_pool_bwd_bn_grid", "sgg_pool_bwd_bn_ws_floats",
           "sgg_pool_bwd_bn")
E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from sgan import _native
    return _native.load(require_gpu=False)


def _plan(lib, sizes, bn, target, fn="sgg_pool_plan_bn"):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    S = len(sizes)
    cap = int(off[-1]) + S + 1
    tab = np.zeros((cap, 4), np.int32)
    mr, gpw = ctypes.c_int(0), ctypes.c_int(0)
    nc = getattr(lib, fn)(off.ctypes.data_as(ctypes.c_void_p), S, bn, target, tab.ctypes.data_as(ctypes.c_void_p),
                          cap, ctypes.byref(mr), ctypes.byref(gpw))
    return nc, tab, mr.value, gpw.value


def test_symbols_exist(lib):
    for name in SYMBOLS:
        assert getattr(lib, name) is not None
    from sgan import kernels as K
    from sgan import scene
    assert K.POOL_BN_MAX == scene.SGG_POOL_BN_MAX == 1024 and K.POOL_MAX_BN == 64


def _refused(lib, rc, *needles):
    assert rc == E_ARG, rc
    msg = lib.sgg_last_error()
    assert msg, "no message"
    for n in needles:
        assert n in msg, (n, msg)


# a non-NULL address that is never dereferenced: every check below fails before any launch (and
# before any device call: there is no device here)
_P = ctypes.c_void_p(64)


def _fwd_args(**kw):
    a = dict(U=_P, pos=_P, A=_P, W2=_P, b2=_P, off=_P, chunks=_P, nchunks=1, max_rows=4, gpw=4, B=8, bn=72, max_n=8,
             out=_P, am=_P)
    a.update(kw)
    return [a[k] for k in ("U", "pos", "A", "W2", "b2", "off", "chunks", "nchunks", "max_rows", "gpw", "B", "bn",
                           "max_n", "out", "am")] + [None]


def _bwd_args(**kw):
    a = dict(U=_P, pos=_P, A=_P, W2=_P, out=_P, am=_P, dout=_P, off=_P, S=2, B=8, bn=72, max_n=8, dU=_P, part=_P,
             nws=1 << 40)
    a.update(kw)
    return [a[k] for k in ("U", "pos", "A", "W2", "out", "am", "dout", "off", "S", "B", "bn", "max_n", "dU", "part",
                           "nws")] + [None]


@pytest.mark.parametrize("op", ["U", "pos", "A", "W2", "b2", "off", "chunks", "out", "am"])
def test_fwd_null_operand(lib, op):
    _refused(lib, lib.sgg_pool_fwd_bn(*_fwd_args(**{op: None})), b"sgg_pool_fwd_bn")


@pytest.mark.parametrize("op", ["U", "pos", "A", "W2", "out", "am", "dout", "off", "dU"])
def test_bwd_null_operand(lib, op):
    _refused(lib, lib.sgg_pool_bwd_bn(*_bwd_args(**{op: None})), b"sgg_pool_bwd_bn")


@pytest.mark.parametrize("bn", [0, -3, 1025])
def test_bad_bn(lib, bn):
    _refused(lib, lib.sgg_pool_fwd_bn(*_fwd_args(bn=bn)), b"sgg_pool_fwd_bn", b"1024")
    _refused(lib, lib.sgg_pool_bwd_bn(*_bwd_args(bn=bn)), b"sgg_pool_bwd_bn", b"1024")
    _refused(lib, lib.sgg_pool_bwd_bn_grid(2, bn, 8), b"sgg_pool_bwd_bn_grid", b"1024")
    _refused(lib, lib.sgg_pool_bwd_bn_ws_floats(2, 8, bn, 8), b"sgg_pool_bwd_bn_ws_floats", b"1024")
    nc, _, _, _ = _plan(lib, [3, 5], bn, 64)
    _refused(lib, nc, b"sgg_pool_plan_bn", b"1024")


@pytest.mark.parametrize("max_n", [0, 1025])
def test_bad_max_n(lib, max_n):
    _refused(lib, lib.sgg_pool_fwd_bn(*_fwd_args(max_n=max_n)), b"sgg_pool_fwd_bn", b"1024")
    _refused(lib, lib.sgg_pool_bwd_bn(*_bwd_args(max_n=max_n)), b"sgg_pool_bwd_bn", b"1024")
    _refused(lib, lib.sgg_pool_bwd_bn_grid(2, 72, max_n), b"sgg_pool_bwd_bn_grid", b"1024")
    _refused(lib, lib.sgg_pool_bwd_bn_ws_floats(2, 8, 72, max_n), b"sgg_pool_bwd_bn_ws_floats", b"1024")


def test_plan_bad_arguments(lib):
    nc, _, _, _ = _plan(lib, [3, 1025], 72, 64)
    _refused(lib, nc, b"sgg_pool_plan_bn", b"1024")
    off = np.array([0, 3], np.int32)
    tab = np.zeros((8, 4), np.int32)
    mr, gpw = ctypes.c_int(0), ctypes.c_int(0)
    o, t = off.ctypes.data_as(ctypes.c_void_p), tab.ctypes.data_as(ctypes.c_void_p)
    for args in ((None, 1, 72, 8, t, 8, ctypes.byref(mr), ctypes.byref(gpw)),
                 (o, 1, 72, 8, None, 8, ctypes.byref(mr), ctypes.byref(gpw)),
                 (o, 1, 72, 8, t, 8, None, ctypes.byref(gpw)),
                 (o, 1, 72, 8, t, 8, ctypes.byref(mr), None)):
        _refused(lib, lib.sgg_pool_plan_bn(*args), b"sgg_pool_plan_bn")


@pytest.mark.parametrize("bn", [1, 65, 72, 1024])
def test_bwd_workspace_too_small(lib, bn):
    need = lib.sgg_pool_bwd_bn_ws_floats(2, 8, bn, 8)
    assert need > 0
    _refused(lib, lib.sgg_pool_bwd_bn(*_bwd_args(bn=bn, nws=need - 1)), b"sgg_pool_bwd_bn", b"workspace")


@pytest.mark.parametrize("max_n", [1, 1024])
@pytest.mark.parametrize("S", [1, 64, 1000])
@pytest.mark.parametrize("bn", [1, 65, 1024])
def test_bwd_workspace_bound(lib, bn, S, max_n):
    """Never more than 16 rows of [dW2 | dA | db2], and it holds the slab rows it reports."""
    P = bn * 512 + 1024 + bn
    need = lib.sgg_pool_bwd_bn_ws_floats(S, S * max_n, bn, max_n)
    rows = lib.sgg_pool_bwd_bn_grid(S, bn, max_n)
    assert rows >= 1 and rows * P <= need <= 16 * P, (rows, need, P)


@pytest.mark.parametrize("bn", [1, 72, 1024])
def test_pool_plan_bn_covers_every_row_once(lib, bn):
    """As test_pool_plan_wide.py checks for the wide plan: whole i-rows of one
    scene, at most 64, every (scene, row) exactly once, also for an empty
    scene and a 1024-ped one; more chunks while the batch is below the target."""
    sizes = [65, 1, 128, 1024, 0, 300]
    counts = []
    for target in (1, 64, 512, 1024, 100000):
        nc, tab, mr, gpw = _plan(lib, sizes, bn, target)
        assert nc > 0 and gpw == 4
        seen = set()
        for s, i0, i1, g in tab[:nc]:
            n = sizes[s]
            assert 0 <= i0 < i1 <= n and i1 - i0 <= 64 and i1 - i0 <= mr and g == gpw
            for i in range(i0, i1):
                assert (s, i) not in seen
                seen.add((s, i))
        assert seen == {(s, i) for s, n in enumerate(sizes) for i in range(n)}
        assert 1 <= mr <= 64
        counts.append(nc)
    assert counts == sorted(counts) and counts[0] < counts[-1]
    assert counts[2] >= 512 or counts[2] == counts[-1]


def test_pool_plan_wide_still_rejects_other_widths(lib):
    nc, _, _, _ = _plan(lib, [65, 3], 72, 64, fn="sgg_pool_plan_wide")
    assert nc == E_ARG and b"sgg_pool_plan_wide" in lib.sgg_last_error()
    nc, _, _, _ = _plan(lib, [65, 3], 48, 64, fn="sgg_pool_plan_wide")
    assert nc > 0


@pytest.mark.parametrize("bn", [72, 1, 1024])
def test_padded_plans_refuse_other_widths_by_name(bn):
    """The fixed-capacity plans (PaddedScenes and its repeat view) take the
    keyword _Pool.forward passes for a width outside the five and refuse it
    with NotImplementedError naming bottleneck_dim -- host code, no device."""
    from sgan.scene import PaddedScenes
    ps = PaddedScenes(4, 32, "cpu", 20, reps=(2,))
    ps.load(np.array([0, 5, 12], np.int32), np.arange(12, dtype=np.int32))
    for sc in (ps, ps.repeat(2)):
        with pytest.raises(NotImplementedError, match="bottleneck_dim=%d" % bn):
            sc.pool_plan(bn, family_bn=True)
        with pytest.raises(NotImplementedError, match="bottleneck_dim=%d" % bn):
            sc.pool_plan(bn)
    assert ps.pool_plan(8)[3] >= 1    # a built width still plans
