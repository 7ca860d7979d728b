"""CPU-side checks of the tiled (wide) attention entry points: the work-buffer
size and the argument errors, all of which return before any launch, so no
GPU is touched."""
import ctypes
import os

import pytest

SGG_E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from sgan import _native
    if not os.path.exists(_native.lib_path()):
        pytest.skip("libsgg.so not built (run __graft_entry__.build())")
    return _native.load(require_gpu=False)


def test_work_floats_positive_and_monotonic(lib):
    base = dict(n=300, nseg=3, heads=2, F=17, max_seg=200)
    order = ("n", "nseg", "heads", "F", "max_seg")
    f = lambda d: int(lib.sgg_gat_wide_work_floats(*(d[k] for k in order)))
    assert f(base) > 0
    assert f(dict(base, n=0, nseg=0)) > 0
    for k, hi in (("n", 5000), ("nseg", 40), ("heads", 64), ("F", 128), ("max_seg", 1024)):
        prev = 0
        for v in sorted(v for v in {1, 2, 3, 63, 64, 65, 128, 129, base[k], base[k] + 1, hi} if v <= hi):
            cur = f(dict(base, **{k: v}))
            assert cur >= prev > -1, (k, v, cur, prev)
            prev = cur
    # the documented parts: 6 x r4(n heads) + units x 4F, units = nseg x ceil(max_seg / 64) x heads
    assert f(base) == 6 * 600 + 3 * 4 * 2 * 4 * 17


def _calls(lib):
    """-> (fwd, bwd): the two entry points on host dummies, with overrides."""
    buf = (ctypes.c_float * 4096)()
    off = (ctypes.c_int32 * 4)(0, 3, 5, 5)
    p = ctypes.cast(buf, ctypes.c_void_p)
    po = ctypes.cast(off, ctypes.c_void_p)

    def args(heads=1, F=16, max_seg=200, epi=1, Wh=p, ldy=None):
        return dict(Wh=Wh, heads=heads, F=F, max_seg=max_seg, epi=epi, ldy=heads * F if ldy is None else ldy)

    def fwd(**kw):
        a = args(**kw)
        return lib.sgg_gat_fwd_wide(a["Wh"], a["heads"], p, p, a["F"], None, None, po, 2, 5, a["F"], 0.2, 1, a["epi"],
                                    a["max_seg"], p, p, a["ldy"], p, None)

    def bwd(**kw):
        a = args(**kw)
        return lib.sgg_gat_bwd_wide(a["Wh"], a["heads"], p, p, a["F"], None, po, 2, 5, a["F"], 0.2, 1, a["epi"],
                                    a["max_seg"], p, p, p, a["ldy"], p, None, None, None, None, None, p, None)
    return fwd, bwd


@pytest.mark.parametrize("bad", [dict(max_seg=0), dict(max_seg=1025), dict(F=129), dict(heads=65),
                                 dict(epi=2, heads=2), dict(Wh=None)])
def test_argument_errors_before_any_launch(lib, bad):
    fwd, bwd = _calls(lib)
    assert fwd(**bad) == SGG_E_ARG, bad
    assert lib.sgg_last_error()
    assert bwd(**bad) == SGG_E_ARG, bad


def test_log_softmax_epilogue_needs_dense_y(lib):
    fwd, _ = _calls(lib)
    assert fwd(epi=2, heads=1, ldy=32) == SGG_E_ARG


def test_resident_entry_points_keep_their_bound(lib):
    buf = (ctypes.c_float * 4096)()
    off = (ctypes.c_int32 * 4)(0, 3, 5, 5)
    p, po = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(off, ctypes.c_void_p)
    assert lib.sgg_gat_fwd(p, 1, p, None, None, po, 2, 5, 16, 0.2, 1, 1, 129, p, p, 16, None) == SGG_E_ARG
    assert lib.sgg_gat_fwd_ex(p, 1, p, p, None, None, po, 2, 5, 16, 0.2, 1, 1, 129, p, p, 16, None) == SGG_E_ARG
