"""CPU-side checks of the pooling forwards' gpw argument (sgg_pool_fwd,
sgg_pool_fwd_bf16, sgg_pool_fwd2): the planners return 1, 2 or 4 pair groups
per wave and only those are built, so anything else is an argument error; an
empty batch returns 0 after the checks.  Both return before any launch -- the
operands are host dummies, which no kernel could take, and they stay as they
were -- so no GPU is touched."""
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


def _calls(lib):
    """-> ({name: call(gpw, nchunks)}, out buffer): the three entry points on host dummies."""
    from sgan._native import PoolBatch
    buf = (ctypes.c_float * 4096)()
    out = (ctypes.c_float * 64)(*([7.0] * 64))
    off = (ctypes.c_int32 * 3)(0, 3, 5)
    tab = (ctypes.c_int32 * 8)(0, 0, 3, 0, 1, 0, 2, 0)
    p, po, pt, pout = (ctypes.cast(x, ctypes.c_void_p) for x in (buf, off, tab, out))

    def one(name):
        return lambda gpw, nchunks: getattr(lib, name)(p, p, p, p, p, po, pt, nchunks, 3, gpw, 5, 8, 3, pout, pout,
                                                      None, None)

    def two(gpw, nchunks, gpw_b=None):
        a = PoolBatch(p, p, po, pt, nchunks, 3, gpw, 5, 3, pout, pout, None)
        b = PoolBatch(p, p, po, pt, nchunks, 3, gpw if gpw_b is None else gpw_b, 5, 3, pout, pout, None)
        return lib.sgg_pool_fwd2(ctypes.byref(a), ctypes.byref(b), p, p, p, 8, 0, None)
    return {"sgg_pool_fwd": one("sgg_pool_fwd"), "sgg_pool_fwd_bf16": one("sgg_pool_fwd_bf16"),
            "sgg_pool_fwd2": two}, out


@pytest.mark.parametrize("entry", ["sgg_pool_fwd", "sgg_pool_fwd_bf16", "sgg_pool_fwd2"])
def test_gpw_outside_1_2_4_is_an_argument_error(lib, entry):
    calls, out = _calls(lib)
    for gpw in (8, 0, 3, 16, -1):
        for nchunks in (2, 0):   # (refused before the empty-batch return, too)
            assert calls[entry](gpw, nchunks) == SGG_E_ARG, (gpw, nchunks)
            msg = lib.sgg_last_error().decode()
            assert entry in msg and "gpw %d" % gpw in msg, msg
    assert list(out) == [7.0] * 64


@pytest.mark.parametrize("entry", ["sgg_pool_fwd", "sgg_pool_fwd_bf16", "sgg_pool_fwd2"])
def test_empty_batch_returns_after_the_checks(lib, entry):
    calls, out = _calls(lib)
    for gpw in (1, 2, 4):
        assert calls[entry](gpw, 0) == 0, gpw   # (a launch would have failed: host pointers, or no device at all)
    assert list(out) == [7.0] * 64


def test_fwd2_second_batch_is_checked_too(lib):
    calls, _ = _calls(lib)
    assert calls["sgg_pool_fwd2"](4, 0, gpw_b=8) == SGG_E_ARG
    assert "gpw 8" in lib.sgg_last_error().decode()
