"""sgg_pool_plan_wide (host function of the C ABI, no GPU): the chunk table of
the tiled pooling forward for scenes of up to SGG_POOL_WIDE_MAX_PEDS peds."""
import ctypes
import os

import numpy as np
import pytest


def _plan(lib, sizes, bn, target):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    S = len(sizes)
    cap = int(off[-1]) + S + 1
    tab = np.zeros((cap, 4), np.int32)
    mr, gpw = ctypes.c_int(0), ctypes.c_int(0)
    nc = lib.sgg_pool_plan_wide(off.ctypes.data_as(ctypes.c_void_p), S, bn, target,
                                tab.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(mr), ctypes.byref(gpw))
    return nc, tab, mr.value, gpw.value


def _lib():
    from sgan import _native
    if not os.path.exists(_native.lib_path()):
        pytest.skip("libsgg.so not built")
    return _native.load(require_gpu=False)


@pytest.mark.parametrize("bn", [8, 48])
def test_pool_plan_wide_covers_every_row_once(bn):
    """Chunks are whole i-rows of one scene, at most 64 (the keys held in
    LDS), and cover every (scene, row) exactly once -- also when a row's n
    pairs exceed one pass of the workgroup (n up to 1024) and for an empty
    scene; more chunks are cut while the batch has fewer than the target."""
    lib = _lib()
    sizes = [65, 1, 128, 1024, 0, 300]
    counts = []
    for target in (1, 64, 512, 1024, 100000):
        nc, tab, mr, gpw = _plan(lib, sizes, bn, target)
        assert nc > 0 and gpw == (2 if bn <= 16 else 4)
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
    # the target is met whenever chunks of >= gpw rows allow it
    assert counts[2] >= 512 or counts[2] == counts[-1]


def test_pool_plan_wide_rejects_a_scene_above_the_bound():
    lib = _lib()
    nc, _, _, _ = _plan(lib, [3, 1025], 8, 64)
    assert nc < 0
    assert b"1024" in lib.sgg_last_error()
