"""CPU-side checks of the per-step pooling decoder's entry points
(include/sgg.h: sgg_dec_step_*): the host predicates only, no launch."""
import os

import pytest


def _lib():
    from sgan import _native
    if not os.path.exists(_native.lib_path()):
        pytest.skip("libsgg.so not built (run __graft_entry__.build())")
    return _native.load(require_gpu=False)


def test_dec_step_ok_truth_table():
    lib = _lib()
    # train.py's defaults (bn, mlp_dim) = (8, 64), and (16, 32): the whole step, U included
    for H in (16, 32, 48, 64):
        for bn, mlp in ((8, 64), (16, 32)):
            assert lib.sgg_dec_step_ok(H, bn, mlp, 512) == 3, (H, bn, mlp)
            assert lib.sgg_dec_step_ok(H, bn, mlp, 0) == 3
    # no instantiation: H off the 16-ped MFMA tiling, H above the LDS tile, another U width
    for H in (0, 8, 24, 40, 80, 128):
        assert lib.sgg_dec_step_ok(H, 8, 64, 512) == 0, H
    assert lib.sgg_dec_step_ok(32, 8, 64, 256) == 0
    # only the mlp out of bounds (mlp_dim <= 256, H + bn <= 256): the step with its mlp part off
    assert lib.sgg_dec_step_ok(32, 8, 256, 512) == 3
    assert lib.sgg_dec_step_ok(32, 8, 257, 512) == 1
    assert lib.sgg_dec_step_ok(32, 8, 1024, 512) == 1
    assert lib.sgg_dec_step_ok(64, 192, 64, 512) == 3
    assert lib.sgg_dec_step_ok(64, 193, 64, 512) == 1
    assert lib.sgg_dec_step_ok(32, 0, 64, 512) == 1


def test_dec_step_saved_floats():
    lib = _lib()
    for H, mlp in ((16, 64), (32, 64), (48, 32), (64, 7)):
        prev = -1
        for B in (0, 1, 2, 15, 16, 17, 33, 1280, 1281):
            n = lib.sgg_dec_step_saved_floats(B, H, mlp)
            assert n % 4 == 0 and n >= B * (5 * H + mlp) and n - B * (5 * H + mlp) < 4
            assert n >= prev and (n > prev or B == 0)
            prev = n


def test_dec_step_structs_mirror_the_header():
    """The ctypes structures list the fields of SggDecStep / SggDecStepBwd in the header's order."""
    import re
    from conftest import ROOT
    from sgan import _native
    txt = open(os.path.join(ROOT, "include", "sgg.h")).read()
    for name, cls in (("SggDecStep", _native.DecStep), ("SggDecStepBwd", _native.DecStepBwd)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, re.S).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names = decl.replace("const float", "").replace("float", "").replace("int", "")
                fields += [n.strip(" *") for n in names.split(",")]
        assert fields == [f[0] for f in cls._fields_], name
