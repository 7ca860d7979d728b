"""Size functions and kernel names of the LSTM entry points across the two
kernel families (CPU test: no GPU function is called).

The four-wave kernels (lstm_mw.hip) are built for H in {16, 32, 48, 64}; every
other 1 <= H <= 128 goes to the generic family (lstm_gen.hip).  The built
sizes keep the values they had before the generic family existed; H = 0 and
H > 128 are errors.
"""
import pytest

from conftest import ROOT  # noqa: F401  (sys.path)

NEW = [1, 8, 40, 72, 99, 128]
BUILT = [16, 32, 48, 64]
SHAPES = [(1, 1), (8, 17), (12, 1280), (20, 33)]


@pytest.fixture(scope="module")
def lib():
    from sgan import _native
    return _native.load(require_gpu=False)


def pad16(b):
    return (b + 15) // 16 * 16


@pytest.mark.parametrize("H", NEW)
def test_new_sizes_have_positive_sizes(lib, H):
    for T, B in SHAPES:
        act, cells = lib.sgg_lstm_state_floats(T, B, H, 0), lib.sgg_lstm_state_floats(T, B, H, 1)
        hp = (H + 15) // 16 * 16
        # tile-native: peds padded to 16, units to 16 ceil(H / 16)
        assert act == T * pad16(B) * 4 * hp and cells == (T + 1) * pad16(B) * hp
        assert act >= T * B * 4 * H and cells >= (T + 1) * B * H
        assert lib.sgg_lstm_wpart_rows(H, B) == (B + 15) // 16 > 0
        assert lib.sgg_lstm_dg_floats(T, B, H) == T * B * 4 * H > 0


@pytest.mark.parametrize("H", BUILT)
def test_built_sizes_are_unchanged(lib, H):
    for T, B in SHAPES:
        assert lib.sgg_lstm_state_floats(T, B, H, 0) == T * pad16(B) * 4 * H
        assert lib.sgg_lstm_state_floats(T, B, H, 1) == (T + 1) * pad16(B) * H
        assert lib.sgg_lstm_wpart_rows(H, B) == (B + 15) // 16
        assert lib.sgg_lstm_dg_floats(T, B, H) == 0   # the weight gradients are formed in the kernel


@pytest.mark.parametrize("H", [0, -1, 129, 256])
def test_out_of_range_sizes_are_errors(lib, H):
    assert lib.sgg_lstm_state_floats(8, 17, H, 0) < 0
    assert lib.sgg_lstm_state_floats(8, 17, H, 1) < 0
    assert lib.sgg_lstm_wpart_rows(H, 17) < 0
    assert lib.sgg_lstm_dg_floats(8, 17, H) < 0
    for bwd in range(5):
        assert lib.sgg_lstm_kernel_name(H, 17, 0, 1, bwd) == b""


def test_kernel_names(lib):
    name = lambda *a: lib.sgg_lstm_kernel_name(*a).decode()
    for H in NEW:
        ht = (H + 15) // 16
        assert name(H, 17, 0, 1, 0) == "sgg::lstm_gen_fwd_kernel<%d, false, true>" % ht
        assert name(H, 17, 0, 0, 0) == "sgg::lstm_gen_fwd_kernel<%d, false, false>" % ht
        assert name(H, 5000, 1, 0, 0) == "sgg::lstm_gen_fwd_kernel<%d, true, false>" % ht
        assert name(H, 17, 1, 1, 1) == "sgg::lstm_gen_bwd_kernel<%d, true>" % ht
        assert name(H, 17, 0, 0, 1) == "sgg::lstm_gen_bwd_kernel<%d, false>" % ht
        # no drel_in = NULL form, no pooled-gradient prologue
        assert name(H, 17, 0, 1, 2) == name(H, 17, 0, 1, 3) == name(H, 17, 0, 1, 4) == ""
    for H in BUILT:
        assert name(H, 17, 0, 1, 0) == "sgg::lstm_mw_fwd_kernel<%d, false, true>" % H
        assert name(H, 17, 1, 1, 1) == "sgg::lstm_mw_bwd_kernel<%d, true, true>" % H
        assert name(H, 17, 0, 1, 2) == ("sgg::lstm_mw_bwd_nodx_kernel<%d>" % H if H != 64 else "")
    assert name(32, 5000, 1, 0, 0).startswith("sgg::lstm_fwd_mfma_kernel<32, ")


def test_fused_forms_decline_the_new_sizes(lib):
    for H in NEW:
        assert lib.sgg_lstm_u_ok(8, 32, H, 0, 1, 512) == 0
        assert lib.sgg_lstm_bwd_pooldh_ok(H) == 0
        assert lib.sgg_lstm_bwd_pooldh_pays(32, H) == 0
        assert lib.sgg_lstm_bwd_pooldh_rides(32, H, 512) == 0
