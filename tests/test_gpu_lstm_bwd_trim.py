"""The encoder's weight-gradient backward without input gradients
(sgg_lstm_bwd / sgg_lstm_bwd_shared with drel_in = NULL, lstm_mw.hip
lstm_mw_bwd_nodx_kernel): the slab and dh0 bit-identical to the call with a
buffer, the cases that keep needing a buffer refused before any launch, and
the autograd path taking the form when the input needs no gradient."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
E_ARG = -1   # SGG_E_ARG (include/sgg.h)


def _f(*s, sc=0.3):
    return (torch.randn(*s, device=DEV) * sc).contiguous()


def _ref64(A, Whh, bias, rel, h0, c0, dh_last):
    """float64 restatement of the encoder and its BPTT (autograd): drel_in,
    dh0, dW_hh, dbias, dA of L = sum(h_T * dh_last)."""
    d = lambda x: x.detach().double().cpu()
    A, Whh, bias, dh_last = d(A).requires_grad_(True), d(Whh).requires_grad_(True), d(bias).requires_grad_(True), d(dh_last)
    rel = d(rel).requires_grad_(True)
    T, B = rel.shape[:2]
    H = Whh.shape[1]
    h = d(h0).requires_grad_(True) if h0 is not None else torch.zeros(B, H, dtype=torch.float64)
    c = d(c0) if c0 is not None else torch.zeros(B, H, dtype=torch.float64)
    hs = h
    for t in range(T):
        g = rel[t] @ A.t() + hs @ Whh.t() + bias
        i, f, gg, o = g[:, :H].sigmoid(), g[:, H:2 * H].sigmoid(), g[:, 2 * H:3 * H].tanh(), g[:, 3 * H:].sigmoid()
        c = f * c + i * gg
        hs = o * c.tanh()
    (hs * dh_last).sum().backward()
    return rel.grad, (h.grad if h0 is not None else None), Whh.grad, bias.grad, A.grad


def _close(a, b, rtol, what):
    a, b = a.detach().double().cpu(), b.double()
    err = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-6)
    assert err <= rtol, "%s max rel err %.3e" % (what, err)


def _slab_sums(wpart, H):
    s = wpart.double().sum(0).cpu()
    G4 = 4 * H
    return s[:G4 * H].view(G4, H), s[G4 * H:G4 * H + G4], s[G4 * H + G4:].view(G4, 2)


@pytest.mark.parametrize("B", [16, 40, 96])
@pytest.mark.parametrize("T", [1, 2, 5, 12])
@pytest.mark.parametrize("H", [32, 48])
def test_null_drel_in_equals_buffer_form(H, T, B):
    """C ABI, sgg_lstm_bwd with weight gradients: drel_in = NULL gives the
    slab and dh0 of the call with a buffer, bitwise, with and without h0 /
    c0 (B = 40: the last block is partly padding).  The buffer call still
    matches the float64 BPTT (drel_in, dh0, and the slab's sums)."""
    from sgan import _native as N
    lib = N.load()
    torch.manual_seed(1000 * H + 10 * T + B)
    A, Whh, bias = _f(4 * H, 2), _f(4 * H, H, sc=0.2), _f(4 * H)
    rel, dh_last = _f(T, B, 2), _f(B, H)
    P = 4 * H * H + 4 * H + 8 * H
    rows = int(lib.sgg_lstm_wpart_rows(H, B))
    assert rows == (B + 15) // 16
    sf = lambda w: torch.empty(int(lib.sgg_lstm_state_floats(T, B, H, w)), device=DEV)
    for state in (False, True):
        h0, c0 = (_f(B, H), _f(B, H)) if state else (None, None)
        h_all, c_all, act = torch.empty(T + 1, B, H, device=DEV), sf(1), sf(0)
        N.check(lib.sgg_lstm_fwd(N.ptr(rel), N.ptr(A), N.ptr(Whh), N.ptr(bias), N.ptr(h0), N.ptr(c0), None, None, T, B,
                                 H, 0, N.ptr(h_all), N.ptr(c_all), N.ptr(act), None, N.stream_ptr()), "fwd")
        res = []
        for null in (False, True):
            wpart = torch.full((rows, P), float("nan"), device=DEV)
            dh0 = torch.full((B, H), float("nan"), device=DEV) if state else None
            drel = None if null else torch.full((T, B, 2), float("nan"), device=DEV)
            N.check(lib.sgg_lstm_bwd(N.ptr(A), N.ptr(Whh), None, N.ptr(h_all), N.ptr(c_all), N.ptr(act), N.ptr(rel),
                                     None, N.ptr(dh_last), None, T, B, H, 0, None, N.ptr(dh0), N.ptr(drel), None,
                                     N.ptr(wpart), N.stream_ptr()), "bwd")
            torch.cuda.synchronize()
            res.append((wpart, dh0, drel))
        (w_buf, dh0_buf, drel_buf), (w_null, dh0_null, _) = res
        assert torch.equal(w_null, w_buf), "slab (state=%s)" % state
        if state:
            assert torch.equal(dh0_null, dh0_buf), "dh0"
        r_drel, r_dh0, r_dW, r_db, r_dA = _ref64(A, Whh, bias, rel, h0, c0, dh_last)
        _close(drel_buf, r_drel, 1e-4, "drel_in")
        if state:
            _close(dh0_buf, r_dh0, 1e-4, "dh0")
        dW, db, dA = _slab_sums(w_buf, H)
        _close(dW, r_dW, 1e-4, "dW_hh")
        _close(db, r_db, 1e-4, "dbias")
        _close(dA, r_dA, 1e-4, "dA")


def test_null_drel_in_shared_prefix_form():
    """sgg_lstm_bwd_shared (the shapes of test_lstm_segments_equal_full_sequence:
    T 11, T0 5, Bs 32, 3 copies, H 48): drel_in = NULL gives the slab of the
    call with a buffer, and of sgg_lstm_bwd with NULL on the full layout."""
    from sgan import _native as N
    lib = N.load()
    torch.manual_seed(2)
    T, T0, Bs, C, H = 11, 5, 32, 3, 48
    B = Bs * C
    A, Whh, bias = _f(4 * H, 2), _f(4 * H, H, sc=0.2), _f(4 * H)
    head = _f(T0, Bs, 2)
    rel = torch.cat([head.repeat(1, C, 1), _f(T - T0, B, 2)], 0).contiguous()
    sf = lambda w: torch.empty(int(lib.sgg_lstm_state_floats(T, B, H, w)), device=DEV)
    P = 4 * H * H + 4 * H + 8 * H
    rows = int(lib.sgg_lstm_wpart_rows(H, B))
    dh_last = _f(B, H)

    def run(shared, null):
        h_all, c_all, act = torch.empty(T + 1, B, H, device=DEV), sf(1), sf(0)
        if shared:
            pre = N.LstmSeg(N.ptr(head), N.ptr(A), N.ptr(Whh), N.ptr(bias), None, None, T0, Bs, B, 0, T, Bs,
                            N.ptr(h_all), N.ptr(c_all), N.ptr(act), None, 0, None, 0, None)
            N.check(lib.sgg_lstm_fwd_seg(N.ctypes.byref(pre), H, N.stream_ptr()), "prefix")
            suf = N.LstmSeg(N.ptr(rel), N.ptr(A), N.ptr(Whh), N.ptr(bias), None, None, T - T0, B, B, T0, T, Bs,
                            N.ptr(h_all), N.ptr(c_all), N.ptr(act), None, 0, None, 0, None)
            N.check(lib.sgg_lstm_fwd_seg(N.ctypes.byref(suf), H, N.stream_ptr()), "suffix")
        else:
            N.check(lib.sgg_lstm_fwd(N.ptr(rel), N.ptr(A), N.ptr(Whh), N.ptr(bias), None, None, None, None, T, B, H, 0,
                                     N.ptr(h_all), N.ptr(c_all), N.ptr(act), None, N.stream_ptr()), "fwd")
        drel = None if null else torch.empty(T, B, 2, device=DEV)
        wpart = torch.full((rows, P), float("nan"), device=DEV)
        if shared:
            N.check(lib.sgg_lstm_bwd_shared(N.ptr(A), N.ptr(Whh), N.ptr(h_all), N.ptr(c_all), N.ptr(act), N.ptr(rel),
                                            N.ptr(dh_last), T, B, H, T0, Bs, N.ptr(drel), N.ptr(wpart),
                                            N.stream_ptr()), "bwd_shared")
        else:
            N.check(lib.sgg_lstm_bwd(N.ptr(A), N.ptr(Whh), None, N.ptr(h_all), N.ptr(c_all), N.ptr(act), N.ptr(rel),
                                     None, N.ptr(dh_last), None, T, B, H, 0, None, None, N.ptr(drel), None,
                                     N.ptr(wpart), N.stream_ptr()), "bwd")
        torch.cuda.synchronize()
        return wpart

    ref = run(True, False)
    assert not torch.isnan(ref).any()
    assert torch.equal(run(True, True), ref), "shared: NULL vs buffer"
    assert torch.equal(run(False, True), ref), "full layout with NULL vs shared"


def test_null_drel_in_refused_elsewhere():
    """drel_in = NULL is an argument error, before any launch, for the
    decoder, without wpart, and for an H the form is not built for (64)."""
    from sgan import _native as N
    lib = N.load()
    T, B = 3, 16

    def call(H, decoder, with_wpart, shared=False):
        # the refused call reads none of these buffers
        z = lambda *s: torch.zeros(*s, device=DEV)
        A, Whh, Wp = z(4 * H, 2), z(4 * H, H), z(2, H)
        h_all = z(T + 1, B, H)
        c_all = z(int(lib.sgg_lstm_state_floats(T, B, H, 1)))
        act = z(int(lib.sgg_lstm_state_floats(T, B, H, 0)))
        rel, rel_out, dout, drel_tot, dhl = z(T, B, 2), z(T, B, 2), z(T, B, 2), z(T, B, 2), z(B, H)
        sentinel = 7.0
        wpart = torch.full((1, 4 * H * H + 12 * H + 2 * H + 2), sentinel, device=DEV) if with_wpart else None
        if shared:
            rc = lib.sgg_lstm_bwd_shared(N.ptr(A), N.ptr(Whh), N.ptr(h_all), N.ptr(c_all), N.ptr(act), N.ptr(rel),
                                         N.ptr(dhl), T, B, H, 1, 16, None, N.ptr(wpart), N.stream_ptr())
        else:
            rc = lib.sgg_lstm_bwd(N.ptr(A), N.ptr(Whh), N.ptr(Wp), N.ptr(h_all), N.ptr(c_all), N.ptr(act), N.ptr(rel),
                                  N.ptr(rel_out), None if decoder else N.ptr(dhl), N.ptr(dout) if decoder else None,
                                  T, B, H, int(decoder), None, None, None, N.ptr(drel_tot) if decoder else None,
                                  N.ptr(wpart), N.stream_ptr())
        torch.cuda.synchronize()
        if wpart is not None and rc != 0:
            assert bool((wpart == sentinel).all()), "a refused call launched"
        return rc

    assert call(32, True, True) == E_ARG, "decoder"
    assert call(48, False, False) == E_ARG, "no wpart"
    assert call(64, False, True) == E_ARG, "H = 64"
    assert call(48, False, False, shared=True) == E_ARG, "shared, no wpart"
    assert call(64, False, True, shared=True) == E_ARG, "shared, H = 64"
    assert call(48, False, True) == 0 and call(32, False, True, shared=True) == 0, "the accepted form"


@pytest.mark.parametrize("H,T,B", [(48, 20, 40), (32, 8, 96)])
def test_autograd_skips_unwanted_input_gradient(H, T, B):
    """An encoder sequence whose input does not require a gradient: the
    backward launches the form without drel_in (kernels.timer's record),
    returns no input gradient, and every weight gradient equals the
    requires_grad=True call's, bitwise."""
    from sgan import kernels as K
    torch.manual_seed(H + B)
    lstm = torch.nn.LSTM(16, H).to(DEV)
    emb = torch.nn.Linear(2, 16).to(DEV)
    params = list(lstm.parameters()) + list(emb.parameters())
    rel0 = torch.randn(T, B, 2, device=DEV) * 0.3
    dh = torch.randn(B, H, device=DEV)
    grads, names = [], []
    for need in (True, False):
        for p in params:
            p.grad = None
        rel = rel0.clone().requires_grad_(need)
        K.timer.start()
        try:
            h, _ = K.lstm_sequence(rel, lstm, emb)
            (h * dh).sum().backward()
        finally:
            recs = K.timer.stop()
        names.append([r[0] for r in recs if "lstm_mw_bwd" in r[0]])
        assert (rel.grad is not None) == need
        grads.append([p.grad.clone() for p in params])
    assert names[0] == ["sgg::lstm_mw_bwd_kernel<%d, false, true>" % H], names[0]
    assert names[1] == ["sgg::lstm_mw_bwd_nodx_kernel<%d>" % H], names[1]
    for a, b in zip(*grads):
        assert torch.equal(a, b)

