"""The four-wave LSTM kernels (lstm_mw.hip, H = 16 / 32 / 48 / 64) and the
batch-MFMA rollout (lstm_mfma.hip) -- the kernels of the benched iteration,
and the root of trust of every fused LSTM form (each is tested bit-identical
to the plain sgg_lstm_fwd / sgg_lstm_bwd) -- against float64 at every built
size and at the edges of B (a block is 16 peds) and T (1, 2, the encoder's
staging limit 64, a decoder past it).

The gate is tests/_lstm_ref.py's: for every output, input
gradient and parameter gradient
    |HIP - f64| <= 4 |CPU32 - f64| + 1e-6 max|f64|     (max over the tensor)
with the oracle's modules in float64 as the yardstick and the same modules in
fp32 on the CPU as the unit of error.  Measured ratios: DESIGN.md 4h ("the
same gate at the four-wave sizes").
"""
import copy

import numpy as np
import pytest
import torch

from conftest import GOLDEN  # noqa: F401
from _lstm_ref import _run, gate, hip_module, reference, reference_state, run_state

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
SIZES = (16, 32, 48, 64)
SGG_E_ARG = -1   # include/sgg.h


def _tf(b):
    return "true" if b else "false"


def _tag(H, Tn, decoder, B):
    return "H=%d T=%d %s B=%d" % (H, Tn, "dec" if decoder else "enc", B)


def _kname(H, B, decoder, save, bwd):
    from sgan import _native as N
    return N.load().sgg_lstm_kernel_name(H, B, int(decoder), int(save), bwd).decode()


@pytest.fixture
def lstm_calls(monkeypatch):
    """The LSTM entry points the run goes through, in order (N.check's names)."""
    from sgan import _native as N
    calls = []
    real = N.check

    def check(rc, name):
        if name.startswith("sgg_lstm"):
            calls.append(name)
        return real(rc, name)
    monkeypatch.setattr(N, "check", check)
    monkeypatch.delenv("SGG_LSTM_NO_MFMA", raising=False)
    monkeypatch.delenv("SGG_LSTM_X3", raising=False)
    return calls


# ---------------------------------------------------------------------------
# a. plain forward + backward through the modules, float64 yardstick
# ---------------------------------------------------------------------------
ENC_TB = [(1, 1), (2, 17), (8, 16), (20, 33), (64, 15)]
DEC_TB = [(1, 17), (3, 1), (12, 16), (12, 33), (65, 15)]
CASES = [(H, Tn, dec, B) for H in SIZES for dec, tbs in ((False, ENC_TB), (True, DEC_TB)) for Tn, B in tbs]


@pytest.mark.parametrize("H,Tn,decoder,B", CASES)
def test_kernels_vs_oracle_f64(H, Tn, decoder, B, lstm_calls):
    ref, inp, r64, r32 = reference(H, Tn, decoder, B)
    got = _run(hip_module(ref, H, Tn, decoder), inp, decoder, DEV, torch.float32)
    # the plain entry points on the four-wave kernels: a re-route to another family or form fails here
    assert lstm_calls == ["sgg_lstm_fwd", "sgg_lstm_bwd"], lstm_calls
    assert _kname(H, B, decoder, True, 0) == "sgg::lstm_mw_fwd_kernel<%d, %s, true>" % (H, _tf(decoder))
    assert _kname(H, B, decoder, True, 1) == "sgg::lstm_mw_bwd_kernel<%d, %s, true>" % (H, _tf(decoder))
    assert set(got) == set(r64) and ("dh0" in got) == decoder and len(got) == (11 if decoder else 8), sorted(got)
    gate(_tag(H, Tn, decoder, B), got, r64, r32)


# ---------------------------------------------------------------------------
# b. an encoder from a nonzero (h0, c0)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("H", SIZES)
def test_nonzero_initial_state_vs_f64(H, lstm_calls):
    from sgan import kernels as K
    Tn, B = 8, 17
    (lstm, emb), inp, r64, r32 = reference_state(H, Tn, B)
    held = {}

    def seq(rel, lstm, emb, h0, c0):
        held["c0"] = c0
        return K.lstm_sequence(rel, lstm, emb, h0, c0)[0]
    got = run_state(copy.deepcopy(lstm).to(DEV), copy.deepcopy(emb).to(DEV), inp, DEV, torch.float32, seq)
    assert lstm_calls == ["sgg_lstm_fwd", "sgg_lstm_bwd"], lstm_calls
    assert _kname(H, B, False, True, 0) == "sgg::lstm_mw_fwd_kernel<%d, false, true>" % H
    assert set(got) == set(r64) and "dh0" in got and len(got) == 9
    gate("state " + _tag(H, Tn, False, B), got, r64, r32)
    # the ABI produces no c0 gradient: none is reported, and asking for one is refused by name
    assert held["c0"].grad is None
    d = lambda k: inp[k].to(DEV)
    with pytest.raises(NotImplementedError, match="initial cell state"):
        K.lstm_sequence(d("rel"), copy.deepcopy(lstm).to(DEV), copy.deepcopy(emb).to(DEV), d("h0"),
                        d("c0").requires_grad_(True))


# ---------------------------------------------------------------------------
# c. forwards without saved states
# ---------------------------------------------------------------------------
_HT = {}


def _final_ref(key, ref, inp):
    """(float64, fp32 CPU) final hidden state of a decoder case (the module
    returns it beside the rollout; _lstm_ref._run keeps the rollout only)."""
    if key not in _HT:
        res = []
        for dtype in (torch.float64, torch.float32):
            c = lambda t: t.detach().to(dtype)
            with torch.no_grad():
                h0 = c(inp["h0"])
                _, h = copy.deepcopy(ref).to(dtype)(c(inp["last_pos"]), c(inp["last_rel"]), (h0, torch.zeros_like(h0)),
                                                    None)
            res.append(h.double().numpy())
        _HT[key] = res
    return _HT[key]


def _no_grad_out(ref, inp, H, Tn, decoder, r64, r32):
    """-> (got, r64, r32) of the forward under no_grad: the output, and for a
    decoder the final hidden state it returns."""
    mod = hip_module(ref, H, Tn, decoder)
    want64, want32 = {"out": r64["out"]}, {"out": r32["out"]}
    with torch.no_grad():
        if decoder:
            h0 = inp["h0"].to(DEV)
            y, h = mod(inp["last_pos"].to(DEV), inp["last_rel"].to(DEV), (h0, torch.zeros_like(h0)), None)
            want64["h_T"], want32["h_T"] = _final_ref((H, Tn, h0.shape[1]), ref, inp)
            assert tuple(h.shape) == want64["h_T"].shape
            return {"out": y.cpu().double().numpy(), "h_T": h.cpu().double().numpy()}, want64, want32
        y = mod(inp["rel"].to(DEV)).reshape(inp["dy"].shape)
    return {"out": y.cpu().double().numpy()}, want64, want32


@pytest.mark.parametrize("H,Tn,decoder,B", [(H, Tn, dec, 17) for H in SIZES for Tn, dec in ((8, False), (12, True))])
def test_no_grad_forward_vs_oracle_f64(H, Tn, decoder, B, lstm_calls):
    ref, inp, r64, r32 = reference(H, Tn, decoder, B)
    out, want64, want32 = _no_grad_out(ref, inp, H, Tn, decoder, r64, r32)
    assert lstm_calls == ["sgg_lstm_fwd"], lstm_calls
    assert _kname(H, B, decoder, False, 0) == "sgg::lstm_mw_fwd_kernel<%d, %s, false>" % (H, _tf(decoder))
    gate("no-grad " + _tag(H, Tn, decoder, B), out, want64, want32)


@pytest.mark.parametrize("x3", [None, "0"], ids=["x3-unset", "x3-0"])
@pytest.mark.parametrize("Tn,decoder", [(1, True), (12, True), (8, False)])
@pytest.mark.parametrize("B", [4096, 4097])
def test_no_grad_rollout_mfma_vs_oracle_f64(B, Tn, decoder, x3, lstm_calls, monkeypatch):
    """The batch-MFMA rollout at its smallest batch (kLstmMfmaMinPeds = 4096:
    64 workgroups of 64 peds) and one ped past it (a last workgroup of one
    ped), in the split-bf16 form (SGG_LSTM_X3 unset) and the fp32 MFMA form
    ("0"; the library reads the variable per call)."""
    H = 32
    if x3 is not None:
        monkeypatch.setenv("SGG_LSTM_X3", x3)
    ref, inp, r64, r32 = reference(H, Tn, decoder, B)
    out, want64, want32 = _no_grad_out(ref, inp, H, Tn, decoder, r64, r32)
    assert lstm_calls == ["sgg_lstm_fwd"], lstm_calls
    assert _kname(H, B, decoder, False, 0) == "sgg::lstm_fwd_mfma_kernel<32, %s, %s>" % (_tf(x3 is None), _tf(decoder))
    assert _kname(H, 4095, decoder, False, 0).startswith("sgg::lstm_mw_fwd_kernel")   # (one ped fewer: four-wave)
    gate("rollout x3=%s %s" % (x3, _tag(H, Tn, decoder, B)), out, want64, want32)


# ---------------------------------------------------------------------------
# d. the projection epilogue, every arm
# ---------------------------------------------------------------------------
def _wu(NU, H, layout):
    """Wu (NU x H, unit column stride) as a view of the pooling net's first
    layer: "e16" = W1[:, 16:] (16-byte aligned base and pitch), "e10" =
    W1[:, 10:] of an (NU, 10 + H) matrix (neither aligned), "p17" = the H
    columns from 16 of an (NU, 16 + H + 1) one (aligned base, odd pitch)."""
    if layout == "e16":
        return (torch.randn(NU, 16 + H, device=DEV) * 0.2)[:, 16:]
    if layout == "e10":
        return (torch.randn(NU, 10 + H, device=DEV) * 0.2)[:, 10:]
    return (torch.randn(NU, 16 + H + 1, device=DEV) * 0.2)[:, 16:16 + H]


PROJ = [
    # the prefetch path (H <= 48, NU <= 512, aligned) with fewer steps than its eight tiles per wave
    (16, 1, 1, 512, False, "e16"), (16, 3, 17, 512, True, "e16"), (16, 7, 17, 512, False, "e16"),
    (32, 1, 17, 512, True, "e16"), (32, 3, 1, 512, False, "e16"), (32, 7, 17, 512, True, "e16"),
    (48, 1, 17, 512, False, "e16"), (48, 3, 17, 512, True, "e16"), (48, 7, 1, 512, True, "e16"),
    # fewer tiles than waves (prefetch path)
    (32, 8, 17, 16, True, "e16"), (48, 8, 17, 48, False, "e16"), (16, 2, 1, 48, True, "e16"),
    # the general path: H = 64 (also with fewer tiles than waves)
    (64, 8, 17, 512, True, "e16"), (64, 1, 1, 512, False, "e16"), (64, 8, 17, 16, False, "e16"),
    (64, 3, 17, 48, True, "e16"),
    # the general path: NU > 512 (33 tiles: a last pair with one tile; 64 tiles)
    (32, 8, 17, 528, True, "e16"), (48, 8, 1, 528, False, "e16"), (16, 8, 17, 1024, False, "e16"),
    (48, 3, 17, 1024, True, "e16"),
    # the general path's scalar-load arm: a Wu whose base or row pitch is not 16-byte aligned
    (32, 8, 17, 512, True, "e10"), (48, 8, 17, 512, False, "e10"), (16, 3, 1, 512, True, "e10"),
    (64, 8, 17, 528, False, "e10"),
    (32, 8, 1, 512, False, "p17"), (48, 7, 17, 512, True, "p17"), (64, 8, 17, 1024, True, "p17"),
    (16, 8, 17, 48, False, "p17"),
]


@pytest.mark.parametrize("H,Tn,B,NU,save,layout", PROJ)
def test_projection_epilogue(H, Tn, B, NU, save, layout, lstm_calls):
    """sgg_lstm_fwd_u: h_T is bitwise the plain run's, U = h_T Wu^T + cu within
    2e-6 of its scale from float64 (test_encoder_projection_epilogue's bound)."""
    from sgan import kernels as K
    torch.manual_seed(1000 * H + 10 * Tn + B + NU)
    lstm, emb = torch.nn.LSTM(16, H).to(DEV), torch.nn.Linear(2, 16).to(DEV)
    rel = torch.randn(Tn, B, 2, device=DEV) * 0.3
    Wu, cu = _wu(NU, H, layout), torch.randn(NU, device=DEV)
    aligned = ((Wu.data_ptr() | (Wu.stride(0) * 4)) & 15) == 0
    assert aligned == (layout == "e16") and Wu.stride(1) == 1 and tuple(Wu.shape) == (NU, H)
    with torch.set_grad_enabled(save):
        if save:
            rel.requires_grad_(True)
        h_ref, _ = K.lstm_sequence(rel, lstm, emb)
        h, U = K.lstm_sequence(rel, lstm, emb, proj_u=(Wu, cu))
    assert U is not None and tuple(U.shape) == (B, NU), "the four-wave family takes the projection at these sizes"
    assert lstm_calls == ["sgg_lstm_fwd", "sgg_lstm_fwd_u"], lstm_calls   # (the slice in place: no aligned copy)
    assert _kname(H, B, False, save, 0) == "sgg::lstm_mw_fwd_kernel<%d, false, %s>" % (H, _tf(save))
    assert torch.equal(h, h_ref)
    ref = (h_ref.detach().double() @ Wu.double().t() + cu.double()).cpu().numpy()
    err = float(np.abs(U.detach().cpu().double().numpy() - ref).max())
    scale = float(np.abs(ref).max())
    print("proj_u H=%d T=%d B=%d NU=%d save=%d %s  err %.3e  scale %.3e  err/scale %.3e" % (H, Tn, B, NU, save, layout,
                                                                                          err, scale, err / scale))
    assert err <= 2e-6 * scale, (err, scale)


# ---------------------------------------------------------------------------
# e. buffers are respected: NaN guard bands around every input and output
# ---------------------------------------------------------------------------
GUARD = 64   # floats: keeps the 16-byte alignment of the saved states


def _guarded(n, fill=None):
    buf = torch.full((n + 2 * GUARD,), NAN, device=DEV)
    view = buf[GUARD:GUARD + n]
    if fill is not None:
        view.copy_(fill.reshape(-1))
    return buf, view


def _bands_ok(buf):
    return bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all())


@pytest.mark.parametrize("decoder,Tn", [(False, 8), (True, 3)])
@pytest.mark.parametrize("H", [16, 48, 64])
def test_guard_bands(H, decoder, Tn):
    from sgan import _native as N
    lib = N.load()
    B, NU = 17, 512
    torch.manual_seed(5 + H)
    r = lambda *s: torch.randn(*s, device=DEV)
    A, Whh, bias = r(4 * H, 2) * .3, r(4 * H, H) * .1, r(4 * H) * .1
    Wp, bp = r(2, H) * .2, r(2) * .1
    Wu, cu = (r(NU, 16 + H) * .2)[:, 16:], r(NU)
    bufs = {}

    def g(name, n, fill=None):
        bufs[name], view = _guarded(n, fill)
        return view
    # the inputs between NaN bands too: a stray read that reaches an output shows up as a NaN
    ins = {}
    ins["rel"], rel = _guarded(B * 2 if decoder else Tn * B * 2, r(B * 2 if decoder else Tn * B * 2) * .3)
    ins["h0"], h0 = _guarded(B * H, r(B, H) * .5)
    ins["c0"], c0 = _guarded(B * H, r(B, H) * .5)
    n_c, n_act = lib.sgg_lstm_state_floats(Tn, B, H, 1), lib.sgg_lstm_state_floats(Tn, B, H, 0)
    assert n_c == (Tn + 1) * 32 * H and n_act == Tn * 32 * 4 * H   # (17 peds: two 16-ped blocks)

    def forward(save, proj):
        bufs.clear()
        h_all = g("h_all", (Tn + 1) * B * H)
        c_all = g("c_all", n_c)
        act = g("act", n_act) if save else None
        rel_out = g("rel_out", Tn * B * 2) if decoder else None
        U = g("U", B * NU) if proj else None
        if proj:
            N.check(lib.sgg_lstm_fwd_u(N.ptr(rel), N.ptr(A), N.ptr(Whh), N.ptr(bias), N.ptr(h0), N.ptr(c0), Tn, B, H,
                                       N.ptr(h_all), N.ptr(c_all), N.ptr(act), N.ptr(Wu), Wu.stride(0), N.ptr(cu), NU,
                                       N.ptr(U), N.stream_ptr()), "sgg_lstm_fwd_u")
        else:
            N.check(lib.sgg_lstm_fwd(N.ptr(rel), N.ptr(A), N.ptr(Whh), N.ptr(bias), N.ptr(h0), N.ptr(c0),
                                     N.ptr(Wp) if decoder else None, N.ptr(bp) if decoder else None, Tn, B, H,
                                     int(decoder), N.ptr(h_all), N.ptr(c_all), N.ptr(act), N.ptr(rel_out),
                                     N.stream_ptr()), "sgg_lstm_fwd")
        torch.cuda.synchronize()
        for k, b in list(bufs.items()) + list(ins.items()):
            assert _bands_ok(b), (save, proj, k, "guard band written")
        assert not torch.isnan(h_all.view(Tn + 1, B, H)[Tn]).any()
        if decoder:
            assert not torch.isnan(rel_out).any()
        if proj:
            assert not torch.isnan(U).any()
        if save:
            assert not torch.isnan(h_all).any() and not torch.isnan(act).any() and not torch.isnan(c_all).any()
            assert torch.equal(h_all.view(Tn + 1, B, H)[0], h0.view(B, H))
        return h_all, c_all, act, rel_out

    for proj in ((True, False) if not decoder else (False,)):
        forward(False, proj)
        h_all, c_all, act, rel_out = forward(True, proj)   # (the last pass: the saved states of the backward below)

    rows = lib.sgg_lstm_wpart_rows(H, B)
    width = 4 * H * H + 4 * H + 8 * H + (2 * H + 2 if decoder else 0)   # sgg.h: [dW_hh | dbias | dA] (+ [dWp | dbp])
    assert rows == 2
    wpart = g("wpart", rows * width)
    dh0 = g("dh0", B * H)
    drel_in = g("drel_in", Tn * B * 2)
    drel_tot = g("drel_tot", Tn * B * 2) if decoder else None
    dh_last = None if decoder else g("dh_last", B * H, r(B, H))
    dout = g("dout", Tn * B * 2, r(Tn, B, 2)) if decoder else None
    assert lib.sgg_lstm_dg_floats(Tn, B, H) == 0   # (no dG at the four-wave sizes)
    N.check(lib.sgg_lstm_bwd(N.ptr(A), N.ptr(Whh), N.ptr(Wp) if decoder else None, N.ptr(h_all), N.ptr(c_all),
                             N.ptr(act), N.ptr(rel), N.ptr(rel_out), N.ptr(dh_last), N.ptr(dout), Tn, B, H,
                             int(decoder), None, N.ptr(dh0), N.ptr(drel_in), N.ptr(drel_tot), N.ptr(wpart),
                             N.stream_ptr()), "sgg_lstm_bwd")
    torch.cuda.synchronize()
    for k, b in list(bufs.items()) + list(ins.items()):
        assert _bands_ok(b), (k, "guard band written")
    for k in ("wpart", "dh0", "drel_in") + (("drel_tot",) if decoder else ()):
        assert not torch.isnan(bufs[k][GUARD:-GUARD]).any(), (k, "NaN in an output")


# ---------------------------------------------------------------------------
# f. the encoder's T limit (its inputs of all steps are staged in LDS: T <= 64)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("H", SIZES)
def test_encoder_past_the_staging_limit_is_refused(H):
    from sgan import _native as N
    from sgan import models as M
    lib = N.load()
    Tn, B = 65, 15
    x = torch.zeros(4 * H * H, device=DEV)
    rel = torch.zeros(Tn, B, 2, device=DEV)
    h_all = torch.full(((Tn + 1) * B * H,), NAN, device=DEV)
    c_all = torch.full((lib.sgg_lstm_state_floats(Tn, B, H, 1),), NAN, device=DEV)
    act = torch.full((lib.sgg_lstm_state_floats(Tn, B, H, 0),), NAN, device=DEV)
    U = torch.full((B * 16,), NAN, device=DEV)
    for a in (act, None):
        rc = lib.sgg_lstm_fwd(N.ptr(rel), N.ptr(x), N.ptr(x), N.ptr(x), None, None, None, None, Tn, B, H, 0,
                              N.ptr(h_all), N.ptr(c_all), N.ptr(a), None, N.stream_ptr())
        assert rc == SGG_E_ARG
        msg = lib.sgg_last_error().decode()
        assert "<= 64 steps" in msg and "T=65" in msg and "H=%d" % H in msg, msg
        rc = lib.sgg_lstm_fwd_u(N.ptr(rel), N.ptr(x), N.ptr(x), N.ptr(x), None, None, Tn, B, H, N.ptr(h_all),
                                N.ptr(c_all), N.ptr(a), N.ptr(x), H, N.ptr(x), 16, N.ptr(U), N.stream_ptr())
        assert rc == SGG_E_ARG and "<= 64 steps" in lib.sgg_last_error().decode()
    torch.cuda.synchronize()
    for t in (h_all, c_all, act, U):
        assert torch.isnan(t).all(), "a refused call wrote an output"
    # the module: the same refusal, by name, under autograd and without
    enc = M.Encoder(16, H).to(DEV)
    for grad in (True, False):
        with torch.set_grad_enabled(grad), pytest.raises(N.NativeError, match=r"hold <= 64 steps \(T=65\)"):
            enc(torch.randn(Tn, B, 2, device=DEV))
    # (T = 64 runs: CASES)


# ---------------------------------------------------------------------------
# g. the decoder's discriminator input on either side of the staging limit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("H,Tn,save", [(32, 64, True), (32, 65, False), (48, 65, True), (16, 64, False)])
def test_decoder_traj_out_across_the_staging_limit(H, Tn, save):
    """sgg_lstm_fwd_dec with an SggTrajOut: up to T = 64 the generated steps
    are staged in LDS and stored after the loop, past it each step stores its
    own (lstm_mw.hip); at these T the head / real-half entries are more than
    the prologue's register set holds.  The discriminator input is exactly
    [head | rel_out], [head | b] and the start positions, inside NaN bands,
    and rel_out is bitwise the plain sgg_lstm_fwd run from the same start."""
    from sgan import _native as N
    lib = N.load()
    B, T0, S, nz = 17, 3, 3, 8
    Dc = H - nz
    torch.manual_seed(7 * H + Tn)
    r = lambda *s: torch.randn(*s, device=DEV)
    A, Whh, bias = r(4 * H, 2) * .3, r(4 * H, H) * .1, r(4 * H) * .1
    Wp, bp = r(2, H) * .2, r(2) * .1
    ctx, z, last = r(B, Dc) * .5, r(1, S, nz) * .5, r(B, 2) * .3
    ps = (torch.arange(B, device=DEV, dtype=torch.int32) * S) // B
    di = N.DecInit(N.ptr(ctx), Dc, Dc, N.ptr(z), nz, None, 0, N.ptr(ps), S, B, N.ptr(last))
    head, bgt, pos0 = r(T0, B, 2), r(Tn, B, 2), r(B, 2)
    trj_buf, trj = _guarded((T0 + Tn) * 2 * B * 2)
    st_buf, st = _guarded(2 * B * 2)
    to = N.TrajOut(N.ptr(trj), 2 * B, T0, 0, B, N.ptr(head), head.stride(0), N.ptr(bgt), bgt.stride(0), N.ptr(pos0),
                   N.ptr(st))

    def state():
        return (torch.full(((Tn + 1) * B * H,), NAN, device=DEV),
                torch.full((lib.sgg_lstm_state_floats(Tn, B, H, 1),), NAN, device=DEV),
                torch.full((lib.sgg_lstm_state_floats(Tn, B, H, 0),), NAN, device=DEV) if save else None,
                torch.full((Tn, B, 2), NAN, device=DEV))
    h_all, c_all, act, rel_out = state()
    rel0 = torch.full((B, 2), NAN, device=DEV)
    assert _kname(H, B, True, save, 0) == "sgg::lstm_mw_fwd_kernel<%d, true, %s>" % (H, _tf(save))
    N.check(lib.sgg_lstm_fwd_dec(N.ctypes.byref(di), N.ptr(A), N.ptr(Whh), N.ptr(bias), N.ptr(Wp), N.ptr(bp), Tn, B, H,
                                 N.ptr(h_all), N.ptr(c_all), N.ptr(act), N.ptr(rel_out), N.ptr(rel0) if save else None,
                                 N.ctypes.byref(to), N.stream_ptr()), "sgg_lstm_fwd_dec")
    h0 = torch.cat([ctx, z[0][ps.long()]], 1).contiguous()
    h_all2, c_all2, act2, rel_out2 = state()
    N.check(lib.sgg_lstm_fwd(N.ptr(last), N.ptr(A), N.ptr(Whh), N.ptr(bias), N.ptr(h0), None, N.ptr(Wp), N.ptr(bp), Tn,
                             B, H, 1, N.ptr(h_all2), N.ptr(c_all2), N.ptr(act2), N.ptr(rel_out2), N.stream_ptr()),
            "sgg_lstm_fwd")
    torch.cuda.synchronize()
    assert _bands_ok(trj_buf) and _bands_ok(st_buf), "guard band written"
    assert not torch.isnan(rel_out).any() and torch.equal(rel_out, rel_out2)
    assert torch.equal(h_all.view(Tn + 1, B, H)[Tn], h_all2.view(Tn + 1, B, H)[Tn])
    if save:
        assert torch.equal(rel0, last) and torch.equal(h_all, h_all2) and torch.equal(act, act2)
    t = trj.view(T0 + Tn, 2 * B, 2)
    assert torch.equal(t[:T0, :B], head) and torch.equal(t[:T0, B:], head), "head steps"
    assert torch.equal(t[T0:, :B], rel_out), "generated steps"
    assert torch.equal(t[T0:, B:], bgt), "real steps"
    assert torch.equal(st.view(2 * B, 2)[:B], pos0) and torch.equal(st.view(2 * B, 2)[B:], pos0), "start positions"
