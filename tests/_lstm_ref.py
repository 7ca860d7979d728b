"""Float64 yardstick of the LSTM sequence kernels, shared by the kernel tests
(test_gpu_lstm_gen.py, test_gpu_lstm_mw.py) and the CPU test of the gate
itself (test_lstm_ref_gate.py).

The fp32 HIP path is judged by the error the oracle's own fp32 CPU modules
make against the same modules in float64:
    |HIP - f64| <= 4 |CPU32 - f64| + 1e-6 max|f64|     (max over the tensor)
"""
import copy

import numpy as np
import torch

DEV = "cuda"


def _build(H, Tn, decoder, seed):
    from oracle import sgan_oracle as O
    torch.manual_seed(seed)
    return O.Decoder(Tn, 16, H, 64, 1, False) if decoder else O.Encoder(16, H)


def _inputs(H, Tn, decoder, B, seed):
    gen = torch.Generator().manual_seed(seed + 1)
    if decoder:
        return dict(last_pos=torch.randn(B, 2, generator=gen), last_rel=torch.randn(B, 2, generator=gen) * 0.3,
                    h0=torch.randn(1, B, H, generator=gen) * 0.5, dy=torch.randn(Tn, B, 2, generator=gen))
    return dict(rel=torch.randn(Tn, B, 2, generator=gen) * 0.3, dy=torch.randn(1, B, H, generator=gen))


def _run(mod, inp, decoder, dev, dtype):
    """Outputs, input gradients and parameter gradients of one module run."""
    c = lambda t: t.detach().to(device=dev, dtype=dtype)
    mod.zero_grad()
    if decoder:
        h0 = c(inp["h0"]).requires_grad_(True)
        lr = c(inp["last_rel"]).requires_grad_(True)
        y, _ = mod(c(inp["last_pos"]), lr, (h0, torch.zeros_like(h0)), None)
        (y * c(inp["dy"])).sum().backward()
        res = {"out": y, "dh0": h0.grad, "drel": lr.grad}
    else:
        rel = c(inp["rel"]).requires_grad_(True)
        y = mod(rel)
        (y.reshape(inp["dy"].shape) * c(inp["dy"])).sum().backward()
        res = {"out": y.reshape(inp["dy"].shape), "drel": rel.grad}
    for k, p in mod.named_parameters():
        res["d" + k] = p.grad
    return {k: v.detach().cpu().double().numpy() for k, v in res.items()}


_REF = {}


def reference(H, Tn, decoder, B):
    """(module, inputs, float64 results, fp32 CPU results) of a case, computed
    once and shared."""
    key = (H, Tn, decoder, B)
    if key not in _REF:
        seed = 1000 * H + 10 * Tn + B
        ref = _build(H, Tn, decoder, seed)
        inp = _inputs(H, Tn, decoder, B, seed)
        r32 = _run(ref, inp, decoder, "cpu", torch.float32)
        torch.set_default_dtype(torch.float64)
        try:
            r64 = _run(copy.deepcopy(ref).double(), inp, decoder, "cpu", torch.float64)
        finally:
            torch.set_default_dtype(torch.float32)
        _REF[key] = (ref, inp, r64, r32)
    return _REF[key]


def gate(tag, got, r64, r32, sel=lambda k, a: a):
    """Every quantity within 4x the fp32 CPU error + 1e-6 of the scale; prints
    each figure, then asserts."""
    bad = []
    for k in r64:
        ref = sel(k, r64[k])
        e = float(np.abs(sel(k, got[k]) - ref).max())
        e32 = float(np.abs(sel(k, r32[k]) - ref).max())
        scale = float(np.abs(ref).max())
        bound = 4 * e32 + 1e-6 * scale
        print("%s %-28s err %.3e  cpu32 %.3e  ratio %6.2f  scale %.3e" % (tag, k, e, e32, e / max(e32, 1e-300), scale))
        if not e <= bound:
            bad.append((k, e, e32, scale))
    assert not bad, (tag, bad)


def hip_module(ref, H, Tn, decoder):
    from sgan import models as M
    mod = M.Decoder(Tn, 16, H, 64, 1, False) if decoder else M.Encoder(16, H)
    mod.load_state_dict(ref.state_dict())
    return mod.to(DEV)


# ---------------------------------------------------------------------------
# an encoder started from a given state (the oracle's Encoder starts from zero)
# ---------------------------------------------------------------------------
def run_state(lstm, emb, inp, dev, dtype, seq=None):
    """h_T of Linear(2, 16) + LSTM(16, H) over rel from (h0, c0), with drel,
    dh0 and every parameter gradient of sum(h_T dy).  seq(rel, lstm, emb, h0,
    c0) -> h_T (B x H) runs the sequence; the default is torch.nn.LSTM."""
    c = lambda t: t.detach().to(device=dev, dtype=dtype)
    lstm.zero_grad()
    emb.zero_grad()
    rel = c(inp["rel"]).requires_grad_(True)
    h0 = c(inp["h0"]).requires_grad_(True)
    c0 = c(inp["c0"])
    if seq is None:
        Tn, B = rel.shape[0], rel.shape[1]
        x = emb(rel.reshape(-1, 2)).view(Tn, B, -1)
        _, (h, _) = lstm(x, (h0.unsqueeze(0), c0.unsqueeze(0)))
        h = h[0]
    else:
        h = seq(rel, lstm, emb, h0, c0)
    (h * c(inp["dy"])).sum().backward()
    res = {"out": h, "drel": rel.grad, "dh0": h0.grad}
    for name, mod in (("encoder", lstm), ("spatial_embedding", emb)):
        for k, p in mod.named_parameters():
            res["d%s.%s" % (name, k)] = p.grad
    return {k: v.detach().cpu().double().numpy() for k, v in res.items()}


def reference_state(H, Tn, B):
    """((lstm, emb), inputs, float64 results, fp32 CPU results) of an encoder
    sequence from a random (h0, c0): torch.nn.LSTM(16, H) + Linear(2, 16),
    computed once and shared."""
    key = ("state", H, Tn, B)
    if key not in _REF:
        seed = 1000 * H + 10 * Tn + B + 500
        torch.manual_seed(seed)
        lstm, emb = torch.nn.LSTM(16, H), torch.nn.Linear(2, 16)
        gen = torch.Generator().manual_seed(seed + 1)
        inp = dict(rel=torch.randn(Tn, B, 2, generator=gen) * 0.3, h0=torch.randn(B, H, generator=gen) * 0.5,
                   c0=torch.randn(B, H, generator=gen) * 0.5, dy=torch.randn(B, H, generator=gen))
        r32 = run_state(lstm, emb, inp, "cpu", torch.float32)
        r64 = run_state(copy.deepcopy(lstm).double(), copy.deepcopy(emb).double(), inp, "cpu", torch.float64)
        _REF[key] = ((lstm, emb), inp, r64, r32)
    return _REF[key]
