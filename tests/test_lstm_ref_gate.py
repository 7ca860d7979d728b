"""The float64 gate of the LSTM kernel tests (tests/_lstm_ref.py) has teeth:
it accepts the oracle's own fp32 CPU result and rejects that result with the
errors a tiled kernel makes planted in it -- a clamped tail ped, a dropped
step of a weight gradient, two units swapped, a lost input gradient.  Runs on
the CPU: nothing here touches the HIP library.
"""
import copy
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN  # noqa: F401  (puts the repository on sys.path)
from _lstm_ref import gate, reference

CASES = [(48, 8, False, 17), (64, 12, True, 17)]


def _tag(H, Tn, decoder, B):
    return "H=%d T=%d %s B=%d" % (H, Tn, "dec" if decoder else "enc", B)


def _lstm_name(decoder):
    return "decoder" if decoder else "encoder"


def _dwhh_steps(ref, inp, decoder):
    """(the last step's contribution to dW_hh, the sum of every step's): the
    module's recurrence restated in float64 with one W_hh leaf per step."""
    mod = copy.deepcopy(ref).double()
    lstm, emb = getattr(mod, _lstm_name(decoder)), mod.spatial_embedding
    d = lambda t: t.detach().double()
    dy = d(inp["dy"])
    Tn = dy.shape[0] if decoder else inp["rel"].shape[0]
    B = dy.shape[1]
    H = lstm.weight_hh_l0.shape[1]
    Ws = [lstm.weight_hh_l0.detach().clone().requires_grad_(True) for _ in range(Tn)]
    b = lstm.bias_ih_l0 + lstm.bias_hh_l0
    h = d(inp["h0"])[0] if decoder else torch.zeros(B, H, dtype=torch.float64)
    c = torch.zeros(B, H, dtype=torch.float64)
    x = emb(d(inp["last_rel"])) if decoder else None
    outs = []
    for t in range(Tn):
        if not decoder:
            x = emb(d(inp["rel"])[t])
        gi, gf, gg, go = (x @ lstm.weight_ih_l0.t() + h @ Ws[t].t() + b).chunk(4, 1)
        c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
        h = torch.sigmoid(go) * torch.tanh(c)
        if decoder:
            rel = mod.hidden2pos(h)
            outs.append(rel)
            x = emb(rel)
    y = torch.stack(outs, 0) if decoder else h.unsqueeze(0)
    (y * dy).sum().backward()
    return Ws[-1].grad.numpy(), sum(W.grad for W in Ws).numpy()


def _plant_clamp(got, decoder, B):
    """The last ped's output row is ped B - 2's (min(p, B - 1) one off)."""
    out = got["out"]
    out[:, B - 1] = out[:, B - 2]
    return "out"


def _plant_drel0(got, decoder, B):
    got["drel"][0] = 0.0
    return "drel"


def _plant_swap(got, decoder, B):
    """Units 1 and H - 2 of the forget gate change places in dbias."""
    k = "d%s.bias_ih_l0" % _lstm_name(decoder)
    H = got[k].shape[0] // 4
    a, b = H + 1, H + H - 2
    got[k][[a, b]] = got[k][[b, a]]
    return k


@pytest.mark.parametrize("H,Tn,decoder,B", CASES)
def test_gate_accepts_the_untouched_fp32_result(H, Tn, decoder, B):
    _, _, r64, r32 = reference(H, Tn, decoder, B)
    assert set(r64) == set(r32) and "out" in r64 and "drel" in r64 and ("dh0" in r64) == decoder
    assert sum(k.startswith("d%s." % _lstm_name(decoder)) for k in r64) == 4
    gate(_tag(H, Tn, decoder, B), {k: v.copy() for k, v in r32.items()}, r64, r32)


@pytest.mark.parametrize("plant", [_plant_clamp, _plant_swap, _plant_drel0], ids=["clamp", "swap", "drel0"])
@pytest.mark.parametrize("H,Tn,decoder,B", CASES)
def test_gate_rejects_a_planted_error(H, Tn, decoder, B, plant):
    _, _, r64, r32 = reference(H, Tn, decoder, B)
    got = {k: v.copy() for k, v in r32.items()}
    key = plant(got, decoder, B)
    assert not np.array_equal(got[key], r32[key]), "nothing was planted"
    with pytest.raises(AssertionError, match=re.escape("'%s'" % key)) as ei:
        gate(_tag(H, Tn, decoder, B) + " planted", got, r64, r32)
    # only the quantity that was touched is reported
    assert all(("'%s'" % k) not in str(ei.value) for k in r64 if k != key)


@pytest.mark.parametrize("H,Tn,decoder,B", CASES)
def test_gate_rejects_a_dropped_last_step_of_dwhh(H, Tn, decoder, B):
    ref, inp, r64, r32 = reference(H, Tn, decoder, B)
    key = "d%s.weight_hh_l0" % _lstm_name(decoder)
    last, total = _dwhh_steps(ref, inp, decoder)
    # the restatement is the module: its per-step pieces sum to the yardstick's dW_hh
    assert np.abs(total - r64[key]).max() <= 1e-12 * np.abs(r64[key]).max()
    got = {k: v.copy() for k, v in r32.items()}
    got[key] = got[key] - last
    with pytest.raises(AssertionError, match=re.escape("'%s'" % key)):
        gate(_tag(H, Tn, decoder, B) + " planted", got, r64, r32)
