"""The generic LSTM kernel family (lstm_gen.hip, H outside 16 / 32 / 48 / 64)
against its two yardsticks, alternating in one process.

    python tools/bench_lstm_gen.py [--rounds 5] [--iters 30] [--out FILE.json]

Shapes: the decoder rollout [T = 12, B = 1280] and the encoder [T = 20,
B = 2560], at H = 40 and H = 128.  Per shape and H, three timings by device
events: the forward without saved states (no_grad), the forward that saves
them, and forward + backward (the backward's sgg_xtw products and its
sgg_grad_finish included).  Variants:
  gen     sgan.models.Encoder / Decoder at H (the generic kernels)
  torch   stock nn.LSTM + nn.Linear on the same GPU (oracle.sgan_oracle's
          modules: the decoder a per-step loop, the encoder one nn.LSTM call)
          -- what a user could run at these sizes before
  mw48    H = 40 only: the same module at H = 48, the four-wave kernels that
          zero-padded weights would run on
One line per run, then one JSON summary (the median of the rounds per entry).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "group-gan-gcn-gat_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def build(kind, H, Tn, decoder):
    from oracle import sgan_oracle as O
    from sgan import models as M
    lib = O if kind == "torch" else M
    Hk = 48 if kind == "mw48" else H
    mod = lib.Decoder(Tn, 16, Hk, 64, 1, False) if decoder else lib.Encoder(16, Hk)
    return mod.cuda(), Hk


def runner(mod, Hk, Tn, B, decoder):
    gen = torch.Generator(device="cuda").manual_seed(1)
    if decoder:
        pos = torch.randn(B, 2, device="cuda", generator=gen)
        rel = torch.randn(B, 2, device="cuda", generator=gen) * 0.3
        h0 = (torch.randn(1, B, Hk, device="cuda", generator=gen) * 0.5).requires_grad_(True)
        c0 = torch.zeros(1, B, Hk, device="cuda")
        dy = torch.randn(Tn, B, 2, device="cuda", generator=gen)
        fwd = lambda: mod(pos, rel, (h0, c0), None)[0]
    else:
        rel = (torch.randn(Tn, B, 2, device="cuda", generator=gen) * 0.3).requires_grad_(True)
        dy = torch.randn(1, B, Hk, device="cuda", generator=gen)
        fwd = lambda: mod(rel)

    def nosave():
        with torch.no_grad():
            fwd()

    def fwd_bwd():
        mod.zero_grad(set_to_none=True)
        (fwd() * dy).sum().backward()
    return {"fwd_nosave": nosave, "fwd_save": fwd, "fwd_bwd": fwd_bwd}


def timed(fn, iters):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters   # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out")
    a = ap.parse_args()
    from sgan import _native
    _native.load()
    res = {}
    for Tn, B, decoder in ((12, 1280, True), (20, 2560, False)):
        for H in (40, 128):
            kinds = ("gen", "torch") + (("mw48",) if H == 40 else ())
            torch.manual_seed(0)
            runs = {k: runner(*build(k, H, Tn, decoder), Tn, B, decoder) for k in kinds}
            times = {(k, w): [] for k in kinds for w in runs[k]}
            for r in range(a.rounds):
                for w in ("fwd_nosave", "fwd_save", "fwd_bwd"):
                    for k in kinds:   # the variants alternate inside every round
                        us = timed(runs[k][w], a.iters)
                        times[(k, w)].append(us)
                        print("round %d %s T=%d B=%d H=%d %-5s %-10s %9.1f us" % (
                            r, "dec" if decoder else "enc", Tn, B, H, k, w, us), flush=True)
            tag = "%s_T%d_B%d_H%d" % ("dec" if decoder else "enc", Tn, B, H)
            res[tag] = {"%s/%s" % kw: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}
                        for kw, v in times.items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
