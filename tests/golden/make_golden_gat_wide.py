"""Golden fixtures for graph attention above 128 nodes per segment, from the
reference code.

    python tests/golden/make_golden_gat_wide.py

gat_encoder_wide.npz  the reference's GATEncoder (n_heads=2) forward + all
                      gradients on scenes of 200, 130, 150 and 20 peds with
                      label_patterns: scene 0 everybody ungrouped (a 200-node
                      inter-group segment), scene 1 one group of 130 (130-edge
                      intra rows), scenes 2 and 3 mixed and many small groups.
                      gat_encoder_h2.npz's keys.
gen_fwd_gat_wide.npz  the gat generator forward + every parameter gradient on a
                      synthetic batch of 129, 3, 200 and 20 peds with the same
                      label kinds (weights: weights.npz, not stored again).

The generator contains the max-pool, whose gradient is discontinuous at near
ties, so the generator batch's seed is the first from
GEN_SEED_FIRST on for which the float32 CPU oracle (oracle/sgan_oracle.py)
reproduces the fixture within half of the GPU test's tolerances (out 1e-4,
gradients 1e-3 on grad_floor's scale): GEN_SEED below, with the margins
observed for it (tests/test_oracle_golden_gat_wide.py asserts them).

    GEN_SEED = 40: out 0.0e+00 (bound 5e-05), gradients 0.0e+00 (bound 5e-04)
    -- on the CPU the oracle runs the reference's torch operations in the
    reference's order and lands on its bits; 40 is the first seed tried.
"""
import os
import sys

import numpy as np
import torch

from make_golden import HERE, M, build_models, grad_arrays, label_patterns, save, sse_of, synth_batch, _gen_forward

ENC_SIZES = [200, 130, 150, 20]
ENC_SEED = 23
GEN_SIZES = [129, 3, 200, 20]
GEN_SEED_FIRST = 40
GEN_SEED = 40
OUT_TOL, GRAD_TOL = 1e-4, 1e-3   # the GPU test's (test_generator_vs_reference_fixture's)


def fx_gat_encoder_wide():
    torch.manual_seed(ENC_SEED)
    mod = M.GATEncoder(n_units=[40, 16, 40], n_heads=2, dropout=0, alpha=0.2)
    B = sum(ENC_SIZES)
    x = torch.randn(B, 40, requires_grad=True)
    lab = torch.from_numpy(label_patterns(ENC_SIZES, ENC_SEED)).float().view(B, 1)
    sse = sse_of(ENC_SIZES)
    y = mod(x, sse, torch.zeros(B, 2), lab)
    dy = torch.randn_like(y)
    mod.zero_grad()
    (y * dy).sum().backward()
    out = dict(x=x.detach().numpy(), labels=lab.numpy()[:, 0], sse=sse.numpy(), out=y.detach().numpy(),
               dout=dy.numpy(), dx=x.grad.numpy())
    for k, p in mod.named_parameters():
        out["w/" + k] = p.detach().numpy()
        if p.grad is not None:
            out["dw/" + k] = p.grad.numpy()
    save("gat_encoder_wide.npz", out)


def gen_case(g, seed):
    b = synth_batch(GEN_SIZES, seed=seed)
    lab = torch.from_numpy(label_patterns(GEN_SIZES, seed)).float()
    b["obs_traj_g"] = lab.view(1, -1, 1).expand(b["obs_traj_g"].shape).contiguous()
    out = {k: b[k].numpy() for k in ("obs_traj", "obs_traj_rel", "obs_traj_g", "seq_start_end")}
    torch.manual_seed(77)
    noise = torch.randn(len(GEN_SIZES), 8)
    out["noise"] = noise.numpy()
    g.zero_grad()
    y = _gen_forward(g, b, noise, "gat")
    torch.manual_seed(78)
    dy = torch.randn_like(y)
    (y * dy).sum().backward()
    out["gat/out"] = y.detach().numpy()
    out["gat/dout"] = dy.numpy()
    out.update(grad_arrays(g, "gat/dw/"))
    return out


def oracle_margins(f):
    """(out, gradient) errors of the float32 CPU oracle against the arrays f,
    as tests/test_oracle_golden_gat_wide.py measures them."""
    root = os.path.dirname(os.path.dirname(HERE))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.append(p)
    from oracle import sgan_oracle as O
    from conftest import load_family
    w = np.load(os.path.join(HERE, "weights.npz"))
    g, _ = O.build_default("gat")
    load_family(g, {k[2:]: torch.from_numpy(w[k]).clone() for k in w.files if k.startswith("g/")})
    T = lambda a: torch.from_numpy(np.asarray(a)).clone()
    y = g(T(f["obs_traj"]), T(f["obs_traj_rel"]), T(f["seq_start_end"]), T(f["obs_traj_g"]), user_noise=T(f["noise"]))
    rel = lambda a, b, floor: float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), floor))
    e_out = rel(y.detach().numpy(), f["gat/out"], 1e-6)
    (y * T(f["gat/dout"])).sum().backward()
    fl = 1e-2 * max(np.abs(v).max() for k, v in f.items() if k.startswith("gat/dw/"))
    e_grad = max(rel(p.grad.numpy(), f["gat/dw/" + k], fl) for k, p in g.named_parameters() if "gat/dw/" + k in f)
    return e_out, e_grad


def fx_gen_gat_wide():
    g, _ = build_models(0)
    for seed in range(GEN_SEED_FIRST, GEN_SEED_FIRST + 50):
        f = gen_case(g, seed)
        e_out, e_grad = oracle_margins(f)
        print("  seed %d: oracle out %.1e (bound %.0e), gradients %.1e (bound %.0e)"
              % (seed, e_out, OUT_TOL / 2, e_grad, GRAD_TOL / 2), flush=True)
        if e_out <= OUT_TOL / 2 and e_grad <= GRAD_TOL / 2:
            break
    else:
        raise AssertionError("no seed met the margins")
    assert seed == GEN_SEED, "update GEN_SEED and the docstring: %d" % seed
    save("gen_fwd_gat_wide.npz", f)


if __name__ == "__main__":
    fx_gat_encoder_wide()
    fx_gen_gat_wide()
