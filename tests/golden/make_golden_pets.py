"""Golden fixtures for per-step pooling (pool_every_timestep=1), from the
reference's own modules on the CPU.  Data only; run next to make_golden.py,
whose helpers it imports:

    python tests/golden/make_golden_pets.py [gen] [train_step] [eval]

train_step_pets_it<i>_<g|d>.npz (fx_train_step_pets) and evaluate_pets.json
(fx_eval_pets) are described at their functions.  gen: two models, each on two
batches ("<batch>/": the inputs, the output, dout and every parameter gradient
"dw/"), within the size limit of a committed file:
  gen_fwd_pets.npz: the generator at scripts/train.py's defaults with
       pool_every_timestep=1 (+ the noise); its state is weights_pets.npz ("g/");
  gen_fwd_pets_dec.npz: a decoder alone (state "w/") with h_dim=48,
       mlp_dim=32, bottleneck_dim=16 (non-square, so a swapped dimension
       shows), rolled out from a random initial state h0 whose gradient dh0
       is recorded too.  The reference's generator cannot
       be built at these sizes: its GAT encoder is 40 wide in and 24 wide out
       whatever the arguments say (models.py:259, :289), which pins the
       decoder to 32 and the bottleneck to 8.
Batches: "synth": scenes of 1, 2, 5, 17 and 3 peds (28 rows: one full 16-row
tile and a ragged one, a one-ped scene, a scene larger than a tile); "wide":
scenes of 70 and 3 peds (the tiled pooling kernels inside the loop).

Conditioning: every case's decoder (the per-step loop; the modules before it
are pinned by the other fixtures) is also run in float64 from the same initial
state; the float32 output and gradients (parameters and initial state) must
agree with it to a tenth of the tests' tolerances (1e-4 on the output, 1e-3
on a gradient, normalised as the tests normalise), else the seed is rejected
-- a max-pool or ReLU tie that flips between implementations would show here.
"""
import copy
import json
import os
import random

import numpy as np
import torch

import make_golden as MG

M, TR, ARGS = MG.M, MG.TR, MG.ARGS

BATCHES = {"synth": [1, 2, 5, 17, 3], "wide": [70, 3]}
DEC_B = dict(h_dim=48, mlp_dim=32, bottleneck_dim=16)
OUT_TOL, GRAD_TOL = 1e-4, 1e-3


def build_generator(seed):
    """scripts/train.py:173-190 with pool_every_timestep=1."""
    torch.manual_seed(seed)
    a = ARGS
    n_units = [40] + [int(x) for x in a.hidden_units.strip().split(",")] + [40]
    g = M.TrajectoryGenerator(
        obs_len=a.obs_len, pred_len=a.pred_len, embedding_dim=a.embedding_dim, encoder_h_dim=a.encoder_h_dim_g,
        decoder_h_dim=a.decoder_h_dim_g, mlp_dim=a.mlp_dim, num_layers=a.num_layers,
        noise_dim=a.noise_dim, noise_type=a.noise_type, noise_mix_type=a.noise_mix_type, pooling_type=a.pooling_type,
        pool_every_timestep=True, dropout=a.dropout, bottleneck_dim=a.bottleneck_dim,
        neighborhood_size=a.neighborhood_size, grid_size=a.grid_size, batch_norm=False, n_units=n_units,
        n_heads=a.n_heads, dropout1=a.dropout1, alpha=a.alpha)
    g.apply(TR.init_weights)
    g.train()
    return g


def build_decoder(seed):
    torch.manual_seed(seed)
    a = ARGS
    d = M.Decoder(a.pred_len, embedding_dim=a.embedding_dim, num_layers=a.num_layers, pool_every_timestep=True,
                  dropout=a.dropout, activation="relu", batch_norm=False, pooling_type=a.pooling_type,
                  grid_size=a.grid_size, neighborhood_size=a.neighborhood_size, **DEC_B)
    d.apply(TR.init_weights)
    d.train()
    return d


def run_generator(g, b, noise, dy):
    """The generator's forward + backward -> (out, {param: grad}, h0): h0 =
    the decoder's initial state, caught on its way in."""
    seen = {}

    def catch(mod, args):
        seen["h"] = args[2][0].detach().clone()

    hook = g.decoder.register_forward_pre_hook(catch)
    try:
        g.zero_grad()
        y = g(b["obs_traj"], b["obs_traj_rel"], b["seq_start_end"], b["obs_traj_g"], user_noise=noise)
        (y * dy).sum().backward()
    finally:
        hook.remove()
    grads = {k: p.grad.detach().numpy().copy() for k, p in g.named_parameters() if p.grad is not None}
    return y.detach().numpy().copy(), grads, seen["h"]


def run_decoder(dec, b, h0, dy, dtype):
    """The reference decoder alone (models.py:142-178) from the state h0
    (1, B, H), c0 = 0, in `dtype` -> (out, {param: grad, "h0": grad})."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        dec = dec.to(dtype)
        dec.zero_grad()
        h = h0.to(dtype).requires_grad_(True)
        y, _ = dec(b["obs_traj"][-1].to(dtype), b["obs_traj_rel"][-1].to(dtype), (h, torch.zeros_like(h)),
                   b["seq_start_end"])
        (y * dy.to(dtype)).sum().backward()
        grads = {k: p.grad.detach().numpy().copy() for k, p in dec.named_parameters() if p.grad is not None}
        grads["h0"] = h.grad.numpy().copy()
        return y.detach().numpy().copy(), grads
    finally:
        torch.set_default_dtype(prev)
        dec.to(torch.float32)


def conditioning(d32, d64):
    """-> (output error, worst gradient error) of (out, grads) pairs, normalised as the tests do."""
    (o32, g32), (o64, g64) = d32, d64
    eo = np.abs(o32 - o64).max() / max(np.abs(o64).max(), 1e-6)
    floor = 1e-2 * max(np.abs(v).max() for v in g64.values())
    eg = max(np.abs(g32[k] - g64[k]).max() / max(np.abs(g64[k]).max(), floor) for k in g64)
    return eo, eg


def case(model, dec, sizes, what):
    """The first seed whose decoder run is well conditioned -> the case's arrays."""
    sd = {k: v.detach().clone() for k, v in dec.state_dict().items()}
    B = sum(sizes)
    for seed in range(5, 25):
        b = MG.synth_batch(sizes, seed=seed)
        torch.manual_seed(77 + seed)
        noise = torch.randn(len(sizes), 8)
        dy = torch.randn(ARGS.pred_len, B, 2)
        arrs = {}
        if model is dec:
            h0 = 0.5 * torch.randn(1, B, DEC_B["h_dim"])
            arrs["h0"] = h0[0].numpy()
        else:
            out, grads, h0 = run_generator(model, b, noise, dy)
            arrs["noise"] = noise.numpy()
        d64 = run_decoder(dec, b, h0, dy, torch.float64)
        dec.load_state_dict(sd)   # (the float32 weights again, bit for bit)
        d32 = run_decoder(dec, b, h0, dy, torch.float32)
        if model is dec:
            out, grads = d32[0], dict(d32[1])
            arrs["dh0"] = grads.pop("h0")[0]
        else:
            assert np.array_equal(d32[0], out)   # the decoder alone = the generator's
        eo, eg = conditioning(d32, d64)
        ok = eo < OUT_TOL / 10 and eg < GRAD_TOL / 10
        print("%s seed %d: f32 vs f64 out %.2e grad %.2e %s" % (what, seed, eo, eg, "ok" if ok else "REJECTED"))
        if not ok:
            continue
        for k in ("obs_traj", "obs_traj_rel", "obs_traj_g", "seq_start_end"):
            arrs[k] = b[k].numpy()
        arrs["out"], arrs["dout"] = out, dy.numpy()
        arrs.update({"dw/" + k: v for k, v in grads.items()})
        return arrs
    raise SystemExit("no well-conditioned seed for " + what)


def fx_gen_pets():
    g, d = build_generator(0), build_decoder(1)
    MG.save("weights_pets.npz", MG.sd_arrays(g, "g/"))
    for fname, model, dec in (("gen_fwd_pets.npz", g, g.decoder), ("gen_fwd_pets_dec.npz", d, d)):
        out = MG.sd_arrays(d, "w/") if model is d else {}
        for bname, sizes in BATCHES.items():
            out.update({bname + "/" + k: v for k, v in case(model, dec, sizes, fname[:-4] + "/" + bname).items()})
        MG.save(fname, out)


TRAIN_BATCHES = [([20] * 2 + [7, 1], 41), ([20, 3, 12], 42)]
KEYS = ["obs_traj", "pred_traj", "obs_traj_rel", "pred_traj_rel", "obs_vel", "pred_vel",
        "obs_traj_g", "pred_traj_g", "non_linear_ped", "loss_mask", "seq_start_end"]


class _NoisyAdam(MG._RecordingAdam):
    """_RecordingAdam whose step() first adds noise at the level of float32
    reassociation to every gradient (eps x the tensor's largest element,
    from a generator of its own: the host RNG streams are untouched) -- what
    separates any two float32 implementations of the same backward pass.
    An element that is exactly zero (a dead ReLU unit) stays zero."""

    def __init__(self, named, rec, eps, **kw):
        super().__init__(named, rec, **kw)
        self._eps, self._gen = eps, torch.Generator().manual_seed(99)

    def step(self, closure=None):
        if self._eps:
            for _, p in self._named:
                if p.grad is not None:
                    noise = self._eps * p.grad.abs().max() * torch.randn(p.grad.shape, generator=self._gen)
                    p.grad.add_(noise * (p.grad != 0))
        return super().step(closure)


def _train_iterations(batches, eps):
    """Two reference iterations on `batches` -> [(g arrays, d arrays)] per iteration."""
    a = copy.copy(ARGS)
    a.pool_every_timestep, a.best_k = 1, 3
    g = build_generator(0)
    _, d = MG.build_models(0)
    rec_g, rec_d = [], []
    opt_g = _NoisyAdam(g.named_parameters(), rec_g, eps, lr=a.g_learning_rate)
    opt_d = _NoisyAdam(d.named_parameters(), rec_d, eps, lr=a.d_learning_rate)
    torch.manual_seed(1234)
    random.seed(1234)
    out = []
    for it, (sizes, seed) in enumerate(batches):
        b = dict(MG.synth_batch(sizes, seed=seed))
        b["obs_vel"] = b["obs_traj_rel"] * 2.5
        b["pred_vel"] = b["pred_traj_rel"] * 2.5
        tup = [b[k] for k in KEYS]
        og = {"b%d/%s" % (it, k): b[k].numpy() for k in KEYS}
        od = {}
        ld = MG.TR.discriminator_step(a, tup, g, d, MG.TR.gan_d_loss, opt_d)
        lg = MG.TR.generator_step(a, tup, g, d, MG.TR.gan_g_loss, opt_g)
        for k, v in ld.items():
            og["it%d/D/%s" % (it, k)] = np.float64(v)
        for k, v in lg.items():
            og["it%d/G/%s" % (it, k)] = np.float64(v)
        og.update(MG.sd_arrays(g, "it%d/g/" % it))
        od.update(MG.sd_arrays(d, "it%d/d/" % it))
        od.update({"it%d/gradD/%s" % (it, k): v for k, v in rec_d[-1].items()})
        og.update({"it%d/gradG/%s" % (it, k): v for k, v in rec_g[-1].items()})
        out.append((og, od))
    return out


def _grad_sensitivity(run, other, it):
    """Worst gradient difference of iteration `it` between two runs, normalised as check_step_grads does."""
    worst = 0.0
    for kind, part in (("G", 0), ("D", 1)):
        prefix = "it%d/grad%s/" % (it, kind)
        a, b = run[it][part], other[it][part]
        keys = [k for k in a if k.startswith(prefix)]
        floor = 1e-2 * max(np.abs(a[k]).max() for k in keys)
        worst = max([worst] + [np.abs(a[k] - b[k]).max() / max(np.abs(a[k]).max(), floor) for k in keys])
    return worst


def fx_train_step_pets():
    """As make_golden.fx_train_step: two iterations of discriminator_step +
    generator_step (scripts/train.py:395-484) with pool_every_timestep=1 and
    best_k=3, fresh Adam, seeded host RNGs, from the generator of
    weights_pets.npz and the discriminator of weights.npz.  One file per
    iteration and network (the size limit of a committed file):
    train_step_pets_it<i>_<g|d>.npz, the batch and the losses in the g file.

    Conditioning: the second iteration starts from weights that Adam's first
    step moved by +-lr per element, by the SIGN of a gradient -- and the sign
    of a noise-level element differs between float32 implementations.  The
    iterations are therefore run again with noise of 1e-6 of each gradient
    tensor's largest element added before every optimizer step; the second
    iteration's gradients should agree between the two runs to a tenth of the
    tests' tolerance (1e-3), else the next pair of batch seeds is tried.  Of
    ten pairs none gets there (the reference moves by 2e-4 to 3e-1: twelve
    max-poolings and the ReLU layers of the loop, behind sign steps of the
    attention vectors); the least sensitive pair is taken, seeds (49, 50), at
    2.1e-4 -- a fifth of the tolerance, which is what the second iteration's
    gradient check can resolve on this configuration."""
    best = None
    for k in range(10):
        batches = [(sizes, seed + 2 * k) for sizes, seed in TRAIN_BATCHES]
        run = _train_iterations(batches, 0.0)
        sens = _grad_sensitivity(run, _train_iterations(batches, 1e-6), 1)
        print("train step, batch seeds %s: second-iteration gradients move by %.2e under gradient noise"
              % ([s for _, s in batches], sens), flush=True)
        if best is None or sens < best[0]:
            best = (sens, batches, run)
        if sens < GRAD_TOL / 10:
            break
    sens, batches, run = best
    print("taken: batch seeds %s (%.2e)" % ([s for _, s in batches], sens))
    for it, (og, od) in enumerate(run):
        MG.save("train_step_pets_it%d_g.npz" % it, og)
        MG.save("train_step_pets_it%d_d.npz" % it, od)


def fx_eval_pets(splits=("eth", "hotel")):
    """As make_golden.fx_eval: scripts/evaluate_model.py:72-99 on the test
    split, 20 samples, seeded host RNG, for the generator of weights_pets.npz."""
    res = {}
    for split in splits:
        g = build_generator(0)
        a = MG.EV.AttrDict(dict(vars(ARGS)))
        a["batch_size"] = 64
        _, loader = MG.DL.data_loader(a, os.path.join(MG.REF, "datasets_group", split, "test"))
        torch.manual_seed(0)
        ade, fde = MG.EV.evaluate(a, loader, g, 20)
        res[split] = dict(ade=float(ade), fde=float(fde), num_seq=len(loader.dataset))
        print(split, res[split], flush=True)
    with open(os.path.join(MG.HERE, "evaluate_pets.json"), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)


ALL = dict(gen=fx_gen_pets, train_step=fx_train_step_pets, eval=fx_eval_pets)

if __name__ == "__main__":
    import sys
    for name in (sys.argv[1:] or list(ALL)):
        ALL[name]()
