"""Per-step pooling decoder: the step kernels (SGG_DEC_STEP=1) against the
per-op loop (SGG_DEC_STEP=0), alternating in one process.

    python tools/bench_dec_step.py [--rounds 5] [--iters 40] [--scenes 64] [--peds 20] [--only 0|1]

The generator at scripts/train.py's defaults with pool_every_timestep=1 on
synthetic scenes, forward + backward, timed by device events; one line per
run, then the summary (the condition to keep the new path: each of its runs
faster than the old path's fastest)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "group-gan-gcn-gat_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--scenes", type=int, default=64)
    ap.add_argument("--peds", type=int, default=20)
    ap.add_argument("--trainer", type=int, default=0, metavar="N",
                    help="instead: time N eager GanTrainer iterations (train.py defaults, best_k 20) with this generator")
    ap.add_argument("--only", choices=("0", "1"), help="run this path alone (a kernel trace of one path)")
    a = ap.parse_args()
    from sgan.data.synthetic import synthetic_batch
    from sgan.models import TrajectoryGenerator
    from sgan.scene import SceneIndex
    torch.manual_seed(0)
    g = TrajectoryGenerator(8, 12, embedding_dim=16, encoder_h_dim=32, decoder_h_dim=32, mlp_dim=64, num_layers=1,
                            noise_dim=(8,), noise_type="gaussian", noise_mix_type="global", pooling_type="pool_net",
                            pool_every_timestep=True, dropout=0.0, bottleneck_dim=8, batch_norm=False,
                            n_units=[40, 16, 40], n_heads=1, dropout1=0.0, alpha=0.2).cuda()
    b = synthetic_batch([a.peds] * a.scenes, seed=1, device="cuda")
    obs, obs_rel, obs_g, sse = b[0], b[2], b[6], b[10]
    sc = SceneIndex.from_seq_start_end(sse, "cuda")
    if a.trainer:
        from sgan.models import TrajectoryDiscriminator
        from sgan.train_step import GanTrainer
        d = TrajectoryDiscriminator(8, 12, embedding_dim=16, h_dim=48, mlp_dim=64, num_layers=1, batch_norm=False,
                                    dropout=0.0, d_type="global").cuda()
        tr = GanTrainer(g, d)
        for _ in range(3):
            tr.step(b, sc)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.trainer):
            tr.step(b, sc)
        e1.record()
        torch.cuda.synchronize()
        print(json.dumps({"shape": [a.scenes, a.peds], "trainer_ms_per_iteration": e0.elapsed_time(e1) / a.trainer,
                          "iterations": a.trainer, "best_k": tr.args.best_k}))
        return
    z = torch.randn(a.scenes, 8, device="cuda")
    dy = torch.randn(12, a.peds * a.scenes, 2, device="cuda")

    def run(n):
        for _ in range(n):
            g.zero_grad(set_to_none=True)
            y = g(obs, obs_rel, sse, obs_g, user_noise=z, scenes=sc)
            (y * dy).sum().backward()

    modes = (a.only,) if a.only else ("0", "1")
    times = {"0": [], "1": []}
    for mode in modes:
        os.environ["SGG_DEC_STEP"] = mode
        run(3)
    for r in range(a.rounds):
        for mode in modes:
            os.environ["SGG_DEC_STEP"] = mode
            run(2)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            run(a.iters)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.iters
            times[mode].append(ms)
            print("round %d SGG_DEC_STEP=%s: %.3f ms per forward + backward (%d iterations)" % (r, mode, ms, a.iters),
                  flush=True)
    if a.only:
        return
    print(json.dumps({"shape": [a.scenes, a.peds], "old_ms": times["0"], "new_ms": times["1"],
                      "old_fastest": min(times["0"]), "new_slowest": max(times["1"]),
                      "every_new_run_faster": max(times["1"]) < min(times["0"])}))


if __name__ == "__main__":
    main()
