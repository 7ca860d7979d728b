"""Micro-benchmarks of single kernels on the training shapes (HIP events on
the launch stream).  Usage: python tools/bench_kernels.py [pool|big|lstm|poolwide|poolbn|pooldrop|poolnorm|gatwide|gatdrop|...]
validate [a|b]: wall time of one check_accuracy pass, three routes; valkernel: sgg_val_metrics alone."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "group-gan-gcn-gat_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sgan import _native as N  # noqa: E402
from sgan import kernels as K  # noqa: E402
from sgan.scene import SceneIndex  # noqa: E402


def run(S, n, hd, bn, gpws=(0,), reps=20):
    torch.manual_seed(0)
    dev = "cuda"
    B = S * n
    sc = SceneIndex(np.arange(0, B + 1, n), dev)
    h = torch.randn(B, hd, device=dev)
    pos = torch.rand(B, 2, device=dev) * 15
    W1h = torch.randn(512, hd, device=dev) * 0.1
    A = torch.randn(512, 2, device=dev) * 0.3
    c = torch.randn(512, device=dev) * 0.1
    W2 = torch.randn(bn, 512, device=dev) * 0.05
    b2 = torch.randn(bn, device=dev) * 0.1
    U = K.xw_raw(h, W1h, c, trans_w=True)
    W2c = W2.contiguous()
    lib = N.load()
    flops = float(S * n * n) * 512 * (4 + 2 * bn)
    for gpw in gpws:
        sc.POOL_MAX_GPW = gpw
        sc.__dict__.pop("_pool_plans", None)
        chunks, nchunks, max_rows, g = sc.pool_plan(bn)
        out = torch.empty(B, bn, device=dev)
        am = torch.empty(B, bn, device=dev, dtype=torch.int32)
        call = lambda: N.check(lib.sgg_pool_fwd(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2c), N.ptr(b2),
                                                N.ptr(sc.scene_off), N.ptr(chunks), nchunks, max_rows, g, B, bn,
                                                sc.max_n, N.ptr(out), N.ptr(am), None, N.stream_ptr()), "pool")
        for _ in range(3):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / reps * 1e3
        print("pool_fwd S=%5d n=%2d bn=%2d chunks=%5d gpw=%d  %8.1f us  %6.1f TF/s" % (
            S, n, bn, nchunks, g, us, flops / us / 1e6), flush=True)


def poolwide(S, n, bn, reps=20):
    """The tiled pooling forward and backward (sgg_pool_fwd_wide /
    sgg_pool_bwd_wide) on S scenes of n peds; n <= 64: the resident kernels
    on the same operands next to them."""
    torch.manual_seed(0)
    dev = "cuda"
    B = S * n
    sc = SceneIndex(np.arange(0, B + 1, n), dev)
    U = torch.randn(B, 512, device=dev) * 0.3
    pos = torch.rand(B, 2, device=dev) * 15
    A = torch.randn(512, 2, device=dev) * 0.3
    W2 = torch.randn(bn, 512, device=dev) * 0.05
    b2 = torch.randn(bn, device=dev) * 0.1
    dout = torch.randn(B, bn, device=dev)
    lib = N.load()
    flops = float(S * n * n) * 512 * (4 + 2 * bn)
    out = torch.empty(B, bn, device=dev)
    am = torch.empty(B, bn, device=dev, dtype=torch.int32)
    dU = torch.empty(B, 512, device=dev)
    P = bn * 512 + 1024 + bn
    forms = [("wide", True)] + ([("resident", False)] if n <= 64 else [])
    for name, wide in forms:
        chunks, nchunks, max_rows, g = sc.pool_plan(bn, wide=wide)
        if wide:
            fwd = lambda: N.check(lib.sgg_pool_fwd_wide(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2), N.ptr(b2),
                                                        N.ptr(sc.scene_off), N.ptr(chunks), nchunks, max_rows, g, B,
                                                        bn, sc.max_n, N.ptr(out), N.ptr(am), N.stream_ptr()), "fwd")
            part = torch.empty(lib.sgg_pool_bwd_wide_grid(S, n), P, device=dev)
            bwd = lambda: N.check(lib.sgg_pool_bwd_wide(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2), N.ptr(out),
                                                        N.ptr(am), N.ptr(dout), N.ptr(sc.scene_off), S, B, bn,
                                                        sc.max_n, N.ptr(dU), N.ptr(part), N.stream_ptr()), "bwd")
        else:
            fwd = lambda: N.check(lib.sgg_pool_fwd(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2), N.ptr(b2),
                                                   N.ptr(sc.scene_off), N.ptr(chunks), nchunks, max_rows, g, B, bn,
                                                   sc.max_n, N.ptr(out), N.ptr(am), None, N.stream_ptr()), "fwd")
            part = torch.empty(lib.sgg_pool_bwd_grid(S), P, device=dev)
            bwd = lambda: N.check(lib.sgg_pool_bwd(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2), N.ptr(out), N.ptr(am),
                                                   N.ptr(dout), N.ptr(sc.scene_off), S, B, bn, sc.max_n, N.ptr(dU),
                                                   N.ptr(part), N.stream_ptr()), "bwd")
        uf = timeit(fwd, reps)
        ub = timeit(bwd, reps)
        print("pool %-8s S=%3d n=%4d bn=%2d chunks=%5d rows=%2d gpw=%d  fwd %8.1f us %6.1f TF/s %5.3f ns/pair  "
              "bwd %8.1f us" % (name, S, n, bn, nchunks, max_rows, g, uf, flops / uf / 1e6, uf * 1e3 / (S * n * n), ub),
              flush=True)


def poolbn(S, n, bn, reps=20):
    """The column-tiled pooling forward and backward (sgg_pool_fwd_bn /
    sgg_pool_bwd_bn, any bottleneck_dim up to 1024) on S scenes of n peds; at
    bn = 64 the wide kernels (sgg_pool_fwd_wide / sgg_pool_bwd_wide) on the
    same operands next to them.  Backward: with weight gradients (both
    launches) and with part = NULL (the dU launch alone)."""
    torch.manual_seed(0)
    dev = "cuda"
    B = S * n
    sc = SceneIndex(np.arange(0, B + 1, n), dev)
    U = torch.randn(B, 512, device=dev) * 0.3
    pos = torch.rand(B, 2, device=dev) * 15
    A = torch.randn(512, 2, device=dev) * 0.3
    W2 = torch.randn(bn, 512, device=dev) * 0.05
    b2 = torch.randn(bn, device=dev) * 0.1
    dout = torch.randn(B, bn, device=dev)
    lib = N.load()
    tiles = (bn + 63) // 64
    flops = float(S * n * n) * 512 * (4 * tiles + 2 * bn)
    out = torch.empty(B, bn, device=dev)
    am = torch.empty(B, bn, device=dev, dtype=torch.int32)
    dU = torch.empty(B, 512, device=dev)
    P = bn * 512 + 1024 + bn
    for name in ["bn"] + (["wide"] if bn == 64 else []):
        if name == "bn":
            chunks, nchunks, max_rows, g = sc.pool_plan(bn, family_bn=True)
            fwd = lambda: N.check(lib.sgg_pool_fwd_bn(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2), N.ptr(b2),
                                                      N.ptr(sc.scene_off), N.ptr(chunks), nchunks, max_rows, g, B, bn,
                                                      sc.max_n, N.ptr(out), N.ptr(am), N.stream_ptr()), "fwd")
            part = torch.empty(lib.sgg_pool_bwd_bn_ws_floats(S, B, bn, n), device=dev)
            bwd_p = lambda p, nf: N.check(lib.sgg_pool_bwd_bn(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2), N.ptr(out),
                                                              N.ptr(am), N.ptr(dout), N.ptr(sc.scene_off), S, B, bn,
                                                              sc.max_n, N.ptr(dU), N.ptr(p), nf, N.stream_ptr()),
                                          "bwd")
            bwd, bwd0 = (lambda: bwd_p(part, part.numel())), (lambda: bwd_p(None, 0))
        else:
            chunks, nchunks, max_rows, g = sc.pool_plan(bn, wide=True)
            fwd = lambda: N.check(lib.sgg_pool_fwd_wide(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2), N.ptr(b2),
                                                        N.ptr(sc.scene_off), N.ptr(chunks), nchunks, max_rows, g, B,
                                                        bn, sc.max_n, N.ptr(out), N.ptr(am), N.stream_ptr()), "fwd")
            part = torch.empty(lib.sgg_pool_bwd_wide_grid(S, n), P, device=dev)
            bwd_p = lambda p: N.check(lib.sgg_pool_bwd_wide(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2), N.ptr(out),
                                                            N.ptr(am), N.ptr(dout), N.ptr(sc.scene_off), S, B, bn,
                                                            sc.max_n, N.ptr(dU), N.ptr(p), N.stream_ptr()), "bwd")
            bwd, bwd0 = (lambda: bwd_p(part)), (lambda: bwd_p(None))
        uf = timeit(fwd, reps)
        ub = timeit(bwd, reps)
        ub0 = timeit(bwd0, reps)
        print("pool %-4s S=%3d n=%4d bn=%4d tiles=%2d chunks=%5d rows=%2d  fwd %8.1f us %6.1f TF/s %6.3f ns/pair  "
              "bwd %8.1f us  bwd(dU only) %8.1f us  ws %.1f MB" % (
                  name, S, n, bn, tiles, nchunks, max_rows, uf, flops / uf / 1e6, uf * 1e3 / (S * n * n), ub, ub0,
                  part.numel() * 4 / 1e6), flush=True)


def pooldrop(S, n, bn, p=0.5, reps=20):
    """The dropout form of the column-tiled pooling kernels (sgg_pool_fwd_bn_drop
    / sgg_pool_bwd_bn_drop at probability p) beside the plain launches
    (sgg_pool_fwd_bn / sgg_pool_bwd_bn) on the same operands: forward, backward
    with weight gradients, dU-only backward; each backward on its own
    forward's out / argmax.  Device events around reps launches after 3
    warm-ups (timeit)."""
    torch.manual_seed(0)
    dev = "cuda"
    B = S * n
    sc = SceneIndex(np.arange(0, B + 1, n), dev)
    U = torch.randn(B, 512, device=dev) * 0.3
    pos = torch.rand(B, 2, device=dev) * 15
    A = torch.randn(512, 2, device=dev) * 0.3
    W2 = torch.randn(bn, 512, device=dev) * 0.05
    b2 = torch.randn(bn, device=dev) * 0.1
    dout = torch.randn(B, bn, device=dev)
    lib = N.load()
    out = torch.empty(B, bn, device=dev)
    am = torch.empty(B, bn, device=dev, dtype=torch.int32)
    dU = torch.empty(B, 512, device=dev)
    chunks, nchunks, max_rows, g = sc.pool_plan(bn, family_bn=True)
    part = torch.empty(lib.sgg_pool_bwd_bn_ws_floats(S, B, bn, n), device=dev)
    fargs = (N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2), N.ptr(b2), N.ptr(sc.scene_off), N.ptr(chunks), nchunks,
             max_rows, g, B, bn, sc.max_n, N.ptr(out), N.ptr(am))
    bargs = (N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2), N.ptr(out), N.ptr(am), N.ptr(dout), N.ptr(sc.scene_off), S, B,
             bn, sc.max_n, N.ptr(dU))
    drop = (p, 12345, 0, None)
    res = {}
    for name, extra, ffn, bfn in (("plain", (), lib.sgg_pool_fwd_bn, lib.sgg_pool_bwd_bn),
                                  ("drop", drop, lib.sgg_pool_fwd_bn_drop, lib.sgg_pool_bwd_bn_drop)):
        fwd = lambda: N.check(ffn(*fargs, *extra, N.stream_ptr()), "fwd")
        bwd = lambda: N.check(bfn(*bargs, N.ptr(part), part.numel(), *extra, N.stream_ptr()), "bwd")
        bwd0 = lambda: N.check(bfn(*bargs, None, 0, *extra, N.stream_ptr()), "bwd")
        res[name] = (timeit(fwd, reps), timeit(bwd0, reps), timeit(bwd, reps))
    for name in ("plain", "drop"):
        uf, ub0, ub = res[name]
        print("pool %-5s S=%3d n=%4d bn=%4d p=%.2f  fwd %8.1f us  bwd(dU only) %8.1f us  bwd %8.1f us" % (
            name, S, n, bn, p if name == "drop" else 0.0, uf, ub0, ub), flush=True)
    print("pool ratio S=%3d n=%4d bn=%4d        fwd %8.2f x   bwd(dU only) %8.2f x   bwd %8.2f x" % (
        (S, n, bn) + tuple(d / q for d, q in zip(res["drop"], res["plain"]))), flush=True)


def poolnorm(S, n, bn, reps=10):
    """The batch-norm pooling kernels in train() (sgg_pool_norm_fwd: first-layer
    statistics, second-layer statistics, apply; sgg_pool_norm_bwd: the dense
    pass and the finish, with and without weight gradients) beside the plain
    column-tiled launches (sgg_pool_fwd_bn / sgg_pool_bwd_bn) on the same
    operands.  Device events around reps launches after 3 warm-ups (timeit)."""
    torch.manual_seed(0)
    dev = "cuda"
    B = S * n
    sc = SceneIndex(np.arange(0, B + 1, n), dev)
    U = torch.randn(B, 512, device=dev) * 0.3
    pos = torch.rand(B, 2, device=dev) * 15
    A = torch.randn(512, 2, device=dev) * 0.3
    W2 = torch.randn(bn, 512, device=dev) * 0.05
    b2 = torch.randn(bn, device=dev) * 0.1
    g1, t1 = 1 + 0.3 * torch.randn(512, device=dev), 0.3 * torch.randn(512, device=dev)
    g2, t2 = 1 + 0.3 * torch.randn(bn, device=dev), 0.3 * torch.randn(bn, device=dev)
    dout = torch.randn(B, bn, device=dev)
    lib = N.load()
    out = torch.empty(B, bn, device=dev)
    am = torch.empty(B, bn, device=dev, dtype=torch.int32)
    dU = torch.empty(B, 512, device=dev)
    chunks, nchunks, max_rows, g = sc.pool_plan(bn, family_bn=True)
    part = torch.empty(lib.sgg_pool_bwd_bn_ws_floats(S, B, bn, n), device=dev)
    fwd = lambda: N.check(lib.sgg_pool_fwd_bn(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2), N.ptr(b2), N.ptr(sc.scene_off),
                                              N.ptr(chunks), nchunks, max_rows, g, B, bn, sc.max_n, N.ptr(out),
                                              N.ptr(am), N.stream_ptr()), "fwd")
    bwd_p = lambda p, nf: N.check(lib.sgg_pool_bwd_bn(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2), N.ptr(out), N.ptr(am),
                                                      N.ptr(dout), N.ptr(sc.scene_off), S, B, bn, sc.max_n, N.ptr(dU),
                                                      N.ptr(p), nf, N.stream_ptr()), "bwd")
    plain = (timeit(fwd, reps), timeit(lambda: bwd_p(None, 0), reps), timeit(lambda: bwd_p(part, part.numel()), reps))
    Un, An = torch.empty(B, 512, device=dev), torch.empty(S, 1024, device=dev)
    mu1, var1 = torch.empty(S, 512, device=dev), torch.empty(S, 512, device=dev)
    mu2, var2 = torch.empty(S, bn, device=dev), torch.empty(S, bn, device=dev)
    dpos = torch.empty(B, 2, device=dev)
    ws = torch.empty(lib.sgg_pool_norm_bwd_ws_floats(S, B, bn), device=dev)
    nfwd = lambda: N.check(lib.sgg_pool_norm_fwd(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(g1), N.ptr(t1), N.ptr(W2),
                                                 N.ptr(b2), N.ptr(g2), N.ptr(t2), N.ptr(sc.scene_off), S, B, bn, n, n,
                                                 1e-5, 1e-5, N.ptr(Un), N.ptr(An), N.ptr(mu1), N.ptr(var1), N.ptr(mu2),
                                                 N.ptr(var2), N.ptr(out), N.ptr(am), N.stream_ptr()), "norm fwd")
    nbwd = lambda w: N.check(lib.sgg_pool_norm_bwd(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(g1), N.ptr(W2), N.ptr(b2),
                                                   N.ptr(g2), N.ptr(t2), N.ptr(Un), N.ptr(An), N.ptr(mu1), N.ptr(var1),
                                                   N.ptr(mu2), N.ptr(var2), N.ptr(out), N.ptr(am), N.ptr(dout),
                                                   N.ptr(sc.scene_off), S, B, bn, n, n, 1e-5, 1e-5, w, N.ptr(dU),
                                                   N.ptr(dpos), N.ptr(ws), ws.numel(), N.stream_ptr()), "norm bwd")
    norm = (timeit(nfwd, reps), timeit(lambda: nbwd(0), reps), timeit(lambda: nbwd(1), reps))
    for name, (uf, ub0, ub) in (("plain", plain), ("norm", norm)):
        print("pool %-5s S=%3d n=%4d bn=%4d  fwd %10.1f us  bwd(dU only) %10.1f us  bwd %10.1f us" % (
            name, S, n, bn, uf, ub0, ub), flush=True)
    print("pool ratio S=%3d n=%4d bn=%4d  fwd %10.2f x   bwd(dU only) %10.2f x   bwd %10.2f x  ws %.1f MB" % (
        (S, n, bn) + tuple(d / q for d, q in zip(norm, plain)) + (ws.numel() * 4 / 1e6,)), flush=True)


def gatwide(S, n, heads, F, reps=20):
    """The tiled attention forward and backward (sgg_gat_fwd_wide /
    sgg_gat_bwd_wide, parameter gradients finished) on S complete-graph
    segments of n nodes; n <= 128: the resident kernels (sgg_gat_fwd_ex /
    sgg_gat_bwd_ex) on the same operands next to them."""
    torch.manual_seed(0)
    dev = "cuda"
    B, HF = S * n, heads * F
    off = torch.arange(0, B + 1, n, dtype=torch.int32, device=dev)
    wh = torch.randn(B, HF, device=dev)
    a_s, a_d = torch.randn(heads, F, device=dev) * 0.5, torch.randn(heads, F, device=dev) * 0.5
    bias = torch.randn(F, device=dev) * 0.1
    dy = torch.randn(B, HF, device=dev)
    y, hp, dWh = (torch.empty(B, HF, device=dev) for _ in range(3))
    da_s, da_d, db = torch.empty_like(a_s), torch.empty_like(a_d), torch.empty_like(bias)
    lib = N.load()
    for name, wide in [("wide", True)] + ([("resident", False)] if n <= 128 else []):
        if wide:
            work = torch.empty(int(lib.sgg_gat_wide_work_floats(B, S, heads, F, n)), device=dev)
            fwd = lambda: N.check(lib.sgg_gat_fwd_wide(N.ptr(wh), heads, N.ptr(a_s), N.ptr(a_d), F, N.ptr(bias), None,
                                                       N.ptr(off), S, B, F, 0.2, 1, 1, n, N.ptr(hp), N.ptr(y), HF,
                                                       N.ptr(work), N.stream_ptr()), "fwd")
            bwd = lambda: N.check(lib.sgg_gat_bwd_wide(N.ptr(wh), heads, N.ptr(a_s), N.ptr(a_d), F, None, N.ptr(off),
                                                       S, B, F, 0.2, 1, 1, n, N.ptr(hp), N.ptr(y), N.ptr(dy), HF,
                                                       N.ptr(dWh), None, None, N.ptr(da_s), N.ptr(da_d), N.ptr(db),
                                                       N.ptr(work), N.stream_ptr()), "bwd")
        else:
            work = torch.empty(int(lib.sgg_gat_bwd_ex_work_bytes(S, heads, F)), device=dev, dtype=torch.uint8)
            fwd = lambda: N.check(lib.sgg_gat_fwd_ex(N.ptr(wh), heads, N.ptr(a_s), N.ptr(a_d), N.ptr(bias), None,
                                                     N.ptr(off), S, B, F, 0.2, 1, 1, n, N.ptr(hp), N.ptr(y), HF,
                                                     N.stream_ptr()), "fwd")
            bwd = lambda: N.check(lib.sgg_gat_bwd_ex(N.ptr(wh), heads, N.ptr(a_s), N.ptr(a_d), None, N.ptr(off), S, B,
                                                     F, 0.2, 1, 1, n, N.ptr(hp), N.ptr(y), N.ptr(dy), HF, N.ptr(dWh),
                                                     N.ptr(da_s), N.ptr(da_d), N.ptr(db), N.ptr(work),
                                                     N.stream_ptr()), "bwd")
        uf = timeit(fwd, reps)
        ub = timeit(bwd, reps)
        pairs = float(S) * n * n * heads   # (i, j, head)
        print("gat %-8s S=%3d n=%4d heads=%d F=%3d  fwd %8.1f us %6.3f ns/pair  bwd %8.1f us %6.3f ns/pair" % (
            name, S, n, heads, F, uf, uf * 1e3 / pairs, ub, ub * 1e3 / pairs), flush=True)


def gatdrop(S, n, heads, F, p=0.3, reps=2000, rounds=5):
    """The attention kernels with dropout (sgg_gat_fwd_drop / sgg_gat_bwd_drop
    at probability p) next to sgg_gat_fwd_ex / sgg_gat_bwd_ex on the same
    operands (S complete-graph segments of n <= 128 nodes, ELU epilogue,
    parameter gradients finished): the four calls alternate over `rounds`
    windows of `reps` back-to-back launches; median (min .. max) per call."""
    torch.manual_seed(0)
    dev = "cuda"
    B, HF = S * n, heads * F
    off = torch.arange(0, B + 1, n, dtype=torch.int32, device=dev)
    wh = torch.randn(B, HF, device=dev)
    a_s, a_d = torch.randn(heads, F, device=dev) * 0.5, torch.randn(heads, F, device=dev) * 0.5
    bias = torch.randn(F, device=dev) * 0.1
    dy = torch.randn(B, HF, device=dev)
    y, hp, dWh = (torch.empty(B, HF, device=dev) for _ in range(3))
    da_s, da_d, db = torch.empty_like(a_s), torch.empty_like(a_d), torch.empty_like(bias)
    lib = N.load()
    work = torch.empty(int(lib.sgg_gat_bwd_ex_work_bytes(S, heads, F)), device=dev, dtype=torch.uint8)
    seed, st = 0x9E3779B97F4A7C15, N.stream_ptr()
    calls = {
        "fwd_ex": lambda: N.check(lib.sgg_gat_fwd_ex(N.ptr(wh), heads, N.ptr(a_s), N.ptr(a_d), N.ptr(bias), None,
                                                     N.ptr(off), S, B, F, 0.2, 1, 1, n, N.ptr(hp), N.ptr(y), HF, st),
                                  "fwd"),
        "fwd_drop": lambda: N.check(lib.sgg_gat_fwd_drop(N.ptr(wh), heads, N.ptr(a_s), N.ptr(a_d), F, N.ptr(bias),
                                                         None, N.ptr(off), S, B, F, 0.2, 1, 1, n, N.ptr(hp), N.ptr(y),
                                                         HF, p, seed, 1, 0, 0, None, st), "fwd_drop"),
        "bwd_ex": lambda: N.check(lib.sgg_gat_bwd_ex(N.ptr(wh), heads, N.ptr(a_s), N.ptr(a_d), None, N.ptr(off), S, B,
                                                     F, 0.2, 1, 1, n, N.ptr(hp), N.ptr(y), N.ptr(dy), HF, N.ptr(dWh),
                                                     N.ptr(da_s), N.ptr(da_d), N.ptr(db), N.ptr(work), st), "bwd"),
        "bwd_drop": lambda: N.check(lib.sgg_gat_bwd_drop(N.ptr(wh), heads, N.ptr(a_s), N.ptr(a_d), F, None,
                                                         N.ptr(off), S, B, F, 0.2, 1, 1, n, N.ptr(hp), N.ptr(y),
                                                         N.ptr(dy), HF, N.ptr(dWh), None, None, N.ptr(da_s),
                                                         N.ptr(da_d), N.ptr(db), N.ptr(work), p, seed, 1, 0, 0, None,
                                                         st), "bwd_drop"),
    }
    us = {k: [] for k in calls}
    for _ in range(rounds):
        for k, c in calls.items():
            us[k].append(timeit(c, reps))
    pairs = float(S) * n * n * heads
    print("gat dropout p=%.1f S=%3d n=%4d heads=%d F=%3d (%d x %d launches each)" % (p, S, n, heads, F, rounds, reps))
    for k, v in us.items():
        print("  %-8s %7.2f us (%.2f .. %.2f)  %6.3f ns/pair" % (k, float(np.median(v)), min(v), max(v),
                                                                  float(np.median(v)) * 1e3 / pairs), flush=True)


def lstm(B, T, H, decoder, reps=10, save=False):
    torch.manual_seed(0)
    dev = "cuda"
    lib = N.load()
    rel = torch.randn(1 if decoder else T, B, 2, device=dev).squeeze(0) * 0.3
    A = torch.randn(4 * H, 2, device=dev) * 0.3
    Whh = torch.randn(4 * H, H, device=dev) * 0.2
    bias = torch.randn(4 * H, device=dev) * 0.1
    h0 = torch.randn(B, H, device=dev) * 0.5
    Wp = torch.randn(2, H, device=dev) * 0.2
    bp = torch.randn(2, device=dev) * 0.1
    h_all = torch.empty(T + 1, B, H, device=dev)
    c_all = torch.empty(T + 1, B, H, device=dev)
    act = torch.empty(T, B, 4 * H, device=dev)
    rel_out = torch.empty(T, B, 2, device=dev)
    call = lambda: N.check(lib.sgg_lstm_fwd(N.ptr(rel), N.ptr(A), N.ptr(Whh), N.ptr(bias), N.ptr(h0), None,
                                            N.ptr(Wp), N.ptr(bp), T, B, H, int(decoder), N.ptr(h_all), N.ptr(c_all),
                                            N.ptr(act) if save else None, N.ptr(rel_out), N.stream_ptr()), "lstm")
    for _ in range(3):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / reps * 1e3
    flops = 2.0 * T * B * 4 * H * (H + 2)
    print("lstm_fwd B=%6d T=%2d H=%2d dec=%d save=%d  %8.1f us  %6.1f TF/s (gate GEMM)" % (
        B, T, H, decoder, save, us, flops / us / 1e6), flush=True)


def lstm_bwd_w(B, T, H, reps=20):
    """The four-wave backward with in-kernel weight gradients (the
    discriminator encoder's launch: sgg_lstm_bwd with wpart), after a saving
    forward; HIP events around back-to-back launches."""
    torch.manual_seed(0)
    dev = "cuda"
    lib = N.load()
    rel = torch.randn(T, B, 2, device=dev) * 0.3
    A = torch.randn(4 * H, 2, device=dev) * 0.3
    Whh = torch.randn(4 * H, H, device=dev) * 0.2
    bias = torch.randn(4 * H, device=dev) * 0.1
    h0 = torch.randn(B, H, device=dev) * 0.5
    h_all = torch.empty(T + 1, B, H, device=dev)
    c_all = torch.empty(int(lib.sgg_lstm_state_floats(T, B, H, 1)), device=dev)
    act = torch.empty(int(lib.sgg_lstm_state_floats(T, B, H, 0)), device=dev)
    drel_in = torch.empty(T, B, 2, device=dev)
    dhl = torch.randn(B, H, device=dev)
    rows = int(lib.sgg_lstm_wpart_rows(H, B))
    wpart = torch.empty(rows * (4 * H * H + 12 * H + 2 * H + 2), device=dev)
    N.check(lib.sgg_lstm_fwd(N.ptr(rel), N.ptr(A), N.ptr(Whh), N.ptr(bias), N.ptr(h0), None, None, None, T, B, H, 0,
                             N.ptr(h_all), N.ptr(c_all), N.ptr(act), None, N.stream_ptr()), "lstm_fwd")
    bwd = lambda: N.check(lib.sgg_lstm_bwd(N.ptr(A), N.ptr(Whh), None, N.ptr(h_all), N.ptr(c_all), N.ptr(act),
                                           N.ptr(rel), None, N.ptr(dhl), None, T, B, H, 0, None, None,
                                           N.ptr(drel_in), None, N.ptr(wpart), N.stream_ptr()), "lstm_bwd")
    us = timeit(bwd, reps)
    # the form without input gradients (drel_in NULL), where the library has it
    nodx = lambda: lib.sgg_lstm_bwd(N.ptr(A), N.ptr(Whh), None, N.ptr(h_all), N.ptr(c_all), N.ptr(act), N.ptr(rel),
                                    None, N.ptr(dhl), None, T, B, H, 0, None, None, None, None, N.ptr(wpart),
                                    N.stream_ptr())
    us0 = timeit(nodx, reps) if nodx() == 0 else float("nan")
    print("lstm_bwd+w B=%5d T=%2d H=%2d  %7.2f us  no drel_in %7.2f us  (%s)" % (
        B, T, H, us, us0, os.environ.get("SGG_LIB", "tree")), flush=True)


def timeit(call, reps=20):
    for _ in range(3):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def dense():
    """sgg_xw / sgg_xtw on the training step's shapes."""
    dev = "cuda"
    for (M, Kd, Nn, tw) in [(2560, 40, 72, False), (2560, 72, 16, False), (1280, 32, 512, True), (2560, 64, 48, True),
                            (25600, 40, 72, False), (1280, 512, 32, False), (2560, 48, 64, True)]:
        x = torch.randn(M, Kd, device=dev)
        w = torch.randn(Nn, Kd, device=dev) if tw else torch.randn(Kd, Nn, device=dev)
        us = timeit(lambda: K.xw_raw(x, w, None, trans_w=tw))
        print("xw   M=%6d K=%4d N=%4d trans=%d  %7.1f us" % (M, Kd, Nn, tw, us), flush=True)
    for (R, M, Nn) in [(1280, 32, 512), (2560, 48, 512), (51200, 48, 192), (20480, 32, 128), (2560, 40, 72),
                       (1280, 64, 1), (2560, 2, 192)]:
        X = torch.randn(R, M, device=dev)
        Y = torch.randn(R, Nn, device=dev)
        us = timeit(lambda: K.xtw(X, Y, colsum=True))
        print("xtw  R=%6d M=%4d N=%4d  %7.1f us  (splits %d)" % (R, M, Nn, us, N.load().sgg_xtw_splits(R, M, Nn)),
              flush=True)


def _val_models():
    """The default (gat) generator and discriminator, seeded random weights."""
    from sgan.models import TrajectoryDiscriminator, TrajectoryGenerator
    torch.manual_seed(0)
    g = TrajectoryGenerator(8, 12, embedding_dim=16, encoder_h_dim=32, decoder_h_dim=32, mlp_dim=64,
                            noise_dim=(8,), noise_mix_type="global", pooling_type="pool_net",
                            pool_every_timestep=False, bottleneck_dim=8, batch_norm=False,
                            n_units=[40, 16, 40], n_heads=1, dropout1=0.0, alpha=0.2)
    d = TrajectoryDiscriminator(8, 12, embedding_dim=16, h_dim=48, mlp_dim=64, batch_norm=False, d_type="global")
    return g.cuda(), d.cuda()


class _ValArgs:
    obs_len, pred_len, skip, delim, batch_size, loader_num_workers, num_samples_check = 8, 12, 1, "tab", 64, 0, 5000


def validate(rounds=5, split=("zara1", "test"), only=None):
    """One check_accuracy pass over zara1/test at batch 64, gat generator:
    (a) the torch restatement of the reference loop (tests/_check_accuracy_ref
        .py) on the GPU modules -- what a user of the fast trainers ran before
        sgan.validate existed;
    (b) sgan.validate.check_accuracy with the host DataLoader;
    (c) the same with the device-resident loader.
    The three alternate over `rounds` rounds in this process; wall time around
    a final torch.cuda.synchronize().  only = "a" / "b": one pass of that
    route and nothing else (a kernel-trace run)."""
    import random
    import time
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _check_accuracy_ref import check_accuracy_ref
    from sgan.data.device import device_data_loader
    from sgan.data.loader import data_loader
    from sgan.validate import check_accuracy
    g, d = _val_models()
    path = os.path.join(ROOT, "tests", "golden", "datasets_group", *split)
    _, host = data_loader(_ValArgs, path)
    _, dev = device_data_loader(_ValArgs, path, "cuda")
    routes = {"a": lambda: check_accuracy_ref(_ValArgs, host, g, d, device="cuda"),
              "b": lambda: check_accuracy(_ValArgs, host, g, d),
              "c": lambda: check_accuracy(_ValArgs, dev, g, d)}

    def timed(k):
        torch.manual_seed(1)
        random.seed(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = routes[k]()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, m

    if only:
        ms, m = timed(only)   # (cold: the trace is about launch counts)
        print("validate route %s: %d batches, %.1f ms, ade %.6f" % (only, len(host), ms, m["ade"]), flush=True)
        return
    for k in routes:          # warm-up: allocator, folds, dataset table
        timed(k)
    ms = {k: [] for k in routes}
    for r in range(rounds):
        vals = {}
        for k in routes:
            t, m = timed(k)
            ms[k].append(t)
            vals[k] = m
        print("validate round %d: (a) torch restatement %8.2f ms  (b) check_accuracy %8.2f ms  (c) device loader "
              "%8.2f ms   ade a %.6f b %.6f c %.6f" % (r, ms["a"][-1], ms["b"][-1], ms["c"][-1], vals["a"]["ade"],
                                                        vals["b"]["ade"], vals["c"]["ade"]), flush=True)
    print("validate medians over %d rounds, %d batches of 64 sequences: (a) %.2f ms  (b) %.2f ms  (c) %.2f ms; "
          "(b) faster than (a) in every round: %s" % (rounds, len(host), float(np.median(ms["a"])),
                                                      float(np.median(ms["b"])), float(np.median(ms["c"])),
                                                      all(b < a for a, b in zip(ms["a"], ms["b"]))), flush=True)


def valkernel(B, T=12, reps=200, rounds=5):
    """sgg_val_metrics alone (with scores): back-to-back launches, median of `rounds` windows."""
    torch.manual_seed(0)
    dev = "cuda"
    lib = N.load()
    pred_rel, gt, gt_rel = (torch.randn(T, B, 2, device=dev) for _ in range(3))
    start, nl = torch.randn(B, 2, device=dev), (torch.rand(B, device=dev) < 0.4).float()
    mask = torch.ones(B, 8 + T, device=dev)[:, 8:]
    scores = torch.randn(2 * B, device=dev)
    acc = torch.zeros(N.VAL_SLOTS, dtype=torch.float64, device=dev)
    work = torch.zeros(int(lib.sgg_val_metrics_work_floats(B)), device=dev)
    call = lambda: N.check(lib.sgg_val_metrics(N.ptr(pred_rel), N.ptr(gt), N.ptr(gt_rel), N.ptr(start), N.ptr(mask),
                                               8 + T, N.ptr(nl), N.ptr(scores), 0.9, T, B, N.ptr(acc), N.ptr(work),
                                               N.stream_ptr()), "sgg_val_metrics")
    us = [timeit(call, reps) for _ in range(rounds)]
    print("sgg_val_metrics B=%6d T=%2d  %6.2f us (%.2f .. %.2f), %d workgroups" % (
        B, T, float(np.median(us)), min(us), max(us), (B + 255) // 256), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "pool"
    if what == "validate":   # the validation pass: torch restatement against sgan.validate.check_accuracy
        validate(only=sys.argv[2] if len(sys.argv) > 2 else None)
        sys.exit(0)
    if what == "valkernel":  # the metrics launch alone: one real batch's peds, and the synthetic leg's
        for B in (450, 20480):
            valkernel(B)
        sys.exit(0)
    if what == "big":     # one config (profiling)
        run(1280, 20, 32, 8, reps=5)
        sys.exit(0)
    if what == "dense":
        dense()
        sys.exit(0)
    if what == "roll":    # the no-grad decoder rollout against its batch (waves per SIMD)
        for B in (4096, 8192, 16384, 20480, 25600, 32768, 49152):
            lstm(B, 12, 32, True, reps=20)
        sys.exit(0)
    if what == "rollb":   # the rollout over batch sizes: waves per SIMD 0.5 .. 2
        for B in (8192, 16384, 20480, 25600, 26880, 32768):
            lstm(B, 12, 32, True, reps=10)
        sys.exit(0)
    if what == "roll2":   # one / two waves per SIMD (counter runs: tools/gpu_sq_rollwaves.sh)
        for B in (16384, 25600):
            lstm(B, 12, 32, True, reps=5)
        sys.exit(0)
    if what == "mwf":     # the four-wave forward of the discriminator's encoder (H 48), saving / not
        for B in (2560, 1280):
            for save in (True, False):
                lstm(B, 12, 48, False, save=save)
        sys.exit(0)
    if what == "dpool":   # the discriminator's pooling (bn 48) at the training shapes
        for (S, n) in ((128, 20), (64, 20), (256, 20), (128, 57)):
            run(S, n, 48, 48)
        sys.exit(0)
    if what == "poolwide":   # the tiled pooling kernels above 64 peds, next to the resident ones at 64
        for bn in (8, 48):
            # (64 x 128: enough rows for chunks above gpw rows -- several passes per j-tile)
            for (S, n) in ((64, 64), (32, 128), (8, 256), (1, 1024), (64, 128)):
                poolwide(S, n, bn)
        sys.exit(0)
    if what == "poolbn":   # the column-tiled pooling kernels: bn 64 next to the wide kernels, 2 and 16 tiles
        for (S, n) in ((64, 20), (512, 20)):
            for bn in (64, 128, 1024):
                poolbn(S, n, bn)
        sys.exit(0)
    if what == "pooldrop":   # what the two dropout masks cost inside the column-tiled pooling kernels
        for bn in (8, 64, 1024):
            pooldrop(64, 20, bn)
        sys.exit(0)
    if what == "poolnorm":   # the batch-norm pooling kernels in train() beside the plain column-tiled launches
        for S in (64, 512):
            for bn in (8, 64, 1024):
                poolnorm(S, 20, bn)
        sys.exit(0)
    if what == "gatwide":   # the tiled attention kernels above 128 nodes, next to the resident ones at 128
        for (S, n) in ((32, 128), (8, 256), (1, 1024)):
            for (heads, F) in ((1, 72), (4, 16)):
                gatwide(S, n, heads, F)
        sys.exit(0)
    if what == "gatdrop":   # what the mask generator costs inside the resident attention kernels
        for F in (72, 16):
            gatdrop(64, 64, 1, F)
        sys.exit(0)
    if what == "lbwd":    # the discriminator encoder's backward with weight gradients
        for (B, T, H) in ((2560, 20, 48), (1280, 20, 48), (2560, 12, 32), (1280, 8, 32), (8192, 20, 48)):
            lstm_bwd_w(B, T, H)
        sys.exit(0)
    if what == "lstm":
        for B in (1280, 2560, 4096, 25600):
            for save in (False, True):
                lstm(B, 8, 32, False, save=save)
                lstm(B, 12, 32, True, save=save)
        for B in (1280, 2560):
            lstm(B, 20, 48, False, save=True)
        sys.exit(0)
    run(1280, 20, 32, 8, gpws=(0, 1, 2, 4))
    run(64, 20, 32, 8, gpws=(0, 1, 2))
    run(128, 20, 32, 8)
    run(128, 20, 48, 48)
    run(256, 57, 32, 8)
