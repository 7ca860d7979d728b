"""Device time of the step's small glue kernels at the bench shape (64 scenes
x 20 peds, T 12, best_k 20), each replayed 50x from a HIP graph; then the two
L2 glue kernels as glue segments of the discriminator encoder's continuation
launch (sgg_lstm_fwd_seg_glue) against the two launches they replace.
usage: python tools/glue_probe.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "group-gan-gcn-gat_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sgan import _native as N  # noqa: E402
from sgan import kernels as K  # noqa: E402
from sgan.scene import SceneIndex  # noqa: E402


def graph_time(fn, reps=50):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def glue_segments(dev, sc, gt, pred, mask, p, k):
    """The carriers of the training iteration -- steps 8 .. 19 of the
    discriminator encoder (H 48) on [12, 2560] (D-step, carries the best-of-k
    selection) and [12, 1280] (G-step, carries the L2 backward) -- alone,
    followed by the stand-alone glue launch, and with the glue segment."""
    lib = K._lib()
    H, Tl, t0 = 48, 20, 8
    S, T, Bg = sc.S, gt.shape[0], sc.B
    so = sc.scene_off
    best = torch.empty(S, device=dev, dtype=torch.int64)
    dpred, term, one = torch.empty(T, Bg, 2, device=dev), torch.empty(S, device=dev), torch.ones((), device=dev)
    sel = N.GlueSeg(N.GLUE_SELECT, N.ptr(pred), 0, N.ptr(gt), N.ptr(mask), mask.stride(0), N.ptr(so), S, T, Bg, k,
                    N.ptr(best), 0.0, None, None, 0, None)
    bwd = N.GlueSeg(N.GLUE_L2BWD, N.ptr(p), p.stride(0), N.ptr(gt), N.ptr(mask), mask.stride(0), N.ptr(so), S, T, Bg,
                    0, None, 1.0, N.ptr(one), N.ptr(dpred), 2 * Bg, N.ptr(term))
    alone = {
        "l2_select": lambda: N.check(lib.sgg_l2_select(N.ptr(pred), N.ptr(gt), N.ptr(mask), mask.stride(0), N.ptr(so),
                                                       S, T, Bg, k, N.ptr(best), N.stream_ptr()), "sgg_l2_select"),
        "l2_bwd_scenes": lambda: N.check(lib.sgg_l2_loss_bwd_scenes(
            N.ptr(p), p.stride(0), N.ptr(gt), N.ptr(mask), mask.stride(0), N.ptr(so), S, T, Bg, 1.0, N.ptr(one),
            N.ptr(dpred), 2 * Bg, N.ptr(term), N.stream_ptr()), "sgg_l2_loss_bwd_scenes")}
    for B, gname, gl in ((2 * Bg, "l2_select", sel), (Bg, "l2_bwd_scenes", bwd)):
        rel = torch.randn(Tl, B, 2, device=dev) * 0.5
        A, Whh, bias = (torch.randn(4 * H, 2, device=dev) * 0.3, torch.randn(4 * H, H, device=dev) * 0.1,
                        torch.randn(4 * H, device=dev) * 0.1)
        h_all = torch.zeros(Tl + 1, B, H, device=dev)
        c_all = torch.zeros(int(lib.sgg_lstm_state_floats(Tl, B, H, 1)), device=dev)
        act = torch.zeros(int(lib.sgg_lstm_state_floats(Tl, B, H, 0)), device=dev)

        def seg(t_from, steps):
            return N.LstmSeg(N.ptr(rel), N.ptr(A), N.ptr(Whh), N.ptr(bias), None, None, steps, B, B, t_from, Tl, B,
                             N.ptr(h_all), N.ptr(c_all), N.ptr(act), None, 0, None, 0, None)
        pre, cont = seg(0, t0), seg(t0, Tl - t0)
        N.check(lib.sgg_lstm_fwd_seg(N.ctypes.byref(pre), H, N.stream_ptr()), "sgg_lstm_fwd_seg")
        plain = lambda: N.check(lib.sgg_lstm_fwd_seg(N.ctypes.byref(cont), H, N.stream_ptr()), "sgg_lstm_fwd_seg")
        ride = lambda: N.check(lib.sgg_lstm_fwd_seg_glue(N.ctypes.byref(cont), H, N.ctypes.byref(gl), N.stream_ptr()),
                               "sgg_lstm_fwd_seg_glue")
        t_plain, t_glue = graph_time(plain), graph_time(alone[gname])
        t_two = graph_time(lambda: (alone[gname](), plain()))
        t_ride = graph_time(ride)
        print("lstm cont [12, %4d] H 48: alone %6.2f us, %s %5.2f us, both launches %6.2f us, one launch with the "
              "glue segment %6.2f us" % (B, t_plain, gname, t_glue, t_two, t_ride))


def main():
    dev = "cuda"
    S, n, T, k = 64, 20, 12, 20
    B = S * n
    sc = SceneIndex(np.arange(0, B + 1, n), dev)
    gt = torch.randn(T, B, 2, device=dev)
    pred = torch.randn(T, k * B, 2, device=dev)
    mask = (torch.rand(B, T, device=dev) > 0.1).float()
    p = torch.randn(T, B, 2, device=dev)
    with torch.no_grad():
        print("l2_select   %6.2f us" % graph_time(lambda: K.l2_select(pred, gt, mask, sc, k)))
        print("l2_loss fwd %6.2f us" % graph_time(lambda: K.l2_loss(p, gt, mask, sc, 1.0)))
    glue_segments(dev, sc, gt, pred, mask, p, k)
    for R, E in ((512, 64), (192, 16)):
        W, We, be = torch.randn(R, E, device=dev), torch.randn(E, 2, device=dev), torch.randn(E, device=dev)
        dA, db = torch.randn(R, 2, device=dev), torch.randn(R, device=dev)
        print("fold_bwd R=%d E=%d %6.2f us" % (R, E, graph_time(lambda: K.fold_bwd(W, We, be, dA, db))))
    sys.path.insert(0, ROOT)
    import bench
    g, d = bench.build_models(0)
    for name, mod, clip in (("G", g, 2.0), ("D", d, 0.0)):
        mod = mod.to(dev)
        ps = [q for q in mod.parameters() if q.requires_grad]
        for q in ps:
            q.grad = torch.randn_like(q) * 1e-2
        opt = K.ClipAdam(ps, lr=1e-4)
        opt.step(clip)   # state
        print("adam %s (%d tensors, %d floats, clip %.1f) %6.2f us" % (
            name, len(ps), sum(q.numel() for q in ps), clip, graph_time(lambda: opt.step(clip), reps=20)))
    x = torch.empty(1, device=dev)
    print("empty fill  %6.2f us" % graph_time(lambda: x.fill_(1.0)))


if __name__ == "__main__":
    main()
