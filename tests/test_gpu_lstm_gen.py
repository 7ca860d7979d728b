"""LSTM sequences at hidden sizes outside {16, 32, 48, 64}: the generic kernel
family (lstm_gen.hip, 1 <= H <= 128) from the kernels up to the trainers.

The kernel tests judge the fp32 HIP path by the error the oracle's own fp32
CPU modules make against the same modules in float64:
    |HIP - f64| <= 4 |CPU32 - f64| + 1e-6 max|f64|     (max over the tensor)
The factor covers a different summation order (4-deep MFMA k-steps against a
CPU GEMM) and hardware exponentials.  Measured ratios per H: DESIGN.md 4h.
"""
import copy
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN, RecordingAdam, load_family  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def npz(name):
    import os
    return np.load(os.path.join(GOLDEN, name))


def T(a, dev=DEV):
    return torch.from_numpy(np.asarray(a)).clone().to(dev)


def close(a, b, rtol=1e-4, floor=1e-6, what=""):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float64)
    b = np.asarray(b, np.float64)
    scale = max(np.abs(b).max(), floor, 1e-300)   # (an all-zero reference with no floor: only zero agrees)
    err = np.abs(a - b).max() / scale
    assert err <= rtol, "%s max rel err %.3e (scale %.3e)" % (what, err, scale)


# ---------------------------------------------------------------------------
# 1. kernels against the oracle's modules, float64 yardstick
# ---------------------------------------------------------------------------
from _lstm_ref import _build, _inputs, _run, reference, gate, hip_module  # noqa: E402,F401  (tests/_lstm_ref.py)


CASES = [(8, 8, False, 17), (8, 3, True, 1), (40, 1, False, 33), (40, 12, True, 16), (40, 8, False, 16),
         (72, 8, False, 1), (72, 12, True, 33), (99, 8, False, 16), (99, 3, True, 17), (128, 1, False, 17),
         (128, 8, False, 33), (128, 12, True, 17), (128, 3, True, 16)]


@pytest.mark.parametrize("H,Tn,decoder,B", CASES)
def test_kernels_vs_oracle_f64(H, Tn, decoder, B):
    ref, inp, r64, r32 = reference(H, Tn, decoder, B)
    got = _run(hip_module(ref, H, Tn, decoder), inp, decoder, DEV, torch.float32)
    gate("H=%d T=%d %s B=%d" % (H, Tn, "dec" if decoder else "enc", B), got, r64, r32)


@pytest.mark.parametrize("H,Tn,decoder,B", [(99, 8, False, 17), (128, 12, True, 33)])
def test_no_grad_forward_vs_oracle_f64(H, Tn, decoder, B):
    """The forward without saved states (inference)."""
    ref, inp, r64, r32 = reference(H, Tn, decoder, B)
    mod = hip_module(ref, H, Tn, decoder)
    with torch.no_grad():
        if decoder:
            h0 = inp["h0"].to(DEV)
            y, _ = mod(inp["last_pos"].to(DEV), inp["last_rel"].to(DEV), (h0, torch.zeros_like(h0)), None)
        else:
            y = mod(inp["rel"].to(DEV)).reshape(inp["dy"].shape)
    out = {"out": y.cpu().double().numpy()}
    gate("no-grad H=%d" % H, out, {"out": r64["out"]}, {"out": r32["out"]})


# ---------------------------------------------------------------------------
# 2. zero padding is exact: H = 40 embedded in an H = 48 four-wave module
# ---------------------------------------------------------------------------
def _pad_state(sd, lstm, H, HP):
    out = {}
    for k, v in sd.items():
        if k.startswith(lstm + "."):
            cols = v.shape[1] if v.dim() == 2 else 1
            w = torch.zeros(4, HP, cols)
            w[:, :H] = v.reshape(4, H, cols)
            w = w.reshape(4 * HP, cols)
            if k.endswith("weight_hh_l0"):
                w2 = torch.zeros(4 * HP, HP)
                w2[:, :H] = w
                w = w2
            out[k] = w if v.dim() == 2 else w.reshape(-1)
        elif k == "hidden2pos.weight":
            w = torch.zeros(2, HP)
            w[:, :H] = v
            out[k] = w
        else:
            out[k] = v.clone()
    return out


def _unpad(k, a, H, HP):
    """(the H = 40 part, the padded rest) of a quantity of the H = 48 run."""
    a = np.asarray(a)
    if "weight_hh_l0" in k:
        full = a.reshape(4, HP, HP)
        keep = np.zeros_like(full, bool)
        keep[:, :H, :H] = True
        return full[:, :H, :H].reshape(4 * H, H), full[~keep]
    if "_l0" in k:   # weight_ih, the biases: gate-blocked rows
        full = a.reshape(4, HP, -1)
        return full[:, :H].reshape((4 * H, -1) if a.ndim == 2 else (4 * H,)), full[:, H:]
    if k in ("out", "dh0", "dhidden2pos.weight") and a.shape[-1] == HP:
        return a[..., :H], a[..., H:]
    return a, np.zeros(0)


@pytest.mark.parametrize("decoder,Tn,B", [(False, 8, 16), (True, 12, 16)])
def test_padding_is_exact(decoder, Tn, B):
    from sgan import models as M
    H, HP = 40, 48
    ref, inp, r64, r32 = reference(H, Tn, decoder, B)
    got40 = _run(hip_module(ref, H, Tn, decoder), inp, decoder, DEV, torch.float32)
    mod48 = M.Decoder(Tn, 16, HP, 64, 1, False) if decoder else M.Encoder(16, HP)
    mod48.load_state_dict(_pad_state(ref.state_dict(), "decoder" if decoder else "encoder", H, HP))
    inp48 = dict(inp)
    if decoder:
        inp48["h0"] = torch.cat([inp["h0"], torch.zeros(1, B, HP - H)], 2)
    else:
        inp48["dy"] = torch.cat([inp["dy"], torch.zeros(1, B, HP - H)], 2)
    got48 = _run(mod48.to(DEV), inp48, decoder, DEV, torch.float32)
    part = {}
    for k, v in got48.items():
        part[k], rest = _unpad(k, v, H, HP)
        assert part[k].shape == r64[k].shape, (k, part[k].shape, r64[k].shape)
        assert rest.size == 0 or not np.any(rest), (k, "padded entries of the H = 48 run are not exactly zero")
    gate("H=40 generic", got40, r64, r32)
    gate("H=40 in 48 four-wave", part, r64, r32)


# ---------------------------------------------------------------------------
# 3. buffers are respected: NaN guard bands around every output
# ---------------------------------------------------------------------------
GUARD = 64   # floats: keeps the 16-byte alignment of the saved states


def _guarded(n):
    buf = torch.full((n + 2 * GUARD,), NAN, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _bands_ok(buf):
    return bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all())


@pytest.mark.parametrize("decoder,Tn", [(False, 8), (True, 3)])
def test_guard_bands(decoder, Tn):
    from sgan import _native as N
    lib = N.load()
    H, B = 99, 17
    torch.manual_seed(5)
    r = lambda *s: torch.randn(*s, device=DEV)
    A, Whh, bias = r(4 * H, 2) * .3, r(4 * H, H) * .1, r(4 * H) * .1
    Wp, bp = r(2, H) * .2, r(2) * .1
    rel = r(B, 2) * .3 if decoder else r(Tn, B, 2) * .3
    h0 = r(B, H) * .5
    bufs = {}

    def g(name, n):
        bufs[name], view = _guarded(n)
        return view
    for save in (True, False):
        bufs.clear()
        h_all = g("h_all", (Tn + 1) * B * H)
        c_all = g("c_all", lib.sgg_lstm_state_floats(Tn, B, H, 1))
        act = g("act", lib.sgg_lstm_state_floats(Tn, B, H, 0)) if save else None
        rel_out = g("rel_out", Tn * B * 2) if decoder else None
        N.check(lib.sgg_lstm_fwd(N.ptr(rel), N.ptr(A), N.ptr(Whh), N.ptr(bias), N.ptr(h0), None,
                                 N.ptr(Wp) if decoder else None, N.ptr(bp) if decoder else None, Tn, B, H,
                                 int(decoder), N.ptr(h_all), N.ptr(c_all), N.ptr(act), N.ptr(rel_out),
                                 N.stream_ptr()), "sgg_lstm_fwd")
        torch.cuda.synchronize()
        for k, b in bufs.items():
            assert _bands_ok(b), (save, k, "guard band written")
        assert not torch.isnan(h_all.view(Tn + 1, B, H)[Tn]).any()
        if decoder:
            assert not torch.isnan(rel_out).any()
        if save:
            assert not torch.isnan(h_all).any() and not torch.isnan(act).any()
            assert torch.equal(h_all.view(Tn + 1, B, H)[0], h0)
    # (the last pass was save = False: run the saving forward again for the backward)
    bufs.clear()
    h_all = g("h_all", (Tn + 1) * B * H)
    c_all = g("c_all", lib.sgg_lstm_state_floats(Tn, B, H, 1))
    act = g("act", lib.sgg_lstm_state_floats(Tn, B, H, 0))
    rel_out = g("rel_out", Tn * B * 2) if decoder else None
    N.check(lib.sgg_lstm_fwd(N.ptr(rel), N.ptr(A), N.ptr(Whh), N.ptr(bias), N.ptr(h0), None,
                             N.ptr(Wp) if decoder else None, N.ptr(bp) if decoder else None, Tn, B, H, int(decoder),
                             N.ptr(h_all), N.ptr(c_all), N.ptr(act), N.ptr(rel_out), N.stream_ptr()), "sgg_lstm_fwd")
    dG = g("dG", lib.sgg_lstm_dg_floats(Tn, B, H))
    dh0 = g("dh0", B * H)
    drel_in = g("drel_in", Tn * B * 2)
    drel_tot = g("drel_tot", Tn * B * 2) if decoder else None
    dh_last = None if decoder else r(B, H)
    dout = r(Tn, B, 2) if decoder else None
    N.check(lib.sgg_lstm_bwd(N.ptr(A), N.ptr(Whh), N.ptr(Wp) if decoder else None, N.ptr(h_all), N.ptr(c_all),
                             N.ptr(act), N.ptr(rel), N.ptr(rel_out), N.ptr(dh_last), N.ptr(dout), Tn, B, H,
                             int(decoder), N.ptr(dG), N.ptr(dh0), N.ptr(drel_in), N.ptr(drel_tot), None,
                             N.stream_ptr()), "sgg_lstm_bwd")
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert _bands_ok(b), (k, "guard band written")
    for k in ("dG", "dh0", "drel_in") + (("drel_tot",) if decoder else ()):
        assert not torch.isnan(bufs[k][GUARD:-GUARD]).any(), (k, "NaN in an output")


def test_refused_sizes_launch_nothing():
    """H = 129 and H = 0 are argument errors of both entry points, and the
    NULL-drel_in form stays an argument error at the generic sizes."""
    from sgan import _native as N
    lib = N.load()
    x = torch.zeros(4096, device=DEV)
    p = N.ptr(x)
    for H in (129, 0):
        assert lib.sgg_lstm_fwd(p, p, p, p, None, None, None, None, 2, 4, H, 0, p, p, None, None, N.stream_ptr()) != 0
        assert lib.sgg_lstm_bwd(p, p, None, p, p, p, p, None, None, None, 2, 4, H, 0, None, None, p, None, None,
                                N.stream_ptr()) != 0
    assert lib.sgg_lstm_bwd(p, p, None, p, p, p, p, None, None, None, 2, 4, 40, 0, p, None, None, None, p,
                            N.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert not x.any()


# ---------------------------------------------------------------------------
# 4. generators against the reference's fixtures
# ---------------------------------------------------------------------------
def _generator(graph, noise, dec_h):
    from sgan.models import TrajectoryGenerator
    return TrajectoryGenerator(8, 12, embedding_dim=16, encoder_h_dim=32, decoder_h_dim=dec_h, mlp_dim=64,
                               num_layers=1, noise_dim=(noise,), noise_type="gaussian", noise_mix_type="global",
                               pooling_type="pool_net", pool_every_timestep=False, dropout=0.0, bottleneck_dim=8,
                               batch_norm=False, n_units=[40, 16, 40], n_heads=1, dropout1=0.0, alpha=0.2,
                               graph=graph)


def _fixture_weights(f):
    return {k[2:]: torch.from_numpy(f[k]) for k in f.files if k.startswith("w/")}


@pytest.mark.parametrize("name,graph,noise,dec_h", [("gen_fwd_h40.npz", "gat", 16, 40),
                                                    ("gen_fwd_h128.npz", "gcn", 8, 128)])
def test_generator_vs_reference_fixture(name, graph, noise, dec_h):
    f = npz(name)
    g = load_family(_generator(graph, noise, dec_h), _fixture_weights(f)).to(DEV)
    y = g(T(f["obs_traj"]), T(f["obs_traj_rel"]), T(f["seq_start_end"]), T(f["obs_traj_g"]), user_noise=T(f["noise"]))
    close(y, f["out"], rtol=1e-4, what="G out")
    (y * T(f["dout"])).sum().backward()
    keys = [k for k in f.files if k.startswith("dw/")]
    fl = 1e-2 * max(np.abs(f[k]).max() for k in keys)
    seen = 0
    for k, p in g.named_parameters():
        if "dw/" + k in f.files:
            close(p.grad, f["dw/" + k], rtol=1e-3, floor=fl, what="G d" + k)
            seen += 1
    assert seen >= 10 and any(k.startswith("dw/decoder.decoder.") for k in keys)


@pytest.mark.parametrize("graph,enc_h,dec_h", [("vanilla", 72, 128), ("sgangat", 32, 56)])
def test_other_families_vs_oracle(graph, enc_h, dec_h):
    """The two families the fixtures above leave out, against the oracle's
    modules: upstream Social-GAN with a 72-wide encoder (its pooling net on a
    72-wide state) and a 128-wide decoder, sgangat with a 56-wide decoder."""
    from oracle import sgan_oracle as O
    from sgan.data.synthetic import synthetic_batch
    from sgan.models import TrajectoryGenerator
    kw = dict(embedding_dim=16, encoder_h_dim=enc_h, decoder_h_dim=dec_h, mlp_dim=64, num_layers=1, noise_dim=(8,),
              noise_type="gaussian", noise_mix_type="global", pooling_type="pool_net", pool_every_timestep=False,
              dropout=0.0, bottleneck_dim=8, batch_norm=False, n_units=[enc_h + 8, 16, 40],
              n_heads=[4, 1] if graph == "sgangat" else 1, dropout1=0.0, alpha=0.2, graph=graph)
    torch.manual_seed(17)
    og = O.TrajectoryGenerator(8, 12, **kw)
    g = TrajectoryGenerator(8, 12, **kw)
    g.load_state_dict(og.state_dict())
    g = g.to(DEV)
    b = synthetic_batch([2, 5, 20], seed=23)
    obs, obs_rel, obs_g, sse = b[0], b[2], b[6], b[10]
    z = torch.randn(3, 8)
    y_ref = og(obs, obs_rel, sse, obs_g, user_noise=z)
    dy = torch.randn_like(y_ref)
    (y_ref * dy).sum().backward()
    y = g(obs.to(DEV), obs_rel.to(DEV), sse.to(DEV), obs_g.to(DEV), user_noise=z.to(DEV))
    (y * dy.to(DEV)).sum().backward()
    close(y, y_ref.detach().numpy(), rtol=1e-4, what="G out")
    ref = {k: p.grad for k, p in og.named_parameters() if p.grad is not None}
    fl = 1e-2 * max(float(v.abs().max()) for v in ref.values())
    mine = dict(g.named_parameters())
    for k, v in ref.items():
        close(mine[k].grad, v.numpy(), rtol=1e-3, floor=fl, what="G d" + k)


# ---------------------------------------------------------------------------
# 5. discriminator
# ---------------------------------------------------------------------------
def test_discriminator_local_h128_vs_oracle():
    from oracle import sgan_oracle as O
    from sgan.data.synthetic import synthetic_batch
    from sgan.models import TrajectoryDiscriminator
    torch.manual_seed(3)
    od = O.TrajectoryDiscriminator(8, 12, embedding_dim=16, h_dim=128, mlp_dim=64, batch_norm=False, d_type="local")
    d = TrajectoryDiscriminator(8, 12, embedding_dim=16, h_dim=128, mlp_dim=64, batch_norm=False, d_type="local")
    d.load_state_dict(od.state_dict())
    d = d.to(DEV)
    b = synthetic_batch([1, 5, 20], seed=12)
    traj, traj_rel = torch.cat([b[0], b[1]], 0), torch.cat([b[2], b[3]], 0)
    tr_ref = traj_rel.clone().requires_grad_(True)
    s_ref = od(traj, tr_ref, b[-1])
    dy = torch.randn_like(s_ref)
    (s_ref * dy).sum().backward()
    tr = traj_rel.to(DEV).requires_grad_(True)
    s = d(traj.to(DEV), tr, b[-1].to(DEV))
    (s * dy.to(DEV)).sum().backward()
    close(s, s_ref.detach().numpy(), rtol=1e-4, what="D scores")
    close(tr.grad, tr_ref.grad.numpy(), rtol=1e-3, floor=1e-3 * float(tr_ref.grad.abs().max()), what="D dtraj_rel")
    fl = 1e-2 * max(float(p.grad.abs().max()) for p in od.parameters())
    for (k, p), (_, q) in zip(od.named_parameters(), d.named_parameters()):
        close(q.grad, p.grad.numpy(), rtol=1e-3, floor=fl, what="D d" + k)


def test_discriminator_global_h128_refused_before_any_launch(monkeypatch):
    """bottleneck_dim = h_dim = 128 is above the pooling kernels' bound (64):
    refused with a message that names it, and nothing was launched."""
    from sgan import _native as N
    from sgan.data.synthetic import synthetic_batch
    from sgan.models import TrajectoryDiscriminator
    d = TrajectoryDiscriminator(8, 12, embedding_dim=16, h_dim=128, mlp_dim=64, batch_norm=False,
                                d_type="global").to(DEV)
    b = synthetic_batch([5, 20], seed=2, device=DEV)
    traj, traj_rel = torch.cat([b[0], b[1]], 0), torch.cat([b[2], b[3]], 0)
    calls = []
    real = N.check
    monkeypatch.setattr(N, "check", lambda rc, name: (calls.append(name), real(rc, name))[1])
    with pytest.raises(N.NativeError, match="bottleneck_dim"):
        d(traj, traj_rel, b[-1])
    assert calls == [], calls


# ---------------------------------------------------------------------------
# 6. training step: GAT generator at H = 40, best_k = 3
# ---------------------------------------------------------------------------
class _Args3:
    obs_len, pred_len, best_k, l2_loss_weight = 8, 12, 3, 1.0
    clipping_threshold_g, clipping_threshold_d, g_learning_rate, d_learning_rate = 2.0, 0.0, 1e-4, 1e-3


def _gd40():
    """(oracle G, oracle D, G, D): the GAT generator at noise_dim 16 (decoder
    H = 40) with the weights of gen_fwd_h40.npz, the default global
    discriminator (H = 48) with those of weights.npz -- both initialised by
    the reference's init_weights."""
    from oracle import sgan_oracle as O
    from sgan.models import TrajectoryDiscriminator
    og = O.TrajectoryGenerator(8, 12, embedding_dim=16, encoder_h_dim=32, decoder_h_dim=40, mlp_dim=64,
                               num_layers=1, noise_dim=(16,), noise_type="gaussian", noise_mix_type="global",
                               pooling_type="pool_net", pool_every_timestep=False, dropout=0.0, bottleneck_dim=8,
                               batch_norm=False, n_units=[40, 16, 40], n_heads=1, dropout1=0.0, alpha=0.2,
                               graph="gat")
    _, od = O.build_default("gat")
    g = _generator("gat", 16, 40)
    d = TrajectoryDiscriminator(8, 12, embedding_dim=16, h_dim=48, mlp_dim=64, num_layers=1, batch_norm=False,
                                dropout=0.0, d_type="global")
    load_family(g, _fixture_weights(npz("gen_fwd_h40.npz")))
    w = npz("weights.npz")
    d.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("d/")})
    og.load_state_dict(g.state_dict())
    od.load_state_dict(d.state_dict())
    return og, od, g.to(DEV), d.to(DEV)


def test_train_step_h40_vs_oracle():
    from oracle import sgan_oracle as O
    from sgan.data.synthetic import synthetic_batch
    from sgan.scene import SceneIndex
    from sgan.train_step import GanTrainer, TrainArgs
    og, od, g, d = _gd40()
    oog = RecordingAdam.make(og.named_parameters(), lr=1e-4)
    ood = RecordingAdam.make(od.named_parameters(), lr=1e-3)
    tr = GanTrainer(g, d, TrainArgs(best_k=3))
    b = synthetic_batch([20, 7, 13], seed=70)
    bd = [t.to(DEV) for t in b]
    sc = SceneIndex.from_seq_start_end(b[-1], DEV)
    ref = []
    torch.manual_seed(21)
    random.seed(21)
    for it in range(2):
        rld = O.discriminator_step(_Args3, b, og, od, ood)
        rlg = O.generator_step(_Args3, b, og, od, oog)
        ref.append((rld, rlg, dict(ood.rec[-1]), dict(oog.rec[-1]),
                    {k: v.clone() for k, v in og.state_dict().items()},
                    {k: v.clone() for k, v in od.state_dict().items()}))
    torch.manual_seed(21)
    random.seed(21)
    for it in range(2):
        rld, rlg, rgd, rgg, wg, wd = ref[it]
        ld, lg = tr.step(bd, sc)
        for k, v in list(ld.items()) + list(lg.items()):
            r = (rld if k.startswith("D") else rlg)[k]
            assert abs(float(v) - r) <= 1e-4 * max(1.0, abs(r)), (it, k, float(v), r)
        for mod, rg in ((d, rgd), (g, rgg)):
            mine = {k: p.grad for k, p in mod.named_parameters() if p.grad is not None}
            assert sorted(mine) == sorted(rg), sorted(set(mine) ^ set(rg))
            fl = 1e-2 * max(float(v.abs().max()) for v in rg.values())
            assert fl > 0, (it, "the reference step has no gradient: nothing would be compared")
            for k in rg:
                close(mine[k], rg[k], rtol=1e-3, floor=fl, what="it%d grad %s" % (it, k))
        for mod, rw, lr in ((g, wg, 1e-4), (d, wd, 1e-3)):
            for k, v in mod.state_dict().items():
                err = (v.detach().cpu().double() - rw[k].double()).abs().max().item()
                assert err <= 2 * lr * (it + 1) + 1e-5 * rw[k].abs().max().item(), (it, k, err)


def test_graphed_trainer_h40_replays_bitwise():
    """GraphedTrainer (one warm-up iteration + two replays) == three eager
    iterations, bit for bit: weights and losses."""
    from sgan.data.synthetic import synthetic_batch
    from sgan.scene import SceneIndex
    from sgan.train_step import GanTrainer, GraphedTrainer, TrainArgs
    batch = synthetic_batch([20, 7, 13], seed=70, device=DEV)
    res = []
    for graphed in (False, True):
        _, _, g, d = _gd40()
        tr = GanTrainer(g, d, TrainArgs(best_k=3), capturable=True)
        sc = SceneIndex.from_seq_start_end(batch[-1], DEV)
        torch.manual_seed(11)
        random.seed(11)
        if graphed:
            gt = GraphedTrainer(tr, batch, sc, warmup=1)
            for _ in range(2):
                ld, lg = gt.step()
        else:
            for _ in range(3):
                ld, lg = tr.step(batch, sc)
        torch.cuda.synchronize()
        ws = {"g." + k: v.detach().cpu().clone() for k, v in g.state_dict().items()}
        ws.update({"d." + k: v.detach().cpu().clone() for k, v in d.state_dict().items()})
        res.append(({k: float(v) for k, v in list(ld.items()) + list(lg.items())}, ws))
    (la, wa), (lb, wb) = res
    assert la == lb, (la, lb)
    for k in wa:
        assert torch.equal(wa[k], wb[k]), (k, (wa[k] - wb[k]).abs().max().item())


def test_bucketed_trainer_refuses_h40_by_name():
    from sgan.train_step import BucketedGraphTrainer, GanTrainer, TrainArgs
    _, _, g, d = _gd40()
    tr = GanTrainer(g, d, TrainArgs(best_k=3), capturable=True)
    with pytest.raises(NotImplementedError, match="H=40"):
        BucketedGraphTrainer(tr, None)


def test_check_accuracy_h40_vs_restatement():
    """validate.check_accuracy with the H = 40 generator against the plain
    restatement of the reference's loop on the CPU oracle (same seeds): 1e-3,
    test_check_accuracy_vs_reference_fixture's gate."""
    from _check_accuracy_ref import check_accuracy_ref
    from oracle import sgan_oracle as O  # noqa: F401
    from sgan.data.synthetic import synthetic_batch
    from sgan.validate import check_accuracy
    og, od, g, d = _gd40()

    class A:
        obs_len, pred_len, batch_size, num_samples_check = 8, 12, 64, 5000
    batches = [tuple(synthetic_batch(s, seed=40 + i)) for i, s in enumerate(([5, 3, 9], [2, 20, 1, 4]))]
    torch.manual_seed(3)
    random.seed(3)
    ref = check_accuracy_ref(A, batches, og, od)
    torch.manual_seed(3)
    random.seed(3)
    got = check_accuracy(A, batches, g, d)
    assert sorted(got) == sorted(ref)
    for k in ref:
        assert abs(got[k] - ref[k]) <= 1e-3 * abs(ref[k]), (k, got[k], ref[k])


# ---------------------------------------------------------------------------
# 7. evaluate.sample_k
# ---------------------------------------------------------------------------
def test_sample_k_h40_equals_separate_calls():
    from sgan import evaluate
    from sgan.data.synthetic import synthetic_batch
    from sgan.scene import SceneIndex
    _, _, g, _ = _gd40()
    batch = synthetic_batch([1, 5, 20], seed=8, device=DEV)
    k, S = 3, 3
    with torch.no_grad():
        torch.manual_seed(4)
        out, _ = evaluate.sample_k(g, batch, k)
        torch.manual_seed(4)
        sc = SceneIndex(np.array([0, 1, 6, 26]), DEV)
        z = evaluate.draw_sample_noise(g, sc, 26, k)
        for r in range(k):
            y = g(batch[0], batch[2], batch[-1], batch[6], user_noise=z[r * S:(r + 1) * S])
            close(out[:, r], y.cpu().numpy(), rtol=1e-6, what="sample %d" % r)
