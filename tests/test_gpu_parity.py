"""GPU parity: the HIP path (through the C ABI) against the reference's golden
fixtures and the CPU oracle.  Tolerances are fp32 reassociation bounds
(north_star: outputs within 1e-3 relative on fp32)."""
import contextlib
import json
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN, check_step_grads, load_family

pytestmark = pytest.mark.gpu

DEV = "cuda"


def npz(name):
    return np.load(os.path.join(GOLDEN, name))


def T(a, dev=DEV):
    return torch.from_numpy(np.asarray(a)).clone().to(dev)


def close(a, b, rtol=1e-4, floor=1e-6, what=""):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float64)
    b = np.asarray(b, np.float64)
    scale = max(np.abs(b).max(), floor)
    err = np.abs(a - b).max() / scale
    assert err <= rtol, "%s max rel err %.3e (scale %.3e)" % (what, err, scale)


def grad_floor(f, prefix, frac=1e-2):
    return frac * max(np.abs(f[k]).max() for k in f.files if k.startswith(prefix))


def build_models(graph="gat"):
    from sgan.models import TrajectoryGenerator, TrajectoryDiscriminator
    g = TrajectoryGenerator(8, 12, embedding_dim=16, encoder_h_dim=32, decoder_h_dim=32, mlp_dim=64, num_layers=1,
                            noise_dim=(8,), noise_type="gaussian", noise_mix_type="global",
                            pooling_type="pool_net", pool_every_timestep=False, dropout=0.0, bottleneck_dim=8,
                            batch_norm=False, n_units=[40, 16, 40], n_heads=[4, 1] if graph == "sgangat" else 1,
                            dropout1=0.0, alpha=0.2, graph=graph)
    d = TrajectoryDiscriminator(8, 12, embedding_dim=16, h_dim=48, mlp_dim=64, num_layers=1, batch_norm=False,
                                dropout=0.0, d_type="global")
    w = npz("weights.npz")
    if graph == "sgangat":   # the family's full state (batched GAT + mlp_decoder_context) is in its fixture
        f = npz("gen_fwd_sgangat.npz")
        g.load_state_dict({k[2:]: torch.from_numpy(f[k]) for k in f.files if k.startswith("w/")})
    else:
        load_family(g, {k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("g/")})
    d.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("d/")})
    return g.to(DEV), d.to(DEV)


def test_native_loaded_on_gpu():
    from sgan import _native
    from sgan._srchash import source_hash
    lib = _native.load()
    assert lib.sgg_version() >= 1
    maps = open("/proc/self/maps").read()
    assert "libsgg.so" in maps
    # the binary under test was built from this tree's kernel sources (HEAD)
    assert lib.sgg_source_hash().decode() == source_hash()


def test_xw_matches_torch():
    from sgan import kernels as K
    torch.manual_seed(0)
    for (M, Kd, Nn) in [(1, 3, 5), (37, 40, 72), (1000, 32, 512), (257, 512, 48), (64, 16, 24), (130, 144, 16)]:
        x = torch.randn(M, Kd, device=DEV)
        w = torch.randn(Kd, Nn, device=DEV)
        b = torch.randn(Nn, device=DEV)
        ref = (x.double() @ w.double() + b.double()).float()
        close(K.xw_raw(x, w, b), ref.cpu(), rtol=2e-6, what="xw %s" % ((M, Kd, Nn),))
        close(K.xw_raw(x, w.t().contiguous(), b, trans_w=True), ref.cpu(), rtol=2e-6)
        close(K.xw_raw(x, w, b, act=1), ref.clamp(min=0).cpu(), rtol=2e-6)


@pytest.mark.parametrize("tag", ["g", "d"])
def test_pool_vs_reference_fixture(tag):
    from sgan.models import PoolHiddenNet
    f = npz("pool.npz")
    hd = f[tag + "/h"].shape[1]
    bn = f[tag + "/out"].shape[1]
    net = PoolHiddenNet(16, hd, 64, bn, "relu", False).to(DEV)
    net.load_state_dict({k[len(tag) + 3:]: torch.from_numpy(f[k]) for k in f.files if k.startswith(tag + "/w/")})
    h = T(f[tag + "/h"]).unsqueeze(0).requires_grad_(True)
    y = net(h, T(f[tag + "/sse"]), T(f[tag + "/pos"]))
    close(y, f[tag + "/out"], rtol=1e-5, what="pool out")
    (y * T(f[tag + "/dout"])).sum().backward()
    close(h.grad[0], f[tag + "/dh"], rtol=1e-4, what="pool dh")
    fl = grad_floor(f, tag + "/dw/")
    for k, p in net.named_parameters():
        close(p.grad, f[tag + "/dw/" + k], rtol=1e-4, floor=fl, what="pool d" + k)


@pytest.mark.parametrize("name,kind", [("gat_encoder.npz", 1), ("gat_encoder_h2.npz", 2), ("gcn_module.npz", 0)])
def test_graph_module_vs_reference_fixture(name, kind):
    from sgan.models import GATEncoder, GCNModule
    f = npz(name)
    mod = GATEncoder([40, 16, 40], kind, 0.0, 0.2) if kind else GCNModule(40, 72, 16, 2, 24)
    mod.load_state_dict({k[2:]: torch.from_numpy(f[k]) for k in f.files if k.startswith("w/")})
    mod = mod.to(DEV)
    x = T(f["x"]).requires_grad_(True)
    y = mod(x, T(f["sse"]), None, T(f["labels"]).view(-1, 1))
    close(y, f["out"], rtol=1e-5 if kind else 1e-4, what=name + " out")
    (y * T(f["dout"])).sum().backward()
    close(x.grad, f["dx"], rtol=1e-4, what=name + " dx")
    fl = grad_floor(f, "dw/")
    for k, p in mod.named_parameters():
        if "dw/" + k in f.files:
            close(p.grad, f["dw/" + k], rtol=2e-4, floor=fl, what=name + " d" + k)


def test_seg_instance_norm_matches_torch():
    """sgg_seg_norm_fwd/bwd vs torch's InstanceNorm1d (affine=False) per
    scene, F in {40, 64, 100}; a one-ped scene normalises to 0."""
    from sgan import kernels as K
    torch.manual_seed(5)
    sizes = [2, 3, 20, 64, 128, 7, 1]
    off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=DEV)
    for F in (40, 64, 100):
        x = (torch.randn(sum(sizes), F, device=DEV) * 3 + 1).requires_grad_(True)
        y = K.seg_instance_norm(x, off, len(sizes))
        dy = torch.randn_like(y)
        (y * dy).sum().backward()
        o = 0
        for n in sizes:
            xs = x.detach()[o:o + n].double().cpu().requires_grad_(True)
            if n == 1:
                assert float(y[o:o + n].detach().abs().max()) == 0.0
                o += n
                continue
            ref = torch.nn.functional.instance_norm(xs.t().unsqueeze(0), eps=1e-5)[0].t()
            (ref * dy[o:o + n].double().cpu()).sum().backward()
            close(y[o:o + n], ref.detach().numpy(), rtol=2e-5, what="norm y n=%d F=%d" % (n, F))
            if n > 2:   # a 2-row segment normalises to +-1 whatever x is: its dx is pure rounding noise
                close(x.grad[o:o + n], xs.grad.numpy(), rtol=1e-4, floor=1e-3, what="norm dx n=%d F=%d" % (n, F))
            o += n


def test_bce_pair_matches_reference_formula():
    """sgg_bce_fwd/bwd vs losses.py:5-21 under torch autograd, incl. the
    scores D's trailing ReLU pins at exactly 0, and an empty range."""
    from sgan import kernels as K
    from sgan.losses import bce_loss
    torch.manual_seed(2)
    for n, split in ((1280 * 2, 1280), (1000, 1000), (37, 0), (5, 2)):
        x = torch.randn(n, 1, device=DEV) * 3
        x[::3] = 0.0
        ya, yb = 0.0, 0.93
        for w in (1.0, 0.25):
            xa = x.clone().requires_grad_(True)
            loss = K.bce_pair(xa, split, ya, torch.tensor(yb, device=DEV), w)
            loss.backward(torch.tensor(1.7, device=DEV))
            xr = x.double().clone().requires_grad_(True)
            parts = [bce_loss(t, torch.ones_like(t) * y) for t, y in ((xr[:split], ya), (xr[split:], yb)) if t.numel()]
            ref = w * sum(parts)
            (ref * 1.7).backward()
            close(loss, np.array(float(ref)), rtol=2e-6, what="bce loss n=%d" % n)
            close(xa.grad, xr.grad.cpu().numpy(), rtol=2e-6, what="bce grad n=%d" % n)
            # (bce, bce + addend) from one launch: the total's gradient reaches the addend
            xb = x.clone().requires_grad_(True)
            l2 = torch.tensor(0.37, device=DEV, requires_grad=True)
            adv, tot = K.bce_pair_total(xb, split, ya, torch.tensor(yb, device=DEV), w, l2 * 1.0)
            tot.backward(torch.tensor(1.7, device=DEV))
            assert torch.equal(adv, loss.detach()), "bce_pair_total loss"
            close(tot, np.array(float(ref) + 0.37), rtol=2e-6, what="bce total n=%d" % n)
            assert torch.equal(xb.grad, xa.grad), "bce_pair_total grad"
            close(l2.grad, np.array(1.7, np.float32), rtol=0, what="bce total d addend")


def test_sgangat_module_vs_reference_fixture():
    """Batched multi-head GAT of the sgangat family (GAT.py:6-106 text, heads
    4,1, instance norm) against the reference's own output."""
    from sgan.models import BatchGATEncoder
    f = npz("sgangat_gat.npz")
    mod = BatchGATEncoder([40, 16, 40], [4, 1], 0.0, 0.2)
    mod.load_state_dict({k[2:]: torch.from_numpy(f[k]) for k in f.files if k.startswith("w/")})
    mod = mod.to(DEV)
    x = T(f["x"]).requires_grad_(True)
    y = mod(x, T(f["sse"]))
    close(y, f["out"], rtol=1e-5, what="sgat out")
    (y * T(f["dout"])).sum().backward()
    close(x.grad, f["dx"], rtol=1e-4, what="sgat dx")
    fl = grad_floor(f, "dw/")
    for k, p in mod.named_parameters():
        # layer 0's bias gradient nearly cancels in the next layer's norm
        close(p.grad, f["dw/" + k], rtol=1e-3 if k.endswith("0.bias") else 2e-4, floor=fl, what="sgat d" + k)


@pytest.mark.parametrize("graph", ["gat", "gcn", "sgangat"])
def test_generator_vs_reference_fixture(graph):
    g, _ = build_models(graph)
    f = npz("gen_fwd_%s.npz" % graph)
    for b in ("synth", "zara1"):
        g.zero_grad()
        y = g(T(f[b + "/obs_traj"]), T(f[b + "/obs_traj_rel"]), T(f[b + "/seq_start_end"]), T(f[b + "/obs_traj_g"]),
              user_noise=T(f[b + "/noise"]))
        close(y, f[b + "/out"], rtol=1e-4, what="G %s out" % b)
        (y * T(f[b + "/dout"])).sum().backward()
        fl = grad_floor(f, b + "/dw/")
        for k, p in g.named_parameters():
            key = b + "/dw/" + k
            if key in f.files:
                close(p.grad, f[key], rtol=1e-3, floor=fl, what="G %s d%s" % (b, k))


def test_discriminator_vs_reference_fixture():
    _, d = build_models()
    f = npz("disc_fwd.npz")
    tr = T(f["traj_rel"]).requires_grad_(True)
    traj, sse = T(f["traj"]), T(f["sse"])
    s = d(traj, tr, sse)
    close(s, f["scores"], rtol=1e-4, what="D scores")
    feat = d.pool_net(d.encoder(tr).squeeze(), sse, traj[0])
    close(feat, f["feat"], rtol=1e-4, what="D pooled features")
    (s * T(f["dscores"])).sum().backward()
    close(tr.grad, f["dtraj_rel"], rtol=1e-3, floor=1e-3 * np.abs(f["dtraj_rel"]).max(), what="D dtraj_rel")
    fl = grad_floor(f, "dw/")
    for k, p in d.named_parameters():
        if "dw/" + k in f.files:
            close(p.grad, f["dw/" + k], rtol=1e-3, floor=fl, what="D d" + k)


def test_group_index_matches_oracle_partition():
    """sgg_group_index partitions every scene exactly as the distinct rows of
    M_intra (models.py:263-271), incl. label-0 singletons (notebook KAT:
    rows [[1,1,0,0],[1,1,0,0],[0,0,1,0],[0,0,0,1]] -> 3 groups)."""
    from sgan.scene import SceneIndex
    from oracle import sgan_oracle as O
    rng = np.random.default_rng(3)
    sizes = [4, 1, 2, 20, 57, 64, 9, 33]
    labs = [np.array([1, 1, 0, 0], float)] + [rng.integers(0, 4, size=n).astype(float) for n in sizes[1:]]
    lab = np.concatenate(labs)
    sc = SceneIndex(np.concatenate([[0], np.cumsum(sizes)]), DEV)
    g = sc.groups(T(lab).float())
    gid = g.ped_gid.cpu().numpy()
    goff = g.group_off.cpu().numpy()
    cnt = g.group_count.cpu().numpy()
    gs = g.group_scene.cpu().numpy()
    o = 0
    for s, n in enumerate(sizes):
        m = O.group_mask(torch.from_numpy(lab[o:o + n]).float())
        rows = torch.unique(m, dim=0)
        assert goff[s + 1] - goff[s] == rows.shape[0]
        local = gid[o:o + n]
        for i in range(n):
            for j in range(n):
                assert (local[i] == local[j]) == bool(m[i, j]), (s, i, j)
        for gg in range(goff[s], goff[s + 1]):
            assert gs[gg] == s and cnt[gg] == (local == gg).sum()
        o += n
    assert goff[0] == 0 and goff[1] == 3


def test_generator_fixture_with_host_noise_stream():
    """With user_noise=None the generator draws torch.randn((S, 8)) from the
    HOST generator, exactly like the reference (models.py:26)."""
    g, _ = build_models()
    f = npz("gen_fwd_gat.npz")
    args = [T(f["synth/" + k]) for k in ("obs_traj", "obs_traj_rel", "seq_start_end", "obs_traj_g")]
    torch.manual_seed(77)  # the fixture drew its noise right after this seed
    with torch.no_grad():
        y = g(*args)
    close(y, f["synth/out"], rtol=1e-4, what="G host-noise out")


def test_evaluate_ade_fde_all_splits():
    """scripts/evaluate_model.py semantics, 20 samples, test split of all five
    ETH/UCY sets, seeded host RNG: ADE/FDE within 1e-3 relative of the
    reference run on CPU (tests/golden/evaluate.json)."""
    from sgan.evaluate import evaluate_split
    ev = json.load(open(os.path.join(GOLDEN, "evaluate.json")))
    for graph in ("gat", "gcn", "sgangat"):
        g, _ = build_models(graph)
        for split in ("eth", "hotel", "univ", "zara1", "zara2"):
            torch.manual_seed(0)
            ade, fde = evaluate_split(g, os.path.join(GOLDEN, "datasets_group", split, "test"), num_samples=20)
            ref = ev["%s/%s" % (graph, split)]
            assert abs(ade - ref["ade"]) <= 1e-3 * ref["ade"], (graph, split, ade, ref)
            assert abs(fde - ref["fde"]) <= 1e-3 * ref["fde"], (graph, split, fde, ref)


KEYS = ["obs_traj", "pred_traj", "obs_traj_rel", "pred_traj_rel", "obs_vel", "pred_vel", "obs_traj_g",
        "pred_traj_g", "non_linear_ped", "loss_mask", "seq_start_end"]


@pytest.mark.parametrize("selective", [True, False])
def test_train_step_vs_reference_fixture(selective):
    """Two reference iterations (discriminator_step + generator_step, fresh
    Adam, seeded host RNGs) reproduced by GanTrainer: losses within 1e-4 rel,
    the gradients each optimizer step consumed (D raw, G after the 2.0 clip)
    within 1e-3 of the tensor max (floor 1 % of the step's largest gradient),
    weights within Adam's sign-flip bound on noise-level gradients, and --
    the update itself pinned -- within 1 % of lr of torch.optim.Adam on CPU
    applied to the same pre-step weights with the gradients the step
    consumed (a CPU twin of each optimizer, stepped alongside)."""
    from sgan.scene import SceneIndex
    from sgan.train_step import GanTrainer
    g, d = build_models()
    tr = GanTrainer(g, d, selective_backward=selective)
    f = npz("train_step.npz")
    # CPU twins: copies of the weights, torch's Adam with the trainer's lrs
    twins = {}
    for mod, tag, lr in ((g, "g", 1e-4), (d, "d", 1e-3)):
        cp = {k: p.detach().cpu().clone().requires_grad_(True) for k, p in mod.named_parameters()}
        twins[tag] = (cp, torch.optim.Adam(list(cp.values()), lr=lr))
    torch.manual_seed(1234)
    random.seed(1234)
    for it in range(2):
        b = [T(f["b%d/%s" % (it, k)]) for k in KEYS]
        sc = SceneIndex.from_seq_start_end(b[-1], DEV)
        ld, lg = tr.step(b, sc)
        for mod, tag, lr in ((g, "g", 1e-4), (d, "d", 1e-3)):
            cp, opt = twins[tag]
            for k, p in mod.named_parameters():
                cp[k].grad = p.grad.detach().cpu().clone() if p.grad is not None else None
            opt.step()
            for k, p in mod.named_parameters():
                err = (p.detach().cpu() - cp[k].detach()).abs().max().item()
                assert err <= 1e-2 * lr + 1e-6 * cp[k].abs().max().item(), ("Adam update", it, tag, k, err)
        for k, v in list(ld.items()) + list(lg.items()):
            tag = "D" if k.startswith("D") else "G"
            ref = float(f["it%d/%s/%s" % (it, tag, k)])
            assert abs(float(v) - ref) <= 1e-4 * max(1.0, abs(ref)), (it, k, float(v), ref)
        # after step(): D holds its D-step gradient (clip 0: raw), G its
        # G-step gradient as clipped in place by the fused clip + Adam
        check_step_grads({k: p.grad for k, p in d.named_parameters() if p.grad is not None}, f, it, "D")
        check_step_grads({k: p.grad for k, p in g.named_parameters() if p.grad is not None}, f, it, "G")
        for mod, tag, lr in ((g, "g", 1e-4), (d, "d", 1e-3)):
            for k, v in mod.state_dict().items():
                ref = f["it%d/%s/%s" % (it, tag, k)]
                err = np.abs(v.detach().cpu().numpy().astype(np.float64) - ref).max()
                assert err <= 2 * lr * (it + 1) + 1e-5 * np.abs(ref).max(), (it, tag, k, err)


@pytest.mark.parametrize("H,T,decoder,B", [(32, 8, False, 37), (48, 20, False, 37), (32, 12, True, 37),
                                            (16, 5, True, 37), (64, 3, False, 37),
                                            # batches that take the MFMA forward (lstm_mfma.hip)
                                            (32, 8, False, 4133), (32, 12, True, 4133), (48, 20, False, 2085)])
def test_fused_lstm_vs_oracle(H, T, decoder, B):
    """sgg_lstm_fwd/bwd (Encoder / Decoder rollout) against the oracle's
    torch-CPU modules: outputs and every parameter / input gradient."""
    from oracle import sgan_oracle as O
    from sgan import models as M
    torch.manual_seed(H + T)
    if decoder:
        ref, mod = O.Decoder(T, 16, H, 64, 1, False), M.Decoder(T, 16, H, 64, 1, False)
    else:
        ref, mod = O.Encoder(16, H), M.Encoder(16, H)
    mod.load_state_dict(ref.state_dict())
    mod = mod.to(DEV)
    if decoder:
        last_pos, last_rel = torch.randn(B, 2), torch.randn(B, 2) * 0.3
        h0 = (torch.randn(1, B, H) * 0.5).requires_grad_(True)
        c0 = torch.zeros(1, B, H)
        y_ref, _ = ref(last_pos, last_rel, (h0, c0), None)
        h0d = h0.detach().to(DEV).requires_grad_(True)
        y, _ = mod(last_pos.to(DEV), last_rel.to(DEV), (h0d, c0.to(DEV)), None)
        dy = torch.randn_like(y_ref)
        (y_ref * dy).sum().backward()
        (y * dy.to(DEV)).sum().backward()
        close(y, y_ref.detach().numpy(), rtol=1e-5, what="decoder out")
        close(h0d.grad, h0.grad.numpy(), rtol=1e-4, what="decoder dh0")
    else:
        rel = (torch.randn(T, B, 2) * 0.3).requires_grad_(True)
        y_ref = ref(rel)
        reld = rel.detach().to(DEV).requires_grad_(True)
        y = mod(reld)
        dy = torch.randn_like(y_ref)
        (y_ref * dy).sum().backward()
        (y * dy.to(DEV)).sum().backward()
        close(y, y_ref.detach().numpy(), rtol=1e-5, what="encoder h")
        close(reld.grad, rel.grad.numpy(), rtol=1e-4, what="encoder drel")
    for (k, p), (_, q) in zip(ref.named_parameters(), mod.named_parameters()):
        close(q.grad, p.grad.numpy(), rtol=1e-4, floor=1e-6, what="lstm d" + k)


@pytest.mark.parametrize("T,decoder,B", [(12, True, 25600), (8, False, 4133), (12, True, 4099)])
def test_no_grad_rollout_mfma_vs_oracle(T, decoder, B):
    """The no-grad batch-MFMA forward (lstm_fwd_mfma_kernel: the best-of-20
    decoder rollout of the training step, 25,600 sequences) against the
    oracle's modules."""
    from oracle import sgan_oracle as O
    from sgan import models as M
    H = 32
    torch.manual_seed(T + B)
    if decoder:
        ref, mod = O.Decoder(T, 16, H, 64, 1, False), M.Decoder(T, 16, H, 64, 1, False)
    else:
        ref, mod = O.Encoder(16, H), M.Encoder(16, H)
    mod.load_state_dict(ref.state_dict())
    mod = mod.to(DEV)
    with torch.no_grad():
        if decoder:
            last_pos, last_rel = torch.randn(B, 2), torch.randn(B, 2) * 0.3
            h0, c0 = torch.randn(1, B, H) * 0.5, torch.zeros(1, B, H)
            y_ref, h_ref = ref(last_pos, last_rel, (h0, c0), None)
            y, h = mod(last_pos.to(DEV), last_rel.to(DEV), (h0.to(DEV), c0.to(DEV)), None)
            close(y, y_ref.numpy(), rtol=1e-5, what="rollout rel")
            close(h, h_ref.numpy(), rtol=1e-5, what="rollout h_T")
        else:
            rel = torch.randn(T, B, 2) * 0.3
            close(mod(rel.to(DEV)), ref(rel).numpy(), rtol=1e-5, what="encoder h")


@pytest.mark.parametrize("H,T,decoder,B", [(16, 5, True, 21)])
def test_fused_lstm_other_families(H, T, decoder, B):
    """What is left of the comparison of the retired unit- and row-per-thread
    families with the oracle: the one shape of it that test_fused_lstm_vs_oracle
    does not have (21 peds: two 16-ped blocks, five peds in the last), now on
    the four-wave kernels like every other sequence."""
    test_fused_lstm_vs_oracle(H, T, decoder, B)


@pytest.mark.parametrize("bn", [8, 48])
def test_pool_v_equals_tiled(bn, monkeypatch):
    """sgg_pool_fwd's fragment-native k-tiles (pool_fwd_v_kernel, the default
    on small grids; SGG_POOL_V=0 turns it off) against the k-tiled form on
    the same chunk table: the same MFMA sequence, so outputs and argmax are
    bitwise equal.  (The split-bf16 form, the default for bn 32 / 48, is off
    here: test_pool_x3_vs_fp32.)"""
    from sgan import _native as N
    from sgan import kernels as K
    from sgan.scene import SceneIndex
    monkeypatch.setenv("SGG_POOL_X3", "0")
    torch.manual_seed(bn)
    sizes = [20, 1, 7, 13, 20, 2, 17] * 3
    B = sum(sizes)
    sc = SceneIndex(np.concatenate([[0], np.cumsum(sizes)]), DEV)
    U = torch.randn(B, 512, device=DEV) * 0.3
    pos = torch.rand(B, 2, device=DEV) * 15
    A = torch.randn(512, 2, device=DEV) * 0.3
    W2 = torch.randn(bn, 512, device=DEV) * 0.05
    b2 = torch.randn(bn, device=DEV) * 0.1
    lib = N.load()
    chunks, nchunks, max_rows, gpw = sc.pool_plan(bn)
    res = []
    for tiled in (False, True):
        monkeypatch.setenv("SGG_POOL_V", "0" if tiled else "1")
        out = torch.empty(B, bn, device=DEV)
        am = torch.empty(B, bn, device=DEV, dtype=torch.int32)
        N.check(lib.sgg_pool_fwd(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2), N.ptr(b2), N.ptr(sc.scene_off),
                                 N.ptr(chunks), nchunks, max_rows, gpw, B, bn, sc.max_n, N.ptr(out), N.ptr(am),
                                 None, N.stream_ptr()), "pool")
        res.append((out.cpu(), am.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    # and against a torch restatement of the pair MLP
    ref = torch.empty(B, bn)
    Uc, pc, Ac, Wc, bc = U.cpu(), pos.cpu(), A.cpu(), W2.cpu(), b2.cpu()
    for s0, s1 in zip(sc.host_off[:-1], sc.host_off[1:]):
        r = pc[s0:s1].unsqueeze(0) - pc[s0:s1].unsqueeze(1)          # [i, j] = p_j - p_i
        hid = torch.relu(Uc[s0:s1].unsqueeze(0) + r @ Ac.t())          # (i, j, 512)
        ref[s0:s1] = torch.relu(hid @ Wc.t() + bc).max(1)[0]
    close(res[0][0], ref.numpy(), rtol=1e-5, what="pool k-tiles")


@pytest.mark.parametrize("bn", [32, 48])
@pytest.mark.parametrize("sizes", [[20] * 64, [20, 1, 7, 13, 20, 2, 17, 57, 33] * 4])
def test_pool_x3_vs_fp32(bn, sizes, monkeypatch):
    """The split-bf16 pooling forward (pool_fwd_x3_kernel, default for bn 32 /
    48) is as accurate as the fp32 MFMA form: against an fp64 restatement of
    the pair MLP on the same inputs, its largest error (relative to the
    output scale) is within twice the fp32 form's and below 1e-5; every
    argmax is equal to the fp32 form's or a near tie (the fp64 values at the
    two j within 1e-5 of the scale)."""
    from sgan import _native as N
    from sgan.scene import SceneIndex
    torch.manual_seed(7 + bn)
    B = sum(sizes)
    sc = SceneIndex(np.concatenate([[0], np.cumsum(sizes)]), DEV)
    U = torch.randn(B, 512, device=DEV) * 0.3
    pos = torch.rand(B, 2, device=DEV) * 15
    A = torch.randn(512, 2, device=DEV) * 0.3
    W2 = torch.randn(bn, 512, device=DEV) * 0.05
    b2 = torch.randn(bn, device=DEV) * 0.1
    lib = N.load()
    chunks, nchunks, max_rows, gpw = sc.pool_plan(bn)
    res = []
    for x3 in ("1", "0"):
        monkeypatch.setenv("SGG_POOL_X3", x3)
        out = torch.empty(B, bn, device=DEV)
        am = torch.empty(B, bn, device=DEV, dtype=torch.int32)
        N.check(lib.sgg_pool_fwd(N.ptr(U), N.ptr(pos), N.ptr(A), N.ptr(W2), N.ptr(b2), N.ptr(sc.scene_off),
                                 N.ptr(chunks), nchunks, max_rows, gpw, B, bn, sc.max_n, N.ptr(out), N.ptr(am),
                                 None, N.stream_ptr()), "pool")
        res.append((out.cpu().double(), am.cpu()))
    (ox, ax), (of, af) = res
    Uc, pc, Ac, Wc, bc = (t.cpu().double() for t in (U, pos, A, W2, b2))
    ref = torch.empty(B, bn, dtype=torch.float64)
    zs = []
    for s0, s1 in zip(sc.host_off[:-1], sc.host_off[1:]):
        r = pc[s0:s1].unsqueeze(0) - pc[s0:s1].unsqueeze(1)          # [i, j] = p_j - p_i
        z = torch.relu(torch.relu(Uc[s0:s1].unsqueeze(0) + r @ Ac.t()) @ Wc.t() + bc)   # (i, j, bn)
        ref[s0:s1] = z.max(1)[0]
        zs.append((int(s0), z))
    scale = float(ref.abs().max())
    ex, ef = float((ox - ref).abs().max()) / scale, float((of - ref).abs().max()) / scale
    assert ex <= 2 * ef + 1e-7 and ex <= 1e-5, (ex, ef)
    diff = (ax != af).nonzero().tolist()
    for i, c in diff:
        s0, z = next((s0, z) for s0, z in reversed(zs) if s0 <= i)
        a, b = int(ax[i, c]) - s0, int(af[i, c]) - s0
        assert abs(float(z[i - s0, a, c] - z[i - s0, b, c])) <= 1e-5 * scale, (i, c)


def test_xtw_matches_torch():
    from sgan import kernels as K
    torch.manual_seed(1)
    for (R, M, Nn) in [(0, 3, 4), (5, 3, 7), (1000, 32, 128), (51200, 48, 192), (25600, 32, 512), (300, 144, 2),
                       (777, 16, 128), (4099, 72, 40), (63, 64, 65)]:
        X = torch.randn(R, M, device=DEV)
        Y = torch.randn(R, Nn, device=DEV)
        C, cs = K.xtw(X, Y, colsum=True)
        ref = (X.double().t() @ Y.double()).float()
        close(C, ref.cpu(), rtol=5e-6, floor=1.0, what="xtw %s" % ((R, M, Nn),))
        close(cs, Y.double().sum(0).float().cpu(), rtol=5e-6, floor=1.0, what="colsum")
        Ct = K.xtw(X, Y, trans_c=True)                               # transposed output
        close(Ct, ref.t().cpu(), rtol=5e-6, floor=1.0, what="xtw^T %s" % ((R, M, Nn),))
        big = torch.full((Nn, M + 5), 7.0, device=DEV)               # in place into a column block
        K.xtw(X, Y, trans_c=True, out=big[:, 3:3 + M])
        close(big[:, 3:3 + M], ref.t().cpu(), rtol=5e-6, floor=1.0, what="xtw^T in place")
        assert float(big[:, :3].sub(7).abs().max()) == 0 and float(big[:, 3 + M:].sub(7).abs().max()) == 0
        if R:                                                        # fused ReLU-backward mask on Y
            Ym = torch.randn(R, Nn, device=DEV)
            Cm = K.xtw(X, Y, mask=Ym)
            refm = (X.double().t() @ (Y * (Ym > 0)).double()).float()
            close(Cm, refm.cpu(), rtol=5e-6, floor=1.0, what="masked xtw %s" % ((R, M, Nn),))


def test_xw_strided_weight_block():
    """sgg_xw on a column block of a wider weight (the pooling layer's h-half
    W1[:, E:], models.py:538) read in place through its row stride."""
    from sgan import kernels as K
    torch.manual_seed(4)
    W1 = torch.randn(512, 16 + 48, device=DEV)
    h = torch.randn(300, 48, device=DEV)
    c = torch.randn(512, device=DEV)
    ref = (h.double() @ W1[:, 16:].double().t() + c.double()).float()
    close(K.xw_raw(h, W1[:, 16:], c, trans_w=True), ref.cpu(), rtol=2e-6, what="xw strided")


def test_fold_matches_torch():
    """sgg_fold_fwd / sgg_fold_bwd against the autograd of W (We r + be) + b1 + b2."""
    from sgan import kernels as K
    torch.manual_seed(6)
    for R, E, ld in ((128, 16, 16), (512, 16, 64), (192, 16, 16)):
        Wfull = torch.randn(R, ld, device=DEV, dtype=torch.float64)
        W = Wfull[:, :E]
        We, be = torch.randn(E, 2, device=DEV, dtype=torch.float64), torch.randn(E, device=DEV, dtype=torch.float64)
        b1, b2 = torch.randn(R, device=DEV, dtype=torch.float64), torch.randn(R, device=DEV, dtype=torch.float64)
        A, bias = K.fold_fwd(W.float(), We.float(), be.float(), b1.float(), b2.float())
        close(A, (W @ We).cpu().numpy(), rtol=2e-6, what="fold A")
        close(bias, (W @ be + b1 + b2).cpu().numpy(), rtol=2e-6, what="fold bias")
        dA, db = torch.randn(R, 2, device=DEV, dtype=torch.float64), torch.randn(R, device=DEV, dtype=torch.float64)
        dW, dWe, dbe = K.fold_bwd(W.float(), We.float(), be.float(), dA.float(), db.float())
        close(dW, (dA @ We.t() + db[:, None] * be[None, :]).cpu().numpy(), rtol=2e-6, what="fold dW")
        close(dWe, (W.t() @ dA).cpu().numpy(), rtol=2e-6, what="fold dWe")
        close(dbe, (W.t() @ db).cpu().numpy(), rtol=2e-6, what="fold dbe")


@pytest.mark.parametrize("H,T,B,save", [(48, 20, 2560, True), (32, 8, 1280, False), (48, 20, 37, True),
                                        (32, 8, 5, True), (16, 8, 17, False)])
def test_encoder_projection_epilogue(H, T, B, save):
    """sgg_lstm_fwd_u: the encoder kernel's U = h_T Wu^T + cu (the pooling
    net's first layer, Wu = W1[:, E:] in place) equals the sgg_xw form, and
    h_T is unchanged by the epilogue."""
    from sgan import kernels as K
    torch.manual_seed(H + B)
    lstm = torch.nn.LSTM(16, H).to(DEV)
    emb = torch.nn.Linear(2, 16).to(DEV)
    rel = torch.randn(T, B, 2, device=DEV)
    W1 = torch.randn(512, 16 + H, device=DEV) * 0.2
    cu = torch.randn(512, device=DEV)
    with torch.set_grad_enabled(save):
        if save:
            rel.requires_grad_(True)
        h_ref, _ = K.lstm_sequence(rel, lstm, emb)
        h, U = K.lstm_sequence(rel, lstm, emb, proj_u=(W1[:, 16:], cu))
    assert U is not None, "the four-wave family should take the projection at these sizes"
    torch.testing.assert_close(h, h_ref, rtol=0, atol=0)
    U_ref = K.xw_raw(h_ref.detach(), W1[:, 16:], cu, trans_w=True)
    ref64 = (h_ref.detach().double() @ W1[:, 16:].double().t() + cu.double()).float()
    close(U, ref64.cpu(), rtol=2e-6, what="U vs float64")
    close(U, U_ref.cpu(), rtol=2e-6, what="U vs sgg_xw")


@pytest.mark.parametrize("M,Kd,N1,relu1,relu2",[(2560, 48, 64, 1, 1), (1000, 64, 32, 1, 0), (1, 16, 16, 0, 1),
                                                 (63, 32, 64, 1, 1), (129, 48, 16, 0, 0)])
def test_fused_head_matches_torch(M, Kd, N1, relu1, relu2):
    """sgg_head_fwd / sgg_head_bwd (+ sgg_grad_finish) against autograd of the
    reference's real_classifier = make_mlp([K, N1, 1]) in float64."""
    from sgan import kernels as K
    from sgan.models import make_mlp
    torch.manual_seed(M + Kd)
    seq = make_mlp([Kd, N1, 1], batch_norm=False).to(DEV)
    mods = [m for m in seq]
    if not relu1:
        mods.pop(1)
    if not relu2:
        mods.pop(-1)
    seq = torch.nn.Sequential(*mods)
    spec = K.head_ok(seq)
    assert spec is not None and spec[2] == relu1 | (2 * relu2)
    x = torch.randn(M, Kd, device=DEV, requires_grad=True)
    y = K.head(x, spec)
    dy = torch.randn(M, 1, device=DEV)
    y.backward(dy)
    ref = torch.nn.Sequential(*[type(m)(m.in_features, m.out_features).double() if isinstance(m, torch.nn.Linear)
                                else m for m in mods]).to(DEV)
    ref.load_state_dict({k: v.double() for k, v in seq.state_dict().items()})
    xd = x.detach().double().requires_grad_(True)
    yr = ref(xd)
    yr.backward(dy.double())
    close(y.detach(), yr.detach().cpu().numpy(), rtol=2e-6, what="head y")
    close(x.grad, xd.grad.cpu().numpy(), rtol=2e-5, what="head dx")
    for (n, p), pr in zip(seq.named_parameters(), ref.parameters()):
        close(p.grad, pr.grad.cpu().numpy(), rtol=2e-5, what="head d%s" % n)


@pytest.mark.parametrize("H,B", [(48, 1280), (48, 37), (32, 100)])
@pytest.mark.parametrize("proj", [False, True])
def test_encoder_backward_tail_equals_full(H, B, proj):
    """Frozen-weight encoder backward over the steps whose input gradients are
    wanted (sgg_lstm_bwd_tail, the generator step's pass through D: traj_cat
    marks the observed steps as not needing a gradient) is bit-identical to
    the full BPTT on those steps.  proj: the discriminator's form, the encoder
    with the pooling projection epilogue (sgg_lstm_fwd_u)."""
    from sgan import kernels as K
    torch.manual_seed(H + B)
    lstm = torch.nn.LSTM(16, H).to(DEV)
    emb = torch.nn.Linear(2, 16).to(DEV)
    for p in list(lstm.parameters()) + list(emb.parameters()):
        p.requires_grad_(False)
    obs = torch.randn(8, B, 2, device=DEV) * 0.3
    pred0 = torch.randn(12, B, 2, device=DEV) * 0.3
    dh = torch.randn(B, H, device=DEV)
    Wu = torch.randn(512, H, device=DEV) * 0.1
    cu = torch.randn(512, device=DEV) * 0.1
    if proj and not K.lstm_u_ok(20, B, H, True, 512):
        pytest.skip("no projection epilogue at this size")
    grads, outs = [], []
    for tail in (True, False):
        pred = pred0.clone().requires_grad_(True)
        rel = K.traj_cat(obs, pred)
        if not tail:
            rel = rel.clone()                     # no step marker: the full backward
        h, U = K.lstm_sequence(rel, lstm, emb, proj_u=(Wu, cu) if proj else None)
        (h * dh).sum().backward()
        grads.append(pred.grad.clone())
        outs.append((h.detach().clone(), U.clone() if U is not None else None))
    torch.testing.assert_close(grads[0], grads[1], rtol=0, atol=0)
    torch.testing.assert_close(outs[0][0], outs[1][0], rtol=0, atol=0)
    if proj:
        assert outs[0][1] is not None
        torch.testing.assert_close(outs[0][1], outs[1][1], rtol=0, atol=0)


@pytest.mark.parametrize("total", [False, True])
def test_head_bce_fused_backward_equals_separate(total, monkeypatch):
    """The BCE loss on the fused head's scores hands its backward to the head
    launch (BceLink): every gradient is bit-identical to sgg_bce_bwd followed
    by sgg_head_bwd (SGG_HEAD_BCE=0)."""
    from sgan import kernels as K
    from sgan.models import make_mlp
    torch.manual_seed(3)
    seq = make_mlp([48, 64, 1], batch_norm=False).to(DEV)
    spec = K.head_ok(seq)
    x0 = torch.randn(2560, 48, device=DEV)
    ya, yb = torch.tensor(0.0, device=DEV), torch.tensor(0.93, device=DEV)
    grads = []
    for fused in (True, False):
        monkeypatch.setattr(K, "HEAD_BCE", fused)
        seq.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        with K.bce_handoff():
            scores = K.head(x, spec)
            assert (getattr(scores, "_sgg_bce_link", None) is not None) == fused
            if total:
                addend = torch.tensor(0.4, device=DEV, requires_grad=True)
                _, loss = K.bce_pair_total(scores, 1280, ya, yb, 0.5, addend * 1.0)
            else:
                loss = K.bce_pair(scores, 1280, ya, yb, 0.5)
            loss.backward(torch.tensor(1.3, device=DEV))
        grads.append([x.grad.clone()] + [p.grad.clone() for p in seq.parameters()])
    for a, b in zip(*grads):
        torch.testing.assert_close(a, b, rtol=0, atol=0)


def test_head_scores_gradient_is_real_outside_the_trainer():
    """Outside the trainer's steps (no bce_handoff scope) the head's scores
    carry no BceLink: autograd.grad of a BCE loss w.r.t. the scores returns
    the BCE gradient itself (sgg_bce_bwd), equal to torch's."""
    from sgan import kernels as K
    from sgan.models import make_mlp
    torch.manual_seed(4)
    seq = make_mlp([48, 64, 1], batch_norm=False).to(DEV)
    x = torch.randn(640, 48, device=DEV, requires_grad=True)
    scores = K.head(x, K.head_ok(seq))
    assert getattr(scores, "_sgg_bce_link", None) is None
    ya, yb = torch.tensor(0.0, device=DEV), torch.tensor(0.9, device=DEV)
    loss = K.bce_pair(scores, 320, ya, yb, 1.0)
    (gs,) = torch.autograd.grad(loss, scores)
    s = scores.detach().double().requires_grad_(True)
    y = torch.cat([torch.zeros(320, 1), torch.full((320, 1), 0.9)]).double().to(DEV)
    bce = lambda v, t: (v.clamp(min=0) - v * t + (1 + (-v.abs()).exp()).log()).mean()
    ref = bce(s[:320], y[:320]) + bce(s[320:], y[320:])
    (gr,) = torch.autograd.grad(ref, s)
    torch.testing.assert_close(gs.double(), gr, rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize("rows,R,E,ld,M,Nn,R_x",[(160, 192, 16, 16, 48, 2, 30720), (80, 512, 16, 64, 32, 512, 1280),
                                                 (1, 128, 16, 16, 16, 2, 70), (257, 512, 16, 16, 64, 65, 4099)])
def test_grad_finish_bitwise_equals_three_launches(rows, R, E, ld, M, Nn, R_x):
    """sgg_grad_finish (one launch: slab row sums, sgg_xtw's reduce pass, fold
    backwards whose (dA, dbias) are slab row sums) is bit-identical to
    sgg_slab_reduce + sgg_xtw + sgg_fold_bwd run one after the other."""
    from sgan import _native as N
    from sgan import kernels as K
    torch.manual_seed(rows)
    lib = K._lib()
    P = 7 + 3 * R + 11                               # [junk | dA (2R) | dbias (R) | junk]
    slab = torch.randn(rows, P, device=DEV)
    Wfull = torch.randn(R, ld, device=DEV)
    W = Wfull[:, :E]
    We, be = torch.randn(E, 2, device=DEV), torch.randn(E, device=DEV)
    X, Y = torch.randn(R_x, M, device=DEV), torch.randn(R_x, Nn, device=DEV)
    # reference: three launches
    flat = torch.empty(P, device=DEV)
    N.check(lib.sgg_slab_reduce(N.ptr(slab), rows, P, N.ptr(flat), N.stream_ptr()), "sgg_slab_reduce")
    C_ref, cs_ref = K.xtw(X, Y, colsum=True, trans_c=True)
    dW_ref, dWe_ref, dbe_ref = K.fold_bwd(W, We, be, flat[7:7 + 2 * R].view(R, 2), flat[7 + 2 * R:7 + 3 * R])
    dW2_ref, dWe2_ref, dbe2_ref = K.fold_bwd(W, We, be, flat[7:7 + 2 * R].view(R, 2), cs_ref) if Nn == R else \
        (None, None, None)
    # one launch
    ws, splits = K.xtw_partial(X, Y, colsum=True)
    gf = K.GradFinish()
    head = torch.empty(7, device=DEV)
    C = torch.full((Nn, M + 3), 5.0, device=DEV)
    cs = torch.empty(Nn, device=DEV)
    copy = torch.empty(R, device=DEV)
    gf.rowsum(slab, rows, P, 0, 7, head)
    gf.xtw_sums(ws, splits, M, Nn, C[:, 1:1 + M], trans_c=True, colsum=cs)
    dW, dWe, dbe = gf.fold(W, We, be, slab, rows, P, 7, slab, rows, P, 7 + 2 * R, dbias_copy=copy)
    if Nn == R:   # the pooling form: dbias from the xtw column-sum partials
        dW2, dWe2, dbe2 = gf.fold(W, We, be, slab, rows, P, 7, ws[splits * M * Nn:], splits, Nn, 0)
    gf.run()
    torch.cuda.synchronize()
    eq = lambda a, b, what: torch.testing.assert_close(a, b, rtol=0, atol=0, msg=what)
    eq(head, flat[:7], "slab row sums")
    eq(C[:, 1:1 + M], C_ref, "xtw C^T")
    assert float(C[:, 0].sub(5).abs().max()) == 0 and float(C[:, 1 + M:].sub(5).abs().max()) == 0
    eq(cs, cs_ref, "xtw colsum")
    eq(copy, flat[7 + 2 * R:7 + 3 * R], "dbias copy")
    eq(dW, dW_ref, "fold dW")
    eq(dWe, dWe_ref, "fold dWe")
    eq(dbe, dbe_ref, "fold dbe")
    if Nn == R:
        eq(dW2, dW2_ref, "fold dW (colsum dbias)")
        eq(dWe2, dWe2_ref, "fold dWe (colsum dbias)")
        eq(dbe2, dbe2_ref, "fold dbe (colsum dbias)")


@pytest.mark.parametrize("replays", [2, 3])
def test_graphed_trainer_equals_eager(replays):
    """The HIP-graph replay of a training iteration (GraphedTrainer) consumes
    the host RNGs in the same order and produces the same updates as the eager
    GanTrainer -- after an even and an odd number of replays (the two
    alternating graphs), and eager code afterwards sees the state of the LAST
    replay: every p.grad is the gradient that replay consumed, and an eager
    discriminator forward uses the updated weights (no stale cached fold)."""
    from sgan.data.synthetic import synthetic_batch
    from sgan.scene import SceneIndex
    from sgan.train_step import GanTrainer, GraphedTrainer, _sse_of
    batch = synthetic_batch([20, 7, 13, 20, 2], seed=3, device=DEV)
    res = []
    for graphed in (False, True):
        g, d = build_models()
        tr = GanTrainer(g, d, capturable=True)
        sc = SceneIndex.from_seq_start_end(batch[-1], DEV)
        torch.manual_seed(9)
        random.seed(9)
        if graphed:
            gt = GraphedTrainer(tr, batch, sc, warmup=2)
            for _ in range(replays):
                ld, lg = gt.step()
        else:
            for _ in range(2 + replays):
                ld, lg = tr.step(batch, sc)
        torch.cuda.synchronize()
        ws = {"g." + k: v.detach().cpu().clone() for k, v in g.state_dict().items()}
        ws.update({"d." + k: v.detach().cpu().clone() for k, v in d.state_dict().items()})
        gr = {"g." + k: p.grad.detach().cpu().clone() for k, p in g.named_parameters() if p.grad is not None}
        gr.update({"d." + k: p.grad.detach().cpu().clone() for k, p in d.named_parameters() if p.grad is not None})
        traj_rel = torch.cat([batch[2], batch[3]], 0)
        with torch.no_grad():
            scores = d(batch[0], traj_rel, _sse_of(sc), scenes=sc).cpu()
        res.append(({k: float(v) for k, v in list(ld.items()) + list(lg.items())}, ws, gr, scores))
    (la, wa, ga, sa), (lb, wb, gb, sb) = res
    for k in la:
        assert abs(la[k] - lb[k]) <= 1e-5 * max(1.0, abs(la[k])), (k, la[k], lb[k])
    for k in wa:
        err = (wa[k] - wb[k]).abs().max().item()
        assert err <= 1e-5 + 1e-5 * wa[k].abs().max().item(), (k, err)
    assert sorted(ga) == sorted(gb)
    for k in ga:
        err = (ga[k] - gb[k]).abs().max().item()
        assert err <= 1e-6 + 1e-5 * ga[k].abs().max().item(), ("grad", k, err)
    assert (sa - sb).abs().max().item() <= 1e-5 + 1e-5 * sa.abs().max().item(), "eager D forward after replays"


@pytest.mark.parametrize("iters", [1, 4])
def test_graphed_trainer_draw_ahead_is_bit_identical(iters):
    """GraphedTrainer(draw_ahead=True) -- each replay's host draws made while
    the previous replay runs -- against draw_ahead=False: the same losses and
    weights after three replays, bitwise (the same draw sequence)."""
    from sgan.data.synthetic import synthetic_batch
    from sgan.scene import SceneIndex
    from sgan.train_step import GanTrainer, GraphedTrainer
    batch = synthetic_batch([20, 7, 13, 20, 2], seed=3, device=DEV)
    batch_g = synthetic_batch([20, 7, 13, 20, 2], seed=4, device=DEV)
    res = []
    for ahead in (False, True):
        g, d = build_models()
        tr = GanTrainer(g, d, capturable=True)
        sc = SceneIndex.from_seq_start_end(batch[-1], DEV)
        scg = SceneIndex.from_seq_start_end(batch_g[-1], DEV)
        torch.manual_seed(11)
        random.seed(11)
        gt = GraphedTrainer(tr, batch, sc, warmup=1, batch_g=batch_g, sc_g=scg, iters=iters, draw_ahead=ahead)
        for _ in range(3):
            ld, lg = gt.step()
        torch.cuda.synchronize()
        ws = {"g." + k: v.detach().clone() for k, v in g.state_dict().items()}
        ws.update({"d." + k: v.detach().clone() for k, v in d.state_dict().items()})
        res.append(({k: float(v) for k, v in list(ld.items()) + list(lg.items())}, ws))
    (la, wa), (lb, wb) = res
    assert la == lb
    for k in wa:
        assert torch.equal(wa[k], wb[k]), k


def test_shared_draw_source_keeps_reference_order():
    """bench.py's timed pattern: a draw-ahead multi-iteration trainer and a
    one-iteration trainer over ONE DrawSource, interleaved (the remainder
    iterations run between draw-ahead replays) == the one-iteration trainer
    alone over the same number of iterations: the host RNG draws reach the
    iterations in the reference's order (draw-ahead before a
    remainder replay had reordered them)."""
    from sgan.data.synthetic import synthetic_batch
    from sgan.scene import SceneIndex
    from sgan.train_step import GanTrainer, GraphedTrainer
    batch = synthetic_batch([20, 7, 13, 20, 2], seed=3, device=DEV)
    batch_g = synthetic_batch([20, 7, 13, 20, 2], seed=4, device=DEV)
    res = []
    for mixed in (False, True):
        g, d = build_models()
        tr = GanTrainer(g, d, capturable=True)
        sc = SceneIndex.from_seq_start_end(batch[-1], DEV)
        scg = SceneIndex.from_seq_start_end(batch_g[-1], DEV)
        torch.manual_seed(11)
        random.seed(11)
        g1 = GraphedTrainer(tr, batch, sc, warmup=1, batch_g=batch_g, sc_g=scg)
        if mixed:
            gk = GraphedTrainer(tr, batch, sc, warmup=0, batch_g=batch_g, sc_g=scg, iters=2, draw_ahead=True,
                                draws=g1.draws)
            plan = [gk, g1, gk, g1, g1]          # 2 + 1 + 2 + 1 + 1 iterations
        else:
            plan = [g1] * 7
        for t in plan:
            t.step()
        torch.cuda.synchronize()
        res.append((float(torch.randn(1)), random.random(),
                    {k: v.detach().clone() for k, v in list(g.state_dict().items()) + list(d.state_dict().items())}))
    (ra, pa, wa), (rb, pb, wb) = res
    # the last draw-ahead (iterations 6, 7) was consumed by the two g1 steps:
    # nothing pending, and both host streams end in the same state
    assert not g1.draws.pending
    assert (ra, pa) == (rb, pb)
    for k in wa:
        err = (wa[k] - wb[k]).abs().max().item()
        assert err <= 1e-6 * max(1.0, wa[k].abs().max().item()), (k, err)


@pytest.mark.parametrize("iters", [1, 2])
def test_graphed_trainer_overlap_equals_eager(iters):
    """The overlapped plan (GraphedTrainer(overlap=True): the G-step's prefix
    graph replayed on a second stream beside the D-step graph, the rest of
    the G-step after both) == the eager sequential iterations, after an odd
    number of replays (both alternating graph sets used); and the eager
    step_split order == step() bitwise."""
    from sgan.data.synthetic import synthetic_batch
    from sgan.scene import SceneIndex
    from sgan.train_step import GanTrainer, GraphedTrainer
    batch = synthetic_batch([20, 7, 13, 20, 2], seed=3, device=DEV)
    batch_g = synthetic_batch([20, 7, 13, 20, 2], seed=4, device=DEV)
    res = []
    for mode in ("eager", "split", "overlap"):
        g, d = build_models()
        tr = GanTrainer(g, d, capturable=True)
        sc = SceneIndex.from_seq_start_end(batch[-1], DEV)
        scg = SceneIndex.from_seq_start_end(batch_g[-1], DEV)
        torch.manual_seed(11)
        random.seed(11)
        n = 1 + 3 * iters
        if mode == "overlap":
            gt = GraphedTrainer(tr, batch, sc, warmup=1, batch_g=batch_g, sc_g=scg, iters=iters, overlap=True)
            for _ in range(3):
                ld, lg = gt.step()
        elif mode == "split":
            for _ in range(n):
                ld, lg = tr.step_split(batch, sc, batch_g, scg, inputs=_inputs(tr, sc))
        else:
            for _ in range(n):
                ld, lg = tr.step(batch, sc, batch_g, scg)
        torch.cuda.synchronize()
        ws = {"g." + k: v.detach().cpu().clone() for k, v in g.state_dict().items()}
        ws.update({"d." + k: v.detach().cpu().clone() for k, v in d.state_dict().items()})
        res.append(({k: float(v) for k, v in list(ld.items()) + list(lg.items())}, ws))
    # eager draws its label-smoothing numbers as Python floats, the other two
    # take them from the float32 StepInputs: 1e-5 there, 1e-6 between those two
    for (la, wa), (lb, wb), tol in ((res[1], res[2], 1e-6), (res[0], res[2], 1e-5)):
        for k in la:
            assert abs(la[k] - lb[k]) <= tol * max(1.0, abs(la[k])), (k, la[k], lb[k])
        for k in wa:
            err = (wa[k] - wb[k]).abs().max().item()
            assert err <= tol * max(1.0, wa[k].abs().max().item()), (k, err)


@pytest.mark.parametrize("graphed,family", [(False, "gat"), (True, "gat"), (False, "gcn"), (True, "gcn"),
                                            (False, "sgangat"), (True, "sgangat")])
def test_paired_context_step_is_bit_identical(graphed, family, monkeypatch):
    """step() with the G-step's context formed at the D-step beside the
    D-step's own (G.context_pair: one GATEncoder launch for both batches; the
    G-step's D forward then runs its whole encoder) == the sequential steps
    (SGG_PAIR=0), bitwise over three iterations, eager and graph-replayed."""
    from sgan import train_step as TS
    from sgan.data.synthetic import synthetic_batch
    from sgan.scene import SceneIndex
    batch = synthetic_batch([20, 7, 13, 20, 2], seed=3, device=DEV)
    # eager: a G batch of other scene / ped counts (its own sizes, not the
    # D batch's, must reach its losses and noise); graphed: the same sizes
    batch_g = synthetic_batch([20, 7, 13, 20, 2] if graphed else [9, 20, 13, 20, 3, 5], seed=4, device=DEV)
    monkeypatch.setattr(TS, "DEC_PAIR", False)   # (test_decoder_pair_step_close: another kernel family)
    res = []
    for pair in (False, True):
        monkeypatch.setattr(TS, "PAIR", pair)
        torch.manual_seed(0)   # (the family's modules the fixture does not cover init alike)
        g, d = build_models(family)
        tr = TS.GanTrainer(g, d, capturable=True)
        sc = SceneIndex.from_seq_start_end(batch[-1], DEV)
        scg = SceneIndex.from_seq_start_end(batch_g[-1], DEV)
        assert tr._pairs(sc, scg) == pair
        torch.manual_seed(5)
        random.seed(5)
        if graphed:
            gt = TS.GraphedTrainer(tr, batch, sc, warmup=1, batch_g=batch_g, sc_g=scg)
            for _ in range(2):
                ld, lg = gt.step()
        else:
            for _ in range(3):
                ld, lg = tr.step(batch, sc, batch_g, scg)
        torch.cuda.synchronize()
        ws = {"g." + k: v.detach().cpu().clone() for k, v in g.state_dict().items()}
        ws.update({"d." + k: v.detach().cpu().clone() for k, v in d.state_dict().items()})
        res.append(({k: float(v) for k, v in list(ld.items()) + list(lg.items())}, ws))
    (la, wa), (lb, wb) = res
    assert la == lb, (la, lb)
    for k in wa:
        assert torch.equal(wa[k], wb[k]), k


@pytest.mark.parametrize("graphed,big", [(False, False), (True, False), (False, True)])
def test_decoder_pair_step_close(graphed, big, monkeypatch):
    """The D-step's generator decoder launched with the G-step's best-of-k
    rollout (kernels.decoder_pair, sgg_lstm_fwd_dec2: the batch-MFMA family,
    which folds the hidden2pos feedback into the recurrence with weights
    pre-scaled for v_exp_f32, where the four-wave family folds it unscaled)
    against the separate launches: the same iterations up to fp32
    reassociation (losses 1e-5, weights within 0.1 lr per step: Adam
    normalises near-zero gradient elements).  big: 4100-ped batches, where
    the D-step decoder itself is on the batch-MFMA family and writes its
    discriminator input as a lone second segment when not paired."""
    from sgan import train_step as TS
    from sgan.data.synthetic import synthetic_batch
    from sgan.scene import SceneIndex
    sizes = [20] * 205 if big else [20, 7, 13, 20, 2]
    batch = synthetic_batch(sizes, seed=3, device=DEV)
    batch_g = synthetic_batch(sizes, seed=4, device=DEV)
    res = []
    for dec_pair in (False, True):
        monkeypatch.setattr(TS, "DEC_PAIR", dec_pair)
        g, d = build_models()
        tr = TS.GanTrainer(g, d, capturable=True)
        sc = SceneIndex.from_seq_start_end(batch[-1], DEV)
        scg = SceneIndex.from_seq_start_end(batch_g[-1], DEV)
        torch.manual_seed(5)
        random.seed(5)
        if graphed:
            gt = TS.GraphedTrainer(tr, batch, sc, warmup=1, batch_g=batch_g, sc_g=scg)
            for _ in range(2):
                ld, lg = gt.step()
        else:
            for _ in range(3):
                ld, lg = tr.step(batch, sc, batch_g, scg)
        torch.cuda.synchronize()
        ws = {"g." + k: v.detach().cpu().clone() for k, v in g.state_dict().items()}
        ws.update({"d." + k: v.detach().cpu().clone() for k, v in d.state_dict().items()})
        res.append(({k: float(v) for k, v in list(ld.items()) + list(lg.items())}, ws))
    (la, wa), (lb, wb) = res
    for k in la:
        assert abs(la[k] - lb[k]) <= 1e-5 * max(1.0, abs(la[k])), (k, la[k], lb[k])
    for k in wa:
        lr = 1e-3 if k.startswith("d.") else 1e-4
        err = (wa[k] - wb[k]).abs().max().item()
        assert err <= 0.1 * lr * 3, (k, err)


def test_rollout_with_second_decoder_segment():
    """sgg_lstm_fwd_dec2: the rollout's sequences bitwise as its own launch
    (sgg_lstm_fwd_dec), the second segment's within 2e-6 of the four-wave
    decoder (another fp32 evaluation order), and its discriminator input
    exactly [head | its own output] (+ [head | b], start positions)."""
    from sgan import _native as N
    lib = N.load()
    torch.manual_seed(21)
    H, T, T0, nz, Dc = 32, 12, 8, 8, 24
    Sc, per, copies = 64, 20, 10
    B1, B2 = copies * Sc * per, Sc * per   # rollout: 10 copies of 64 scenes x 20 peds = 12,800; decoder 1,280
    A, Whh, bias = torch.randn(4 * H, 2, device=DEV) * .3, torch.randn(4 * H, H, device=DEV) * .2, \
        torch.randn(4 * H, device=DEV) * .1
    Wp, bp = torch.randn(2, H, device=DEV) * .3, torch.randn(2, device=DEV) * .1

    def dinit(copies):
        Bper = Sc * per
        ctx = torch.randn(Bper, Dc, device=DEV)
        z = torch.randn(copies, Sc, nz, device=DEV)
        ps = torch.arange(Bper, device=DEV, dtype=torch.int32) // per
        last = torch.randn(Bper, 2, device=DEV) * .3
        d = N.DecInit(N.ptr(ctx), Dc, Dc, N.ptr(z), nz, None, 0, N.ptr(ps), Sc, Bper, N.ptr(last))
        d._keep = (ctx, z, ps, last)
        return d
    d1, d2 = dinit(copies), dinit(1)
    head = torch.randn(T0, B2, 2, device=DEV)
    bgt = torch.randn(T, B2, 2, device=DEV)
    pos0 = torch.randn(B2, 2, device=DEV)
    outs = {}
    for mode in ("two", "one"):
        r1 = torch.full((T, B1, 2), float("nan"), device=DEV)
        r2 = torch.full((T, B2, 2), float("nan"), device=DEV)
        trj = torch.full((T0 + T, 2 * B2, 2), float("nan"), device=DEV)
        st = torch.full((1, 2 * B2, 2), float("nan"), device=DEV)
        to = N.TrajOut(N.ptr(trj), 2 * B2, T0, 0, B2, N.ptr(head), head.stride(0), N.ptr(bgt), bgt.stride(0),
                       N.ptr(pos0), N.ptr(st))
        if mode == "two":
            N.check(lib.sgg_lstm_fwd_dec2(N.ctypes.byref(d1), N.ctypes.byref(d2), N.ptr(A), N.ptr(Whh), N.ptr(bias),
                                          N.ptr(Wp), N.ptr(bp), T, B1, B2, H, N.ptr(r1), N.ptr(r2),
                                          N.ctypes.byref(to), N.stream_ptr()), "dec2")
        else:
            N.check(lib.sgg_lstm_fwd_dec(N.ctypes.byref(d1), N.ptr(A), N.ptr(Whh), N.ptr(bias), N.ptr(Wp),
                                         N.ptr(bp), T, B1, H, None, None, None, N.ptr(r1), None, None,
                                         N.stream_ptr()), "dec rollout")
            N.check(lib.sgg_lstm_fwd_dec(N.ctypes.byref(d2), N.ptr(A), N.ptr(Whh), N.ptr(bias), N.ptr(Wp),
                                         N.ptr(bp), T, B2, H, None, None, None, N.ptr(r2), None, N.ctypes.byref(to),
                                         N.stream_ptr()), "dec four-wave")
        torch.cuda.synchronize()
        outs[mode] = (r1, r2, trj, st)
    (a1, a2, at, ast), (b1, b2, bt, bst) = outs["two"], outs["one"]
    assert torch.equal(a1, b1), "rollout segment"
    close(a2, b2.cpu().numpy(), rtol=2e-6, what="second segment vs four-wave decoder")
    assert torch.equal(at[:T0, :B2], head) and torch.equal(at[:T0, B2:], head), "head steps"
    assert torch.equal(at[T0:, :B2], a2) and torch.equal(at[T0:, B2:], bgt), "generated / real steps"
    assert torch.equal(ast[0, :B2], pos0) and torch.equal(ast[0, B2:], pos0), "start positions"


def _inputs(tr, sc):
    """StepInputs of one iteration drawn in the reference's order (device)."""
    from sgan.train_step import StepInputs
    z_d, z_g, y = tr.draw_inputs(sc.S, 0, sc.S)
    dv = lambda t: t.to(DEV) if t is not None else None
    return StepInputs(dv(z_d), dv(z_g), dv(y))


def test_graphed_trainer_multi_iteration_equals_eager():
    """A graph of two iterations (GraphedTrainer(iters=2), the bench's form:
    the per-replay launch paid once per two iterations) replayed twice ==
    four eager iterations: the host draws of both iterations are made in
    order before each replay."""
    from sgan.data.synthetic import synthetic_batch
    from sgan.scene import SceneIndex
    from sgan.train_step import GanTrainer, GraphedTrainer
    batch = synthetic_batch([20, 7, 13, 20, 2], seed=3, device=DEV)
    batch_g = synthetic_batch([20, 7, 13, 20, 2], seed=4, device=DEV)
    res = []
    for graphed in (False, True):
        g, d = build_models()
        tr = GanTrainer(g, d, capturable=True)
        sc = SceneIndex.from_seq_start_end(batch[-1], DEV)
        scg = SceneIndex.from_seq_start_end(batch_g[-1], DEV)
        torch.manual_seed(11)
        random.seed(11)
        if graphed:
            gt = GraphedTrainer(tr, batch, sc, warmup=1, batch_g=batch_g, sc_g=scg, iters=2)
            for _ in range(2):
                ld, lg = gt.step()
        else:
            for _ in range(5):
                ld, lg = tr.step(batch, sc, batch_g, scg)
        torch.cuda.synchronize()
        ws = {"g." + k: v.detach().cpu().clone() for k, v in g.state_dict().items()}
        ws.update({"d." + k: v.detach().cpu().clone() for k, v in d.state_dict().items()})
        res.append(({k: float(v) for k, v in list(ld.items()) + list(lg.items())}, ws))
    (la, wa), (lb, wb) = res
    for k in la:
        assert abs(la[k] - lb[k]) <= 1e-5 * max(1.0, abs(la[k])), (k, la[k], lb[k])
    for k in wa:
        err = (wa[k] - wb[k]).abs().max().item()
        assert err <= 1e-5 + 1e-5 * wa[k].abs().max().item(), (k, err)


@pytest.mark.parametrize("nh,sizes", [(1, [1, 2, 20, 48, 13, 5]), (1, [20] * 70), (2, [20, 7, 24, 1]),
                                      # past the full backward plan: the compact one (57 / 64 peds), and
                                      # 49 (the full plan's last size) -- real zara1 scenes reach 57
                                      (1, [49, 57, 64, 20, 3]), (1, [64] * 40 + [57] * 7),
                                      (2, [49, 57, 64, 20])])
def test_gat_encoder_fused_equals_per_layer(nh, sizes):
    """The one-launch GATEncoder (sgg_gatenc_fwd / _bwd + sgg_slab_reduce)
    against the per-layer kernels on the same module: outputs, input and
    parameter gradients; label patterns with singletons (label 0), one big
    group, mixed groups, one-ped scenes.  Two heads at 49+ peds exceed every
    LDS plan: the module takes the per-layer kernels there (checked to be
    refused, and the module's result checked against the oracle instead)."""
    from sgan import kernels as K
    from sgan.models import GATEncoder
    from sgan.scene import SceneIndex
    torch.manual_seed(nh)
    mod = GATEncoder([40, 16, 40], nh, 0.0, 0.2).to(DEV)
    B = sum(sizes)
    sc = SceneIndex(np.concatenate([[0], np.cumsum(sizes)]), DEV)
    labs = []
    for k, n in enumerate(sizes):
        pat = k % 3
        labs.append(np.zeros(n) if pat == 0 else np.full(n, 3.0) if pat == 1 else np.random.RandomState(k).randint(0, 4, n))
    lab = torch.from_numpy(np.concatenate(labs).astype(np.float32)).to(DEV).view(-1, 1)
    x = torch.randn(B, 40, device=DEV)
    dy = torch.randn(B, 24, device=DEV)
    if nh > 1 and max(sizes) > 48:
        assert not K.gat_encoder_fused_ok(sc, nh, True)
        _gat_encoder_vs_oracle(mod, nh, x, lab, sc, dy)
        return
    res = []
    for fused in (True, False):
        K.GATENC_FUSED = fused
        try:
            assert K.gat_encoder_fused_ok(sc, nh, True) == fused
            mod.zero_grad(set_to_none=True)
            xi = x.clone().requires_grad_(True)
            y = mod(xi, None, None, lab, scenes=sc)
            (y * dy).sum().backward()
            res.append((y.detach(), xi.grad, {k: p.grad.clone() for k, p in mod.named_parameters()}))
        finally:
            K.GATENC_FUSED = True
    # the two-block input ([encoder state | pooled vector], no cat): bitwise the one-block result
    mod.zero_grad(set_to_none=True)
    x1, x2 = x[:, :32].clone().requires_grad_(True), x[:, 32:].clone().requires_grad_(True)
    y2 = mod((x1, x2), None, None, lab, scenes=sc)
    (y2 * dy).sum().backward()
    assert torch.equal(y2, res[0][0]), "split-input output"
    assert torch.equal(torch.cat([x1.grad, x2.grad], 1), res[0][1]), "split-input dx"
    for k, q in mod.named_parameters():
        assert torch.equal(q.grad, res[0][2][k]), "split-input d" + k
    (yf, dxf, gf), (yr, dxr, gr) = res
    close(yf, yr.cpu().numpy(), rtol=2e-5, what="fused out")
    close(dxf, dxr.cpu().numpy(), rtol=1e-4, what="fused dx")
    fl = 1e-2 * max(float(g.abs().max()) for g in gr.values())
    for k in gr:
        close(gf[k], gr[k].cpu().numpy(), rtol=2e-4, floor=fl, what="fused d" + k)


@pytest.mark.parametrize("nh,sizes_a,sizes_b", [(1, [20, 7, 13, 20, 2], [20, 20, 1, 9]),
                                                  (2, [5, 31, 12], [12, 40, 3, 3]),
                                                  (1, [57, 20, 64], [64, 1, 33])])
def test_gat_encoder_pair_equals_two_launches(nh, sizes_a, sizes_b):
    """sgg_gatenc_fwd2 (a no-grad batch beside one with autograd: the D-step's
    generator and the G-step's context) == two sgg_gatenc_fwd launches,
    bitwise: both outputs, and batch b's saved state through its backward
    (input and parameter gradients)."""
    from sgan import kernels as K
    from sgan.models import GATEncoder
    from sgan.scene import SceneIndex
    torch.manual_seed(7 + nh)
    mod = GATEncoder([40, 16, 40], nh, 0.0, 0.2).to(DEV)
    sca, scb = (SceneIndex(np.concatenate([[0], np.cumsum(sz)]), DEV) for sz in (sizes_a, sizes_b))
    sca.max_n = scb.max_n = max(sca.max_n, scb.max_n)   # one LDS plan for both (a capacity bucket's np_cap)
    Ba, Bb = sum(sizes_a), sum(sizes_b)
    lab_a = torch.randint(0, 4, (Ba,), device=DEV).float()
    lab_b = torch.randint(0, 4, (Bb,), device=DEV).float()
    xa, pa = torch.randn(Ba, 32, device=DEV), torch.randn(Ba, 8, device=DEV)
    xb, pb = torch.randn(Bb, 32, device=DEV), torch.randn(Bb, 8, device=DEV)
    dy = torch.randn(Bb, 24, device=DEV)
    res = []
    for paired in (False, True):
        mod.zero_grad(set_to_none=True)
        xbi, pbi = xb.clone().requires_grad_(True), pb.clone().requires_grad_(True)
        if paired:
            comp = K.GatEncCompanion(xa, lab_a, sca, x2=pa)
            yb = mod((xbi, pbi), None, None, lab_b, scenes=scb, companion=comp)
            ya = comp.y
        else:
            with torch.no_grad():
                ya = mod((xa, pa), None, None, lab_a, scenes=sca)
            yb = mod((xbi, pbi), None, None, lab_b, scenes=scb)
        (yb * dy).sum().backward()
        res.append((ya, yb.detach(), xbi.grad, pbi.grad, {k: q.grad.clone() for k, q in mod.named_parameters()}))
    (a0, b0, dx0, dp0, g0), (a1, b1, dx1, dp1, g1) = res
    assert torch.equal(a0, a1), "companion output"
    assert torch.equal(b0, b1), "carrying batch output"
    assert torch.equal(dx0, dx1) and torch.equal(dp0, dp1), "dx"
    for k in g0:
        assert torch.equal(g0[k], g1[k]), "d" + k


@pytest.mark.parametrize("bf16", [False, True])
def test_gcn_module_pair_equals_two_launches(bf16):
    """sgg_gcnmod_fwd2 (a no-grad batch beside one with autograd) == two
    sgg_gcnmod_fwd launches, bitwise: both outputs and batch b's gradients."""
    from sgan import kernels as K
    from sgan.models import GCNModule
    from sgan.scene import SceneIndex
    torch.manual_seed(3)
    mod = GCNModule(input_dim=40, hidden_dim=72, out_dim=16, gcn_layers=2, final_dim=24).to(DEV)
    sizes_a, sizes_b = [20, 7, 13, 20, 2], [20, 1, 20, 9, 33]
    sca, scb = (SceneIndex(np.concatenate([[0], np.cumsum(sz)]), DEV) for sz in (sizes_a, sizes_b))
    sca.max_n = scb.max_n = max(sca.max_n, scb.max_n)
    Ba, Bb = sum(sizes_a), sum(sizes_b)
    lab_a = torch.randint(0, 4, (Ba,), device=DEV).float()
    lab_b = torch.randint(0, 4, (Bb,), device=DEV).float()
    xa, pa = torch.randn(Ba, 32, device=DEV), torch.randn(Ba, 8, device=DEV)
    xb, pb = torch.randn(Bb, 32, device=DEV), torch.randn(Bb, 8, device=DEV)
    dy = torch.randn(Bb, 24, device=DEV)
    prev = K.precision()
    K.set_precision("bf16" if bf16 else "fp32")
    try:
        res = []
        for paired in (False, True):
            mod.zero_grad(set_to_none=True)
            xbi, pbi = xb.clone().requires_grad_(True), pb.clone().requires_grad_(True)
            if paired:
                comp = K.GcnModCompanion(xa, lab_a, sca, x2=pa)
                yb = mod((xbi, pbi), None, None, lab_b, scenes=scb, companion=comp)
                ya = comp.y
            else:
                with torch.no_grad():
                    ya = mod((xa, pa), None, None, lab_a, scenes=sca)
                yb = mod((xbi, pbi), None, None, lab_b, scenes=scb)
            (yb * dy).sum().backward()
            res.append((ya, yb.detach(), xbi.grad, pbi.grad, {k: q.grad.clone() for k, q in mod.named_parameters()}))
    finally:
        K.set_precision(prev)
    (a0, b0, dx0, dp0, g0), (a1, b1, dx1, dp1, g1) = res
    assert torch.equal(a0, a1) and torch.equal(b0, b1), "outputs"
    assert torch.equal(dx0, dx1) and torch.equal(dp0, dp1), "dx"
    for k in g0:
        assert torch.equal(g0[k], g1[k]), "d" + k


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_gat_layer_pair_equals_two_launches(prec, monkeypatch):
    """sgg_gat_layer_fwd2 (BatchGAT.forward_pair: each batched-GAT layer of a
    no-grad batch and a batch with autograd in one launch) == the two
    batches' own layer launches, bitwise: both outputs, batch b's input and
    parameter gradients (equal segment bounds: one LDS plan either way)."""
    from sgan import kernels as K
    from sgan.models import BatchGATEncoder
    from sgan.scene import SceneIndex
    torch.manual_seed(5)
    enc = BatchGATEncoder([40, 16, 40], [4, 1], 0.0, 0.2).to(DEV)
    for prm in enc.parameters():
        torch.nn.init.normal_(prm, std=0.3)
    sizes_a, sizes_b = [20, 7, 13, 64, 2], [64, 1, 20, 9, 33, 17]
    sca, scb = (SceneIndex(np.concatenate([[0], np.cumsum(sz)]), DEV) for sz in (sizes_a, sizes_b))
    Ba, Bb = sum(sizes_a), sum(sizes_b)
    ha, pa = torch.randn(Ba, 32, device=DEV), torch.randn(Ba, 8, device=DEV)
    hb, pb = torch.randn(Bb, 32, device=DEV), torch.randn(Bb, 8, device=DEV)
    dy = torch.randn(Bb, 40, device=DEV)
    carried = []
    carry = K.GatLayerRider.carry
    monkeypatch.setattr(K.GatLayerRider, "carry", lambda self, *a: (carried.append(1), carry(self, *a))[1])
    prev = K.precision()
    K.set_precision(prec)
    try:
        res = []
        for paired in (False, True):
            enc.zero_grad(set_to_none=True)
            hbi, pbi = hb.clone().requires_grad_(True), pb.clone().requires_grad_(True)
            if paired:
                ya, yb = enc.forward_pair((ha, pa), sca, (hbi, pbi), scb)
                assert len(carried) == 2, "each of the two layers must run as ONE paired launch"
            else:
                with torch.no_grad():
                    ya = enc((ha, pa), None, scenes=sca)
                yb = enc((hbi, pbi), None, scenes=scb)
            (yb * dy).sum().backward()
            res.append((ya, yb.detach(), hbi.grad, pbi.grad, {k: q.grad.clone() for k, q in enc.named_parameters()}))
    finally:
        K.set_precision(prev)
    (a0, b0, dh0, dp0, g0), (a1, b1, dh1, dp1, g1) = res
    assert torch.equal(a0, a1) and torch.equal(b0, b1), "outputs"
    assert torch.equal(dh0, dh1) and torch.equal(dp0, dp1), "input gradients"
    for k in g0:
        assert torch.equal(g0[k], g1[k]), "d" + k


@pytest.mark.parametrize("bn,prec,sizes_a,sizes_b", [
    (8, "fp32", [20, 7, 13, 20, 2, 33], [20, 1, 20, 9, 33, 17]),
    (48, "fp32", [20, 20, 20, 20], [20, 20, 20, 20]),
    (48, "fp32", [64, 3, 57], [64, 64, 1, 12]),
    (8, "bf16", [20, 7, 13, 20, 2, 33], [20, 1, 20, 9, 33, 17]),
    (48, "bf16", [64, 3, 57], [64, 64, 1, 12]),
])
def test_pool_pair_equals_two_launches(bn, prec, sizes_a, sizes_b):
    """sgg_pool_fwd2 (pool_pair: a no-grad batch held, carried by the next
    forward of the same net) == two single-batch launches, bitwise: both
    outputs, batch b's dh and parameter gradients."""
    from sgan import kernels as K
    from sgan.models import PoolHiddenNet
    from sgan.scene import SceneIndex
    torch.manual_seed(bn + len(sizes_a))
    mod = PoolHiddenNet(embedding_dim=16, h_dim=32, mlp_dim=64, bottleneck_dim=bn, batch_norm=False).to(DEV)
    sca, scb = (SceneIndex(np.concatenate([[0], np.cumsum(sz)]), DEV) for sz in (sizes_a, sizes_b))
    Ba, Bb = sum(sizes_a), sum(sizes_b)
    ha, hb0 = torch.randn(Ba, 32, device=DEV), torch.randn(Bb, 32, device=DEV)
    pa, pb = torch.rand(Ba, 2, device=DEV) * 10, torch.rand(Bb, 2, device=DEV) * 10
    dout = torch.randn(Bb, bn, device=DEV)
    prev = K.precision()
    K.set_precision(prec)
    try:
        res = []
        for paired in (False, True):
            mod.zero_grad(set_to_none=True)
            hb = hb0.clone().requires_grad_(True)
            with (K.pool_pair() if paired else contextlib.nullcontext()) as r:
                with torch.no_grad():
                    ya = mod(ha, None, pa, scenes=sca)
                yb = mod(hb, None, pb, scenes=scb)
            if paired:
                assert r.carried, "the second forward did not carry the first"
            (yb * dout).sum().backward()
            res.append((ya, yb.detach(), hb.grad, {k: q.grad.clone() for k, q in mod.named_parameters()}))
    finally:
        K.set_precision(prev)
    (a0, b0, d0, g0), (a1, b1, d1, g1) = res
    assert torch.equal(a0, a1) and torch.equal(b0, b1), "outputs"
    assert torch.equal(d0, d1), "dh"
    for k in g0:
        assert torch.equal(g0[k], g1[k]), "d" + k


def _gat_encoder_vs_oracle(mod, nh, x, lab, sc, dy):
    """The product GATEncoder (whatever path it takes) against the oracle's
    reference-formulation module with the same weights: output, dx, grads."""
    from oracle import sgan_oracle as O
    ref = O.GATEncoder([40, 16, 40], nh, 0.0, 0.2)
    ref.load_state_dict({k: v.detach().cpu() for k, v in mod.state_dict().items()})
    sse = torch.tensor(np.stack([sc.host_off[:-1], sc.host_off[1:]], 1))
    xr = x.detach().cpu().clone().requires_grad_(True)
    yr = ref(xr, sse, None, lab.cpu())
    (yr * dy.cpu()).sum().backward()
    mod.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(True)
    y = mod(xi, None, None, lab, scenes=sc)
    (y * dy).sum().backward()
    close(y, yr.detach().numpy(), rtol=2e-5, what="out vs oracle")
    close(xi.grad, xr.grad.numpy(), rtol=1e-4, what="dx vs oracle")
    gref = dict(ref.named_parameters())
    fl = 1e-2 * max(float(g.grad.abs().max()) for g in gref.values())
    for k, q in mod.named_parameters():
        close(q.grad, gref[k].grad.numpy(), rtol=2e-4, floor=fl, what="d%s vs oracle" % k)


@pytest.mark.parametrize("prec,sizes", [("fp32", [1, 2, 20, 48, 13, 5, 64]), ("fp32", [20] * 600),
                                        ("fp32", [3, 0, 7, 1]), ("bf16", [20, 7, 24, 1, 64])])
def test_gcn_module_fused_equals_per_op(prec, sizes):
    """The one-launch GCNModule (sgg_gcnmod_fwd / _bwd + sgg_slab_reduce)
    against the per-op kernels (group pooling + sgg_xw per layer) on the same
    module: outputs, input and parameter gradients; singletons (label 0), one
    big group, mixed groups, one-ped and empty scenes; 600 scenes (more than
    the backward's 512 workgroups: a workgroup accumulates several scenes);
    the bf16 node transforms of set_precision("bf16")."""
    from sgan import kernels as K
    from sgan.models import GCNModule
    from sgan.scene import SceneIndex
    torch.manual_seed(len(sizes))
    mod = GCNModule(40, 72, 16, 2, 24).to(DEV)
    with torch.no_grad():   # the reference's unscaled randn init makes ReLU-dead columns the rule; tame it
        for p in mod.parameters():
            if p.dim() == 2 and p.shape[1] in (72, 16):
                p.mul_(0.2)
    B = sum(sizes)
    sc = SceneIndex(np.concatenate([[0], np.cumsum(sizes)]), DEV)
    labs = []
    for k, n in enumerate(sizes):
        pat = k % 3
        labs.append(np.zeros(n) if pat == 0 else np.full(n, 3.0) if pat == 1 else np.random.RandomState(k).randint(0, 4, n))
    lab = torch.from_numpy(np.concatenate(labs).astype(np.float32)).to(DEV).view(-1, 1)
    x = torch.randn(B, 40, device=DEV)
    dy = torch.randn(B, 24, device=DEV)
    res = []
    K.set_precision(prec)
    try:
        for fused in (True, False):
            K.GCNMOD_FUSED = fused
            assert K.gcn_module_fused_ok(sc, 40, 24) == fused
            mod.zero_grad(set_to_none=True)
            xi = x.clone().requires_grad_(True)
            y = mod(xi, None, None, lab, scenes=sc)
            (y * dy).sum().backward()
            res.append((y.detach(), xi.grad, {k: p.grad.clone() for k, p in mod.named_parameters()}))
        K.GCNMOD_FUSED = True
        # the two-block input ([encoder state | pooled vector], no cat): bitwise the one-block result
        mod.zero_grad(set_to_none=True)
        x1, x2 = x[:, :32].clone().requires_grad_(True), x[:, 32:].clone().requires_grad_(True)
        y2 = mod((x1, x2), None, None, lab, scenes=sc)
        (y2 * dy).sum().backward()
    finally:
        K.GCNMOD_FUSED = True
        K.set_precision("fp32")
    assert torch.equal(y2, res[0][0]), "split-input output"
    assert torch.equal(torch.cat([x1.grad, x2.grad], 1), res[0][1]), "split-input dx"
    for k, q in mod.named_parameters():
        assert torch.equal(q.grad, res[0][2][k]), "split-input d" + k
    (yf, dxf, gf), (yr, dxr, gr) = res
    # bf16: both paths round their own (differently summed) operands to bf16
    t_out, t_dx, t_dw = (2e-2, 2e-2, 2e-2) if prec == "bf16" else (2e-5, 1e-4, 2e-4)
    close(yf, yr.cpu().numpy(), rtol=t_out, what="fused out")
    close(dxf, dxr.cpu().numpy(), rtol=t_dx, what="fused dx")
    fl = 1e-2 * max(float(g.abs().max()) for g in gr.values())
    for k in gr:
        close(gf[k], gr[k].cpu().numpy(), rtol=t_dw, floor=fl, what="fused d" + k)


@pytest.mark.parametrize("graph", ["gat", "sgangat"])
def test_deferred_grad_finish_is_bit_identical(graph):
    """The trainer's deferred weight-gradient finish (every backward op's
    GradFinish queued, then issued together: defer_grad_finish / grad_flush)
    against each op finishing in its own launches: every gradient of a D-step
    and a G-step bit-identical."""
    import contextlib
    from sgan.data.synthetic import synthetic_batch
    from sgan.scene import SceneIndex
    from sgan.train_step import GanTrainer, KernelOps
    sizes = [20, 7, 13, 20, 2] if graph == "gat" else [64, 30, 5]
    batch = synthetic_batch(sizes, seed=5, device=DEV)
    sc = SceneIndex.from_seq_start_end(batch[-1], DEV)

    class Immediate(KernelOps):
        defer_finish = staticmethod(contextlib.nullcontext)
    res = []
    for ops in (KernelOps(), Immediate()):
        g, d = build_models(graph)
        tr = GanTrainer(g, d, ops=ops)
        torch.manual_seed(3)
        random.seed(3)
        grads = {}
        tr.d_step(batch, sc)
        grads.update({"d." + k: p.grad.detach().clone() for k, p in d.named_parameters() if p.grad is not None})
        tr.g_step(batch, sc)
        grads.update({"g." + k: p.grad.detach().clone() for k, p in g.named_parameters() if p.grad is not None})
        res.append(grads)
    a, b = res
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (k, (a[k] - b[k]).abs().max().item())


@pytest.mark.parametrize("graph", ["gat", "sgangat"])
def test_head_fused_is_bit_identical(graph, monkeypatch):
    """The discriminator head's forward held until the BCE forward and issued
    with its backward for the backward seed (sgg_head_fwdbwd, BceLink.run_fused)
    against the two launches: losses and every gradient of a D-step and a
    G-step bit-identical; the fused runs issue no separate head forward and
    accept the seed (no fallback recompute)."""
    from sgan import kernels as K
    from sgan.data.synthetic import synthetic_batch
    from sgan.scene import SceneIndex
    from sgan.train_step import GanTrainer
    sizes = [20, 7, 13, 20, 2] if graph == "gat" else [64, 30, 5]
    batch = synthetic_batch(sizes, seed=5, device=DEV)
    sc = SceneIndex.from_seq_start_end(batch[-1], DEV)
    calls = [0]
    plain = K._head_fwd

    def counted(*a, **k):
        calls[0] += 1
        return plain(*a, **k)
    monkeypatch.setattr(K, "_head_fwd", counted)
    res = []
    for fuse in (True, False):
        monkeypatch.setattr(K, "HEAD_FUSE", fuse)
        calls[0] = 0
        g, d = build_models(graph)
        tr = GanTrainer(g, d)
        torch.manual_seed(3)
        random.seed(3)
        out = {}
        out.update({"loss." + k: torch.tensor(float(v)) for k, v in tr.d_step(batch, sc).items()})
        out.update({"d." + k: p.grad.detach().clone() for k, p in d.named_parameters() if p.grad is not None})
        out.update({"loss." + k: torch.tensor(float(v)) for k, v in tr.g_step(batch, sc).items()})
        out.update({"g." + k: p.grad.detach().clone() for k, p in g.named_parameters() if p.grad is not None})
        res.append(out)
        assert (calls[0] == 0) == fuse, (fuse, calls[0])
    a, b = res
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (k, (a[k] - b[k]).abs().max().item())


@pytest.mark.parametrize("graph,sizes", [("gat", [20, 7, 13, 20, 4]), ("gat", [20, 7, 13, 20, 2]),
                                         ("gcn", [64, 30, 2])])
def test_shared_prefix_is_bit_identical(graph, sizes):
    """The discriminator encoder's observed steps run once beside the
    generator's encoder (kernels.SharedPrefix: sgg_lstm_fwd_seg2, the
    suffix from step obs_len by sgg_lstm_fwd_seg, the D-step backward through
    sgg_lstm_bwd_shared) against the full 20-step sequences: losses and every
    gradient of a D-step and a G-step bit-identical.  B = 64 takes the shared
    path in both steps; B = 62 (not a multiple of 16) only in the G-step."""
    import contextlib
    from sgan import kernels as K
    from sgan.data.synthetic import synthetic_batch
    from sgan.scene import SceneIndex
    from sgan.train_step import GanTrainer, KernelOps
    batch = synthetic_batch(sizes, seed=5, device=DEV)
    sc = SceneIndex.from_seq_start_end(batch[-1], DEV)
    seen = []

    class Probe(KernelOps):
        @staticmethod
        @contextlib.contextmanager
        def shared_prefix(*a):
            with K.shared_prefix(*a) as p:
                yield p
            seen.append((p.ok, p.ran, p.used))

    class Full(KernelOps):
        shared_prefix = None
    res = []
    for ops in (Probe(), Full()):
        g, d = build_models(graph)
        tr = GanTrainer(g, d, ops=ops)
        torch.manual_seed(3)
        random.seed(3)
        out = {}
        ld = tr.d_step(batch, sc)
        out.update({"d." + k: p.grad.detach().clone() for k, p in d.named_parameters() if p.grad is not None})
        lg = tr.g_step(batch, sc)
        out.update({"g." + k: p.grad.detach().clone() for k, p in g.named_parameters() if p.grad is not None})
        out.update({"loss." + k: torch.tensor(float(v)) for k, v in list(ld.items()) + list(lg.items())})
        res.append(out)
    B = sum(sizes)
    assert seen == [(B % 16 == 0, B % 16 == 0, B % 16 == 0), (True, True, True)], seen
    a, b = res
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (k, (a[k] - b[k]).abs().max().item())


@pytest.mark.parametrize("H", [32, 48])
def test_lstm_backward_nonzero_c0_per_block(H):
    """C ABI: a batch of three 16-ped blocks with a nonzero initial cell c0
    (sgg_lstm_fwd / sgg_lstm_bwd with weight gradients and dh0) equals the
    three blocks run one at a time, bitwise: drel_in, dh0 and each block's
    slab row.  (Regression: the four-wave backward once read block 0's
    c_{-1} for every block.)"""
    from sgan import _native as N
    lib = N.load()
    torch.manual_seed(H)
    T, B = 6, 48
    f = lambda *s, sc=0.3: (torch.randn(*s, device=DEV) * sc).contiguous()
    A, Whh, bias = f(4 * H, 2), f(4 * H, H, sc=0.2), f(4 * H)
    rel, h0, c0, dh_last = f(T, B, 2), f(B, H), f(B, H), f(B, H)
    P = 4 * H * H + 4 * H + 8 * H

    def run(lo, hi):
        n = hi - lo
        r, h, c, d = (rel[:, lo:hi].contiguous(), h0[lo:hi].contiguous(), c0[lo:hi].contiguous(),
                      dh_last[lo:hi].contiguous())
        sf = lambda w: torch.empty(int(lib.sgg_lstm_state_floats(T, n, H, w)), device=DEV)
        h_all, c_all, act = torch.empty(T + 1, n, H, device=DEV), sf(1), sf(0)
        N.check(lib.sgg_lstm_fwd(N.ptr(r), N.ptr(A), N.ptr(Whh), N.ptr(bias), N.ptr(h), N.ptr(c), None, None, T, n,
                                 H, 0, N.ptr(h_all), N.ptr(c_all), N.ptr(act), None, N.stream_ptr()), "fwd")
        rows = int(lib.sgg_lstm_wpart_rows(H, n))
        assert rows == n // 16
        wpart = torch.empty(rows, P, device=DEV)
        drel, dh0 = torch.empty(T, n, 2, device=DEV), torch.empty(n, H, device=DEV)
        N.check(lib.sgg_lstm_bwd(N.ptr(A), N.ptr(Whh), None, N.ptr(h_all), N.ptr(c_all), N.ptr(act), N.ptr(r), None,
                                 N.ptr(d), None, T, n, H, 0, None, N.ptr(dh0), N.ptr(drel), None, N.ptr(wpart),
                                 N.stream_ptr()), "bwd")
        torch.cuda.synchronize()
        return drel, dh0, wpart

    full = run(0, B)
    parts = [run(16 * k, 16 * k + 16) for k in range(3)]
    assert torch.equal(full[0], torch.cat([p[0] for p in parts], 1)), "drel_in"
    assert torch.equal(full[1], torch.cat([p[1] for p in parts], 0)), "dh0"
    assert torch.equal(full[2], torch.cat([p[2] for p in parts], 0)), "slab rows"


def test_lstm_segments_equal_full_sequence():
    """C ABI: a 3-copy batch whose first 5 steps are shared -- prefix on 32
    peds beside another encoder in one launch (sgg_lstm_fwd_seg2), suffix on
    96 peds (sgg_lstm_fwd_seg, t0 = 5, Bsrc = 32), backward with weight
    gradients (sgg_lstm_bwd_shared) -- against sgg_lstm_fwd / sgg_lstm_bwd of
    the full sequence: h, U, drel_in and the slab bit-identical."""
    from sgan import _native as N
    lib = N.load()
    torch.manual_seed(2)
    T, T0, Bs, C, H, NU = 11, 5, 32, 3, 48, 64
    B = Bs * C
    f = lambda *s, sc=0.3: (torch.randn(*s, device=DEV) * sc).contiguous()
    A, Whh, bias = f(4 * H, 2), f(4 * H, H, sc=0.2), f(4 * H)
    Wu, cu = f(NU, H), f(NU)
    head = f(T0, Bs, 2)
    rel = torch.cat([head.repeat(1, C, 1), f(T - T0, B, 2)], 0).contiguous()
    sf = lambda w: torch.empty(int(lib.sgg_lstm_state_floats(T, B, H, w)), device=DEV)
    P = 4 * H * H + 4 * H + 8 * H
    rows = int(lib.sgg_lstm_wpart_rows(H, B))
    dh_last = f(B, H)

    def run(shared):
        h_all, c_all, act = torch.empty(T + 1, B, H, device=DEV), sf(1), sf(0)
        U = torch.empty(B, NU, device=DEV)
        if shared:
            # another encoder (H = 32, 32 peds, 5 steps) in the same launch as the prefix
            A2, W2, b2 = f(128, 2), f(128, 32, sc=0.2), f(128)
            h2 = torch.empty(T0 + 1, Bs, 32, device=DEV)
            g2 = N.LstmSeg(N.ptr(head), N.ptr(A2), N.ptr(W2), N.ptr(b2), None, None, T0, Bs, Bs, 0, T0, Bs,
                           N.ptr(h2), None, None, None, 0, None, 0, None)
            pre = N.LstmSeg(N.ptr(head), N.ptr(A), N.ptr(Whh), N.ptr(bias), None, None, T0, Bs, B, 0, T, Bs,
                            N.ptr(h_all), N.ptr(c_all), N.ptr(act), None, 0, None, 0, None)
            N.check(lib.sgg_lstm_fwd_seg2(N.ctypes.byref(g2), 32, N.ctypes.byref(pre), H, N.stream_ptr()), "seg2")
            suf = N.LstmSeg(N.ptr(rel), N.ptr(A), N.ptr(Whh), N.ptr(bias), None, None, T - T0, B, B, T0, T, Bs,
                            N.ptr(h_all), N.ptr(c_all), N.ptr(act), N.ptr(Wu), Wu.stride(0), N.ptr(cu), NU, N.ptr(U))
            N.check(lib.sgg_lstm_fwd_seg(N.ctypes.byref(suf), H, N.stream_ptr()), "seg")
        else:
            N.check(lib.sgg_lstm_fwd_u(N.ptr(rel), N.ptr(A), N.ptr(Whh), N.ptr(bias), None, None, T, B, H,
                                       N.ptr(h_all), N.ptr(c_all), N.ptr(act), N.ptr(Wu), Wu.stride(0), N.ptr(cu),
                                       NU, N.ptr(U), N.stream_ptr()), "fwd_u")
        drel = torch.empty(T, B, 2, device=DEV)
        wpart = torch.empty(rows, P, device=DEV)
        if shared:
            N.check(lib.sgg_lstm_bwd_shared(N.ptr(A), N.ptr(Whh), N.ptr(h_all), N.ptr(c_all), N.ptr(act), N.ptr(rel),
                                            N.ptr(dh_last), T, B, H, T0, Bs, N.ptr(drel), N.ptr(wpart),
                                            N.stream_ptr()), "bwd_shared")
        else:
            N.check(lib.sgg_lstm_bwd(N.ptr(A), N.ptr(Whh), None, N.ptr(h_all), N.ptr(c_all), N.ptr(act), N.ptr(rel),
                                     None, N.ptr(dh_last), None, T, B, H, 0, None, None, N.ptr(drel), None,
                                     N.ptr(wpart), N.stream_ptr()), "bwd")
        torch.cuda.synchronize()
        return h_all[T0 + 1:].clone(), U, drel, wpart

    for x, y, nm in zip(run(True), run(False), ("h", "U", "drel_in", "slab")):
        assert torch.equal(x, y), (nm, (x - y).abs().max().item())


def test_step_glue_kernels_match_torch():
    """glue.hip (sgg_traj_cat, sgg_decoder_init, sgg_l2_select,
    sgg_l2_loss_fwd/bwd) against the reference's torch expressions
    (train.py:409-415, 443-470; losses.py:52-71; models.py:827-850)."""
    from sgan import kernels as K
    from sgan.scene import SceneIndex
    torch.manual_seed(11)
    sizes = [20, 1, 7, 13, 20, 2]
    B, S, T, k = sum(sizes), len(sizes), 12, 5
    sc = SceneIndex(np.concatenate([[0], np.cumsum(sizes)]), DEV)
    seg = sc.ped_scene_long()
    obs_rel, a, b = torch.randn(8, B, 2, device=DEV), torch.randn(T, B, 2, device=DEV), torch.randn(T, B, 2, device=DEV)
    wide = torch.randn(T, 2 * B, 2, device=DEV)
    close(K.traj_cat(obs_rel, a, b), torch.cat([torch.cat([obs_rel, a]), torch.cat([obs_rel, b])], 1).cpu().numpy(),
          rtol=0, what="traj_cat")
    ar = wide[:, B:].requires_grad_(False)
    close(K.traj_cat(obs_rel, ar), torch.cat([obs_rel, ar]).cpu().numpy(), rtol=0, what="traj_cat slice")
    pos0 = torch.randn(B, 2, device=DEV)
    tr, st = K.traj_cat(obs_rel, a, b, pos0)
    close(tr, torch.cat([torch.cat([obs_rel, a]), torch.cat([obs_rel, b])], 1).cpu().numpy(), rtol=0,
          what="traj_cat + start")
    close(st, pos0.unsqueeze(0).repeat(1, 2, 1).cpu().numpy(), rtol=0, what="traj_cat start positions")
    # decoder init: copies with a best index
    ctx = torch.randn(B, 24, device=DEV, requires_grad=True)
    z = torch.randn(k, S, 8, device=DEV)
    best = torch.randint(0, k, (S,), device=DEV)
    last = torch.randn(B, 2, device=DEV)
    h0, rel0 = K.decoder_init(ctx, z, best, k - 1, 2, sc, last)
    zc = torch.cat([z[best, torch.arange(S, device=DEV)], z[k - 1]], 0)
    ref = torch.cat([ctx.repeat(2, 1), zc.index_select(0, sc.repeat(2).ped_scene_long())], 1)
    close(h0, ref.detach().cpu().numpy(), rtol=0, what="decoder_init h0")
    close(rel0, last.repeat(2, 1).cpu().numpy(), rtol=0, what="decoder_init rel0")
    g = torch.randn_like(h0)
    (h0 * g).sum().backward()
    close(ctx.grad, (g[:B, :24] + g[B:, :24]).cpu().numpy(), rtol=1e-6, what="decoder_init dctx")
    # best-of-k selection and the selected sample's l2 term
    gt = torch.randn(T, B, 2, device=DEV)
    pred = torch.randn(T, k * B, 2, device=DEV)
    lm = (torch.rand(B, 8 + T, device=DEV) > 0.2).float()
    mask = lm[:, 8:]
    l2 = ((gt.unsqueeze(1) - pred.view(T, k, B, 2)) ** 2).sum(3) * mask.t().unsqueeze(1)
    ref_best = torch.zeros(k, S, device=DEV).index_add_(1, seg, l2.sum(0)).argmin(0)
    assert torch.equal(K.l2_select(pred, gt, mask, sc, k), ref_best)
    p = torch.randn(T, 2 * B, 2, device=DEV)
    pv = p[:, :B].clone().requires_grad_(True)
    loss = K.l2_loss(p[:, :B], gt, mask, sc, 1.0)
    num = torch.zeros(S, device=DEV).index_add_(0, seg, (mask.t().unsqueeze(2) * (gt - pv) ** 2).sum((0, 2)))
    den = torch.zeros(S, device=DEV).index_add_(0, seg, mask.sum(1))
    ref_loss = (num / den).sum()
    close(loss, ref_loss.detach().cpu().numpy(), rtol=1e-5, what="l2 loss")
    ref_loss.backward()
    pk = p[:, :B].clone().requires_grad_(True)
    K.l2_loss(pk, gt, mask, sc, 1.0).backward()
    close(pk.grad, pv.grad.cpu().numpy(), rtol=1e-5, what="l2 loss grad")


@pytest.mark.parametrize("max_norm", [0.0, 2.0, 1e6])
def test_clip_adam_matches_torch(max_norm):
    """sgg_adam_step (ClipAdam) against nn.utils.clip_grad_norm_ + optim.Adam
    (scripts/train.py:418-427, :472-482) over 3 steps, one parameter without a
    gradient in the second step (skipped by both, its step does not advance)."""
    from sgan.kernels import ClipAdam
    torch.manual_seed(7)
    shapes = [(512, 48), (512,), (48, 512), (48,), (7,), (192, 48), (3, 5, 2)]
    ref = [torch.randn(s, device=DEV) for s in shapes]
    ours = [r.clone() for r in ref]
    o_ref = torch.optim.Adam(ref, lr=1e-3)
    o_our = ClipAdam(ours, lr=1e-3)
    for it in range(3):
        for i, (a, b) in enumerate(zip(ref, ours)):
            if it == 1 and i == 4:
                a.grad = b.grad = None
                continue
            g = torch.randn_like(a) * (0.5 + i)
            a.grad, b.grad = g.clone(), g.clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(ref, max_norm)
        o_ref.step()
        o_our.step(max_norm=max_norm)
        for i, (a, b) in enumerate(zip(ref, ours)):
            close(b.detach(), a.detach().cpu(), rtol=2e-6, floor=1e-6, what="param %d it %d" % (i, it))
            if a.grad is not None:
                close(b.grad, a.grad.cpu(), rtol=2e-6, floor=1e-6, what="clipped grad %d it %d" % (i, it))
            sa, sb = o_ref.state[a], o_our.opt.state[b]
            assert float(sa["step"]) == float(sb["step"]), (i, it)
            close(sb["exp_avg_sq"], sa["exp_avg_sq"].cpu(), rtol=2e-6, floor=1e-9, what="v %d it %d" % (i, it))


@pytest.mark.parametrize("bn,H,sizes", [(48, 48, [20] * 12 + [64, 3]), (8, 32, [20] * 40 + [57, 1])])
def test_pool_backward_one_launch_equals_two(bn, H, sizes):
    """The pooling backward's dh = dU W1h and h^T dU partials in one launch
    (sgg_pool_dh_dw) are bit-identical to the two separate launches (sgg_xw,
    sgg_xtw_partial): same bodies, same split order -- with and without the
    accumulated gradient of h from the graph module (GradLink)."""
    from sgan import kernels as K
    from sgan.models import PoolHiddenNet
    from sgan.scene import SceneIndex
    torch.manual_seed(bn + H)
    mod = PoolHiddenNet(embedding_dim=16, h_dim=H, mlp_dim=64, bottleneck_dim=bn, batch_norm=False).to(DEV)
    off = np.concatenate([[0], np.cumsum(sizes)])
    sc = SceneIndex(off, DEV)
    B = int(off[-1])
    h0 = torch.randn(B, H, device=DEV)
    pos = torch.rand(B, 2, device=DEV) * 10
    dout = torch.randn(B, bn, device=DEV)
    res = []
    for dual in (True, False):
        K.DUAL_POOL_BWD = dual
        try:
            mod.zero_grad(set_to_none=True)
            h = h0.clone().requires_grad_(True)
            y = mod(h, None, pos, scenes=sc)
            (y * dout).sum().backward()
            res.append((h.grad.clone(), {k: p.grad.clone() for k, p in mod.named_parameters()}))
        finally:
            K.DUAL_POOL_BWD = True
    (da, ga), (db, gb) = res
    assert torch.equal(da, db), "dh"
    for k in ga:
        assert torch.equal(ga[k], gb[k]), "d" + k


def _gat_attention_ref(wh, a, bias, labels, seg_off, mode, epi, heads, alpha=0.2):
    """fp64 torch restatement of the attention layer (models.py:184-220, the
    multi-head GAT.py:6-55 text): per segment and head, masked softmax of
    LeakyReLU(s_i + t_j), att @ Wh + bias, then the epilogue."""
    n, HF = wh.shape
    F = HF // heads
    y = torch.zeros(n, HF, dtype=torch.float64, device=wh.device)
    ys = []
    so = seg_off.tolist()
    for g in range(len(so) - 1):
        o, e = so[g], so[g + 1]
        if e == o:
            continue
        cols = []
        for h in range(heads):
            W = wh[o:e, h * F:(h + 1) * F]
            s = W @ a[h, :F]
            t = W @ a[h, F:]
            z = torch.nn.functional.leaky_relu(s[:, None] + t[None, :], alpha)
            if mode == 0:
                lab = labels[o:e].view(-1)
                m = (lab[:, None] == lab[None, :]) & (lab[:, None] != 0)
                m = m | torch.eye(e - o, dtype=torch.bool, device=wh.device)
                z = z.masked_fill(~m, float("-inf"))
            out = torch.softmax(z, 1) @ W
            if bias is not None:
                out = out + bias
            if epi:
                out = torch.nn.functional.elu(out)
            if epi == 2:
                out = torch.log_softmax(out, 1)
            cols.append(out)
        ys.append((o, e, torch.cat(cols, 1)))
    for o, e, v in ys:
        y = torch.cat([y[:o], v, y[e:]], 0)
    return y


@pytest.mark.parametrize("heads,F,sizes,mode,epi,use_bias,pad", [
    (4, 16, [64] * 9, 1, 1, True, 0),           # configs[4] batched GAT, layer 1
    (1, 40, [64] * 9, 1, 0, True, 0),           # layer 2
    (4, 16, [20, 1, 64, 7, 33], 1, 1, True, 3),  # ragged, pad rows past the last segment
    (1, 16, [20, 7, 1, 33, 5], 0, 1, False, 0),  # GAT family layer 1, label mask
    (1, 40, [5, 20, 64, 3], 0, 2, False, 0),     # layer 2: log_softmax epilogue
    (2, 17, [100, 128, 9], 0, 1, False, 0),      # > 64 nodes, F not a multiple of 4
    (1, 128, [30, 2], 1, 0, True, 0),            # widest F
    (3, 1, [12, 40], 1, 1, True, 0),             # F = 1
])
def test_gat_attention_vs_torch(heads, F, sizes, mode, epi, use_bias, pad):
    """sgg_gat_fwd / sgg_gat_bwd (MFMA tiles) against an fp64 torch
    restatement: the output, and the gradients of Wh, a and the bias through
    the kernel's dWh / ds / dt; pad rows past the last segment stay zero.
    The same for sgg_gat_fwd_ex / _bwd_ex (a_src / a_dst apart, da and dbias
    reduced on the device)."""
    from sgan import kernels as K
    torch.manual_seed(heads * 100 + F)
    n_seg = sum(sizes)
    n = n_seg + pad
    seg_off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=DEV)
    labels = None
    if mode == 0:
        rs = np.random.RandomState(F)
        labels = torch.from_numpy(rs.randint(0, 4, n).astype(np.float32)).to(DEV).view(-1, 1)
    graph = K.SegmentGraph(seg_off, len(sizes), max(sizes), mode, labels)
    wh = torch.randn(n, heads * F, device=DEV)
    if pad:
        wh[n_seg:] = 0
    a = torch.randn(heads, 2 * F, device=DEV) * 0.5
    bias = torch.randn(F, device=DEV) * 0.1 if use_bias else None
    dy = torch.randn(n, heads * F, device=DEV)
    dy[n_seg:] = 0      # pad rows are read by no consumer
    wr = wh.double().requires_grad_(True)
    ar = a.double().requires_grad_(True)
    br = bias.double().requires_grad_(True) if use_bias else None
    yr = _gat_attention_ref(wr, ar, br, labels, seg_off, mode, epi, heads)
    (yr * dy.double()).sum().backward()
    for ex in (False, True):
        whg = wh.clone().requires_grad_(True)
        bg = bias.clone().requires_grad_(True) if use_bias else None
        if ex:    # sgg_gat_fwd_ex / _bwd_ex: a_src, a_dst apart, parameter gradients on the device
            asg = a[:, :F].clone().view(heads, F, 1).requires_grad_(True)
            adg = a[:, F:].clone().view(heads, F, 1).requires_grad_(True)
            y = K.gat_attention_ex(whg, asg, adg, 0.2, graph, epi, heads=heads, bias=bg)
        else:
            ag = a.clone().requires_grad_(True)
            y = K.gat_attention(whg, ag, 0.2, graph, epi, heads=heads, bias=bg)
        (y * dy).sum().backward()
        w = "ex " if ex else ""
        close(y, yr.detach().cpu().numpy(), rtol=2e-5, what=w + "y")
        if pad:
            assert torch.equal(y[n_seg:], torch.zeros_like(y[n_seg:]))
            assert torch.equal(whg.grad[n_seg:], torch.zeros_like(whg.grad[n_seg:]))
        close(whg.grad[:n_seg], wr.grad[:n_seg].cpu().numpy(), rtol=1e-4, what=w + "dWh")
        da = torch.cat([asg.grad.view(heads, F), adg.grad.view(heads, F)], 1) if ex else ag.grad
        close(da, ar.grad.cpu().numpy(), rtol=1e-4, what=w + "da")
        if use_bias:
            close(bg.grad, br.grad.cpu().numpy(), rtol=1e-4, what=w + "dbias")


def _batch_gat_ref(x, mod, seg_off):
    """fp64 torch restatement of the sgangat batched GAT (GAT.py:58-89 text):
    per layer InstanceNorm1d over each segment's rows (biased variance, eps
    1e-5), then per head softmax(LeakyReLU(s_i + t_j)) @ Wh + bias, heads
    concatenated, ELU on all but the last layer."""
    layers = mod.gat_net.layer_stack
    for i, l in enumerate(layers):
        so = seg_off.tolist()
        parts = []
        for g in range(len(so) - 1):
            v = x[so[g]:so[g + 1]]
            mu = v.mean(0, keepdim=True)
            var = ((v - mu) ** 2).mean(0, keepdim=True)
            parts.append((v - mu) / torch.sqrt(var + 1e-5))
        xn = torch.cat(parts, 0)
        H, Fo = l.n_head, l.f_out
        wh = torch.cat([xn @ l.w.double()[h] for h in range(H)], 1)
        a = torch.cat([l.a_src.double().view(H, Fo), l.a_dst.double().view(H, Fo)], 1)
        x = _gat_attention_ref(wh, a, l.bias.double(), None, seg_off, 1, 0 if i + 1 == len(layers) else 1, H)
    return x


@pytest.mark.parametrize("sizes,prec", [([64] * 9, "fp32"), ([20, 1, 64, 7, 33], "fp32"), ([64] * 9, "bf16"),
                                        ([5, 100, 128, 2], "fp32")])
def test_gat_layer_fused_equals_per_op(sizes, prec):
    """The sgangat batched GAT with each layer in one sgg_gat_layer_fwd launch
    (instance norm + node transform + attention) against the per-op path
    (sgg_seg_norm_fwd, sgg_xw / sgg_xw_bf16, sgg_gat_fwd_ex) on the same
    module.  Both are measured against an fp64 torch restatement: the fused
    path's error is at most twice the largest error of the per-op path on
    the exact input and three 1-ulp perturbations of it, plus 1e-5 of scale
    (the bias gradients are near-cancelling sums over each scene's rows:
    equally exact fp32 evaluations spread by ~1e-4 there; bf16: the shared
    bf16 rounding of the node transform dominates both paths);
    the two-block input ([h | pool_h], no concatenation) is bitwise the
    one-block result."""
    from sgan import kernels as K
    from sgan.models import BatchGAT, BatchGATEncoder
    from sgan.scene import SceneIndex
    torch.manual_seed(len(sizes))
    mod = BatchGATEncoder([40, 16, 40], [4, 1], 0.0, 0.2).to(DEV)
    with torch.no_grad():
        for l in mod.gat_net.layer_stack:
            l.bias.normal_(0, 0.1)
    B = sum(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)])
    sc = SceneIndex(off, DEV)
    x = torch.randn(B, 40, device=DEV)
    dy = torch.randn(B, 40, device=DEV)
    res = []
    gen = torch.Generator(device="cpu").manual_seed(7)
    K.set_precision(prec)
    try:
        # fused; per-op on x and on three 1-ulp random perturbations of x
        for v, fused in enumerate((True, False, False, False, False)):
            BatchGAT.LAYER_FUSED = fused
            mod.zero_grad(set_to_none=True)
            xv = x if v < 2 else x * (1 + torch.randint(-1, 2, x.shape, generator=gen).float().to(DEV) * 2.0 ** -23)
            xi = xv.clone().requires_grad_(True)
            y = mod(xi, None, scenes=sc)
            (y * dy).sum().backward()
            res.append((y.detach(), xi.grad, {k: p.grad.clone() for k, p in mod.named_parameters()}))
        BatchGAT.LAYER_FUSED = True
        mod.zero_grad(set_to_none=True)
        x1, x2 = x[:, :32].clone().requires_grad_(True), x[:, 32:].clone().requires_grad_(True)
        y2 = mod((x1, x2), None, scenes=sc)
        (y2 * dy).sum().backward()
    finally:
        BatchGAT.LAYER_FUSED = True
        K.set_precision("fp32")
    assert torch.equal(y2, res[0][0]), "two-block output"
    assert torch.equal(torch.cat([x1.grad, x2.grad], 1), res[0][1]), "two-block dx"
    for k, q in mod.named_parameters():
        assert torch.equal(q.grad, res[0][2][k]), "two-block d" + k
    # fp64 reference
    ref = BatchGATEncoder([40, 16, 40], [4, 1], 0.0, 0.2).to(DEV).double()
    ref.load_state_dict({k: v.double() for k, v in mod.state_dict().items()})
    xr = x.double().requires_grad_(True)
    yr = _batch_gat_ref(xr, ref, torch.from_numpy(off))
    (yr * dy.double()).sum().backward()
    refs = [("out", yr.detach()), ("dx", xr.grad)] + [("d" + k, p.grad) for k, p in ref.named_parameters()]
    got = [{"out": yv, "dx": dxv, **{"d" + k: v for k, v in gv.items()}} for yv, dxv, gv in res]
    for name, r in refs:
        scale = float(r.abs().max())
        ef = float((got[0][name].double() - r).abs().max()) / scale
        # the spread of equally valid fp32 evaluations (per-op, exact and
        # perturbed inputs): the bias gradients are near-cancelling sums over
        # the scene rows, so a 1e-7 change of the forward moves them ~1e-4
        ep = max(float((gv[name].double() - r).abs().max()) for gv in got[1:]) / scale
        assert ef <= 2 * ep + 1e-5, "%s: fused err %.3e vs per-op spread %.3e" % (name, ef, ep)
        if prec == "fp32":   # north_star: 1e-3 relative on fp32 (the layer-0 bias gradient sits at ~5e-4)
            assert ef <= 1e-3, "%s: fused err %.3e" % (name, ef)
