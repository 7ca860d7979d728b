"""Social pooling with batch norm (sgg_pool_norm_fwd / sgg_pool_norm_bwd /
sgg_pool_norm_running): symbols, argument checks, the workspace bound, the
closed forms the kernels rest on restated in numpy against the oracle (first-
layer statistics against hooked pre-activations, the whole backward against
autograd), the running-statistics recurrence and the eval() fold against
torch, the yardstick's own cases, and the refusals.  Host code only, no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import _pool_norm_ref as R

SYMBOLS = ("sgg_pool_norm_fwd", "sgg_pool_norm_running", "sgg_pool_norm_bwd_rows", "sgg_pool_norm_bwd")
E_ARG = -1
_P = ctypes.c_void_p(64)    # non-NULL, never dereferenced: every check below fails before any launch

FWD_PTRS = ("U", "pos", "A", "gamma1", "beta1", "W2", "b2", "gamma2", "beta2", "off")
FWD_OUTS = ("Un", "An", "mu1", "var1", "mu2", "var2", "out", "am")
BWD_PTRS = ("U", "pos", "A", "gamma1", "W2", "b2", "gamma2", "beta2", "Un", "An", "mu1", "var1", "mu2", "var2", "out",
            "am", "dout", "off")


@pytest.fixture(scope="module")
def lib():
    from sgan import _native
    return _native.load(require_gpu=False)


def _refused(lib, rc, *needles):
    assert rc == E_ARG, rc
    msg = lib.sgg_last_error()
    assert msg, "no message"
    for n in needles:
        assert n in msg, (n, msg)


def _fwd_args(**kw):
    a = dict({k: _P for k in FWD_PTRS + FWD_OUTS}, S=2, B=8, bn=72, min_n=3, max_n=5, eps1=1e-5, eps2=1e-5)
    a.update(kw)
    return [a[k] for k in FWD_PTRS + ("S", "B", "bn", "min_n", "max_n", "eps1", "eps2") + FWD_OUTS] + [None]


def _bwd_args(**kw):
    a = dict({k: _P for k in BWD_PTRS + ("dU", "dpos", "ws")}, S=2, B=8, bn=72, min_n=3, max_n=5, eps1=1e-5, eps2=1e-5,
             wgrad=1, nws=1 << 40)
    a.update(kw)
    return [a[k] for k in BWD_PTRS + ("S", "B", "bn", "min_n", "max_n", "eps1", "eps2", "wgrad", "dU", "dpos", "ws",
                                      "nws")] + [None]


def _run_args(**kw):
    a = dict(mean=_P, var=_P, off=_P, S=2, C=512, momentum=0.1, rm=_P, rv=_P)
    a.update(kw)
    return [a[k] for k in ("mean", "var", "off", "S", "C", "momentum", "rm", "rv")] + [None]


def test_symbols_declared_and_exported(lib):
    import os
    from sgan import _native, kernels as K, scene
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sgg.h")).read()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None
        assert name in _native.SIGNATURES and ("int %s(" % name) in hdr
    assert "long long sgg_pool_norm_bwd_ws_floats(" in hdr and lib.sgg_pool_norm_bwd_ws_floats is not None
    assert "long long sgg_pool_norm_bwd_slab_offset(" in hdr and lib.sgg_pool_norm_bwd_slab_offset is not None
    assert "#define SGG_POOL_NORM_MAX_PEDS %d" % K.POOL_NORM_MAX_PEDS in hdr
    assert scene.SGG_POOL_NORM_MAX_PEDS == K.POOL_NORM_MAX_PEDS


@pytest.mark.parametrize("op", FWD_PTRS + FWD_OUTS)
def test_fwd_null_operand(lib, op):
    _refused(lib, lib.sgg_pool_norm_fwd(*_fwd_args(**{op: None})), b"sgg_pool_norm_fwd", b"null")


@pytest.mark.parametrize("op", BWD_PTRS + ("dU", "ws"))
def test_bwd_null_operand(lib, op):
    _refused(lib, lib.sgg_pool_norm_bwd(*_bwd_args(**{op: None})), b"sgg_pool_norm_bwd", b"null")


@pytest.mark.parametrize("op", ["mean", "var", "off", "rm", "rv"])
def test_running_null_operand(lib, op):
    _refused(lib, lib.sgg_pool_norm_running(*_run_args(**{op: None})), b"sgg_pool_norm_running", b"null")


@pytest.mark.parametrize("bn", [0, 1025])
def test_bad_bn(lib, bn):
    _refused(lib, lib.sgg_pool_norm_fwd(*_fwd_args(bn=bn)), b"sgg_pool_norm_fwd", b"1024")
    _refused(lib, lib.sgg_pool_norm_bwd(*_bwd_args(bn=bn)), b"sgg_pool_norm_bwd", b"1024")
    _refused(lib, lib.sgg_pool_norm_bwd_rows(bn), b"1024")
    assert lib.sgg_pool_norm_bwd_ws_floats(2, 8, bn) == E_ARG


@pytest.mark.parametrize("eps", [0.0, -1e-5, float("nan"), float("inf")])
@pytest.mark.parametrize("which", ["eps1", "eps2"])
def test_bad_eps(lib, which, eps):
    _refused(lib, lib.sgg_pool_norm_fwd(*_fwd_args(**{which: eps})), b"sgg_pool_norm_fwd", b"eps")
    _refused(lib, lib.sgg_pool_norm_bwd(*_bwd_args(**{which: eps})), b"sgg_pool_norm_bwd", b"eps")


@pytest.mark.parametrize("m", [-0.1, 1.5, float("nan")])
def test_bad_momentum(lib, m):
    _refused(lib, lib.sgg_pool_norm_running(*_run_args(momentum=m)), b"sgg_pool_norm_running", b"momentum")


def test_scene_sizes(lib):
    """A scene of one ped is an argument error; so is one above the bound."""
    for fn, args in ((lib.sgg_pool_norm_fwd, _fwd_args), (lib.sgg_pool_norm_bwd, _bwd_args)):
        _refused(lib, fn(*args(min_n=1)), b"1 ped")
        _refused(lib, fn(*args(max_n=257)), b"256")
        _refused(lib, fn(*args(min_n=6, max_n=5)), b"max scene size")
        _refused(lib, fn(*args(S=-1)), b"bad sizes")


def test_workspace_bound_and_short_workspace(lib):
    """The parameter-gradient slabs do not grow with the batch; what does is
    3 B x 512 + 4 S x 512 floats of per-ped sums (two of them doubles)."""
    for bn in (1, 8, 64, 65, 1024):
        rows = lib.sgg_pool_norm_bwd_rows(bn)
        cols = bn * 512 + 2 * bn
        assert 8 <= rows <= 128 and rows * cols <= max(8 * cols, 1 << 24)
        fixed = rows * cols + 32 * 2048
        for S, B in ((1, 2), (64, 1280), (512, 10240)):
            assert lib.sgg_pool_norm_bwd_ws_floats(S, B, bn) == fixed + 3 * B * 512 + 4 * S * 512
            assert lib.sgg_pool_norm_bwd_slab_offset(S, B) == 2 * B * 512 + 4 * S * 512
    need = lib.sgg_pool_norm_bwd_ws_floats(2, 8, 72)
    _refused(lib, lib.sgg_pool_norm_bwd(*_bwd_args(nws=need - 1)), b"sgg_pool_norm_bwd", b"workspace")


# ---- the yardstick's cases ---------------------------------------------------------
@pytest.mark.parametrize("bn,sizes_id", R.CASES + R.MANY_CASES)
def test_every_case_used_is_decided(bn, sizes_id):
    c = R.case(bn, sizes_id)
    assert c["excluded"] == 0, (bn, sizes_id, c["excluded"])
    assert 0 < c["live"] < c["h"].shape[1] * bn and int(c["compare"].sum()) == c["live"]
    g2 = c["state0"]["mlp_pre_pool.4.weight"]
    assert float(g2.min()) < 0 < float(g2.max()) and float(c["state0"]["mlp_pre_pool.4.bias"].abs().min()) > 0
    if (bn, sizes_id) in R.MANY_CASES:    # more scenes than the dense backward has slab rows and the finish has workgroups
        from sgan import _native
        assert len(c["sizes"]) > max(_native.load(require_gpu=False).sgg_pool_norm_bwd_rows(bn), 32)
    for k in R.ZERO_BIASES:      # the reference's own gradient there is rounding noise
        assert float(c["r64"]["dw." + k].abs().max()) < 1e-9 * float(c["r64"]["dw.mlp_pre_pool.0.weight"].abs().max())
    assert all(v >= R.FLOOR for v in c["tol"].values())


# ---- the closed forms, in numpy, against the oracle -----------------------------------
def _numpy_algorithm(c):
    """What the kernels compute, in float64 numpy: the fold U / A, the first
    layer's statistics in closed form, the dense backward's sums R, C, G and
    the finish."""
    sd = {k: v.numpy() for k, v in c["state0"].items()}
    E, eps = R.E_DIM, 1e-5
    We, be = sd["spatial_embedding.weight"], sd["spatial_embedding.bias"]
    W1, b1 = sd["mlp_pre_pool.0.weight"], sd["mlp_pre_pool.0.bias"]
    g1, t1 = sd["mlp_pre_pool.1.weight"], sd["mlp_pre_pool.1.bias"]
    W2, b2 = sd["mlp_pre_pool.3.weight"], sd["mlp_pre_pool.3.bias"]
    g2, t2 = sd["mlp_pre_pool.4.weight"], sd["mlp_pre_pool.4.bias"]
    h, pos, dout = c["h"][0].numpy(), c["pos"].numpy(), c["dout"].numpy()
    A = W1[:, :E] @ We
    U = h @ W1[:, E:].T + (W1[:, :E] @ be + b1)
    off = np.concatenate([[0], np.cumsum(c["sizes"])])
    r = dict(out=np.zeros_like(dout), dU=np.zeros_like(U), dpos=np.zeros_like(pos), dA=np.zeros_like(A),
             dg1=np.zeros(512), dt1=np.zeros(512), dW2=np.zeros_like(W2), dg2=np.zeros_like(g2), dt2=np.zeros_like(t2),
             mu1=[], var1=[])
    for s, n in enumerate(c["sizes"]):
        o, M = off[s], n * n
        p, u = pos[o:o + n], U[o:o + n]
        a, q = u + p @ A.T, p @ A.T
        mu1, var1 = u.mean(0), a.var(0) + q.var(0)        # no pass over pairs
        r["mu1"].append(mu1), r["var1"].append(var1)
        rs = 1 / np.sqrt(var1 + eps)
        g = g1 * rs
        rel = p[None, :, :] - p[:, None, :]                 # [i, j] = p_j - p_i
        a1 = np.maximum((g * (u - mu1) + t1)[None] + rel @ (g[:, None] * A).T, 0)
        y2 = a1 @ W2.T + b2
        mu2, var2 = y2.reshape(M, -1).mean(0), y2.reshape(M, -1).var(0)
        rs2 = 1 / np.sqrt(var2 + eps)
        v = np.maximum(g2 * rs2 * (y2 - mu2) + t2, 0)       # the affine map before the max
        am, ov = v.argmax(1), v.max(1)
        r["out"][o:o + n] = ov
        dzr = np.where(ov > 0, dout[o:o + n], 0)
        db, dg = dzr.sum(0), (dzr * (ov - t2) / g2).sum(0)
        r["dg2"] += dg
        r["dt2"] += db
        dz = np.zeros_like(y2)
        ii, cc = np.meshgrid(np.arange(n), np.arange(y2.shape[2]), indexing="ij")
        dz[ii, am, cc] = dzr
        dy2 = g2 * rs2 * (dz - db / M - (y2 - mu2) * rs2 * dg / M)
        r["dW2"] += np.einsum("ijc,ijk->ck", dy2, a1)
        dz1 = (dy2 @ W2) * (a1 > 0)
        Rj, Ci, G = dz1.sum(0), dz1.sum(1), np.einsum("ijk,ijd->kd", dz1, rel)
        uh, ah = (u - mu1) * rs, A * rs[:, None]
        d = p - p.mean(0)
        dbet, dgam = Rj.sum(0), (uh * Rj).sum(0) + (ah * G).sum(1)
        dd = d @ ah.T
        du = g * (Rj - dbet / n - (uh + dd) * dgam / n)
        di = g * (Ci - dbet / n + dd * dgam / n)
        r["dU"][o:o + n] = du
        r["dpos"][o:o + n] = (du - di) @ A
        r["dA"] += g[:, None] * (G - (dgam / n)[:, None] * (uh.T @ d + 2 * ah @ (d.T @ d)))
        r["dg1"] += dgam
        r["dt1"] += dbet
    r["dh"] = r["dU"] @ W1[:, E:]
    r["dW1"] = np.concatenate([r["dA"] @ We.T, r["dU"].T @ h], 1)
    r["dWe"] = W1[:, :E].T @ r["dA"]
    return r


def test_closed_forms_against_the_oracle():
    c = R.case(24, 0)
    r = _numpy_algorithm(c)
    # first-layer statistics against the oracle's hooked pre-activations
    net = R.build_net(24, c["seed"])
    net.load_state_dict(c["state0"])
    net.train()
    pre = []
    hook = net.mlp_pre_pool[0].register_forward_hook(lambda m, i, o: pre.append(o.detach().numpy()))
    net(c["h"], R.sse_of(c["sizes"]), c["pos"])
    hook.remove()
    assert len(pre) == len(c["sizes"])
    for y1, mu1, var1 in zip(pre, r["mu1"], r["var1"]):
        np.testing.assert_allclose(mu1, y1.mean(0), rtol=0, atol=1e-12 * np.abs(y1).max())
        np.testing.assert_allclose(var1, y1.var(0), rtol=1e-11)
    ref = c["r64"]
    for mine, theirs in (("out", "out"), ("dh", "dh"), ("dpos", "dpos"), ("dW1", "dw.mlp_pre_pool.0.weight"),
                         ("dWe", "dw.spatial_embedding.weight"), ("dg1", "dw.mlp_pre_pool.1.weight"),
                         ("dt1", "dw.mlp_pre_pool.1.bias"), ("dW2", "dw.mlp_pre_pool.3.weight"),
                         ("dg2", "dw.mlp_pre_pool.4.weight"), ("dt2", "dw.mlp_pre_pool.4.bias")):
        assert R.rel_err(torch.from_numpy(r[mine]), ref[theirs]) < 1e-12, mine
    assert np.abs(r["dU"].sum(0)).max() < 1e-12 * np.abs(r["dU"]).max()      # the bias in front of BatchNorm 1


def test_running_statistics_recurrence_against_torch():
    """r <- (1 - m) r + m stat_s in scene order, the variance unbiased: what
    sgg_pool_norm_running does per column, against nn.BatchNorm1d called once
    per scene; and the closed form after S scenes."""
    torch.manual_seed(2)
    sizes, C, m = [2, 5, 3], 7, 0.1
    norm = torch.nn.BatchNorm1d(C, momentum=m).double().train()
    with torch.no_grad():
        norm.running_mean.copy_(torch.randn(C).double())
        norm.running_var.copy_(torch.rand(C).double() + 0.5)
    rm, rv = norm.running_mean.numpy().copy(), norm.running_var.numpy().copy()
    rm0, rv0 = rm.copy(), rv.copy()
    means, uvars = [], []
    for n in sizes:
        x = torch.randn(n * n, C).double()
        norm(x)
        M = float(n * n)
        means.append(x.mean(0).numpy()), uvars.append(x.var(0, unbiased=False).numpy() * (M / (M - 1)))
        rm, rv = (1 - m) * rm + m * means[-1], (1 - m) * rv + m * uvars[-1]
    np.testing.assert_allclose(rm, norm.running_mean.numpy(), rtol=1e-13)
    np.testing.assert_allclose(rv, norm.running_var.numpy(), rtol=1e-13)
    S = len(sizes)
    w = [m * (1 - m) ** (S - 1 - s) for s in range(S)]
    np.testing.assert_allclose((1 - m) ** S * rm0 + sum(a * b for a, b in zip(w, means)), rm, rtol=1e-13)
    np.testing.assert_allclose((1 - m) ** S * rv0 + sum(a * b for a, b in zip(w, uvars)), rv, rtol=1e-13)
    assert int(norm.num_batches_tracked) == S


def test_eval_fold_against_batchnorm_eval():
    from sgan import kernels as K
    torch.manual_seed(4)
    lin, norm = torch.nn.Linear(9, 13).double(), torch.nn.BatchNorm1d(13, eps=1e-3).double()
    with torch.no_grad():
        norm.weight.copy_(torch.randn(13).double())
        norm.bias.copy_(torch.randn(13).double())
        norm.running_mean.copy_(torch.randn(13).double())
        norm.running_var.copy_(torch.rand(13).double() + 0.1)
    norm.eval()
    x = torch.randn(31, 9).double()
    W, b = K.pool_norm_fold(lin, norm)
    np.testing.assert_allclose((x @ W.T + b).detach().numpy(), norm(lin(x)).detach().numpy(), rtol=1e-12, atol=1e-13)
    assert W.requires_grad and b.requires_grad        # autograd reaches the raw parameters
    (x @ W.T + b).sum().backward()
    assert all(p.grad is not None for p in (lin.weight, lin.bias, norm.weight, norm.bias))


# ---- the module and the refusals (nothing is launched: there is no GPU here) -----------
def test_module_layers_found_by_type_and_state_dict_keys():
    from sgan import kernels as K
    from sgan.models import PoolHiddenNet
    net = PoolHiddenNet(16, 32, 64, 24)          # batch_norm=True is the constructor default
    assert net.batch_norm and not net.fused_ok()
    keys = set(net.state_dict())
    assert {"mlp_pre_pool.0.weight", "mlp_pre_pool.1.running_var", "mlp_pre_pool.3.weight", "mlp_pre_pool.4.bias",
            "mlp_pre_pool.4.num_batches_tracked"} <= keys
    l1, l2 = K.pool_linears(net)
    n1, n2 = K.pool_norms(net)
    assert l1 is net.mlp_pre_pool[0] and n1 is net.mlp_pre_pool[1] and l2 is net.mlp_pre_pool[3]
    assert n2 is net.mlp_pre_pool[4] and n2.num_features == 24


def _cpu_scenes(sizes):
    from sgan.scene import SceneIndex
    return SceneIndex(np.concatenate([[0], np.cumsum(sizes)]), "cpu")


@pytest.fixture
def no_launch(monkeypatch):
    from sgan import _native as N
    calls = []
    real = N.check
    monkeypatch.setattr(N, "check", lambda rc, name: (calls.append(name), real(rc, name))[1])
    yield calls
    assert calls == [], calls


def _call(net, sc):
    return net(torch.zeros(1, sc.B, 32), None, torch.zeros(sc.B, 2), scenes=sc)


def test_one_ped_scene_in_train_is_torchs_value_error(no_launch):
    from sgan.models import PoolHiddenNet
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        _call(PoolHiddenNet(16, 32, 64, 24).train(), _cpu_scenes([3, 1, 5]))


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("how", ["momentum", "track_running_stats"])
def test_cumulative_or_untracked_statistics_refused(how, training, no_launch):
    from sgan.models import PoolHiddenNet
    net = PoolHiddenNet(16, 32, 64, 24).train(training)
    if how == "momentum":
        net.mlp_pre_pool[4].momentum = None
    else:
        net.mlp_pre_pool[1] = torch.nn.BatchNorm1d(512, track_running_stats=False)
    with pytest.raises(NotImplementedError, match="momentum=None|track_running_stats=False"):
        _call(net, _cpu_scenes([3, 5]))


def test_batch_norm_with_dropout_in_train_refused(no_launch):
    from sgan.models import PoolHiddenNet
    with pytest.raises(NotImplementedError, match="batch_norm.*dropout"):
        _call(PoolHiddenNet(16, 32, 64, 24, "relu", True, dropout=0.25).train(), _cpu_scenes([3, 5]))


def test_scene_above_the_bound_refused(no_launch):
    from sgan.models import PoolHiddenNet
    with pytest.raises(NotImplementedError, match="batch_norm.*256"):
        _call(PoolHiddenNet(16, 32, 64, 24).train(), _cpu_scenes([3, 257]))


@pytest.mark.parametrize("training", [True, False])
def test_padded_plans_refuse_batch_norm_by_name(training, no_launch):
    from sgan.models import PoolHiddenNet
    from sgan.scene import PaddedScenes
    ps = PaddedScenes(4, 32, "cpu", 20, reps=(2,))
    ps.load(np.array([0, 5, 12], np.int32), np.arange(12, dtype=np.int32))
    net = PoolHiddenNet(16, 32, 64, 8).train(training)
    for sc in (ps, ps.repeat(2)):
        with pytest.raises(NotImplementedError, match="batch_norm"):
            sc.pool_plan(8, batch_norm=True)
        with pytest.raises(NotImplementedError, match="batch_norm"):
            _call(net, sc)
    assert ps.pool_plan(8)[3] >= 1    # a batch_norm=0 net of a built width still plans


def test_non_relu_activation_still_refused(no_launch):
    from sgan.models import PoolHiddenNet
    with pytest.raises(NotImplementedError, match="relu"):
        _call(PoolHiddenNet(16, 32, 64, 24, "leakyrelu", True).train(), _cpu_scenes([3, 5]))
