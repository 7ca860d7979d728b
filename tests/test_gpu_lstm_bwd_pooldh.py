"""The pooling backward's dh = dU W1h (+ base) formed in the prologue of the
encoder-LSTM backward that consumes it, the h^T dU partials riding in the
same launch (sgg_lstm_bwd_pooldh, lstm_mw.hip mw_bwd_body PDH): bitwise the
composition of sgg_pool_dh_dw / sgg_xw and the plain backward, kernel by
kernel and through autograd (kernels.PoolDhSlot, SGG_POOL_DH_IN_LSTM)."""
import random

import pytest
import torch

from test_gpu_parity import DEV, build_models

pytestmark = pytest.mark.gpu

NU, E = 512, 16
E_ARG = -1   # SGG_E_ARG (include/sgg.h)


def _f(*s, sc=0.3):
    return (torch.randn(*s, device=DEV) * sc).contiguous()


def _nan(*s):
    return torch.full(s, float("nan"), device=DEV)


def _forward(lib, N, H, T, B, rel, A, Whh, bias, h0, c0, t_sh, Bsrc):
    sf = lambda w: torch.empty(int(lib.sgg_lstm_state_floats(T, B, H, w)), device=DEV)
    h_all, c_all, act = torch.empty(T + 1, B, H, device=DEV), sf(1), sf(0)
    if t_sh:   # the first t_sh steps run once for Bsrc peds (the rest of the batch repeats them)
        pre = N.LstmSeg(N.ptr(rel), N.ptr(A), N.ptr(Whh), N.ptr(bias), None, None, t_sh, Bsrc, B, 0, T, Bsrc,
                        N.ptr(h_all), N.ptr(c_all), N.ptr(act), None, 0, None, 0, None)
        N.check(lib.sgg_lstm_fwd_seg(N.ctypes.byref(pre), H, N.stream_ptr()), "prefix")
        suf = N.LstmSeg(N.ptr(rel), N.ptr(A), N.ptr(Whh), N.ptr(bias), None, None, T - t_sh, B, B, t_sh, T, Bsrc,
                        N.ptr(h_all), N.ptr(c_all), N.ptr(act), None, 0, None, 0, None)
        N.check(lib.sgg_lstm_fwd_seg(N.ctypes.byref(suf), H, N.stream_ptr()), "suffix")
    else:
        N.check(lib.sgg_lstm_fwd(N.ptr(rel), N.ptr(A), N.ptr(Whh), N.ptr(bias), N.ptr(h0), N.ptr(c0), None, None, T, B,
                                 H, 0, N.ptr(h_all), N.ptr(c_all), N.ptr(act), None, N.stream_ptr()), "fwd")
    return h_all, c_all, act


def _both_paths(form, H, B, with_base, T=4):
    """-> (the stand-alone launches, the new entry point): dicts of the outputs."""
    from sgan import _native as N
    lib = N.load()
    torch.manual_seed(100 * H + B + 7 * with_base + len(form))
    t_sh, Bsrc = (2, 32) if form == "shared" else (0, 0)
    t_stop = 2 if form == "tail" else 0
    wgrad = form != "tail"
    state = form in ("dx", "nodx")      # these also return dh0
    A, Whh, bias = _f(4 * H, 2), _f(4 * H, H, sc=0.2), _f(4 * H)
    if t_sh:
        rel = torch.cat([_f(t_sh, Bsrc, 2).repeat(1, B // Bsrc, 1), _f(T - t_sh, B, 2)], 0).contiguous()
    else:
        rel = _f(T, B, 2)
    h0, c0 = (_f(B, H), _f(B, H)) if state else (None, None)
    h_all, c_all, act = _forward(lib, N, H, T, B, rel, A, Whh, bias, h0, c0, t_sh, Bsrc)
    h = h_all[T]
    dU = _f(B, NU)
    W1 = _f(NU, E + H, sc=0.1)
    W1h = W1[:, E:]                      # a strided view: row stride E + H
    assert W1h.stride(0) == E + H
    base = _f(B, H) if with_base else None
    P = 4 * H * H + 4 * H + 8 * H
    rows = int(lib.sgg_lstm_wpart_rows(H, B))
    splits = int(lib.sgg_xtw_splits(B, H, NU))
    nws = splits * (H * NU + NU)

    def outputs():
        return dict(wpart=_nan(rows, P) if wgrad else None, dh0=_nan(B, H) if state else None,
                    drel=None if form == "nodx" else _nan(T, B, 2), ws=_nan(nws) if wgrad else None)

    # the parent's path: the stand-alone product(s), then the plain backward on the finished dh_last
    old = outputs()
    dh = base.clone() if with_base else _nan(B, H)
    if wgrad:
        N.check(lib.sgg_pool_dh_dw(N.ptr(dU), NU, N.ptr(W1h), W1h.stride(0), N.ptr(dh), H, int(with_base), N.ptr(h), H,
                                   B, H, N.ptr(old["ws"]), nws * 4, N.stream_ptr()), "sgg_pool_dh_dw")
    else:
        N.check(lib.sgg_xw(N.ptr(dU), NU, None, 0, N.ptr(W1h), W1h.stride(0), 0, None, N.ptr(dh), H, B, NU, H,
                           2 if with_base else 0, N.stream_ptr()), "sgg_xw")
    if form == "shared":
        N.check(lib.sgg_lstm_bwd_shared(N.ptr(A), N.ptr(Whh), N.ptr(h_all), N.ptr(c_all), N.ptr(act), N.ptr(rel),
                                        N.ptr(dh), T, B, H, t_sh, Bsrc, N.ptr(old["drel"]), N.ptr(old["wpart"]),
                                        N.stream_ptr()), "sgg_lstm_bwd_shared")
    elif form == "tail":
        N.check(lib.sgg_lstm_bwd_tail(N.ptr(A), N.ptr(Whh), N.ptr(h_all), N.ptr(c_all), N.ptr(act), N.ptr(rel),
                                      N.ptr(dh), T, B, H, t_stop, N.ptr(old["drel"]), N.stream_ptr()),
                "sgg_lstm_bwd_tail")
    else:
        N.check(lib.sgg_lstm_bwd(N.ptr(A), N.ptr(Whh), None, N.ptr(h_all), N.ptr(c_all), N.ptr(act), N.ptr(rel), None,
                                 N.ptr(dh), None, T, B, H, 0, None, N.ptr(old["dh0"]), N.ptr(old["drel"]), None,
                                 N.ptr(old["wpart"]), N.stream_ptr()), "sgg_lstm_bwd")
    # the change: one entry point, dU in place of dh_last
    new = outputs()
    pd = N.PoolDh(N.ptr(dU), NU, N.ptr(W1h), W1h.stride(0), N.ptr(base), NU, N.ptr(h), H, N.ptr(new["ws"]),
                  nws * 4 if wgrad else 0, splits)
    N.check(lib.sgg_lstm_bwd_pooldh(N.ptr(A), N.ptr(Whh), N.ptr(h_all), N.ptr(c_all), N.ptr(act), N.ptr(rel),
                                    N.ctypes.byref(pd), T, B, H, t_stop, t_sh, Bsrc, N.ptr(new["dh0"]),
                                    N.ptr(new["drel"]), N.ptr(new["wpart"]), N.stream_ptr()), "sgg_lstm_bwd_pooldh")
    torch.cuda.synchronize()
    if with_base:
        assert not torch.isnan(base).any()
    return old, new


def _same(old, new, what):
    for k in old:
        if old[k] is None:
            assert new[k] is None
            continue
        assert not torch.isnan(old[k]).any(), (what, k, "the stand-alone path left it unwritten")
        assert torch.equal(old[k], new[k]), (what, k)   # (slab rows, the xtw slab and its column slab: every element)


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("B", [40, 64])
@pytest.mark.parametrize("H", [32, 48])
@pytest.mark.parametrize("form", ["dx", "nodx", "tail"])
def test_prologue_product_is_bitwise_the_standalone_launches(form, H, B, with_base):
    """Full form with drel_in, without it (nodx), and the input-gradient tail
    form (t_stop = 2): drel_in, dh0, every slab row of wpart, the xtw slab
    and the column slab equal those of sgg_pool_dh_dw / sgg_xw + the plain
    backward.  B = 40: the last 16-ped tile is ragged; W1h a strided view."""
    _same(*_both_paths(form, H, B, with_base), what=(form, H, B, with_base))


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("H", [32, 48])
def test_shared_prefix_form(H, with_base):
    """sgg_lstm_bwd_shared's form (B = 64, Bsrc = 32, t_sh = 2)."""
    _same(*_both_paths("shared", H, 64, with_base), what=("shared", H, with_base))


@pytest.mark.parametrize("H", [32, 48])
def test_single_workgroup_and_its_riders(H):
    """B = 16: one recurrence workgroup, the riders behind it."""
    from sgan import _native as N
    assert N.load().sgg_lstm_bwd_pooldh_rides(16, H, NU) == 1
    _same(*_both_paths("nodx", H, 16, True), what=("one workgroup", H))


def test_partials_keep_their_launch_behind_a_full_device():
    """More recurrence workgroups than CUs (B = 16 x 257 on 256 CUs): the
    riding rule says no, the entry point issues sgg_xtw_partial itself, and
    the results are the same."""
    from sgan import _native as N
    lib = N.load()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 16 * (cus + 1)
    assert lib.sgg_lstm_bwd_pooldh_rides(B, 48, NU) == 0 and lib.sgg_lstm_bwd_pooldh_rides(2560, 48, NU) == 1
    # (the host hands over only a single round of workgroups; the entry point itself takes any B)
    assert lib.sgg_lstm_bwd_pooldh_pays(16 * cus, 48) == 1 and lib.sgg_lstm_bwd_pooldh_pays(B, 48) == 0
    assert lib.sgg_lstm_bwd_pooldh_pays(64, 64) == 0
    _same(*_both_paths("nodx", 48, B, False, T=2), what="stand-alone partials")


def test_source_refused_where_not_built():
    """H = 16 / 64 have no prologue: SGG_E_ARG, nothing launched."""
    from sgan import _native as N
    lib = N.load()
    assert lib.sgg_lstm_bwd_pooldh_ok(32) == 1 and lib.sgg_lstm_bwd_pooldh_ok(48) == 1
    T, B = 3, 16
    for H in (16, 64):
        assert lib.sgg_lstm_bwd_pooldh_ok(H) == 0
        z = lambda *s: torch.zeros(*s, device=DEV)
        A, Whh, h_all, rel = z(4 * H, 2), z(4 * H, H), z(T + 1, B, H), z(T, B, 2)
        c_all = z(int(lib.sgg_lstm_state_floats(T, B, H, 1)))
        act = z(int(lib.sgg_lstm_state_floats(T, B, H, 0)))
        dU, W1h = z(B, NU), z(NU, H)
        drel = torch.full((T, B, 2), 7.0, device=DEV)
        pd = N.PoolDh(N.ptr(dU), NU, N.ptr(W1h), H, None, NU, None, 0, None, 0, 0)
        rc = lib.sgg_lstm_bwd_pooldh(N.ptr(A), N.ptr(Whh), N.ptr(h_all), N.ptr(c_all), N.ptr(act), N.ptr(rel),
                                     N.ctypes.byref(pd), T, B, H, 0, 0, 0, None, N.ptr(drel), None, N.stream_ptr())
        torch.cuda.synchronize()
        assert rc == E_ARG and bool((drel == 7.0).all())


# ---------------------------------------------------------------------------
# autograd level
# ---------------------------------------------------------------------------
def _steps(monkeypatch, armed, graph="gat"):
    """One discriminator and one generator step on 3 scenes of (2, 5, 20)
    peds -> every parameter gradient after its step, the hidden sizes of the
    slots that were filled, and the backward kernels' names."""
    from sgan import kernels as K
    from sgan import train_step as TS
    from sgan.data.synthetic import synthetic_batch
    from sgan.scene import SceneIndex
    monkeypatch.setattr(K, "POOL_DH_IN_LSTM", armed)
    puts = []
    put = K.PoolDhSlot.put

    def counting_put(self, *a):
        puts.append(int(a[3].shape[1]))
        return put(self, *a)
    monkeypatch.setattr(K.PoolDhSlot, "put", counting_put)
    batch = synthetic_batch([2, 5, 20], seed=3, device=DEV)
    torch.manual_seed(0)
    g, d = build_models(graph)
    tr = TS.GanTrainer(g, d, capturable=True)
    sc = SceneIndex.from_seq_start_end(batch[-1], DEV)
    torch.manual_seed(5)
    random.seed(5)
    grads = {}
    tr.d_step(batch, sc)
    torch.cuda.synchronize()
    grads.update({"d." + n: p.grad.detach().clone() for n, p in d.named_parameters() if p.grad is not None})
    tr.g_step(batch, sc)
    torch.cuda.synchronize()
    grads.update({"g." + n: p.grad.detach().clone() for n, p in g.named_parameters() if p.grad is not None})
    assert not K._PDH_OPEN
    return grads, puts


def _same_grads(a, b):
    assert sorted(a) == sorted(b) and len(a) > 20
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_steps_armed_equal_switch_off(monkeypatch):
    """A D-step-shaped and a G-step-shaped backward, armed versus
    SGG_POOL_DH_IN_LSTM=0: every parameter gradient bitwise equal.  Armed, the
    discriminator's pooling (H = 48) hands over in both steps and the
    generator's (H = 32) in the generator step; switched off, nothing does."""
    on, puts_on = _steps(monkeypatch, True)
    off, puts_off = _steps(monkeypatch, False)
    assert puts_on == [48, 48, 32] and puts_off == [], (puts_on, puts_off)
    _same_grads(on, off)


def test_sgangat_context_does_not_arm(monkeypatch):
    """The batched GAT of sgangat reads the encoder state a second time
    through autograd: the generator's pooling must not hand over (only the
    discriminator's slots fill), and the gradients equal the switch-off run."""
    on, puts_on = _steps(monkeypatch, True, graph="sgangat")
    off, puts_off = _steps(monkeypatch, False, graph="sgangat")
    assert 32 not in puts_on and puts_on == [48, 48] and puts_off == [], (puts_on, puts_off)
    _same_grads(on, off)


def test_unpaired_use_raises():
    """Arming where the encoder state has a second autograd consumer: the
    encoder's backward receives autograd's sum, not the pooling's buffer, and
    raises instead of using it."""
    from sgan import kernels as K
    from sgan.models import Encoder, PoolHiddenNet
    from sgan.scene import SceneIndex
    torch.manual_seed(1)
    enc = Encoder(embedding_dim=16, h_dim=32, mlp_dim=64, num_layers=1, dropout=0.0).to(DEV)
    pool = PoolHiddenNet(embedding_dim=16, h_dim=32, mlp_dim=64, bottleneck_dim=8, activation="relu",
                         batch_norm=False).to(DEV)
    sse = torch.tensor([[0, 2], [2, 7], [7, 27]], device=DEV)
    sc = SceneIndex.from_seq_start_end(sse, DEV)
    rel, pos = _f(8, 27, 2), _f(27, 2, sc=3.0)

    def run(second_consumer):
        h, U = enc(rel, proj_u=K.pool_u_spec(pool))
        assert U is not None
        out = pool(h, sse, pos, scenes=sc, U=U, dh_in_lstm=True)
        loss = out.sum() + (h.sum() if second_consumer else 0.0)
        loss.backward()
        torch.cuda.synchronize()

    run(False)   # paired: fine
    assert not K._PDH_OPEN
    with pytest.raises(RuntimeError, match="second autograd consumer"):
        run(True)
    assert not K._PDH_OPEN
