"""The pos_grad flag of the pooling ops (K._Pool's four families, K._PoolNorm)
as a path through one shared op: the same launches and parameter gradients as
the plain form, bitwise, plus the gradient of the positions -- what
sgg_pool_dpos / sgg_pool_dpos_drop gives on the saved operands -- and the
parameter gradients written at once inside defer_grad_finish()."""
import numpy as np
import pytest
import torch

from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

DROP = (0.5, 0x5EED5EED1234, 77)
# (family, bottleneck_dim, scene sizes)
CASES = [("resident", 8, (1, 2, 5, 20)), ("wide", 8, (3, 70)), ("coltiled", 24, (1, 2, 5, 20)),
         ("dropout", 24, (1, 2, 5, 20)), ("batch_norm", 8, (2, 5, 20))]


def _run(family, bn, sizes, pos_grad, defer=False):
    """One forward and backward of the case's op on fresh copies of fixed
    inputs -> dict of out, am, dh, dpos, the parameter gradients (read inside
    the defer_grad_finish() scope when defer) and, for the families of _Pool,
    the dpos of the library called directly on the op's saved operands."""
    from sgan import kernels as K
    from sgan.models import PoolHiddenNet
    from sgan.scene import SceneIndex
    N = K.N
    torch.manual_seed(11)
    norm = family == "batch_norm"
    net = PoolHiddenNet(embedding_dim=16, h_dim=32, mlp_dim=64, bottleneck_dim=bn, batch_norm=norm,
                        dropout=DROP[0] if family == "dropout" else 0.0).to(DEV).train()
    B = sum(sizes)
    g = torch.Generator().manual_seed(5)
    h = torch.randn(B, 32, generator=g).to(DEV).requires_grad_(True)
    pos = (4.0 * torch.randn(B, 2, generator=g)).to(DEV).requires_grad_(True)
    w = torch.randn(B, bn, generator=g).to(DEV)
    sc = SceneIndex(np.concatenate([[0], np.cumsum(sizes)]), DEV)
    l1, l2 = K.pool_linears(net)
    emb = net.spatial_embedding
    r = {}
    with (K.defer_grad_finish() if defer else torch.enable_grad()):
        if norm:
            n1, n2 = K.pool_norms(net)
            min_n = K.pool_norm_check(sc, bn, (n1, n2), dropout=net.dropout)
            stats = tuple((float(m.eps), float(m.momentum), m.running_mean, m.running_var, m.num_batches_tracked)
                          for m in (n1, n2))
            out, am = K._PoolNorm.apply(h, pos, l1.weight, emb.weight, emb.bias, l1.bias, n1.weight, n1.bias,
                                        l2.weight, l2.bias, n2.weight, n2.bias, sc, None, stats, min_n, pos_grad)
        else:
            drop = DROP if family == "dropout" else None
            out, am = K._Pool.apply(h, pos, l1.weight, emb.weight, emb.bias, l1.bias, l2.weight, l2.bias, sc, None,
                                    None, None, drop, pos_grad)
            assert out.grad_fn.fam is {"resident": K._POOL_RESIDENT, "wide": K._POOL_WIDE, "coltiled": K._POOL_BN,
                                       "dropout": K._POOL_DROP}[family]
            if pos_grad:
                _h, p_, _W1, _We, _be, A, W2, U, o_, a_ = out.grad_fn.saved_tensors
                direct = torch.empty(B, 2, device=DEV)
                lib = N.load()
                if drop is None:
                    N.check(lib.sgg_pool_dpos(N.ptr(U), N.ptr(p_), N.ptr(A), N.ptr(W2), N.ptr(o_), N.ptr(a_), N.ptr(w),
                                              N.ptr(sc.scene_off), sc.S, B, bn, N.ptr(direct), N.stream_ptr()),
                            "sgg_pool_dpos")
                else:
                    N.check(lib.sgg_pool_dpos_drop(N.ptr(U), N.ptr(p_), N.ptr(A), N.ptr(W2), N.ptr(o_), N.ptr(a_),
                                                   N.ptr(w), N.ptr(sc.scene_off), sc.S, B, bn, N.ptr(direct), drop[0],
                                                   drop[1], drop[2], None, N.stream_ptr()), "sgg_pool_dpos_drop")
                r["direct"] = direct
        (out * w).sum().backward()
        # (inside the scope when defer: before grad_flush)
        r["pending"] = len(K._PENDING)
        r["dw"] = {k: (None if v.grad is None else v.grad.clone()) for k, v in net.named_parameters()}
    torch.cuda.synchronize()
    r.update(out=out.detach(), am=am, dh=h.grad, dpos=pos.grad)
    return r


@pytest.mark.parametrize("family,bn,sizes", CASES, ids=[c[0] for c in CASES])
def test_pos_grad_form_equals_plain_form(family, bn, sizes):
    a = _run(family, bn, sizes, False)
    b = _run(family, bn, sizes, True)
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["am"], b["am"]) and torch.equal(a["dh"], b["dh"])
    assert a["dw"].keys() == b["dw"].keys() and a["dw"]
    for k, v in a["dw"].items():
        assert v is not None and torch.equal(v, b["dw"][k]), k
    assert a["dpos"] is None
    assert b["dpos"] is not None and b["dpos"].shape == (sum(sizes), 2) and bool(torch.isfinite(b["dpos"]).all())
    if family != "batch_norm":
        assert torch.equal(b["dpos"], b["direct"])
        assert bool(b["dpos"].any())


@pytest.mark.parametrize("family,bn,sizes", CASES, ids=[c[0] for c in CASES])
def test_pos_grad_form_writes_parameter_gradients_at_once(family, bn, sizes):
    """Inside defer_grad_finish() the pos_grad form queues nothing: on return
    from backward(), before grad_flush, every parameter's .grad holds what the
    undeferred run gives (the plain form's finish is queued there)."""
    import os
    from sgan import kernels as K
    b = _run(family, bn, sizes, True)
    d = _run(family, bn, sizes, True, defer=True)
    assert d["pending"] == 0 and not K._PENDING
    if os.environ.get("SGG_CHECK_DEFER") != "1":    # (the scope is then a no-op)
        assert _run(family, bn, sizes, False, defer=True)["pending"] == 1
    for k, v in b["dw"].items():
        assert d["dw"][k] is not None and torch.equal(v, d["dw"][k]), k
    assert torch.equal(b["dpos"], d["dpos"]) and torch.equal(b["dh"], d["dh"])
