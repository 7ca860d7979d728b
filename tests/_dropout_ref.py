"""fp64 torch restatements of the graph-attention modules with the dropout
masks of the kernels' contract applied explicitly (sgan.kernels
.dropout_keep_host), shared by test_dropout_rng.py (CPU) and
test_gpu_gat_dropout.py.  Not a test module.

drop arguments here are (p, seed, offset, site, head0) as the kernels take
them, or (p, seed, offset) for a whole module (the sites are the module's).
Everything runs on the CPU in float64 and is differentiable by autograd (the
masks are constants)."""
import numpy as np
import torch


def close(a, b, rtol=1e-4, floor=1e-6, what=""):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, np.float64)
    scale = max(np.abs(b).max(), floor)
    err = np.abs(a - b).max() / scale
    assert err <= rtol, "%s max rel err %.3e (scale %.3e)" % (what, err, scale)


def scaled_mask(p, seed, offset, site, head, rows, cols):
    """The scaled mask m (scale where kept, 0 where dropped) as a float64 tensor."""
    from sgan import kernels as K
    keep = K.dropout_keep_host(p, seed, offset, site, head, rows, cols)
    _, scale = K.dropout_thr_scale_host(p)
    return torch.from_numpy(np.where(keep, np.float64(scale), 0.0))


def feature_dropout_ref(x, drop):
    if drop is None:
        return x
    p, seed, offset, site = drop[:4]
    return x * scaled_mask(p, seed, offset, site, 0, np.arange(x.shape[0]), np.arange(x.shape[1]))


def gat_attention_ref(wh, a, bias, labels, seg_off, mode, epi, heads, alpha=0.2, drop=None):
    """The attention layer (models.py:184-220, the multi-head GAT.py:6-55
    text): per segment and head, masked softmax of LeakyReLU(s_i + t_j), the
    dropout mask on the softmax (row = the node's row in the whole array,
    column = the in-segment j, head = head0 + h), att @ Wh + bias, then the
    epilogue.  a: heads x 2F."""
    n, HF = wh.shape
    F = HF // heads
    so = [int(v) for v in seg_off]
    blocks, at = [], 0
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
                lab = labels[o:e].reshape(-1)
                m = (lab[:, None] == lab[None, :]) & (lab[:, None] != 0)
                m = m | torch.eye(e - o, dtype=torch.bool)
                z = z.masked_fill(~m, float("-inf"))
            att = torch.softmax(z, 1)
            if drop is not None:
                p, seed, offset, site, head0 = drop
                att = att * scaled_mask(p, seed, offset, site, head0 + h, np.arange(o, e), np.arange(e - o))
            out = att @ W
            if bias is not None:
                out = out + bias
            if epi:
                out = torch.nn.functional.elu(out)
            if epi == 2:
                out = torch.log_softmax(out, 1)
            cols.append(out)
        if o > at:
            blocks.append(torch.zeros(o - at, HF, dtype=torch.float64))
        blocks.append(torch.cat(cols, 1))
        at = e
    if n > at:
        blocks.append(torch.zeros(n - at, HF, dtype=torch.float64))
    return torch.cat(blocks, 0)


def groups_by_first_member(labels, scene_off):
    """This project's group order: scene by scene, groups numbered
    by their first member; a label-0 ped is a group of its own.  -> (R: the
    row-normalised total-groups x B membership matrix, float64; group_off:
    the scenes' CSR over the group rows)."""
    lab = [float(v) for v in np.asarray(labels).reshape(-1)]
    so = [int(v) for v in scene_off]
    rows, goff = [], [0]
    for s in range(len(so) - 1):
        first = {}
        members = []
        for i in range(so[s], so[s + 1]):
            if lab[i] != 0.0 and lab[i] in first:
                members[first[lab[i]]].append(i)
            else:
                if lab[i] != 0.0:
                    first[lab[i]] = len(members)
                members.append([i])
        rows += members
        goff.append(len(rows))
    R = torch.zeros(len(rows), so[-1], dtype=torch.float64)
    for g, mem in enumerate(rows):
        R[g, mem] = 1.0 / len(mem)
    return R, goff


def _gat_ref(gat, x, labels, seg_off, mode, rng, site0):
    """GAT.forward (models.py:231-237) with its four dropout sites."""
    d = (lambda site, head=0: None) if rng is None else (lambda site, head=0: rng + (site0 + site, head))
    alpha = gat.out_att.alpha
    x = feature_dropout_ref(x, d(0))
    heads = []
    for i, att in enumerate(gat.attentions):
        heads.append(gat_attention_ref(x @ att.W.double(), att.a.double().reshape(1, -1), None, labels, seg_off, mode,
                                       1, 1, alpha, drop=d(1, i)))
    x = feature_dropout_ref(torch.cat(heads, 1), d(2))
    o = gat.out_att
    return gat_attention_ref(x @ o.W.double(), o.a.double().reshape(1, -1), None, labels, seg_off, mode, 2, 1, alpha,
                             drop=d(3))


def gat_encoder_ref(mod, x, labels, scene_off, rng=None):
    """GATEncoder.forward (models.py:239-294) on the whole batch: the
    intra-group GAT over each scene (sites 0..3), the groups' means, the
    inter-group GAT over each scene's groups (complete graph, sites 4..7; its
    node array is the group rows in this project's order), un-pooling, the
    output Linear.  mod: the module of sgan.models or of the oracle (same
    parameter names).  rng = (p, seed, offset), or None for no dropout."""
    R, goff = groups_by_first_member(labels, scene_off)
    lab = torch.as_tensor(np.asarray(labels, np.float64)).reshape(-1)
    intra = _gat_ref(mod.gat_intra, x, lab, scene_off, 0, rng, 0)
    gout = _gat_ref(mod.gat_inter, R @ intra, None, goff, 1, rng, 4)
    cat = torch.cat([intra, R.t() @ gout], 1)
    return cat @ mod.out_embedding.weight.double().t() + mod.out_embedding.bias.double()


def batch_gat_ref(mod, x, seg_off, rng=None):
    """The sgangat batched GAT (GAT.py:58-89 text): per layer l InstanceNorm1d
    over each segment's rows (biased variance, eps 1e-5), per head softmax(
    LeakyReLU(s_i + t_j)) with the attention dropout of site 2l, @ Wh + bias,
    heads concatenated; ELU then the dropout of site 2l + 1 on all but the
    last layer.  mod: a BatchGATEncoder; rng = (p, seed, offset) or None."""
    layers = mod.gat_net.layer_stack
    so = [int(v) for v in seg_off]
    for i, l in enumerate(layers):
        last = i + 1 == len(layers)
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
        bias = l.bias.double() if l.bias is not None else None
        x = gat_attention_ref(wh, a, bias, None, so, 1, 0 if last else 1, H,
                              drop=None if rng is None else rng + (2 * i, 0))
        if not last and rng is not None:
            x = feature_dropout_ref(x, rng + (2 * i + 1,))
    return x
