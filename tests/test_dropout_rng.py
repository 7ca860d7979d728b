"""The dropout-mask contract on the host (include/sgg.h "Dropout masks"):
sgan.kernels.dropout_keep_host, the numpy restatement of csrc/dropout_common.h,
and the fp64 module restatements the GPU dropout tests compare against
(tests/_dropout_ref.py), tied to the reference-derived oracle at dropout 0."""
import numpy as np
import pytest
import torch

from _dropout_ref import batch_gat_ref, close, gat_encoder_ref

SEED = 0x1234ABCD5678EF01


def _K():
    from sgan import kernels as K
    return K


@pytest.mark.parametrize("counter,key,words", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, words):
    """Philox4x32-10 known answers, through the generator and through
    dropout_keep_host: with the counter laid out as the contract says --
    (row >> 2, col, (site << 8) | head, offset), key (seed lo, seed hi) -- the
    keep decisions of rows 4 c0 .. 4 c0 + 3 at column c1 are `word >= thr`."""
    K = _K()
    want = [int(w, 16) for w in words.split()]
    got = [int(v) for v in K.philox4x32_10_host(counter, key)]
    assert got == want
    c0, c1, c2, c3 = counter
    if c0 >= 1 << 30:       # 4 c0 is no 32-bit row: the generator check above covers this vector
        return
    seed = key[0] | (key[1] << 32)
    for p in (0.1, 0.5, 0.9):
        thr, _ = K.dropout_thr_scale_host(p)
        keep = K.dropout_keep_host(p, seed, c3, c2 >> 8, c2 & 255, np.arange(4 * c0, 4 * c0 + 4), [c1])
        assert keep.shape == (4, 1)
        assert [bool(k) for k in keep[:, 0]] == [w >= int(thr) for w in want]


def test_threshold_and_scale():
    K = _K()
    for p in (0.0, 0.1, 0.5):
        thr, scale = K.dropout_thr_scale_host(p)
        assert int(thr) == int(float(np.float32(p)) * 4294967296.0)
        assert scale.dtype == np.float32 and scale == np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    thr, scale = K.dropout_thr_scale_host(0.0)
    assert int(thr) == 0 and float(scale) == 1.0
    assert K.dropout_keep_host(0.0, SEED, 3, 1, 0, np.arange(37), np.arange(11)).all()
    assert int(K.dropout_thr_scale_host(0.5)[0]) == 1 << 31 and float(K.dropout_thr_scale_host(0.5)[1]) == 2.0
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            K.dropout_thr_scale_host(bad)


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
def test_keep_rate(p):
    """65,536 elements at a fixed seed: the kept fraction within 5 binomial
    standard deviations of 1 - p (a deterministic draw)."""
    K = _K()
    keep = K.dropout_keep_host(p, SEED, 7, 2, 1, np.arange(256), np.arange(256))
    n = keep.size
    assert n == 65536
    sd = np.sqrt(p * (1 - p) / n)
    assert abs(keep.mean() - (1 - p)) <= 5 * sd, (keep.mean(), sd)


def test_masks_differ_between_offsets_sites_heads():
    K = _K()
    rows, cols = np.arange(64), np.arange(64)
    base = K.dropout_keep_host(0.5, SEED, 0, 0, 0, rows, cols)
    assert (base == K.dropout_keep_host(0.5, SEED, 0, 0, 0, rows, cols)).all()
    for other in (K.dropout_keep_host(0.5, SEED, 1, 0, 0, rows, cols),
                  K.dropout_keep_host(0.5, SEED, 0, 1, 0, rows, cols),
                  K.dropout_keep_host(0.5, SEED, 0, 0, 1, rows, cols),
                  K.dropout_keep_host(0.5, SEED + 1, 0, 0, 0, rows, cols)):
        # independent fair bits agree on about half of 4096 elements (sd 32)
        agree = (base == other).mean()
        assert 0.4 < agree < 0.6, agree
    # a row of the node array has one mask whatever segment it is addressed from
    assert (K.dropout_keep_host(0.5, SEED, 0, 0, 0, np.arange(17, 40), cols) == base[17:40]).all()


def test_dropout_rng_follows_the_torch_seed():
    K = _K()
    state = torch.random.get_rng_state()
    try:
        torch.manual_seed(1234)
        probe = torch.rand(3)
        torch.manual_seed(1234)
        rng = K.DropoutRng()
        assert rng.next() == (1234, 0) and rng.next() == (1234, 1)
        assert torch.equal(torch.rand(3), probe), "DropoutRng.next() consumed from the torch generator"
        torch.manual_seed(99)
        assert rng.next() == (99, 2)
        assert K.DropoutRng(seed=5, offset=0xFFFFFFFF).next() == (5, 0xFFFFFFFF)
        wrap = K.DropoutRng(seed=5, offset=0xFFFFFFFF)
        wrap.next()
        assert wrap.next() == (5, 0)
        assert isinstance(K.DROPOUT_RNG, K.DropoutRng)
    finally:
        torch.random.set_rng_state(state)


def _scene_batch(sizes, seed):
    rs = np.random.RandomState(seed)
    off = np.concatenate([[0], np.cumsum(sizes)])
    labels = rs.randint(0, 4, off[-1]).astype(np.float32)      # 0: a ped in no group
    sse = torch.tensor([[int(off[i]), int(off[i + 1])] for i in range(len(sizes))])
    return off, labels, sse


@pytest.mark.parametrize("n_heads", [1, 2])
def test_gat_encoder_restatement_is_the_oracle(n_heads):
    """oracle GATEncoder (eval, dropout 0) == the dense fp64 restatement in
    this project's group order: both in float64, so they differ by
    reassociation only (bound 1e-10 of scale, ~1e6 ulp of headroom)."""
    from oracle import sgan_oracle as O
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        torch.manual_seed(3)
        mod = O.GATEncoder([40, 16, 40], n_heads, 0.0, 0.2).eval()
        off, labels, sse = _scene_batch([3, 7, 20], 5)
        x = torch.randn(int(off[-1]), 40)
        with torch.no_grad():
            want = mod(x, sse, None, torch.from_numpy(labels))
            got = gat_encoder_ref(mod, x, labels, off)
    finally:
        torch.set_default_dtype(old)
    close(got, want, rtol=1e-10, what="GATEncoder restatement")


def test_batch_gat_restatement_is_the_oracle():
    from oracle import sgan_oracle as O
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        torch.manual_seed(4)
        mod = O.BatchGATEncoder([40, 16, 40], [4, 1], 0.0, 0.2).eval()
        with torch.no_grad():
            for l in mod.gat_net.layer_stack:
                l.bias.normal_(0, 0.1)
        off, _, sse = _scene_batch([5, 20, 33], 6)
        x = torch.randn(int(off[-1]), 40)
        with torch.no_grad():
            want = mod(x, sse)
            got = batch_gat_ref(mod, x, off)
    finally:
        torch.set_default_dtype(old)
    close(got, want, rtol=1e-10, what="BatchGATEncoder restatement")
