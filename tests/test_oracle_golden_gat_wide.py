"""The float32 CPU oracle against the fixtures of make_golden_gat_wide.py
(scenes above 128 peds): within HALF of the tolerances the GPU tests apply
to the same fixtures, so a GPU failure there is the kernels', not a near tie
of the generator's max-pool the fixture happened to sit on."""
import numpy as np

from oracle import sgan_oracle as O

from test_oracle_golden import T, close, grad_floor, load_models, npz


def test_gat_encoder_wide_fixture():
    """GATEncoder, two heads, scenes of 200 / 130 / 150 / 20 peds: half of
    test_graph_module_vs_reference_fixture's out 1e-5, dx 1e-4, dw 2e-4."""
    f = npz("gat_encoder_wide.npz")
    assert np.diff(f["sse"], axis=1).ravel().tolist() == [200, 130, 150, 20]
    mod = O.GATEncoder([40, 16, 40], 2, 0.0, 0.2)
    mod.load_state_dict({k[2:]: T(f[k]) for k in f.files if k.startswith("w/")})
    x = T(f["x"]).requires_grad_(True)
    y = mod(x, T(f["sse"]), None, T(f["labels"]).view(-1, 1))
    close(y.detach(), f["out"], rtol=0.5e-5)
    (y * T(f["dout"])).sum().backward()
    close(x.grad, f["dx"], rtol=0.5e-4)
    for k, p in mod.named_parameters():
        if "dw/" + k in f.files:
            close(p.grad, f["dw/" + k], rtol=1e-4, floor=grad_floor(f, "dw/"))


def test_generator_gat_wide_fixture():
    """The gat generator on 129 / 3 / 200 / 20 peds: half of
    test_generator_vs_reference_fixture's out 1e-4, gradients 1e-3."""
    f = npz("gen_fwd_gat_wide.npz")
    assert np.diff(f["seq_start_end"], axis=1).ravel().tolist() == [129, 3, 200, 20]
    g, _ = load_models(graph="gat")
    y = g(T(f["obs_traj"]), T(f["obs_traj_rel"]), T(f["seq_start_end"]), T(f["obs_traj_g"]), user_noise=T(f["noise"]))
    close(y.detach(), f["gat/out"], rtol=0.5e-4)
    (y * T(f["gat/dout"])).sum().backward()
    fl = grad_floor(f, "gat/dw/")
    n = 0
    for k, p in g.named_parameters():
        if "gat/dw/" + k in f.files:
            close(p.grad, f["gat/dw/" + k], rtol=0.5e-3, floor=fl)
            n += 1
    assert n > 20
