"""The HDR/exposure path without a GPU: the fp64 specification (tests/tonemap_ref.py) against
torch.autograd on a straight restatement, tcnn's parameter counts, the construction of
NGP(rgb_act='None') with the reference's state-dict keys, and the three guards."""
import pytest
import torch

import tonemap_ref as R


class HP:
    grid, L, F, T, N_min, N_max, N_tables, rgb_channels, rgb_layers = "Hash", 16, 2, 12, 4, 256, 1, 64, 2


def _inputs(n, C, seed):
    g = torch.Generator().manual_seed(seed)
    lograd = torch.empty(n, C).uniform_(-6, 6, generator=g).half()
    dy = torch.empty(n, C, dtype=torch.float64).uniform_(-1, 1, generator=g)
    return lograd, dy, g


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("exposure", ["none", "scalar", "per_sample"])
def test_reference_matches_autograd(C, exposure):
    n = 257
    lograd, dy, g = _inputs(n, C, seed=1)
    params = R.xavier_params(C, seed=0)
    e = {"none": None, "scalar": torch.tensor(1 / 60),
         "per_sample": torch.tensor([0.25, 1.0, 4.0])[torch.randint(3, (n,), generator=g)]}[exposure]
    f = R.forward(lograd, e, params)
    assert not bool(f["kink"].any()), "pick another seed: a sample sits on a ReLU kink"
    # autograd on the restatement: padded rows, two matmuls per channel
    l64 = lograd.double().requires_grad_(True)
    p64 = params.half().double().requires_grad_(True)
    y = R.restatement(l64, R.log_exposure(e, n).double(), p64, C)
    assert torch.allclose(y, f["y"], rtol=0, atol=1e-13)
    (y * dy).sum().backward()
    # the specification's backward, fed the unrounded output so that both differentiate the same y
    b = R.backward(lograd, e, params, f["y"], dy)
    assert torch.allclose(b["dx"], l64.grad, rtol=1e-11, atol=1e-13)
    assert torch.allclose(b["g"], p64.grad, rtol=1e-11, atol=1e-13)
    # the absolute sums bound the values they belong to
    assert bool((b["dx"].abs() <= b["A_s"] * (1 + 1e-12)).all())
    assert bool((b["g"].abs() <= b["A"] * (1 + 1e-12)).all())
    gC = b["g"].reshape(C, 2048)
    w1 = gC[:, :1024].reshape(C, 64, 16)
    assert bool((w1[:, :, 1:] == w1[:, :, 1:2]).all()) and float(gC[:, 1024 + 64:].abs().max()) == 0


def test_reference_keep_mask_drops_samples():
    lograd, dy, _ = _inputs(65, 3, seed=2)
    params = R.xavier_params(3)
    y = R.forward(lograd, None, params)["y"]
    keep = torch.ones(65, dtype=torch.bool)
    keep[[3, 64]] = False
    dy0 = dy.clone()
    dy0[~keep] = 0
    a = R.backward(lograd, None, params, y, dy, keep=keep)
    b = R.backward(lograd, None, params, y, dy0)
    assert float(a["g"].abs().max()) > 0
    for k in ("g", "A"):  # the same terms, the dropped ones as zeros: equal up to the fp64 sum's order
        assert torch.allclose(a[k], b[k], rtol=1e-12, atol=0)


def test_kink_rate_of_the_gpu_test_inputs():
    """The GPU test leaves kink-flagged samples out and caps them at 1 %: on its inputs (seed-0 Xavier
    parameters, U(-6,6) half log-radiance) the specification flags well under that at n = 4099 and
    stays within the cap at every size the GPU test runs."""
    for C in (1, 3):
        for name in R.EXPOSURES:
            for n in (1, 63, 64, 65, 257, 4099):
                lograd, e, params = R.make_inputs(n, C, name)
                flagged = int(R.forward(lograd, e, params)["kink"].sum())
                assert flagged <= 0.01 * n, (n, C, name, flagged)
                if n == 4099:
                    assert flagged <= 0.005 * n, (C, name, flagged)


def test_mlp_shapes_pad_the_input_width():
    from mfnerf import tcnn
    assert sum(o * k for o, k in tcnn.mlp_shapes(1, 1, 64, 1)) == 2048
    assert tcnn.mlp_shapes(1, 1, 64, 1) == [(64, 16), (16, 64)]
    assert tcnn.mlp_shapes(32, 3, 64, 2) == [(64, 32), (64, 64), (16, 64)]
    assert tcnn.mlp_shapes(32, 16, 64, 1) == [(64, 32), (16, 64)]
    net = tcnn.Network(1, 1, {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "Sigmoid",
                              "n_neurons": 64, "n_hidden_layers": 1})
    assert net.params.numel() == 2048 and net.is_tonemapper()


def test_ngp_hdr_constructs_with_the_reference_keys():
    from mfnerf.networks import NGP
    m = NGP(0.5, HP, rgb_act="None")
    sd = m.state_dict()
    for i in range(3):
        assert sd[f"tonemapper_net_{i}.params"].shape == (2048,)
    assert m.rgb_net.output_activation == "None" and m.rgb_act == "None"
    ldr = NGP(0.5, HP)
    assert not any(k.startswith("tonemapper") for k in ldr.state_dict())
    assert sd["rgb_net.params"].shape == ldr.state_dict()["rgb_net.params"].shape
    with pytest.raises(RuntimeError):  # no CPU path, like the other modules
        m.log_radiance_to_rgb(torch.zeros(1, 3))
    with pytest.raises(NotImplementedError):
        NGP(0.5, HP, rgb_act="Exponential")


def test_guards_name_the_hdr_gap():
    from mfnerf import mesh, rendering, trainer
    from mfnerf.networks import NGP
    m = NGP(0.5, HP, rgb_act="None")
    o = torch.zeros(4, 3)
    with pytest.raises(NotImplementedError, match="HDR/exposure"):
        rendering.render_fused(m, o, o)
    with pytest.raises(NotImplementedError, match="HDR/exposure"):
        mesh.extract_mesh(m, resolution=8, colors=True)
    assert trainer.HParams().use_exposure is False
    with pytest.raises(NotImplementedError, match="HDR/exposure"):
        trainer.Trainer(trainer.HParams(use_exposure=True), train=None)
