"""The HDR tonemapper kernels (csrc/tonemap.hip) and the host path around them on the GPU, against
the fp64 specification tests/tonemap_ref.py (same fp16 points) and the fixture tests/golden/
hdr_forward.npz captured from the reference's own NGP(rgb_act='None') host code.

Bounds.  Forward: |y - y_ref| <= 2^-10 + 2^-13 B, B = sum_j |W2h[0,j] h_j|: one half-ulp of the half
output at 1, doubled, plus a half-ulp flip in every hidden unit through the sigmoid's slope of at most
1/4.  Gradients, the specification fed the kernel's own saved y: |dx - ref| <= (2^-9 + 64 2^-23) A_s and
|g - ref| <= (2^-9 + n 2^-23) A with A_s, A the sums of the absolute terms.  Samples with a hidden
pre-activation within 1e-5 of the ReLU kink (at most 1 % of them) get a zero upstream gradient and
are left out of the gradient comparisons.
"""
import functools
import os

import numpy as np
import pytest
import torch

import tonemap_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 257, 4099]  # wave, workgroup and second-stage seams
TCNN_CFG = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "Sigmoid", "n_neurons": 64,
            "n_hidden_layers": 1}


class HP:
    grid, L, F, T, N_min, N_max, N_tables, rgb_channels, rgb_layers = "Hash", 16, 2, 14, 4, 256, 1, 64, 2


def _dev_exposure(e, dev):
    """(device f32 tensor or None, stride) of a make_inputs exposure."""
    if e is None:
        return None, 0
    e = e.to(dev).float().reshape(-1).contiguous()
    return e, 0 if e.numel() == 1 else 1


@functools.lru_cache(maxsize=None)
def _case(n, C, name):
    """One kernel run (forward, backward twice) and its specification values, shared by the tests."""
    from mfnerf import tonemap
    dev = torch.device("cuda:0")
    lograd, e, params = R.make_inputs(n, C, name)
    f = R.forward(lograd, e, params)
    dy = torch.empty(n, C).uniform_(-1, 1, generator=torch.Generator().manual_seed(n + 7))
    dy[f["kink"]] = 0
    l_d, p_d, dy_d = lograd.to(dev), params.to(dev), dy.to(dev)
    e_d, stride = _dev_exposure(e, dev)
    y = tonemap.tonemap_fw(l_d, e_d, stride, p_d)
    dx, g = tonemap.tonemap_bw(l_d, e_d, stride, p_d, y, dy_d)
    dx2, g2 = tonemap.tonemap_bw(l_d, e_d, stride, p_d, y, dy_d)
    torch.cuda.synchronize()
    b = R.backward(lograd, e, params, y.cpu(), dy)
    return {"f": f, "b": b, "y": y.cpu(), "dx": dx.cpu(), "g": g.cpu(), "dx2": dx2.cpu(), "g2": g2.cpu()}


CASES = [(n, C, name) for C in (1, 3) for name in R.EXPOSURES for n in SIZES]


def _id(c):
    return f"n{c[0]}-C{c[1]}-{c[2]}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_vs_specification(gpu, case):
    r = _case(*case)
    assert r["y"].dtype == torch.float16 and r["y"].shape == (case[0], case[1])
    err = (r["y"].double() - r["f"]["y"]).abs()
    bound = 2.0 ** -10 + 2.0 ** -13 * r["f"]["B"]
    print("forward max err/bound", float((err / bound).max()) if err.numel() else 0.0)
    assert bool((err <= bound).all())


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_backward_vs_specification(gpu, case):
    n, C, _ = case
    r = _case(*case)
    kink = r["f"]["kink"]
    assert int(kink.sum()) <= 0.01 * n, "too many samples on a ReLU kink for this comparison"
    b = r["b"]
    keep = ~kink
    err = (r["dx"].double() - b["dx"]).abs()[keep]
    bound = ((2.0 ** -9 + 64 * 2.0 ** -23) * b["A_s"])[keep]
    print("dx max err/bound", float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0)
    assert bool((err <= bound).all())
    gerr = (r["g"].double() - b["g"]).abs()
    gbound = (2.0 ** -9 + n * 2.0 ** -23) * b["A"]
    print("grad_params max err/bound", float((gerr / gbound.clamp(min=1e-300)).max()))
    assert bool((gerr <= gbound).all())
    g = r["g"].reshape(C, 2048)
    w1 = g[:, :1024].reshape(C, 64, 16)
    assert bool((w1[:, :, 1:] == w1[:, :, 1:2]).all()), "dW1 columns 1..15 all carry the bias gradient"
    assert float(g[:, 1024 + 64:].abs().max()) == 0, "dW2 rows 1..15 are unused"
    if n >= 63:
        assert float(g.abs().max()) > 0
    # a fixed-order reduction: the same bits on every run
    assert torch.equal(r["dx"], r["dx2"]) and torch.equal(r["g"], r["g2"])


@pytest.mark.parametrize("C", [1, 3])
def test_empty_call_zeroes_the_parameter_gradient(gpu, C):
    from mfnerf._lib import call, ptr, stream
    p = R.xavier_params(C).to(gpu)
    g = torch.full((C * 2048,), float("nan"), device=gpu)
    call("mfnerf_tonemap_bw", ptr(None), ptr(None), 0, 0, C, ptr(p), ptr(None), ptr(None), ptr(None), ptr(g), ptr(None),
         stream())
    call("mfnerf_tonemap_fw", ptr(None), ptr(None), 0, 0, C, ptr(p), ptr(None), stream())
    assert float(g.abs().max()) == 0


def test_bad_arguments_are_refused(gpu):
    from mfnerf import tonemap
    p = R.xavier_params(3).to(gpu)
    with pytest.raises(RuntimeError):
        tonemap.tonemap_fw(torch.zeros(4, 2, dtype=torch.float16, device=gpu), None, 0, p[:4096])
    with pytest.raises(RuntimeError, match="exposure_stride"):
        tonemap.tonemap_fw(torch.zeros(4, 3, dtype=torch.float16, device=gpu), torch.ones(8, device=gpu), 2, p)
    with pytest.raises(RuntimeError, match="exposure"):
        tonemap.TonemapFunction.apply(torch.zeros(4, 3, device=gpu), torch.ones(3, device=gpu), p)
    with pytest.raises(RuntimeError, match="GPU"):
        tonemap.TonemapFunction.apply(torch.zeros(4, 3), None, p.cpu())


def _hdr_model(gpu, table_seed=7, gain=2.0):
    from mfnerf.networks import NGP
    model = NGP(0.5, HP, rgb_act="None").to(gpu)
    n_net = model.xyz_encoder.n_net
    with torch.no_grad():
        g = torch.Generator().manual_seed(table_seed)
        tab = torch.empty(model.xyz_encoder.params.numel() - n_net).uniform_(-0.5, 0.5, generator=g)
        model.xyz_encoder.params[n_net:].copy_(tab)
        model.xyz_encoder.params[:n_net].mul_(gain)
        model.rgb_net.params.mul_(gain)
    return model


def test_unit_exposure_call_of_the_training_step(gpu):
    """train.py:172-177: log_radiance_to_rgb(zeros(1,3), exposure=ones(1,1)), its loss and gradient."""
    model = _hdr_model(gpu)
    zero = torch.zeros(1, 3, device=gpu, requires_grad=True)
    rgb = model.log_radiance_to_rgb(zero, exposure=torch.ones(1, 1, device=gpu))
    assert rgb.shape == (1, 3) and bool(torch.isfinite(rgb).all())
    (0.5 * (rgb.float() - 0.5) ** 2).mean().backward()
    assert zero.grad.dtype == torch.float32 and bool(torch.isfinite(zero.grad).all())
    for i in range(3):
        gp = getattr(model, f"tonemapper_net_{i}").params.grad
        assert gp.shape == (2048,) and bool(torch.isfinite(gp).all()) and float(gp.abs().max()) > 0
    ref = R.forward(torch.zeros(1, 3).half(), None,
                    torch.cat([getattr(model, f"tonemapper_net_{i}").params.detach().cpu() for i in range(3)]))
    assert bool(((rgb.detach().cpu().double() - ref["y"]).abs() <= 2.0 ** -10 + 2.0 ** -13 * ref["B"]).all())


def test_model_forward_composition(gpu):
    """NGP('None').forward = the specification's tonemap of the model's own module outputs + log e;
    output_radiance = exp of them."""
    model = _hdr_model(gpu)
    g = torch.Generator().manual_seed(3)
    n = 300
    x = torch.empty(n, 3).uniform_(-0.5, 0.5, generator=g).to(gpu)
    d = torch.randn(n, 3, generator=g).to(gpu)
    e = torch.tensor([0.25, 1.0, 4.0])[torch.randint(3, (n,), generator=g)]
    with torch.no_grad():
        h = model.xyz_encoder((x - model.xyz_min) / (model.xyz_max - model.xyz_min))
        dn = d / torch.norm(d, dim=1, keepdim=True)
        lograd = model.rgb_net(torch.cat([model.dir_encoder((dn + 1) / 2), h], 1))
        params = torch.cat([getattr(model, f"tonemapper_net_{i}").params for i in range(3)]).cpu()
        for exposure, kw in ((e, {"exposure": e.to(gpu).reshape(n, 1)}), (torch.tensor(4.0), {"exposure": torch.tensor(4.0, device=gpu)}),
                             (None, {})):
            sigmas, rgbs = model(x, d, **kw)
            ref = R.forward(lograd.cpu(), exposure, params)
            assert rgbs.shape == (n, 3)
            assert bool(((rgbs.cpu().double() - ref["y"]).abs() <= 2.0 ** -10 + 2.0 ** -13 * ref["B"]).all())
            assert torch.equal(sigmas, torch.exp(h[:, 0].float()))
        sig_r, rad = model(x, d, output_radiance=True, exposure=e.to(gpu).reshape(n, 1))
        assert torch.equal(rad, torch.exp(lograd.float())) and torch.equal(sig_r, sigmas)


def test_tcnn_network_swap_route(gpu):
    """tcnn.Network(1, 1, ...)(x) -- what the reference's log_radiance_to_rgb calls over the module
    swap -- equals channel 0 of the fused call with no exposure; other widths still raise."""
    from mfnerf import tcnn, tonemap
    net = tcnn.Network(1, 1, TCNN_CFG).to(gpu)
    lograd, _, other = R.make_inputs(257, 3, "none")
    lograd = lograd.to(gpu)
    x = lograd[:, :1].float().requires_grad_(True)
    y = net(x)
    fused = tonemap.tonemap_fw(lograd, None, 0, torch.cat([net.params.detach(), other[2048:].to(gpu)]))
    assert y.shape == (257, 1) and y.dtype == torch.float16 and torch.equal(y[:, 0], fused[:, 0])
    y.float().sum().backward()
    assert x.grad.shape == x.shape and net.params.grad.shape == (2048,) and float(net.params.grad.abs().max()) > 0
    with pytest.raises(NotImplementedError):
        tcnn.Network(2, 1, TCNN_CFG).to(gpu)(torch.zeros(4, 2, device=gpu))


def test_train_mode_render_backpropagates_everywhere(gpu):
    from mfnerf import synthetic, vren
    from mfnerf.rendering import render
    model = _hdr_model(gpu, gain=1.0)
    grid = synthetic.ball_density_grid(G=model.grid_size, cascades=model.cascades, scale=0.5, seed=3).to(gpu)
    vren.packbits(grid.contiguous(), 0.01 * 1024 / 3 ** 0.5, model.density_bitfield)
    N = 256
    o, d = synthetic.random_rays(N, synthetic.camera_poses(n_cams=8, seed=2), seed=4, device=gpu)
    g = torch.Generator().manual_seed(5)
    e = torch.tensor([0.25, 1.0, 4.0])[torch.randint(3, (N,), generator=g)].reshape(N, 1).to(gpu)
    res = render(model, o, d, exposure=e)
    assert int(res["rm_samples"]) > 0
    target = torch.rand(N, 3, generator=g).to(gpu)
    ((res["rgb"] - target) ** 2).mean().backward()
    names = [k for k, _ in model.named_parameters()]
    assert {f"tonemapper_net_{i}.params" for i in range(3)} <= set(names)
    for k, p in model.named_parameters():
        if p.numel() == 0:  # the SH encoding owns no parameters
            continue
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k


def test_tonemappers_learn_a_camera_response(gpu):
    """The three tonemappers alone fit clip(radiance * e, 0, 1)^(1/2.2): after 300 Adam steps the MSE is
    at most 1/20 of the initial one (the fp16-point torch restatement reaches 1/380 - 1/1800)."""
    from mfnerf.tonemap import TonemapFunction
    g = torch.Generator().manual_seed(0)
    n = 4096
    lograd = torch.empty(n, 3).uniform_(-5, 3, generator=g).half()
    e = torch.tensor([0.25, 1.0, 4.0])[torch.randint(3, (n,), generator=g)].reshape(n, 1)
    target = (torch.exp(lograd.float()) * e).clamp(0, 1) ** (1 / 2.2)
    lograd, e, target = lograd.to(gpu), e.to(gpu), target.to(gpu)
    params = torch.nn.Parameter(R.xavier_params(3, seed=0).to(gpu))
    opt = torch.optim.Adam([params], lr=1e-2, eps=1e-15)
    first = last = None
    for _ in range(300):
        opt.zero_grad()
        loss = ((TonemapFunction.apply(lograd, e, params).float() - target) ** 2).mean()
        loss.backward()
        opt.step()
        last = loss.detach()
        first = last if first is None else first
    first, last = float(first), float(last)
    print("mse", first, "->", last, "ratio", first / last)
    assert last <= first / 20


def test_reference_host_composition_fixture(gpu):
    """tests/golden/hdr_forward.npz (the reference's own NGP(rgb_act='None').forward and
    log_radiance_to_rgb over restatements, make_golden_hdr.py): + log(exposure) and the channel order at
    the forward bound on the fixture's own log-radiance; the normalisation, (d + 1) / 2 and the
    concatenation order through output_radiance, where the fp16 MFMA networks meet the fixture's fp32
    ones (three layers of half-ulp roundings, 2^-10 of absolute sums some ten times the output: within
    2^-6 (1 + |log-radiance|), while a swapped or unmapped input moves it by O(1))."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "hdr_forward.npz"))
    z = {k: torch.from_numpy(z[k]) for k in z.files}
    model = _hdr_model(gpu, table_seed=int(z["table_seed"]), gain=1.0)
    n_net = model.xyz_encoder.n_net
    with torch.no_grad():
        model.xyz_encoder.params[:n_net].copy_(z["xyz_net_params"])
        model.rgb_net.params.copy_(z["rgb_params"])
        for i in range(3):
            getattr(model, f"tonemapper_net_{i}").params.copy_(z["tonemapper_params"][i])
        params = z["tonemapper_params"].reshape(-1)
        lograd = z["lograd"].to(gpu)
        for key, exposure, kw in (("rgb", z["exposure"], {"exposure": z["exposure"].to(gpu)}),
                                  ("rgb_scalar4", torch.tensor(4.0), {"exposure": torch.tensor(4.0, device=gpu)}),
                                  ("rgb_unit", None, {})):
            B = R.forward(z["lograd"], exposure, params)["B"]
            got = model.log_radiance_to_rgb(lograd, **kw).cpu().double()
            assert bool(((got - z[key]).abs() <= 2.0 ** -10 + 2.0 ** -13 * B).all()), key
        unit = model.log_radiance_to_rgb(torch.zeros(1, 3, device=gpu), exposure=torch.ones(1, 1, device=gpu))
        B1 = R.forward(torch.zeros(1, 3).half(), None, params)["B"]
        assert bool(((unit.cpu().double() - z["unit_exposure_rgb"]).abs() <= 2.0 ** -10 + 2.0 ** -13 * B1).all())
        sigmas, rad = model(z["x"].to(gpu), z["d"].to(gpu), output_radiance=True)
        lr = torch.log(rad).cpu()
        ref = z["lograd"].float()
        assert bool(((lr - ref).abs() <= 2.0 ** -6 * (1 + ref.abs())).all()), float((lr - ref).abs().max())
        ls, ls_ref = torch.log(sigmas).cpu(), torch.log(z["sigmas"])
        assert bool(((ls - ls_ref).abs() <= 2.0 ** -6 * (1 + ls_ref.abs())).all())
