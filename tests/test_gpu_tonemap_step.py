"""The tonemap kernels as the fused training step runs them (csrc/tonemap.hip: the live-count pair,
the per-ray exposure expansion, the unit-exposure term, the side Adam) against the module kernels
(bit for bit where the arithmetic is the same) and the fp64 specification tests/tonemap_ref.py.

Bounds are test_gpu_tonemap.py's: forward 2^-10 + 2^-13 B, parameter gradient (2^-9 + n 2^-23) A;
the side Adam's tolerance is test_gpu_optim.py's.
"""
import functools

import pytest
import torch

import tonemap_ref as R

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 257, 4099]  # wave, workgroup and second-stage seams (test_gpu_tonemap.py's)
PAD = 77                               # capacity = n + PAD rows: the rows past the live count
SENTINEL = -7.0


def _count(n, dev):
    return torch.tensor([n], dtype=torch.int32, device=dev)


@functools.lru_cache(maxsize=None)
def _case(n):
    """One run of the module pair at n and of the live pair at capacity n + PAD (backward twice),
    with NaN in every input row past the live count, shared by the tests."""
    from mfnerf import tonemap
    dev = torch.device("cuda:0")
    cap = n + PAD
    lograd, e, params = R.make_inputs(n, 3, "per_sample")
    f = R.forward(lograd, e, params)
    dy = torch.empty(n, 3).uniform_(-1, 1, generator=torch.Generator().manual_seed(n + 7))
    dy[f["kink"]] = 0
    l_d, e_d, p_d, dy_d = lograd.to(dev), e.to(dev).float().contiguous(), params.to(dev), dy.to(dev)
    y = tonemap.tonemap_fw(l_d, e_d, 1, p_d)
    dx, g = tonemap.tonemap_bw(l_d, e_d, 1, p_d, y, dy_d)

    def padded(t, fill=float("nan")):
        out = torch.full((cap,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=dev)
        out[:n] = t
        return out
    l_c, e_c, dy_c = padded(l_d), padded(e_d), padded(dy_d)
    cnt = _count(n, dev)
    y_live = torch.full((cap, 3), SENTINEL, device=dev)
    tonemap.tonemap_fw_live(l_c, e_c, cnt, p_d, y_live)
    ws = tonemap.live_workspace(cap, dev)
    ws.fill_(0xff)  # (NaN patterns: the workspace may hold anything)
    outs = []
    for _ in range(2):
        dx_live = torch.full((cap, 3), SENTINEL, device=dev)
        g_live = torch.full((3 * 2048,), float("nan"), device=dev)
        tonemap.tonemap_bw_live(l_c, e_c, cnt, p_d, y_live, dy_c, dx_live, g_live, ws)
        outs.append((dx_live.cpu(), g_live.cpu()))
    torch.cuda.synchronize()
    b = R.backward(lograd, e, params, y.cpu(), dy)
    return {"n": n, "f": f, "b": b, "y": y.cpu(), "dx": dx.cpu(), "g": g.cpu(), "y_live": y_live.cpu(), "bw": outs}


@pytest.mark.parametrize("n", SIZES)
def test_live_forward_equals_the_module_kernel(gpu, n):
    r = _case(n)
    assert r["y_live"].dtype == torch.float32
    assert torch.equal(r["y_live"][:n], r["y"].float())
    assert bool((r["y_live"][n:] == SENTINEL).all()), "rows past the live count are untouched"


@pytest.mark.parametrize("n", SIZES)
def test_live_backward(gpu, n):
    r = _case(n)
    kink = r["f"]["kink"]
    assert int(kink.sum()) <= 0.01 * n, "too many samples on a ReLU kink for this comparison"
    (dx1, g1), (dx2, g2) = r["bw"]
    assert torch.equal(dx1[:n], r["dx"]), "dL/dlograd is the module kernel's, bit for bit"
    assert bool((dx1[n:] == SENTINEL).all()), "rows past the live count are untouched"
    b = r["b"]
    gerr = (g1.double() - b["g"]).abs()
    gbound = (2.0 ** -9 + n * 2.0 ** -23) * b["A"]
    print("grad_params max err/bound", float((gerr / gbound.clamp(min=1e-300)).max()))
    assert bool((gerr <= gbound).all())
    assert torch.equal(dx1, dx2) and torch.equal(g1, g2), "a fixed-order reduction: the same bits on every run"
    if n == 0:
        assert float(g1.abs().max()) == 0, "*n_dev == 0 zeroes the gradient"
    elif n >= 63:
        assert float(g1.abs().max()) > 0


def test_live_pair_is_capturable(gpu):
    """Both launches inside a HIP graph, the count changed between replays."""
    from mfnerf import tonemap
    n = 257
    r = _case(n)
    lograd, e, params = R.make_inputs(n, 3, "per_sample")
    l_d, e_d, p_d = lograd.to(gpu), e.to(gpu).float().contiguous(), params.to(gpu)
    cnt = _count(n, gpu)
    y = torch.full((n, 3), SENTINEL, device=gpu)
    dy = torch.ones(n, 3, device=gpu)
    dx = torch.full((n, 3), SENTINEL, device=gpu)
    g = torch.empty(3 * 2048, device=gpu)
    ws = tonemap.live_workspace(n, gpu)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tonemap.tonemap_fw_live(l_d, e_d, cnt, p_d, y)
        tonemap.tonemap_bw_live(l_d, e_d, cnt, p_d, y, dy, dx, g, ws)
    graph.replay()
    assert torch.equal(y.cpu(), r["y"].float())
    y.fill_(SENTINEL)
    cnt.fill_(64)
    graph.replay()
    assert torch.equal(y[:64].cpu(), r["y"][:64].float()) and bool((y[64:] == SENTINEL).all())
    cnt.zero_()
    graph.replay()
    assert float(g.abs().max()) == 0


# ---------------------------------------------------------------------------- expansion
def test_expand_exposure(gpu):
    """rendering.py:142-145 over rays of {0, 1, 63, 64, 65, 1024} samples (twice each, shuffled), a
    permuted rays_a[:,0]: equal to the torch construction, nothing written past the count."""
    from mfnerf import tonemap
    g = torch.Generator().manual_seed(0)
    counts = torch.tensor([0, 1, 63, 64, 65, 1024] * 2)[torch.randperm(12, generator=g)]
    n_rays = counts.numel()
    starts = torch.cumsum(counts, 0) - counts
    rays_a = torch.stack([torch.randperm(n_rays, generator=g), starts, counts], 1).to(gpu)
    n = int(counts.sum())
    exposure_ray = torch.tensor([0.25, 1.0, 4.0])[torch.randint(3, (n_rays,), generator=g)] * \
        (1 + torch.rand(n_rays, generator=g))
    exposure_ray = exposure_ray.to(gpu)
    want = torch.repeat_interleave(exposure_ray[rays_a[:, 0]], rays_a[:, 2], 0)
    assert want.numel() == n
    cap = n + PAD
    out = torch.full((cap,), SENTINEL, device=gpu)
    tonemap.expand_exposure(exposure_ray, rays_a, _count(n, gpu), out)
    assert torch.equal(out[:n], want) and bool((out[n:] == SENTINEL).all())
    # a device count below the marched total (an overflowing march clips rays_a itself; the kernel
    # clips too): nothing at or past the count is written
    low = n - 700
    out.fill_(SENTINEL)
    tonemap.expand_exposure(exposure_ray, rays_a, _count(low, gpu), out)
    assert torch.equal(out[:low], want[:low]) and bool((out[low:] == SENTINEL).all())
    out.fill_(SENTINEL)
    tonemap.expand_exposure(exposure_ray, rays_a, _count(0, gpu), out)
    assert bool((out == SENTINEL).all())


# ---------------------------------------------------------------------------- unit-exposure term
@pytest.mark.parametrize("target", [0.5, 0.73])
def test_unit_exposure_term(gpu, target):
    """train.py:172-177 at n = 1: the loss and the gradient ADDED on top of a non-zero one, against
    the specification at log-radiance 0 / no exposure, under the forward and gradient bounds."""
    from mfnerf import tonemap
    params = R.xavier_params(3, seed=2)
    zero = torch.zeros(1, 3).half()
    f = R.forward(zero, None, params)
    p_d = params.to(gpu)
    y16 = tonemap.tonemap_fw(zero.to(gpu), None, 0, p_d)  # the half output the kernel's gradient starts from
    assert bool(((y16.cpu().double() - f["y"]).abs() <= 2.0 ** -10 + 2.0 ** -13 * f["B"]).all())
    y = y16.cpu().double()
    b = R.backward(zero, None, params, y16.cpu(), (y - target) / 3)
    base = torch.empty(3 * 2048).uniform_(-1, 1, generator=torch.Generator().manual_seed(1))
    grad = base.clone().to(gpu)
    loss = torch.full((3,), float("nan"), device=gpu)
    amp = torch.zeros(8, dtype=torch.int32, device=gpu)
    tonemap.unit_loss(p_d, target, grad, loss, amp)
    # the loss: each channel's share 0.5 (y_c - u)^2 / 3 from the kernel's own half output (fp32 arithmetic)
    # d = y - u carries at most 2^-24 (u rounded to fp32, one subtraction below 1); d*d and /3 round once each
    d = (y - target).reshape(3)
    want = 0.5 * d ** 2 / 3
    assert bool(((loss.cpu().double() - want).abs() <= d.abs() * 2.0 ** -24 / 3 + 3 * 2.0 ** -24 * want + 1e-14).all())
    # ... and from the specification's y, through the forward bound: |d loss| <= |y - u| |dy| / 3 (+ dy^2 / 6)
    dyb = (2.0 ** -10 + 2.0 ** -13 * f["B"]).reshape(3)
    spec = (0.5 * (f["y"] - target) ** 2 / 3).reshape(3)
    assert bool(((loss.cpu().double() - spec).abs() <= ((f["y"].reshape(3) - target).abs() * dyb + dyb ** 2 / 2) / 3
                 + 2.0 ** -22 * spec).all())
    added = grad.cpu().double() - base.double()
    # n = 1, plus one fp32 rounding of the sum base + term (|base| <= 1)
    bound = (2.0 ** -9 + 2.0 ** -23) * b["A"] + 2.0 ** -23 * (base.double().abs() + b["g"].abs())
    assert bool(((added - b["g"]).abs() <= bound).all())
    assert float(b["g"].abs().max()) > 0
    assert int(amp[0]) == 0
    # deterministic, and a non-finite summed gradient raises the step's flag
    grad2 = base.clone().to(gpu)
    tonemap.unit_loss(p_d, target, grad2, loss, amp)
    assert torch.equal(grad, grad2)
    grad2[1024 + 5] = float("inf")
    tonemap.unit_loss(p_d, target, grad2, loss, amp)
    assert int(amp[0]) == 1


# ---------------------------------------------------------------------------- side Adam
def test_side_adam_vs_fp64(gpu):
    """Three steps of mfnerf_side_adam_step on 6144 parameters against fp64 Adam (test_gpu_optim.py's
    tolerance), the device step counter and lr; with the non-finite flag up nothing moves and the
    flag stays."""
    from mfnerf import tonemap
    g = torch.Generator().manual_seed(0)
    n, lr, b1, b2, eps = 3 * 2048, 1e-2, 0.9, 0.999, 1e-15
    p = torch.randn(n, generator=g)
    pd, md, vd = p.to(gpu), torch.zeros(n, device=gpu), torch.zeros(n, device=gpu)
    step = torch.zeros(1, dtype=torch.int32, device=gpu)
    lr_dev = torch.full((1,), lr, device=gpu)
    amp = torch.zeros(8, dtype=torch.int32, device=gpu)
    P, M, V = p.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)

    def f32(x):
        return float(torch.tensor(x, dtype=torch.float32))
    lr_sum = 0.0
    for t in range(1, 4):
        gr = torch.randn(n, generator=g) * 10.0 ** (t - 3)
        if t == 3:
            lr = 5e-3
            lr_dev.fill_(lr)
        tonemap.side_adam_step(pd, gr.to(gpu), md, vd, 123.0, (b1, b2), eps, step, lr_dev, amp)  # (lr_dev overrides lr)
        # test_gpu_optim.py's apex_adam: fp64 with the hyper-parameters as the fp32 values the kernel receives
        G, c1, c2 = gr.double(), f32(b1), f32(b2)
        M = c1 * M + (1 - c1) * G
        V = c2 * V + (1 - c2) * G * G
        P = P - f32(lr) * ((M / (1 - c1 ** t)) / (torch.sqrt(V / (1 - c2 ** t)) + f32(eps)))
        lr_sum += lr
        assert int(step) == t
        # ... and its checks: _check_params (2 ulps + 1e-5 of the summed steps), _check (2e-6 of the scale)
        perr = (pd.double().cpu() - P).abs() / (P.abs() * 2.0 ** -22 + 1e-5 * lr_sum)
        assert float(perr.max()) < 1.0, float(perr.max())
        for got, ref in ((md, M), (vd, V)):
            assert float((got.double().cpu() - ref).abs().max() / ref.abs().max()) < 2e-6
    amp[0] = 1
    before = [t.clone() for t in (pd, md, vd, step)]
    tonemap.side_adam_step(pd, torch.full((n,), float("nan"), device=gpu), md, vd, lr, (b1, b2), eps, step, lr_dev, amp)
    for a, b_ in zip(before, (pd, md, vd, step)):
        assert torch.equal(a, b_)
    assert int(amp[0]) == 1, "the flag is left for the main optimizer call"
