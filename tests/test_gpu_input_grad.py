"""The field's input gradients on the GPU: dL/dx through the grid encoding (mfnerf_grid_encode_bw_input),
dL/ddirs through the SH + colour head (mfnerf_field_bw_inputs), their per-ray reduction
(mfnerf_rays_input_grad), the autograd surface (rays that require a gradient, the tcnn route) and the
fused engine's ray_grads option.  References: tests/input_grad_ref.py (fp64)."""
import functools
import math
import types

import pytest
import torch

import input_grad_ref as R
from mfnerf import engine, synthetic, tcnn
from mfnerf import field as FLD
from mfnerf._lib import call, ptr, stream
from mfnerf.custom_functions import RayMarcher
from oracle import field_oracle as FO

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _setup(kind, n_tables):
    olay, lay = R.layouts(kind, n_tables)
    assert any(k == 0 and lay.res[l] ** 3 <= lay.sizes[l] for l, k in enumerate(lay.kind)), "no dense level"
    assert any(k == 1 or lay.res[l] ** 3 > lay.sizes[l] for l, k in enumerate(lay.kind)), "no hashed/shared level"
    return olay, lay, lay.desc(), R.random_table16(olay, seed=7)


def _face_point(olay):
    """x in [0,1] whose fp32 pos = fmaf(scale, x, 0.5) is an integer at the finest level: a point
    exactly on a cell face (w = 0 there)."""
    s = float(olay.scales[-1])
    for k in range(300, 400):
        x = torch.tensor((k - 0.5) / s, dtype=torch.float32)
        pos = (x.double() * s + 0.5).float()
        if float(pos) == float(k):
            return float(x)
    raise AssertionError("no exactly representable face point found")


def _points(n, olay, seed):
    x = R.points(n, seed)
    if n >= 4:
        x[3] = torch.tensor([_face_point(olay), 0.3, 0.6])
    return x


def _check_dx(got, ref, A, what):
    err = (got.double() - ref).abs()
    ratio = float((err / A.clamp_min(1e-300)).max())
    print(f"{what}: max |got - ref| / A = {ratio:.3e} (bound 2^-15 = {2 ** -15:.3e})")
    assert torch.isfinite(got).all()
    assert (err <= 2.0 ** -15 * A).all(), (what, ratio)


# ------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2049])
@pytest.mark.parametrize("kind,n_tables", R.KINDS)
def test_grid_encode_bw_input_matches_fp64(gpu, kind, n_tables, n):
    """Per component |got - ref| <= 2^-15 A, A the fp64 sum of the absolute values of its 256 terms (a
    256-term fp32 sum plus ~4 roundings per term is <= 2^-16 A; 2x allowed).  Corner points, a point on
    a cell face of the finest level; the second call gives the same bits."""
    olay, lay, desc, table = _setup(kind, n_tables)
    x = _points(n, olay, seed=n)
    dy = torch.randn(n, 32, generator=torch.Generator().manual_seed(100 + n))
    ref, A = R.dx_ref(x, table, dy, olay)
    t16, xg, dyg = table.to(gpu), x.to(gpu), dy.to(gpu)
    got = FLD.grid_encode_bw_input(xg, n, t16, dyg, desc)
    again = FLD.grid_encode_bw_input(xg, n, t16, dyg, desc)
    _check_dx(got.cpu(), ref, A, f"{kind} n={n}")
    assert torch.equal(got, again)


@pytest.mark.parametrize("kind,n_tables", R.KINDS)
def test_grid_encode_bw_input_world_coordinates_and_live_count(gpu, kind, n_tables):
    """x_min = -0.5, x_range = 1 (world coordinates), and n_dev < n: rows past it keep a sentinel."""
    olay, lay, desc, table = _setup(kind, n_tables)
    n, live = 65, 40
    xw = _points(n, olay, seed=5) - 0.5
    dy = torch.randn(n, 32, generator=torch.Generator().manual_seed(6))
    x01 = R.normalise(xw, -0.5, 1.0)
    ref, A = R.dx_ref(x01, table, dy, olay, x_range=1.0)
    t16, xg, dyg = table.to(gpu), xw.to(gpu), dy.to(gpu)
    got = FLD.grid_encode_bw_input(xg, n, t16, dyg, desc, x_min=-0.5, x_range=1.0)
    _check_dx(got.cpu(), ref, A, f"{kind} world")
    out = torch.full((n, 3), -7.0, device=gpu)
    n_dev = torch.tensor([live], dtype=torch.int32, device=gpu)
    FLD.grid_encode_bw_input(xg, n, t16, dyg, desc, x_min=-0.5, x_range=1.0, n_dev=n_dev, out=out)
    assert torch.equal(out[:live], got[:live])
    assert bool((out[live:] == -7.0).all())
    # a range other than 1: the chain rule's 1/x_range
    ref2, A2 = R.dx_ref(R.normalise(xw * 2, -1.0, 2.0), table, dy, olay, x_range=2.0)
    got2 = FLD.grid_encode_bw_input((xw * 2).to(gpu), n, t16, dyg, desc, x_min=-1.0, x_range=2.0)
    _check_dx(got2.cpu(), ref2, A2, f"{kind} x_range=2")


# ------------------------------------------------------------------------------------------- (b)
def _field_inputs(N, seed=8, width=64):
    """test_gpu_field's _field_inputs (Xavier weights) plus the incoming gradients of test_field_bw.  The directions are not unit length: random unit vectors times a length in
    [0.5, 2], row 0 the axis-aligned (0, 0, 2).  dL/dd scales with 1/|d|, so lengths drawn as a
    normal vector's (down to ~0.1) would let the few shortest directions carry the whole cosine
    against the fp32 reference: it would measure those samples' fp16 rounding, not the batch's.

    The seed is one on which the two references are usable at the limits test_field_bw sets, judged on
    the references alone (CPU, no kernel): the fp16-point emulation depends on its fp32 accumulation
    order wherever a hidden unit's pre-activation rounds to a different fp16 value or sign -- over
    seeds 5..13 its dL/ddirs moves by up to 1.6e-2 of the largest component (one ReLU flip in one of
    3000 samples) between fp32 and fp64 accumulation, and its cosine against the fp32 reference ranges
    0.9959..0.9998.  test_field_bw_inputs asserts the first of these preconditions (_dsh16_wide)."""
    g = torch.Generator().manual_seed(seed)
    feat = (torch.rand(N, 32, generator=g) - 0.5).half()
    u = torch.randn(N, 3, generator=g)
    dirs = u / u.norm(dim=1, keepdim=True) * (0.5 + 1.5 * torch.rand(N, 1, generator=g))
    dirs[0] = torch.tensor([0.0, 0.0, 2.0])
    px = FO.xavier_uniform_(torch.empty(3072), FO.mlp_shapes(32, 16, 64, 1), g)
    pr = FO.xavier_uniform_(torch.empty(FLD.rgb_net_params(width)), FO.mlp_shapes(32, 3, width, 2), g)
    dsig = torch.randn(N, generator=g) * 1e-6
    drgb = torch.randn(N, 3, generator=g) * 1e-5
    return feat, dirs, px, pr, dsig, drgb


def _dsh16(acts, drgb, S):
    """The fp16-point emulation's dL/dSH: ngp_field_bw16's chain up to dR1, then columns [:16] of
    dR1 @ R1 (the rows of the product whose rows 16..31 are dh), unscaled."""
    h = lambda t: t.half().float()  # noqa: E731
    a, rgb = acts, acts["rgb"]
    dO = torch.zeros(rgb.shape[0], 16)
    dO[:, :3] = drgb * S * rgb * (1 - rgb)
    dO = h(dO)
    dr2 = h((dO @ a["R3"]) * (a["r2"] > 0))
    dr1 = h((dr2 @ a["R2"]) * (a["r1"] > 0))
    return (dr1 @ a["R1"])[:, :16] / S


def _dsh16_wide(feat, dirs, px, pr, drgb, W, S):
    """_dsh16 with every product accumulated in fp64 (the same fp16 rounding points): where it and the
    fp32 emulation part, the emulation is deciding a rounding by its accumulation order."""
    dt = torch.float64
    h = lambda t: t.half().to(dt)  # noqa: E731
    W1 = h(px[:2048].view(64, 32)); W2 = h(px[2048:3072].view(16, 64))
    R1 = h(pr[:W * 32].view(W, 32)); R2 = h(pr[W * 32:W * 32 + W * W].view(W, W)); R3 = h(pr[W * 32 + W * W:].view(16, W))
    y1 = h(torch.relu(feat.to(dt) @ W1.t())); hh = h(y1 @ W2.t())
    dn = dirs / torch.norm(dirs, dim=1, keepdim=True)
    r1 = h(torch.relu(torch.cat([h(FO.sh4((dn + 1) / 2)), hh], 1) @ R1.t())); r2 = h(torch.relu(r1 @ R2.t()))
    rgb = torch.sigmoid((r2 @ R3.t())[:, :3])
    dO = torch.zeros(feat.shape[0], 16, dtype=dt)
    dO[:, :3] = drgb.to(dt) * S * rgb * (1 - rgb)
    dr2 = h((h(dO) @ R3) * (r2 > 0))
    dr1 = h((dr2 @ R2) * (r1 > 0))
    return (dr1 @ R1)[:, :16] / S


def _ddirs_fp32_autograd(feat, dirs, px, pr, dsig, drgb, W):
    d = dirs.clone().requires_grad_(True)
    a, b = px.half().float(), pr.half().float()
    W1 = a[:2048].view(64, 32); W2 = a[2048:3072].view(16, 64)
    R1 = b[:W * 32].view(W, 32); R2 = b[W * 32:W * 32 + W * W].view(W, W); R3 = b[W * 32 + W * W:].view(16, W)
    y1 = torch.relu(feat.float() @ W1.t()); h = y1 @ W2.t()
    dn = d / torch.norm(d, dim=1, keepdim=True)
    r1 = torch.relu(torch.cat([FO.sh4((dn + 1) / 2), h], 1) @ R1.t()); r2 = torch.relu(r1 @ R2.t())
    c = torch.sigmoid(r2 @ R3.t())[:, :3]
    ((torch.exp(h[:, 0]) * dsig).sum() + (c * drgb).sum()).backward()
    return d.grad


@pytest.mark.parametrize("N", [1, 31, 33, 3000])
@pytest.mark.parametrize("width", [64, 128])
def test_field_bw_inputs(gpu, width, N):
    """Everything mfnerf_field_bw writes comes out bit-identical (the deferred fold too); dL_ddirs
    against the fp16-point emulation (max error / max reference < 2e-3) and against fp32 autograd of
    the whole head (cosine > 0.9995): the limits test_field_bw applies to dL_dfeat, dL/dSH being rows
    of the same MFMA product."""
    feat, dirs, px, pr, dsig, drgb = _field_inputs(N, width=width)
    S = 16384.0
    _, _, acts = FO.ngp_field_fw16(feat, dirs, px, pr, width)
    ref16 = R.ddirs_from_dsh(dirs, _dsh16(acts, drgb, S))
    ref32 = _ddirs_fp32_autograd(feat, dirs, px, pr, dsig, drgb, width)
    wide = R.ddirs_from_dsh(dirs, _dsh16_wide(feat, dirs, px, pr, drgb, width, S))
    assert float((ref16 - wide).abs().max() / wide.abs().max()) < 2e-4, "the emulation is order-sensitive here"
    packed = FLD.pack_field_weights(px.to(gpu), pr.to(gpu), width)
    fg, dg, sg, cg = feat.to(gpu), dirs.to(gpu), dsig.to(gpu), drgb.to(gpu)

    def run(inputs, deferred):
        dfeat = torch.full((N, 32), float("nan"), device=gpu)
        gx, gr = torch.zeros(3072, device=gpu), torch.zeros(FLD.rgb_net_params(width), device=gpu)
        ws = FLD.field_bw_workspace(N, width, gpu)
        dd = torch.full((N, 3), float("nan"), device=gpu)
        flag = torch.zeros(8, dtype=torch.int32, device=gpu)
        a = (fg, dg, N, packed, sg, cg, S, dfeat, None if deferred else gx, None if deferred else gr, ws)
        if inputs:
            FLD.field_bw_inputs(*a, dd, width, nonfinite=flag)
        else:
            FLD.field_bw(*a, width, nonfinite=flag)
        if deferred:
            call("mfnerf_field_bw_reduce", width, ptr(ws), ptr(gx), ptr(gr), ptr(flag), stream())
        torch.cuda.synchronize()
        assert int(flag[0]) == 0
        return dfeat, gx, gr, dd

    base = run(False, False)
    for deferred in (False, True):
        got = run(True, deferred)
        assert torch.equal(got[0], base[0]), "dL_dfeat differs from mfnerf_field_bw's"
        assert torch.equal(got[1], base[1]) and torch.equal(got[2], base[2]), "weight gradients differ"
    dd = got[3].cpu().double()
    assert torch.isfinite(dd).all()
    err = float((dd - ref16).abs().max() / ref16.abs().max())
    cos = float(torch.nn.functional.cosine_similarity(dd.flatten(), ref32.double().flatten(), dim=0))
    print(f"W={width} N={N}: dL_ddirs err vs fp16 emulation {err:.3e}, cosine vs fp32 autograd {cos:.6f}")
    assert err < 2e-3, err
    assert cos > 0.9995, cos
    # a direction gradient is tangent to the unit sphere: d . dL/dd = 0 (to fp32 rounding)
    assert float(((dd * dirs.double()).sum(1).abs() / (dd.norm(dim=1) * dirs.double().norm(dim=1) + 1e-30)).max()) < 1e-3


def test_field_bw_inputs_flags_nonfinite_direction_gradient(gpu):
    """A zero-length direction has no normalised direction: dL_ddirs is NaN there and raises the flag
    mfnerf_field_bw's outputs raise."""
    N = 33
    feat, dirs, px, pr, dsig, drgb = _field_inputs(N, seed=9)
    dirs[7] = 0.0
    packed = FLD.pack_field_weights(px.to(gpu), pr.to(gpu), 64)
    flag = torch.zeros(8, dtype=torch.int32, device=gpu)
    dd = torch.zeros(N, 3, device=gpu)
    FLD.field_bw_inputs(feat.to(gpu), dirs.to(gpu), N, packed, dsig.to(gpu), drgb.to(gpu), 16384.0,
                        torch.empty(N, 32, device=gpu), torch.zeros(3072, device=gpu),
                        torch.zeros(FLD.rgb_net_params(64), device=gpu), FLD.field_bw_workspace(N, 64, gpu), dd, 64,
                        nonfinite=flag)
    torch.cuda.synchronize()
    assert int(flag[0]) == 1 and not bool(torch.isfinite(dd[7]).all())


# ------------------------------------------------------------------------------------------- (c)
C_BOUND = 2.0 ** -13  # a 1024-term fp32 sum on top of (a)'s 2^-15 per sample


def _check_rays(got_o, got_d, ref, what):
    o, d, Ao, Ad = ref
    for got, want, A, nm in ((got_o, o, Ao, "rays_o"), (got_d, d, Ad, "rays_d")):
        err = (got.double().cpu() - want).abs()
        ratio = float((err / A.clamp_min(1e-300)).max())
        print(f"{what} dL_d{nm}: max |got - ref| / sum|terms| = {ratio:.3e} (bound 2^-13 = {C_BOUND:.3e})")
        assert (err <= C_BOUND * A).all(), (what, nm, ratio)


@pytest.mark.parametrize("kind,n_tables", R.KINDS)
def test_rays_input_grad_matches_segmented_fp64_sums(gpu, kind, n_tables):
    olay, lay, desc, table = _setup(kind, n_tables)
    g = torch.Generator().manual_seed(11)
    counts = [0, 1, 63, 64, 65, 1024]
    order = torch.randperm(len(counts), generator=g).tolist()      # segments in shuffled ray order
    ray_ids = torch.randperm(len(counts), generator=g).tolist()    # and written at shuffled rows
    rays_a, start = [], 0
    for k in order:
        rays_a.append([ray_ids[k], start, counts[k]])
        start += counts[k]
    rays_a = torch.tensor(rays_a, dtype=torch.int64)
    n = start
    xw = _points(n, olay, seed=12) - 0.5
    ts = torch.rand(n, generator=g) * 1.5 + 0.05
    dfeat = torch.randn(n, 32, generator=g)
    ddirs = torch.randn(n, 3, generator=g)
    dxyz, A = R.dx_ref(R.normalise(xw, -0.5, 1.0), table, dfeat, olay, x_range=1.0)
    ref = R.segmented_ref(dxyz, A, ts, ddirs, rays_a)
    args = (xw.to(gpu), ts.to(gpu), dfeat.to(gpu), ddirs.to(gpu), rays_a.to(gpu), table.to(gpu), desc, -0.5, 1.0)
    o1 = torch.full((len(counts), 3), 5.0, device=gpu)
    d1 = torch.full((len(counts), 3), 5.0, device=gpu)
    FLD.rays_input_grad(*args, out_o=o1, out_d=d1)
    o2, d2 = FLD.rays_input_grad(*args)
    _check_rays(o1, d1, ref, kind)
    empty = ray_ids[0]  # the ray of counts[0] == 0 samples
    assert bool((o1[empty] == 0).all()) and bool((d1[empty] == 0).all())
    assert torch.equal(o1, o2) and torch.equal(d1, d2)
    # the same sums as (a) followed by RayMarcher.backward (float atomics), to the same bound
    dx = FLD.grid_encode_bw_input(args[0], n, args[5], args[2], desc, -0.5, 1.0)
    ctx = types.SimpleNamespace(saved_tensors=(args[4], args[1]))
    bo, bd = RayMarcher.backward(ctx, None, dx, args[3], None, None, None)[:2]
    _check_rays(bo, bd, ref, kind + " (a)+RayMarcher.backward")


# ------------------------------------------------------------------------------------ autograd
def _tiny_ngp(gpu, seed=0):
    from mfnerf.networks import NGP
    from mfnerf.trainer import HParams
    torch.manual_seed(seed)
    model = NGP(0.5, HParams(T=14)).to(gpu)
    with torch.no_grad():  # a table large enough for the field (and its gradient) to vary in space
        p = model.xyz_encoder.params
        p[FLD.XYZ_NET_PARAMS:].uniform_(-0.5, 0.5)
    model.update_density_grid(0.01 * 1024 / 3 ** 0.5, warmup=True)  # the warm-up occupancy (train.py:165-168)
    return model


def test_render_backpropagates_to_rays(gpu):
    """render() with rays that require a gradient: rays_o.grad / rays_d.grad exist, are finite and
    equal mfnerf_rays_input_grad on the same marched samples (the eager path against the fused one),
    within (c)'s bound; without them the parameter gradients are unchanged."""
    from mfnerf.rendering import render
    model = _tiny_ngp(gpu)
    o, d = synthetic.random_rays(64, synthetic.camera_poses(seed=2), seed=3)
    target = torch.rand(64, 3, generator=torch.Generator().manual_seed(4)).to(gpu)
    seen = {}

    def hook(mod, args, out):
        seen["x"], seen["d"] = args[0].detach(), args[1].detach()
        if out[0].requires_grad:
            out[0].register_hook(lambda g: seen.__setitem__("dsig", g.detach().float()))
            out[1].register_hook(lambda g: seen.__setitem__("drgb", g.detach().float()))

    handle = model.register_forward_hook(hook)

    def run(rays_grad, gen_seed=9):
        model.zero_grad(set_to_none=True)
        ro, rd = o.to(gpu).requires_grad_(rays_grad), d.to(gpu).requires_grad_(rays_grad)
        torch.manual_seed(gen_seed)  # the march's perturbation
        res = render(model, ro, rd)
        loss = ((res["rgb"] - target) ** 2).mean() + 1e-3 * (-res["opacity"] * torch.log(res["opacity"] + 1e-10)).mean()
        loss.backward()
        return ro, rd, res, model.xyz_encoder.params.grad.clone(), model.rgb_net.params.grad.clone()

    ro, rd, res, gx_on, gr_on = run(True)
    assert ro.grad is not None and rd.grad is not None
    assert torch.isfinite(ro.grad).all() and torch.isfinite(rd.grad).all()
    assert float(ro.grad.abs().max()) > 0 and float(rd.grad.abs().max()) > 0
    # (c) on the same marched samples, from the same per-sample gradients the eager backward formed
    xs, ds, dsig, drgb = seen["x"].float(), seen["d"].float(), seen["dsig"], seen["drgb"]
    n = xs.shape[0]
    assert n > 1000
    packed, table16 = FLD.field_weights(model.xyz_encoder.params, model.rgb_net.params, model.rgb_width)
    feat = FLD.grid_encode_fw(xs, n, table16, model.layout, model.desc, model._x_min, model._x_range)
    sigma, _ = FLD.field_fw(feat, ds, n, packed, model.rgb_width)
    S = FLD.pow2_grad_scale(float(torch.maximum(drgb.abs().max(), (dsig * sigma.clamp(max=3.3e6)).abs().max())))
    dfeat, ddirs = torch.empty(n, 32, device=gpu), torch.empty(n, 3, device=gpu)
    FLD.field_bw_inputs(feat, ds, n, packed, dsig.contiguous(), drgb.contiguous(), S, dfeat,
                        torch.zeros(3072, device=gpu), torch.zeros(FLD.rgb_net_params(model.rgb_width), device=gpu),
                        FLD.field_bw_workspace(n, model.rgb_width, gpu), ddirs, model.rgb_width)
    rays_a, ts = res["rays_a"], res["ts"].detach().float().contiguous()
    fo, fd = FLD.rays_input_grad(xs, ts, dfeat, ddirs, rays_a, table16, model.desc, model._x_min, model._x_range)
    olay = FO.GridLayout(16, 2, 14, 16, model.layout.b, "Hash", 1)
    _, A = R.dx_ref(R.normalise(xs.cpu(), model._x_min, model._x_range), table16.cpu(), dfeat.cpu(), olay,
                    x_range=model._x_range)
    _, _, Ao, Ad = R.segmented_ref(torch.zeros(n, 3, dtype=torch.float64), A, ts.cpu(), ddirs.cpu(), rays_a.cpu())
    for got, want, bound, nm in ((ro.grad, fo, Ao, "rays_o"), (rd.grad, fd, Ad, "rays_d")):
        err = (got.double() - want.double()).abs().cpu()
        print(f"eager vs fused dL_d{nm}: max err / sum|terms| = {float((err / bound.clamp_min(1e-300)).max()):.3e}")
        assert (err <= C_BOUND * bound).all(), nm
    # no input requires a gradient: the same parameter gradients
    ro2, rd2, _, gx_off, gr_off = run(False)
    assert ro2.grad is None and rd2.grad is None
    assert torch.equal(gr_on, gr_off)
    assert torch.equal(gx_on[:FLD.XYZ_NET_PARAMS], gx_off[:FLD.XYZ_NET_PARAMS])
    gx_off2 = run(False)[3]
    handle.remove()
    tab_on, tab_off, tab_off2 = (g[FLD.XYZ_NET_PARAMS:] for g in (gx_on, gx_off, gx_off2))
    if torch.equal(tab_off, tab_off2):
        assert torch.equal(tab_on, tab_off)
    else:
        # the eager table gradient is a float-atomic scatter (mfnerf_grid_encode_bw without fixed point):
        # two identical runs already differ in summation order, so the comparison holds to that spread
        spread = float((tab_off - tab_off2).abs().max())
        assert float((tab_on - tab_off).abs().max()) <= 4 * spread


def test_optimize_ext_lines_reach_dR_and_dT(gpu):
    """train.py:91-94 over mfnerf.render: poses refined by PoseRefiner, rays from get_rays, the loss
    backpropagated -- dR.grad and dT.grad are there, finite and non-zero on the images drawn, and the
    pose optimizer moves them."""
    from mfnerf import data
    from mfnerf.pose import PoseRefiner
    from mfnerf.rendering import render
    model = _tiny_ngp(gpu)
    W = 16
    focal = 0.5 * W / math.tan(0.5 * 0.6911112)
    K = torch.tensor([[focal, 0, W / 2], [0, focal, W / 2], [0, 0, 1]])
    directions = data.get_ray_directions(W, W, K).to(gpu)
    poses = synthetic.camera_poses(n_cams=5, seed=1)[:, :3].float().to(gpu)
    refiner = PoseRefiner(len(poses)).to(gpu)
    g = torch.Generator().manual_seed(2)
    img_idxs = torch.randint(0, 4, (64,), generator=g).to(gpu)   # image 4 is never drawn
    pix_idxs = torch.randint(0, W * W, (64,), generator=g).to(gpu)
    rays_o, rays_d = data.get_rays(directions[pix_idxs], refiner(poses[img_idxs], img_idxs))
    res = render(model, rays_o, rays_d)
    ((res["rgb"] - 0.5) ** 2).mean().backward()
    for p in (refiner.dR, refiner.dT):
        assert p.grad is not None and torch.isfinite(p.grad).all()
        assert float(p.grad[:4].abs().sum(1).min()) > 0 and float(p.grad[4].abs().max()) == 0
    before = refiner.refined_poses(poses)
    refiner.optimizer().step()
    assert float((refiner.refined_poses(poses) - before).abs().max()) > 0


def test_pose_gradient_points_along_a_translation_offset(gpu):
    """One cheap end-to-end sanity check: a tiny field trained on 32x32 views of the ball scene (the
    fused trainer, a few hundred steps), one pose's translation moved by a known offset -- the loss
    gradient with respect to that image's dT has a positive component along the offset (descending
    it moves the camera back).  A sanity check of the sign, not the proof of the gradients."""
    from mfnerf import data
    from mfnerf.networks import NGP
    from mfnerf.pose import PoseRefiner
    from mfnerf.rendering import render
    from mfnerf.trainer import HParams, Trainer
    W = 32
    focal = 0.5 * W / math.tan(0.5 * 0.6911112)
    imgs, poses, dirs, K = data.ball_scene_views(data.BallScene(n_balls=6, seed=1), 40, W, focal, seed=0)
    ds = data.DeviceDataset(imgs, poses, dirs, K=K, img_wh=(W, W), device=gpu, seed=5)
    hp = HParams(batch_size=1024, T=14, num_epochs=1, steps_per_epoch=400)
    tr = Trainer(hp, ds, device=gpu)
    tr.fit(log_every=400)
    st = tr.step
    model = NGP(0.5, hp).to(gpu)
    with torch.no_grad():
        model.xyz_encoder.params.copy_(torch.cat([st.params[:st.off_rgb], st.params[st.off_table:st.n_params]]))
        model.rgb_net.params.copy_(st.params[st.off_rgb:st.off_table])
        model.density_bitfield.copy_(st.bitfield)
    img = 7
    refiner = PoseRefiner(len(poses)).to(gpu)
    target = imgs[img].to(gpu)
    idx = torch.full((W * W,), img, device=gpu)
    pg = poses.float().to(gpu)
    for k, offset in enumerate(([0.03, -0.02, 0.025], [-0.025, 0.03, 0.02])):
        off = torch.tensor(offset, device=gpu)
        refiner.zero_grad(set_to_none=True)
        with torch.no_grad():
            refiner.dT.zero_()
            refiner.dT[img] = off
        rays_o, rays_d = data.get_rays(dirs.to(gpu), refiner(pg[idx], idx))
        torch.manual_seed(k)
        loss = ((render(model, rays_o, rays_d)["rgb"] - target) ** 2).mean()
        loss.backward()
        dot = float((refiner.dT.grad[img] * off).sum())
        print(f"offset {offset}: loss {float(loss.detach()):.5f}, dT.grad . offset = {dot:.3e}")
        assert dot > 0


@pytest.mark.parametrize("kind,n_tables", R.KINDS)
def test_tcnn_encoding_input_gradient(gpu, kind, n_tables):
    """tcnn.Encoding(x) with x.requires_grad: x.grad is mfnerf_grid_encode_bw_input's, the table
    gradient is still there, and nothing changes for an input without a gradient."""
    enc = tcnn.Encoding(3, {"otype": f"{kind}Grid", "type": kind, "n_levels": 16, "n_features_per_level": 2,
                            "log2_hashmap_size": 14, "base_resolution": 16, "n_tables": n_tables,
                            "per_level_scale": R.B_HALF}).to(gpu)
    with torch.no_grad():
        enc.params.uniform_(-1, 1)
    g = torch.Generator().manual_seed(3)
    x = torch.rand(777, 3, generator=g).to(gpu).requires_grad_(True)
    dy = torch.randn(777, 32, generator=g).to(gpu)
    out = enc(x)
    out.backward(dy.half())
    want = FLD.grid_encode_bw_input(x.detach(), 777, enc.params.detach().half(), dy.half().float(), enc.desc)
    assert x.grad is not None and torch.equal(x.grad, want)
    assert enc.params.grad is not None and float(enc.params.grad.abs().max()) > 0
    out2 = enc(x.detach())
    assert torch.equal(out2, out.detach())
    # through the whole tcnn route: encoding -> FullyFusedMLP
    net = tcnn.NetworkWithInputEncoding(3, 16, enc.encoding_config, {
        "otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64,
        "n_hidden_layers": 1}).to(gpu)
    with torch.no_grad():
        net.params[net.n_net:].uniform_(-1, 1)
    x2 = x.detach().clone().requires_grad_(True)
    net(x2).float().sum().backward()
    assert x2.grad is not None and torch.isfinite(x2.grad).all() and float(x2.grad.abs().max()) > 0


# -------------------------------------------------------------------------------------- engine
def _engine(gpu, ray_grads):
    st = engine.TrainStep(engine.StepConfig(n_rays=256, log2_T=14, ray_grads=ray_grads), device=gpu, seed=0)
    st.set_occupancy(synthetic.ball_density_grid())
    return st


def test_engine_ray_grads(gpu):
    """Three steps with ray_grads on and off from the same seed and batches: the same parameters, bit
    for bit.  The on-run's dL_drays_* equal the autograd path's tail -- mfnerf_grid_encode_bw_input
    on the step's dL_dfeat, then RayMarcher.backward with the step's dL_ddirs -- within (c)'s bound
    (the loss scale is already divided out of dL_dfeat and dL_ddirs).  A captured-and-replayed step
    gives the eager step's bits."""
    a, b, c = _engine(gpu, True), _engine(gpu, False), _engine(gpu, True)
    batches = a.make_batches(3, seed=5)
    for k in range(3):
        if k == 2:  # the table the last step's backward reads (its Adam update comes after)
            table16 = a.p16[a.off_table:a.off_table + a.layout.n_params].clone()
        a.run(batches[k])
        b.run(batches[k])
    torch.cuda.synchronize()
    assert torch.equal(a.params, b.params) and torch.equal(a.m, b.m) and torch.equal(a.p16, b.p16)
    assert not hasattr(b.parts[0], "dL_drays_o")
    t, m = a.parts[0], a.state.march.part[0]
    n = int(m.counter[0])
    assert n > 1000
    go, gd = t.dL_drays_o.clone(), t.dL_drays_d.clone()
    assert torch.isfinite(go).all() and torch.isfinite(gd).all() and float(gd.abs().max()) > 0
    xs, ts = m.xyzs[:n].contiguous(), m.ts[:n].contiguous()
    dfeat, ddirs = t.dfeat[:n].contiguous(), t.ddirs[:n].contiguous()
    dx = FLD.grid_encode_bw_input(xs, n, table16, dfeat, a.desc, a.x_min, a.x_range)
    ctx = types.SimpleNamespace(saved_tensors=(m.rays_a, ts))
    eo, ed = RayMarcher.backward(ctx, None, dx, ddirs, None, None, None)[:2]
    olay = FO.GridLayout(16, 2, 14, 16, a.layout.b, "Hash", 1)
    _, A = R.dx_ref(R.normalise(xs.cpu(), a.x_min, a.x_range), table16.cpu(), dfeat.cpu(), olay, x_range=a.x_range)
    _, _, Ao, Ad = R.segmented_ref(torch.zeros(n, 3, dtype=torch.float64), A, ts.cpu(), ddirs.cpu(), m.rays_a.cpu())
    for got, want, bound, nm in ((go, eo, Ao, "rays_o"), (gd, ed, Ad, "rays_d")):
        err = (got.double() - want.double()).abs().cpu()
        print(f"engine vs autograd tail dL_d{nm}: max err / sum|terms| = "
              f"{float((err / bound.clamp_min(1e-300)).max()):.3e}")
        assert (err <= C_BOUND * bound).all(), nm
    # captured and replayed: c runs step 0 eagerly, captures, replays steps 1 and 2
    c.run(batches[0])
    torch.cuda.synchronize()
    c.capture()
    for k in (1, 2):
        c.replay(batches[k], next_batch=batches[k + 1] if k + 1 < 3 else None)
    torch.cuda.synchronize()
    assert torch.equal(c.params, a.params)
    assert torch.equal(c.parts[0].dL_drays_o, go) and torch.equal(c.parts[0].dL_drays_d, gd)
