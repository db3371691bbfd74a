"""mfnerf.rendering.render_fused (mfnerf_render_test_fused: march + encode + field + composite in one
persistent launch) against the test-time loop render(test_time=True), the golden vectors, itself
under other batch compositions, and inside a captured graph."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
UNCAPPED = 1 << 20


class HP:
    pass


def table_values(n, seed=1):
    """The Lego fixture's table (make_golden.table_values): U(-0.5, 0.5) from a seeded CPU generator."""
    g = torch.Generator().manual_seed(seed)
    return torch.empty(n).uniform_(-0.5, 0.5, generator=g)


def _setup(gpu, name):
    """test_gpu_golden.py's `setup`: the fixture's arrays and the NGP model holding its weights."""
    from mfnerf.networks import NGP
    z = np.load(os.path.join(GOLD, f"golden_render{name}.npz"))
    z = {k: torch.from_numpy(z[k]) for k in z.files}
    meta = json.load(open(os.path.join(GOLD, f"golden_render{name}.json")))
    hp = HP()
    for k, v in meta["hparams"].items():
        setattr(hp, k, v)
    model = NGP(scale=meta["scale"], hparams=hp).to(gpu)
    with torch.no_grad():
        if name == "_lego":  # the real-size table is regenerated, not stored
            n_net = z["xyz_params"].numel()
            model.xyz_encoder.params[:n_net].copy_(z["xyz_params"])
            model.xyz_encoder.params[n_net:].copy_(table_values(model.xyz_encoder.params.numel() - n_net))
        else:
            model.xyz_encoder.params.copy_(z["xyz_params"])
        model.rgb_net.params.copy_(z["rgb_params"])
        model.density_bitfield.copy_(z["bitfield"])
    return z, model


_cache = {}


def _fixture(gpu, name):
    if name not in _cache:
        z, model = _setup(gpu, name)
        _cache[name] = (z, model, z["rays_o"].to(gpu), z["rays_d"].to(gpu))
    return _cache[name]


@pytest.fixture(scope="module", params=["", "_mf128"], ids=["hash-rgb64", "mixedfeature-rgb128"])
def setup(gpu, request):
    return _fixture(gpu, request.param)


@pytest.fixture(scope="module", params=["", "_mf128", "_lego"],
                ids=["hash-rgb64", "mixedfeature-rgb128", "lego-T19-1024rays"])
def setup3(gpu, request):
    return _fixture(gpu, request.param)


def _loop(model, o, d, **kw):
    from mfnerf import rendering
    with torch.no_grad():
        return rendering.render(model, o, d, test_time=True, **kw)


def _same(a, b, keys=("opacity", "depth", "rgb", "samples")):
    return all(torch.equal(a[k], b[k]) for k in keys)


def test_one_sample_per_ray_is_bit_exact(setup):
    """ray_budget = 1 against one round of the loop (one sample per ray, T = 1): the encode, the field
    and the composite arithmetic are the existing kernels', with no tolerance."""
    from mfnerf import rendering
    z, model, o, d = setup
    ref = _loop(model, o, d, max_samples=1)
    got = rendering.render_fused(model, o, d, max_samples=1)
    assert int(got["samples"].max()) == 1 and int(got["opacity"].gt(0).sum()) > 0
    for k in ("opacity", "depth", "rgb"):
        assert torch.equal(got[k], ref[k]), k


def test_whole_rays_vs_loop(setup):
    """Neither cap binds (max_samples = 2^20).  The loop re-derives T = 1 - O at each chunk start, so
    its termination test may flip by one sample: at most the remaining transmittance T_threshold
    (1e-4) per ray, plus fp32 drift over <= 1024 samples (1024 * 2^-24 = 6.1e-5): atol 2e-4 on
    opacity and rgb, 2e-4 * max t2 on depth."""
    from mfnerf import rendering
    from mfnerf.custom_functions import RayAABBIntersector
    z, model, o, d = setup
    ref = _loop(model, o, d, max_samples=UNCAPPED)
    got = rendering.render_fused(model, o, d, max_samples=UNCAPPED)
    _, hits_t, _ = RayAABBIntersector.apply(o, d, model.center, model.half_size, 1)
    t_max = float(hits_t[:, 0, 1].max())
    err = {k: float((got[k] - ref[k]).abs().max()) for k in ("opacity", "depth", "rgb")}
    print("whole rays: max abs error", err, "t_max", t_max, "samples fused/loop", int(got["total_samples"]),
          int(ref["total_samples"]))
    assert err["opacity"] <= 2e-4 and err["rgb"] <= 2e-4
    assert err["depth"] <= 2e-4 * t_max
    assert int(got["samples"].sum()) == int(got["total_samples"]) <= int(ref["total_samples"])
    assert int(got["total_samples"]) > o.shape[0]  # (more than one sample per ray: whole rays were marched)


def test_batch_independence(gpu):
    """4099 ball-scene rays (occupied and empty regions; not a multiple of the wave's 32 rows or the
    workgroup's 128): every ray's five outputs are the same bits in the whole batch, in a random
    permutation of it and in its first 1, 31, 33 and 257 rays -- counts below a wave, partial tiles,
    and refill across the queue."""
    from mfnerf import rendering, synthetic
    z, model, _, _ = _fixture(gpu, "")
    o, d = synthetic.random_rays(4099, synthetic.camera_poses(), seed=3, device=gpu)
    full = rendering.render_fused(model, o, d)
    assert int(full["samples"].gt(1).sum()) > 1000 and int(full["samples"].eq(0).sum()) > 100
    assert int(full["samples"].sum()) == int(full["total_samples"])
    perm = torch.randperm(4099, generator=torch.Generator().manual_seed(5)).to(gpu)
    shuffled = rendering.render_fused(model, o[perm].contiguous(), d[perm].contiguous())
    for k in ("opacity", "depth", "rgb", "samples"):
        assert torch.equal(shuffled[k], full[k][perm]), k
    for n in (1, 31, 33, 257):
        part = rendering.render_fused(model, o[:n].contiguous(), d[:n].contiguous())
        for k in ("opacity", "depth", "rgb", "samples"):
            assert torch.equal(part[k], full[k][:n]), (n, k)
        assert int(part["total_samples"]) == int(full["samples"][:n].sum())


def test_edges(gpu):
    from mfnerf import rendering
    z, model, o, d = _fixture(gpu, "")
    n = o.shape[0]
    bg = torch.ones(n, 3, device=gpu)

    def blank(res, rows):
        return (not res["opacity"][rows].any() and not res["depth"][rows].any() and not res["samples"][rows].any()
                and torch.equal(res["rgb"][rows], bg[rows]))

    # rays that miss the box (cameras outside it, looking away), among rays that hit it
    away = d.clone()
    away[::3] = -away[::3]
    res = rendering.render_fused(model, o, away)
    assert blank(res, slice(0, None, 3))
    assert int(res["samples"].sum()) == int(res["total_samples"]) > 0
    saved = model.density_bitfield.clone()
    try:
        model.density_bitfield.zero_()
        res = rendering.render_fused(model, o, d)
        assert blank(res, slice(None)) and int(res["total_samples"]) == 0
        model.density_bitfield.fill_(255)
        res = rendering.render_fused(model, o, d)
        assert int(res["samples"].max()) <= 1024 and int(res["samples"].max()) > 1
        assert int(res["samples"].sum()) == int(res["total_samples"])
    finally:
        model.density_bitfield.copy_(saved)
    res = rendering.render_fused(model, o[:0], d[:0])
    assert res["opacity"].shape == (0,) and res["depth"].shape == (0,) and res["rgb"].shape == (0, 3)
    assert res["samples"].shape == (0,) and int(res["total_samples"]) == 0


def test_graph_capture(setup):
    """Captured once with static inputs, replayed twice with other rays copied in: every replay equals
    the eager call, so the launch resets its own queue counter and sample total."""
    from mfnerf import rendering
    z, model, o, d = setup
    flipped = (o.flip(0).contiguous(), d.flip(0).contiguous())
    eager = [rendering.render_fused(model, a, b) for a, b in ((o, d), flipped)]
    so, sd = o.clone(), d.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = rendering.render_fused(model, so, sd)
    for (a, b), ref in list(zip((flipped, (o, d)), eager[::-1])):
        so.copy_(a)
        sd.copy_(b)
        g.replay()
        torch.cuda.synchronize()
        assert _same(out, ref)
        assert int(out["total_samples"]) == int(ref["total_samples"]) == int(ref["samples"].sum())


def test_fused_vs_golden(gpu, setup3):
    """test_render_test_time_vs_golden's assertions for the fused path, the sample count one-sided
    (the fused path evaluates no sample past a ray's termination).  The default-cap loop and the
    2^20 loop agree on all three fixtures (the loop's cross-ray cap binds on none), so all three are
    compared against the golden values."""
    from mfnerf import rendering
    z, model, o, d = setup3
    capped, free = _loop(model, o, d), _loop(model, o, d, max_samples=UNCAPPED)
    assert all(torch.equal(capped[k], free[k]) for k in ("opacity", "depth", "rgb"))
    rt = rendering.render_fused(model, o, d)
    assert torch.allclose(rt["opacity"].cpu(), z["test_opacity"], atol=1e-2)
    assert torch.allclose(rt["rgb"].cpu(), z["test_rgb"], atol=1e-2)
    golden = int(z["test_total_samples"])
    assert int(rt["total_samples"]) <= golden + max(4, golden // 200)


def test_trainer_evaluate_fused_opt_in(gpu):
    """Trainer.evaluate(fused=True) is render_fused on each view's rays (the default stays the loop,
    whose per-pixel values it matches to the whole-ray bound, 2e-4)."""
    import math
    from mfnerf import data, rendering
    from mfnerf.trainer import HParams, Trainer, psnr
    W = 32
    focal = 0.5 * W / math.tan(0.5 * 0.6911112)
    scene = data.BallScene(n_balls=6, seed=1)
    imgs, poses, dirs, K = data.ball_scene_views(scene, 8, W, focal, seed=0)
    ds = data.DeviceDataset(imgs, poses, dirs, K=K, img_wh=(W, W), device=gpu, seed=5)
    tr = Trainer(HParams(batch_size=1024, T=16, num_epochs=1, steps_per_epoch=40), ds, device=gpu)
    tr.fit(log_every=0)
    mean_f, per_view = tr.evaluate(imgs[:2], poses[:2], dirs, fused=True)
    model = tr.to_ngp()
    for i in range(2):
        o, d = data.get_rays(dirs.to(gpu), poses[i].to(gpu))
        res = rendering.render_fused(model, o, d)
        assert per_view[i] == psnr(res["rgb"].float(), imgs[i].to(gpu))
        ref = rendering.render(model, o, d, test_time=True, max_samples=UNCAPPED)
        full = rendering.render_fused(model, o, d, max_samples=UNCAPPED)
        assert float((full["rgb"] - ref["rgb"]).abs().max()) <= 2e-4
    assert mean_f == sum(per_view) / 2


def _abi_call(model, o, d, **over):
    """mfnerf_render_test_fused called directly, `over` replacing arguments by name."""
    from mfnerf import field
    from mfnerf._lib import call, ptr, stream
    n, dev = o.shape[0], o.device
    packed, table16 = field.field_weights(model.xyz_encoder.params, model.rgb_net.params, model.rgb_width)
    out = [torch.empty(n, device=dev), torch.empty(n, device=dev), torch.empty(n, 3, device=dev)]
    a = dict(n_rays=n, ray_budget=1024, rgb_width=model.rgb_width, desc=model.desc)
    a.update(over)
    call("mfnerf_render_test_fused", ptr(o), ptr(d), a["n_rays"], ptr(model.center), ptr(model.half_size),
         ptr(model.density_bitfield), model.cascades, model.scale, 0.0, model.grid_size, 1024, a["ray_budget"], 1e-4,
         model._x_min, model._x_range, a["desc"], ptr(table16), ptr(packed), a["rgb_width"],
         ptr(torch.empty(1, dtype=torch.int32, device=dev)), ptr(out[0]), ptr(out[1]), ptr(out[2]), None,
         ptr(torch.empty(1, dtype=torch.int64, device=dev)), stream())


def test_errors(gpu):
    from mfnerf import rendering
    from mfnerf._lib import GridDesc
    z, model, o, d = _fixture(gpu, "")
    with pytest.raises(RuntimeError, match="rgb_width=96 is not supported"):
        _abi_call(model, o, d, rgb_width=96)
    with pytest.raises(RuntimeError, match="ray_budget=0 must be at least 1"):
        rendering.render_fused(model, o, d, max_samples=0)
    with pytest.raises(RuntimeError, match="bad n_rays=-1"):
        _abi_call(model, o, d, n_rays=-1)
    short = GridDesc.from_buffer_copy(bytes(model.desc))
    short.n_levels = 12
    with pytest.raises(RuntimeError, match=r"n_levels \* F = 32"):
        _abi_call(model, o, d, desc=ctypes.byref(short))
    _abi_call(model, o, d)  # the unmodified arguments are accepted
    torch.cuda.synchronize()
