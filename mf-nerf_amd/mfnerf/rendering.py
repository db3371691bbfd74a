"""models/rendering.py restated over the gfx950 ops: render() and its train/test paths.

Same entry point, constants, kwargs and result keys as the reference (rendering.py:1-163):
near clamp of the AABB hit (:29), the progressive test-time march (:46-118, including
N_samples = max(min(N//N_alive, 64), min_samples)) and the background blend (:112-116,
:153-161).
"""
import torch
from einops import rearrange

from . import vren
from .custom_functions import RayAABBIntersector, RayMarcher, VolumeRenderer

MAX_SAMPLES = 1024
NEAR_DISTANCE = 0.01
# what render_fused and everything built on it (viewer.FrameRenderer) say to an HDR model
HDR_GAP = ("render_fused: the single-launch renderer's field head applies the sigmoid; an "
           "HDR/exposure model (rgb_act='None') renders with render(test_time=True)")


def render(model, rays_o, rays_d, **kwargs):
    """rendering.py:11-43 (the reference runs it under torch.cuda.amp.autocast())."""
    with torch.autocast("cuda", enabled=rays_o.is_cuda):
        return _render(model, rays_o, rays_d, **kwargs)


def _render(model, rays_o, rays_d, **kwargs):
    rays_o = rays_o.contiguous()
    rays_d = rays_d.contiguous()
    _, hits_t, _ = RayAABBIntersector.apply(rays_o, rays_d, model.center, model.half_size, 1)
    hits_t[(hits_t[:, 0, 0] >= 0) & (hits_t[:, 0, 0] < NEAR_DISTANCE), 0, 0] = NEAR_DISTANCE

    render_func = _render_rays_test if kwargs.get("test_time", False) else _render_rays_train
    results = render_func(model, rays_o, rays_d, hits_t, **kwargs)
    for k, v in results.items():
        if kwargs.get("to_cpu", False):
            v = v.cpu()
            if kwargs.get("to_numpy", False):
                v = v.numpy()
        results[k] = v
    return results


@torch.no_grad()
def _render_rays_test(model, rays_o, rays_d, hits_t, **kwargs):
    """rendering.py:46-118: march alive rays N_samples at a time until they converge."""
    exp_step_factor = kwargs.get("exp_step_factor", 0.0)
    results = {}
    N_rays = len(rays_o)
    device = rays_o.device
    opacity = torch.zeros(N_rays, device=device)
    depth = torch.zeros(N_rays, device=device)
    rgb = torch.zeros(N_rays, 3, device=device)

    samples = total_samples = 0
    alive_indices = torch.arange(N_rays, device=device)
    min_samples = 1 if exp_step_factor == 0 else 4

    while samples < kwargs.get("max_samples", MAX_SAMPLES):
        N_alive = len(alive_indices)
        if N_alive == 0:
            break
        N_samples = max(min(N_rays // N_alive, 64), min_samples)
        samples += N_samples

        xyzs, dirs, deltas, ts, N_eff_samples = vren.raymarching_test(
            rays_o, rays_d, hits_t[:, 0], alive_indices, model.density_bitfield, model.cascades, model.scale,
            exp_step_factor, model.grid_size, MAX_SAMPLES, N_samples)
        total_samples += N_eff_samples.sum()
        xyzs = rearrange(xyzs, "n1 n2 c -> (n1 n2) c")
        dirs = rearrange(dirs, "n1 n2 c -> (n1 n2) c")
        valid_mask = ~torch.all(dirs == 0, dim=1)
        # the valid samples' indices once (one host sync), instead of a mask sum plus a nonzero per
        # boolean index below; same values as the reference's masked assignments
        valid = valid_mask.nonzero()[:, 0]
        if len(valid) == 0:
            break

        sigmas = torch.zeros(len(xyzs), device=device)
        rgbs = torch.zeros(len(xyzs), 3, device=device)
        _sigmas, _rgbs = model(xyzs.index_select(0, valid), dirs.index_select(0, valid), **kwargs)
        sigmas.index_copy_(0, valid, _sigmas.float())
        rgbs.index_copy_(0, valid, _rgbs.float())
        sigmas = rearrange(sigmas, "(n1 n2) -> n1 n2", n2=N_samples)
        rgbs = rearrange(rgbs, "(n1 n2) c -> n1 n2 c", n2=N_samples)

        vren.composite_test_fw(sigmas.contiguous(), rgbs.contiguous(), deltas, ts, hits_t[:, 0], alive_indices,
                               kwargs.get("T_threshold", 1e-4), N_eff_samples, opacity, depth, rgb)
        alive_indices = alive_indices[alive_indices >= 0]

    results["opacity"] = opacity
    results["depth"] = depth
    results["rgb"] = rgb
    results["total_samples"] = total_samples

    rgb_bg = torch.ones(3, device=device) if exp_step_factor == 0 else torch.zeros(3, device=device)
    results["rgb"] += rgb_bg * rearrange(1 - opacity, "n -> n 1")
    return results


@torch.no_grad()
def render_fused(model, rays_o, rays_d, **kwargs):
    """The test-time render (render(test_time=True): rendering.py:27-29 + :46-118) in one persistent
    kernel launch, mfnerf_render_test_fused: ray/box test, march, grid encode, field head and
    compositing per ray, no intermediate in memory, no host sync -- legal inside a captured graph
    (every output is allocated here, before the launch).

    Same kwargs as the test path (exp_step_factor, T_threshold, max_samples, to_cpu, to_numpy) and
    the same result keys, plus `samples` (int32 per ray).  Two differences from the loop:
    max_samples is a PER-RAY budget of evaluated samples (the loop caps the sum of its rounds' chunk
    sizes), and total_samples (a 0-d device tensor) counts the samples the field evaluated, i.e.
    samples.sum() (the loop also counts those marched past a ray's termination inside a chunk)."""
    from . import field
    from ._lib import call, check_input, ptr, stream
    if getattr(model, "rgb_act", "Sigmoid") != "Sigmoid":
        raise NotImplementedError(HDR_GAP)
    rays_o = rays_o.contiguous()
    rays_d = rays_d.contiguous()
    check_input("rays_o", rays_o, torch.float32)
    check_input("rays_d", rays_d, torch.float32)
    if rays_o.dim() != 2 or rays_o.shape[1] != 3 or rays_d.shape != rays_o.shape:
        raise RuntimeError("rays_o and rays_d must both be (N, 3)")
    exp_step_factor = kwargs.get("exp_step_factor", 0.0)
    N_rays = rays_o.shape[0]
    device = rays_o.device
    opacity = torch.empty(N_rays, device=device)
    depth = torch.empty(N_rays, device=device)
    rgb = torch.empty(N_rays, 3, device=device)
    samples = torch.empty(N_rays, dtype=torch.int32, device=device)
    total_samples = torch.zeros((), dtype=torch.int64, device=device)
    queue = torch.empty(1, dtype=torch.int32, device=device)
    packed, table16 = field.field_weights(model.xyz_encoder.params, model.rgb_net.params, model.rgb_width)
    call("mfnerf_render_test_fused", ptr(rays_o), ptr(rays_d), int(N_rays), ptr(model.center), ptr(model.half_size),
         ptr(model.density_bitfield), int(model.cascades), float(model.scale), float(exp_step_factor),
         int(model.grid_size), MAX_SAMPLES, int(kwargs.get("max_samples", MAX_SAMPLES)),
         float(kwargs.get("T_threshold", 1e-4)), float(model._x_min), float(model._x_range), model.desc,
         ptr(table16), ptr(packed), int(model.rgb_width), ptr(queue), ptr(opacity), ptr(depth), ptr(rgb),
         ptr(samples), ptr(total_samples), stream())

    rgb_bg = torch.ones(3, device=device) if exp_step_factor == 0 else torch.zeros(3, device=device)
    rgb += rgb_bg * rearrange(1 - opacity, "n -> n 1")
    results = {"opacity": opacity, "depth": depth, "rgb": rgb, "total_samples": total_samples, "samples": samples}
    for k, v in results.items():
        if kwargs.get("to_cpu", False):
            v = v.cpu()
            if kwargs.get("to_numpy", False):
                v = v.numpy()
        results[k] = v
    return results


def _render_rays_train(model, rays_o, rays_d, hits_t, **kwargs):
    """rendering.py:121-163."""
    exp_step_factor = kwargs.get("exp_step_factor", 0.0)
    results = {}

    (rays_a, xyzs, dirs, results["deltas"], results["ts"], results["rm_samples"]) = RayMarcher.apply(
        rays_o, rays_d, hits_t[:, 0], model.density_bitfield, model.cascades, model.scale, exp_step_factor,
        model.grid_size, MAX_SAMPLES)

    for k, v in kwargs.items():
        if isinstance(v, torch.Tensor):
            kwargs[k] = torch.repeat_interleave(v[rays_a[:, 0]], rays_a[:, 2], 0)
    sigmas, rgbs = model(xyzs, dirs, **kwargs)

    (results["vr_samples"], results["opacity"], results["depth"], results["rgb"], results["ws"]) = \
        VolumeRenderer.apply(sigmas, rgbs.contiguous(), results["deltas"], results["ts"], rays_a,
                             kwargs.get("T_threshold", 1e-4))
    results["rays_a"] = rays_a

    if exp_step_factor == 0:
        rgb_bg = torch.ones(3, device=rays_o.device)
    elif kwargs.get("random_bg", False):
        rgb_bg = torch.rand(3, device=rays_o.device)
    else:
        rgb_bg = torch.zeros(3, device=rays_o.device)
    results["rgb"] = results["rgb"] + rgb_bg * rearrange(1 - results["opacity"], "n -> n 1")
    return results
