"""The whole-ray reference of the fused test-time renderer (csrc/render.hip) and the rays and models
its seam suite runs (tests/test_gpu_render_seams.py, tests/test_render_ref_cpu.py).

staged_whole_rays is rendering._render_rays_test with exactly one round: the ray/box test and near
clamp of rendering.render, one mfnerf_raymarching_test with N_samples = the ray budget, the field
through model() on the valid samples, one mfnerf_composite_test_fw from opacity 0 (T = 1 - 0 is
exact: no re-derivation between rounds).  Each of those kernels has its own fp64 or oracle suite;
the fused kernel's contract (csrc/ray_march.hpp) is bit-for-bit equality with them.

Rays.  base_rays: the 4099 ball-scene rays of test_batch_independence (4099 is prime: a tiled copy
lands every ray on other lanes, waves and workgroups).  edge_rays: misses, origins inside the box,
exits behind the origin, zero direction components, a ray through a box edge; no zero direction
vector, no non-finite component, and no origin on a slab plane of a zero component (0 * inf).

Real-scene models.  benchmark_mipnerf360_mf.sh's march setting (exp_step_factor 1/256, scale 16: six
cascades, the reference's calc_dt(..., cascades) quirk, black background) and the scale 1 / two
cascade setting of test_gpu_vren*.py.  With dt = t / 256 a ray takes ~256 * chord / t samples of a
ball whatever the scene's size, and synthetic.ball_density_grid keeps its balls inside
[-0.5, 0.5]^3 (mip 0): under those rays it gives 276 rays of more than 64 samples and two mips.  So
the same seeded balls are scaled by SCENES[..]['content'] (to +-3 at scale 16) and the cameras moved to
1.5 * SCENES[..]['cameras'] from the origin, directions normalised as colmap's get_rays gives them:
3164 | 2967 rays of more than 64 samples, 586 | 640 of none, mips {1, 2, 3} | {0, 1} (the CPU oracle
march, asserted in test_render_ref_cpu.py)."""
import functools

import numpy as np
import torch

from mfnerf import synthetic

SQRT3 = 3 ** 0.5
MAX_SAMPLES = 1024      # rendering.MAX_SAMPLES
NEAR_DISTANCE = 0.01    # rendering.NEAR_DISTANCE
GRID = 128
N_BASE = 4099
EXP_STEP = 1 / 256
SCENES = {16.0: dict(cascades=6, content=6.0, cameras=2.0, grid="Hash", seed=0, gain=0.8, shift=0.3, spread=3.0),
          1.0: dict(cascades=2, content=1.5, cameras=0.6, grid="MixedFeature", seed=0, gain=1.6, shift=0.0, spread=1.0)}
# gain, shift, spread: set_weights.  Measured on an MI355X (fraction of the base rays with a sample that
# terminate inside the content at T_threshold 1e-4 | 1e-2 | 0.5 | 0.9): scale 16 0.15 | 0.31 | 0.83 | 0.97,
# scale 1 0.54 | 0.72 | 0.95 | 0.99; the golden fixture models 0 | 0 | 0.19 | 0.89
RGB_GAIN = 0.5


class HP:
    pass


@functools.lru_cache(maxsize=None)
def base_rays():
    """(rays_o, rays_d) (4099, 3) on the CPU: cameras 1.5 from the origin, unnormalised directions."""
    return synthetic.random_rays(N_BASE, synthetic.camera_poses(), seed=3)


def edge_rays(scale=0.5):
    """(rays_o, rays_d) of the edge cases for the box [-scale, scale]^3 (scale a power of two keeps
    every product below exact)."""
    s = float(scale)
    rows = [
        # origin / s          direction
        ((2.0, 2.0, 2.0),     (1.0, 0.3, -0.2)),    # outside, moving away: miss
        ((0.0, 2.0, 0.0),     (1.0, 0.0, 0.0)),     # parallel to a face it never reaches: miss (two zeros)
        ((3.0, 0.25, 0.0),    (0.0, 1.0, 0.2)),     # one zero component, outside its slab: miss
        ((0.0, 0.0, 2.0),     (0.1, 0.05, 1.0)),    # outside looking away: the exit is behind the origin
        ((-2.0, -2.0, -2.0),  (-1.0, -1.0, -1.0)),  # the same along the diagonal
        ((0.1, -0.2, 0.3),    (0.3, 0.5, -0.8)),    # origin inside: the near clamp
        ((0.05, 0.05, 0.05),  (0.0, 0.0, 1.0)),     # inside, axis-parallel (two zeros)
        ((-0.3, 0.2, -0.1),   (1.0, 0.0, 0.4)),     # inside, one zero component
        ((0.0, 0.0, 0.4),     (0.0, 0.25, -1.0)),   # inside, through the centre
        ((-2.0, 0.1, 0.2),    (1.0, 0.0, 0.1)),     # outside, one zero component, hits
        ((0.2, 0.3, -2.0),    (0.0, 0.0, 1.0)),     # outside, axis-parallel, hits
        ((-1.0, 3.0, 0.25),   (1.0, -1.0, 0.0)),    # through the edge x = y = scale: t1 == t2
        ((-1.0, 2.96875, 0.25), (1.0, -1.0, 0.0)),  # just inside that edge: a short chord
        ((-1.0, 3.03125, 0.25), (1.0, -1.0, 0.0)),  # just outside it: miss
    ]
    o = torch.tensor([r[0] for r in rows], dtype=torch.float32) * s
    d = torch.tensor([r[1] for r in rows], dtype=torch.float32)
    return o.contiguous(), d.contiguous()


def fixture_rays():
    """base_rays + edge_rays for the scale 0.5 golden fixture models."""
    (bo, bd), (eo, ed) = base_rays(), edge_rays(0.5)
    return torch.cat([bo, eo]).contiguous(), torch.cat([bd, ed]).contiguous()


def real_scene_rays(scale, edges=True):
    """base_rays from cameras at 1.5 * SCENES[scale]['cameras'] (+ edge_rays(scale)), directions normalised."""
    bo, bd = base_rays()
    o, d = bo * SCENES[scale]["cameras"], bd
    if edges:
        eo, ed = edge_rays(scale)
        o, d = torch.cat([o, eo]), torch.cat([d, ed])
    return o.contiguous(), (d / d.norm(dim=1, keepdim=True)).contiguous()


@functools.lru_cache(maxsize=None)
def real_scene_bitfield(scale):
    """synthetic.ball_density_grid's seeded balls scaled by SCENES[scale]['content'], every cascade, packed."""
    c = SCENES[scale]
    g = np.random.default_rng(c["seed"])
    radius = (0.065, 0.18)  # ball_density_grid's defaults and draw order
    centers = g.uniform(-0.5 + radius[1], 0.5 - radius[1], size=(12, 3))
    radii = g.uniform(radius[0], radius[1], size=12)
    grid = synthetic.balls_to_grid(centers * c["content"], radii * c["content"], G=GRID, cascades=c["cascades"],
                                   scale=scale)
    return synthetic.packbits_np(grid, 0.01 * MAX_SAMPLES / SQRT3)


def set_weights(model, seed, gain, shift=0.0, spread=1.0):
    """Seeded weights: the table U(-0.5, 0.5) as the Lego fixture's, the xyz MLP U(-gain, gain), the rgb
    MLP U(-RGB_GAIN, RGB_GAIN).  The MLPs have no bias, so h0 (sigma = exp(h0)) would be centred on 0
    whatever the gain and no ray of a scale-16 chord would stay above T = 0.5: the 64 weights of the
    density output (row 0 of the xyz MLP's second matrix, on ReLU outputs >= 0) are spread * U(-gain,
    gain) - shift, which moves h0's mean down by shift and widens it by spread."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        p = model.xyz_encoder.params
        xyz = torch.empty(p.numel()).uniform_(-0.5, 0.5, generator=g)
        xyz[:3072] *= 2 * gain
        xyz[2048:2112] = xyz[2048:2112] * spread - shift
        p.copy_(xyz)
        q = model.rgb_net.params
        q.copy_(torch.empty(q.numel()).uniform_(-RGB_GAIN, RGB_GAIN, generator=g))


_models = {}


def real_scene_model(gpu, width, scale=16.0):
    """NGP(scale) with SCENES[scale]'s cascades and bitfield, T = 16 and seeded uniform weights (the
    table U(-0.5, 0.5) as the Lego fixture's, the MLPs U(-gain, gain))."""
    from mfnerf.networks import NGP
    key = (str(gpu), width, scale)
    if key not in _models:
        c = SCENES[scale]
        hp = HP()
        hp.grid, hp.L, hp.F, hp.T, hp.N_min, hp.N_max = c["grid"], 16, 2, 16, 16, 2048
        hp.N_tables, hp.rgb_channels, hp.rgb_layers = (8 if c["grid"] == "MixedFeature" else 1), width, 2
        model = NGP(scale=scale, hparams=hp).to(gpu)
        assert model.cascades == c["cascades"]
        set_weights(model, 1000 + int(scale) + width, c["gain"], c["shift"], c["spread"])
        model.density_bitfield.copy_(real_scene_bitfield(scale))
        _models[key] = model
    return _models[key]


@torch.no_grad()
def staged_whole_rays(model, o, d, budget, T_threshold, exp_step_factor):
    """One round of the staged test-time path over whole rays -> dict of device tensors: opacity,
    depth, rgb (before the background blend), samples (int32: the samples composited, the
    terminating one included -- what the fused kernel counts), terminated (bool), and the per-sample
    sigmas, rgbs, deltas, ts, xyzs (n, budget[, 3]) with n_eff (n) for the fp64 leg and the census."""
    from mfnerf import vren
    from mfnerf.custom_functions import RayAABBIntersector
    o, d = o.contiguous(), d.contiguous()
    n, dev = o.shape[0], o.device
    _, hits_t, _ = RayAABBIntersector.apply(o, d, model.center, model.half_size, 1)
    hits_t[(hits_t[:, 0, 0] >= 0) & (hits_t[:, 0, 0] < NEAR_DISTANCE), 0, 0] = NEAR_DISTANCE
    alive = torch.arange(n, device=dev)
    xyzs, dirs, deltas, ts, n_eff = vren.raymarching_test(
        o, d, hits_t[:, 0], alive, model.density_bitfield, model.cascades, model.scale, exp_step_factor,
        model.grid_size, MAX_SAMPLES, budget)
    xyzs_f, dirs = xyzs.reshape(-1, 3), dirs.reshape(-1, 3)
    valid = (~torch.all(dirs == 0, dim=1)).nonzero()[:, 0]
    sigmas = torch.zeros(n * budget, device=dev)
    rgbs = torch.zeros(n * budget, 3, device=dev)
    if len(valid):
        s, c = model(xyzs_f.index_select(0, valid), dirs.index_select(0, valid))
        sigmas.index_copy_(0, valid, s.float())
        rgbs.index_copy_(0, valid, c.float())
    sigmas, rgbs = sigmas.view(n, budget).contiguous(), rgbs.view(n, budget, 3).contiguous()

    def composite(ne):
        out = torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, 3, device=dev)
        left = alive.clone()
        vren.composite_test_fw(sigmas, rgbs, deltas, ts, hits_t[:, 0], left, T_threshold, ne, *out)
        return out, (left < 0) & (ne > 0)

    (opacity, depth, rgb), terminated = composite(n_eff)
    # the compositing kernel reports that a ray terminated, not where.  Termination within the first k
    # samples is monotone in k, so the sample it happened at is found by bisection with the same
    # kernel on the same inputs (each call from opacity 0): no second statement of its arithmetic
    lo, hi = torch.ones_like(n_eff), n_eff.clone()
    while bool((terminated & (lo < hi)).any()):
        mid = torch.where(terminated, (lo + hi) // 2, n_eff)
        _, t = composite(mid.contiguous())
        hi = torch.where(terminated & t, mid, hi)
        lo = torch.where(terminated & ~t, mid + 1, lo)
    samples = torch.where(terminated, hi, n_eff).int()
    return dict(opacity=opacity, depth=depth, rgb=rgb, samples=samples, terminated=terminated, sigmas=sigmas,
                rgbs=rgbs, deltas=deltas, ts=ts, n_eff=n_eff, xyzs=xyzs)


def ambiguous(sigmas, deltas, n_eff, thr):
    """Rays whose fp64 transmittance passes within 1e-5 (relative) of thr (test_gpu_vren._ambiguous_rays
    on the row-per-ray layout): their termination sample may differ by one between exp implementations."""
    from test_gpu_vren import _ambiguous_rays
    n, S = sigmas.shape
    rays_a = torch.stack([torch.arange(n), torch.arange(n) * S, n_eff.long()], 1)
    return _ambiguous_rays(sigmas.reshape(-1), deltas.reshape(-1), rays_a, thr)


def march_census(deltas, xyzs, n_eff, cascades):
    """Of a (n, S) march: rays of more than 64 samples, rays of none, and samples per mip (the cell
    lookup's max(mip_from_pos, mip_from_dt), raymarching.cu:22-32, restated with torch.frexp)."""
    live = torch.arange(deltas.shape[1], device=deltas.device)[None] < n_eff[:, None]
    mip_dt = torch.frexp(deltas * GRID)[1].clamp(0, cascades - 1)
    mip_pos = (torch.frexp(xyzs.abs().amax(-1))[1] + 1).clamp(0, cascades - 1)
    mips = torch.bincount(torch.maximum(mip_dt, mip_pos)[live].long(), minlength=cascades)
    return dict(long=int((n_eff > 64).sum()), empty=int((n_eff == 0).sum()), mips=mips.tolist(),
                mips_dt=torch.bincount(mip_dt[live].long(), minlength=cascades).tolist())
