"""What tests/test_gpu_render_seams.py takes for granted, checked without a GPU: its edge rays end in
the CPU oracle's ray/box test and march (before any of them reaches the fused kernel), its real-scene
ray sets meet the census the GPU tests assert, the fp64 test-time compositing reference
(composite_ref.composite_test64) agrees with the designed seam batch's reference and bounds the fp32
C oracle's own error E on whole marched rays, and csrc/render.hip still caps its launch the way the
queue-seam sizes restate it."""
import os
import re

import pytest
import torch

import composite_ref as R
import render_ref as RR
from conftest import PKG
from mfnerf import synthetic

E_CEILING = 8e-6  # test_composite_ref_cpu.E_CEILING: the same sums, the same bound
THR = R.T_THRESHOLD

# (scale, cascades, exp_step_factor) of every configuration the GPU suite renders
CONFIGS = [(0.5, 1, 0.0), (1.0, 2, RR.EXP_STEP), (16.0, 6, RR.EXP_STEP)]


def _bitfield(scale, cascades):
    if scale in RR.SCENES:
        return RR.real_scene_bitfield(scale)
    return synthetic.packbits_np(synthetic.ball_density_grid(cascades=cascades, scale=scale, seed=3),
                                 0.01 * RR.MAX_SAMPLES / RR.SQRT3)  # the golden fixtures' grid (make_golden.py)


def _march(oracle, o, d, bf, scale, cascades, exp_step, n_samples):
    """rendering.render's ray/box test and near clamp, then one test-time march, all in the oracle."""
    _, ht, _ = oracle.ray_aabb_intersect(o, d, torch.zeros(1, 3), torch.full((1, 3), float(scale)), 1)
    ht[(ht[:, 0, 0] >= 0) & (ht[:, 0, 0] < RR.NEAR_DISTANCE), 0, 0] = RR.NEAR_DISTANCE
    hits = ht.clone()  # (the march advances hits_t[:, 0] in place)
    out = oracle.raymarching_test(o, d, hits[:, 0], torch.arange(o.shape[0]), bf, cascades, scale, exp_step, RR.GRID,
                                  RR.MAX_SAMPLES, n_samples)
    return ht, out


@pytest.mark.parametrize("scale,cascades,exp_step", CONFIGS)
@pytest.mark.parametrize("occupancy", ["balls", "full"])
def test_edge_rays_end_in_the_oracle(oracle, scale, cascades, exp_step, occupancy):
    o, d = RR.edge_rays(scale)
    if scale in RR.SCENES:
        d = (d / d.norm(dim=1, keepdim=True)).contiguous()
    assert torch.isfinite(o).all() and torch.isfinite(d).all() and bool((d != 0).any(1).all())
    bf = _bitfield(scale, cascades)
    if occupancy == "full":
        bf = torch.full_like(bf, 255)
    for n_samples in (1, 65, RR.MAX_SAMPLES):
        ht, (xyzs, dirs, deltas, ts, n_eff) = _march(oracle, o, d, bf, scale, cascades, exp_step, n_samples)
        assert torch.isfinite(ht).all()
        assert torch.isfinite(ts).all() and torch.isfinite(deltas).all() and torch.isfinite(xyzs).all()
        assert int(n_eff.min()) >= 0 and int(n_eff.max()) <= n_samples
    # the cases are what their comments say: misses, hits, the zero-length hit on the box edge
    miss = ht[:, 0, 0] < 0
    assert miss.tolist() == [True] * 5 + [False] * 8 + [True]
    assert float(ht[11, 0, 0]) == float(ht[11, 0, 1]) > 0 and int(n_eff[11]) == 0
    assert torch.equal(ht[5:9, 0, 0], torch.full((4,), RR.NEAR_DISTANCE))  # origins inside the box: the near clamp
    if occupancy == "full":
        assert bool((n_eff[~miss & (torch.arange(14) != 11)] > 0).all())


@pytest.fixture(scope="module")
def marched(oracle):
    """The CPU oracle march of base_rays on the fixtures' ball grid, whole rays."""
    o, d = RR.base_rays()
    _, out = _march(oracle, o, d, _bitfield(0.5, 1), 0.5, 1, 0.0, RR.MAX_SAMPLES)
    return out


def test_base_rays_census(marched):
    xyzs, dirs, deltas, ts, n_eff = marched
    c = RR.march_census(deltas, xyzs, n_eff, 1)
    print("base rays on the fixture grid:", c)
    assert c["long"] >= 1000 and c["empty"] >= 100


@pytest.mark.parametrize("scale", sorted(RR.SCENES))
def test_real_scene_census(oracle, scale):
    """The census test_gpu_render_seams.py asserts on the staged march, here on the oracle's (the two
    marches are held bit-equal by test_gpu_vren.py)."""
    c = RR.SCENES[scale]
    o, d = RR.real_scene_rays(scale)
    assert torch.allclose(d.norm(dim=1), torch.ones(d.shape[0]), atol=1e-6)
    _, (xyzs, dirs, deltas, ts, n_eff) = _march(oracle, o, d, RR.real_scene_bitfield(scale), scale, c["cascades"],
                                                 RR.EXP_STEP, RR.MAX_SAMPLES)
    cen = RR.march_census(deltas, xyzs, n_eff, c["cascades"])
    print(f"scale {scale}:", cen)
    assert cen["long"] >= 1000 and cen["empty"] >= 100
    assert sum(m > 0 for m in cen["mips"]) >= (3 if c["cascades"] > 2 else 2)


def test_composite_test64_is_the_seam_reference():
    """composite_test64 (vectorised, row per ray) against composite_fw64 (_ray64 per ray) on the designed
    seam batch, one row per ray: the same fp64 numbers, and the count is total + 1 up to the ray's end."""
    b = R.seam_rays(0)
    ra, S = b["rays_a"], max(R.LENGTHS)
    n = ra.shape[0]
    sig, dl, ts = torch.zeros(n, S), torch.zeros(n, S), torch.zeros(n, S)
    rgb, n_eff = torch.zeros(n, S, 3), torch.zeros(n, dtype=torch.int32)
    for ray, s0, N in ra.tolist():
        sig[ray, :N], dl[ray, :N], ts[ray, :N] = b["sigmas"][s0:s0 + N], b["deltas"][s0:s0 + N], b["ts"][s0:s0 + N]
        rgb[ray, :N], n_eff[ray] = b["rgbs"][s0:s0 + N], N
        sig[ray, N:] = float("nan")  # nothing past n_eff is read
    ref = R.composite_fw64(R.dense(b["sigmas"], b["in_ray"]), R.dense(b["rgbs"], b["in_ray"]),
                           R.dense(b["deltas"], b["in_ray"]), R.dense(b["ts"], b["in_ray"]), ra)
    O, D, C, count = R.composite_test64(sig, rgb, dl, ts, n_eff)
    assert torch.equal(count, torch.minimum(ref["total"] + 1, n_eff.long()))
    for got, want in ((O, ref["opacity"]), (D, ref["depth"]), (C, ref["rgb"])):
        assert torch.allclose(got, want, rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("density", [1.0, 40.0], ids=["fixed64-sigma", "terminating"])
def test_oracle_E_on_marched_rays(oracle, marched, density):
    """The fp32 C oracle's test-time compositing against composite_test64 on inputs with the GPU test's
    shape statistics: the marched ray lengths, deltas and ts, sigma = exp(N(0, 1.5^2)) and uniform rgb
    as test_gpu_vren.fixed64_batch draws them.  Those sigmas never bring T to 1e-4 within a ray of these
    lengths (sum sigma dt ~ 1), so the batch runs a second time 40 x as dense, where most rays terminate."""
    _, _, deltas, ts, n_eff = marched
    n, S = deltas.shape
    g = torch.Generator().manual_seed(1)
    sig = torch.exp(torch.randn(n, S, generator=g) * 1.5) * density
    rgb = torch.rand(n, S, 3, generator=g)
    amb = RR.ambiguous(sig, deltas, n_eff, THR)
    print(f"ambiguous rays: {int(amb.sum())} of {n}")
    assert int(amb.sum()) <= n // 100
    O64, D64, C64, count = R.composite_test64(sig, rgb, deltas, ts, n_eff, THR)
    early, whole = int((count < n_eff).sum()), int(((count == n_eff) & (n_eff > 0)).sum())
    print(f"rays ended early {early}, composited whole {whole}")
    assert whole > 50 and (early > 500 if density > 1 else early == 0)
    alive = torch.arange(n)
    op, de, col = torch.zeros(n), torch.zeros(n), torch.zeros(n, 3)
    oracle.composite_test_fw(sig, rgb, deltas, ts, None, alive, THR, n_eff, op, de, col)
    # the oracle marks a ray (alive = -1) when it terminated or had no sample: the fp64 reference says the same
    T_end = torch.exp(-(sig.double() * deltas.double() * (torch.arange(S)[None] < count[:, None])).sum(1))
    assert torch.equal((alive < 0)[~amb], ((T_end <= THR) | (n_eff == 0))[~amb])
    keep = ~amb
    for name, got, want in (("opacity", op, O64), ("depth", de, D64), ("rgb", col, C64)):
        e = R.err(got[keep], want[keep])
        print(f"oracle E {name:8s} {e:.3e}")
        assert e <= E_CEILING, (name, e)


def test_render_launch_cap_is_what_the_queue_seams_restate():
    """test_gpu_render_seams.py sizes its queue seams as CUs * waves_per_simd(W) * 128 ray slots.  A change
    to the launch cap of csrc/render.hip fails here and moves those sizes with it."""
    src = open(os.path.join(PKG, "csrc", "render.hip")).read()
    flat = re.sub(r"\s+", " ", src)
    assert "constexpr int waves_per_simd(int W) { return W == 64 ? 3 : 2; }" in flat
    assert "const int64_t want = div_up<int64_t>(p.n_rays, 32 * (FIELD_BLOCK / 64));" in flat
    assert "const int64_t cap = (int64_t)cu_count() * waves_per_simd(W);" in flat
    assert "dim3((unsigned)(want < cap ? want : cap)), dim3(FIELD_BLOCK)" in flat
    assert "amdgpu_waves_per_eu(waves_per_simd(W), waves_per_simd(W))" in flat
    # the drain test and the bounds guard the seam sizes aim at
    assert "if (base >= p.n_rays - cnt) drained = true;" in flat and "if (idx < p.n_rays) {" in flat
    hdr = re.sub(r"\s+", " ", open(os.path.join(PKG, "csrc", "field_fwd.hpp")).read())
    assert re.search(r"FIELD_BLOCK = 256\b", hdr), "rays per workgroup: 32 * (256 / 64) = 128"
