"""The fused test-time renderer (csrc/render.hip, mfnerf_render_test_fused) bit for bit on whole rays
and at its seams, against one round of the staged kernels (tests/render_ref.staged_whole_rays: march,
field, composite from opacity 0), and its composited rays against fp64.

csrc/ray_march.hpp states the contract: bit-for-bit equality with the staged path, every ray's outputs
a function of that ray alone.  So opacity, depth, rgb and the per-ray sample count are compared with
torch.equal: whole rays on the two golden fixture models (exp_step_factor 0, scale 0.5) and on two
real-scene models (exp_step_factor 1/256: scale 16 with six cascades, scale 1 with two; render_ref),
ray budgets around the 64-sample chunk with nothing terminating, T_threshold from 1e-4 to 0.9, and
batches around one, two and three fills of the persistent queue, where a lane pair finishes a ray
with live sums and refills while its 31 neighbours are mid-ray.  slots = CUs * waves_per_simd(W) * 128
restates the launch cap; tests/test_render_ref_cpu.py pins it to the source.

The C ABI is called directly (_fused): opacity, depth and rgb prefilled with NaN, samples with -7,
every output 64 rows longer than n_rays with a sentinel in the extra rows (the queue counter
overshoots n_rays by up to 32 per resident wave).  Every call asserts that each of the first n rows
was written, that the extra rows were not, and that total_samples == samples.sum().

fp64 (the convention of test_gpu_vren_seams.py).  E = max|x - ref64| / max|ref64| per output over the
rays that are not ambiguous (fp64 transmittance within 1e-5 relative of T_threshold), ref64 =
composite_ref.composite_test64 on the staged per-sample sigmas, rgbs, deltas, ts.  The fused kernel's E
must stay within 8 x the E of the fp32 C oracle (oracle.composite_test_fw) on the same inputs -- 8 x
for __expf (hardware exp2, 1-2 ulp) where the oracle's expf is below 1, amplified by the cancellation
in 1 - exp(-x) -- and away from ambiguous rays its sample count is the fp64 count exactly.

Measured (oracle E on the CPU -> tolerance 8 E; kernel E on an MI355X; the test prints them):
    model                 output    oracle E   tolerance  kernel E   kernel / oracle
    hash-rgb64            opacity   9.601e-07  7.681e-06  2.097e-06  2.18
    hash-rgb64            depth     9.226e-07  7.381e-06  2.149e-06  2.33
    hash-rgb64            rgb       7.557e-07  6.046e-06  2.143e-06  2.84
    mixedfeature-rgb128   opacity   8.812e-07  7.049e-06  1.735e-06  1.97
    mixedfeature-rgb128   depth     7.731e-07  6.185e-06  1.567e-06  2.03
    mixedfeature-rgb128   rgb       1.004e-06  8.029e-06  1.685e-06  1.68
    scale1-rgb128         opacity   1.129e-06  9.034e-06  1.156e-06  1.02
    scale1-rgb128         depth     4.174e-07  3.339e-06  4.122e-07  0.99
    scale1-rgb128         rgb       1.016e-06  8.126e-06  1.087e-06  1.07
    scale16-rgb64         opacity   2.591e-06  2.073e-05  2.790e-06  1.08
    scale16-rgb64         depth     8.622e-07  6.898e-06  1.729e-06  2.01
    scale16-rgb64         rgb       1.496e-06  1.197e-05  2.669e-06  1.78
(no ambiguous ray among the 4113 of any model; no kernel needed more than 2.9 of its 8 x).  Rays that terminate
inside the content at T_threshold 1e-4: none on the fixture models, 529 at scale 16, 1869 at scale 1; at
0.5 | 0.9 the fixture terminates 19 % | 89 % of its rays with a sample, the scale-16 model 83 % | 97 %.
"""
import functools

import pytest
import torch

import composite_ref as R
import render_ref as RR
from test_gpu_render_fused import _fixture

pytestmark = pytest.mark.gpu

NAN = float("nan")
UNSET, TAIL, GUARD = -7, -9, 64  # samples prefill; the sentinel and length of every output's extra rows
KEYS = ("opacity", "depth", "rgb", "samples")
CONFIGS = {  # name -> (fixture name | (rgb width, scale), exp_step_factor)
    "hash-rgb64": ("", 0.0),
    "mixedfeature-rgb128": ("_mf128", 0.0),
    "scale16-rgb64": ((64, 16.0), RR.EXP_STEP),
    "scale1-rgb128": ((128, 1.0), RR.EXP_STEP),
}
ALL = sorted(CONFIGS)


def _config(gpu, name):
    """-> (model, rays_o, rays_d, exp_step_factor): base rays first, the edge rays after them."""
    what, exp_step = CONFIGS[name]
    if isinstance(what, str):
        model = _fixture(gpu, what)[1]
        o, d = RR.fixture_rays()
    else:
        model = RR.real_scene_model(gpu, *what)
        o, d = RR.real_scene_rays(what[1])
    return model, o.to(gpu), d.to(gpu), exp_step


def _fused(model, o, d, exp_step, budget=1024, thr=1e-4, with_samples=True):
    """mfnerf_render_test_fused into guarded, prefilled outputs -> dict of the first n rows (device)."""
    from mfnerf import field
    from mfnerf._lib import call, ptr, stream
    n, dev = o.shape[0], o.device
    packed, table16 = field.field_weights(model.xyz_encoder.params, model.rgb_net.params, model.rgb_width)

    def out(fill, *shape, dtype=torch.float32):
        t = torch.full((n + GUARD, *shape), TAIL, dtype=dtype, device=dev)
        t[:n] = fill
        return t
    op, de, rgb, smp = out(NAN), out(NAN), out(NAN, 3), out(UNSET, dtype=torch.int32)
    total = torch.full((1,), UNSET, dtype=torch.int64, device=dev)
    queue = torch.full((1,), UNSET, dtype=torch.int32, device=dev)
    call("mfnerf_render_test_fused", ptr(o), ptr(d), n, ptr(model.center), ptr(model.half_size),
         ptr(model.density_bitfield), int(model.cascades), float(model.scale), float(exp_step), int(model.grid_size),
         RR.MAX_SAMPLES, int(budget), float(thr), float(model._x_min), float(model._x_range), model.desc, ptr(table16),
         ptr(packed), int(model.rgb_width), ptr(queue), ptr(op), ptr(de), ptr(rgb), ptr(smp if with_samples else None),
         ptr(total), stream())
    torch.cuda.synchronize()
    for name, t in (("opacity", op), ("depth", de), ("rgb", rgb)):
        assert not torch.isnan(t[:n]).any(), f"{name}: a row was not written (or holds NaN)"
        assert bool((t[n:] == TAIL).all()), f"{name}: a row past n_rays was written"
    assert bool((smp[n:] == TAIL).all()), "samples: a row past n_rays was written"
    if with_samples:
        assert bool((smp[:n] >= 0).all()), "samples: a row was not written"
        assert int(total) == int(smp[:n].sum())
    else:
        assert bool((smp[:n] == UNSET).all())
    assert int(total) >= 0
    return dict(opacity=op[:n], depth=de[:n], rgb=rgb[:n], samples=smp[:n], total=int(total))


def _first_difference(got, ref):
    """For the report of a bit mismatch: per output the number of differing rays and the first one."""
    msg = []
    for k in KEYS:
        bad = (got[k] != ref[k])
        bad = bad.any(1) if bad.dim() > 1 else bad
        if bool(bad.any()):
            r = int(bad.nonzero()[0])
            msg.append(f"{k}: {int(bad.sum())} rays differ, first ray {r}: fused {got[k][r].tolist()} staged "
                       f"{ref[k][r].tolist()} (samples fused {int(got['samples'][r])} staged {int(ref['samples'][r])})")
    return "; ".join(msg)


def _assert_same(got, ref, what):
    for k in KEYS:
        assert torch.equal(got[k], ref[k]), f"{what}: {_first_difference(got, ref)}"


@functools.lru_cache(maxsize=None)
def _whole(gpu, name):
    """Test 1's pair, shared with the fp64 and queue tests: (fused, staged) at budget 1024, T_threshold 1e-4."""
    model, o, d, exp_step = _config(gpu, name)
    return _fused(model, o, d, exp_step), RR.staged_whole_rays(model, o, d, 1024, 1e-4, exp_step)


# ---------------------------------------------------------------- 1. whole rays, bit for bit
@pytest.mark.parametrize("name", ALL)
def test_whole_rays_bit_for_bit(gpu, name):
    model, o, d, exp_step = _config(gpu, name)
    got, ref = _whole(gpu, name)
    cen = RR.march_census(ref["deltas"], ref["xyzs"], ref["n_eff"], model.cascades)
    long, empty = int((ref["samples"] > 64).sum()), int((ref["samples"] == 0).sum())
    print(f"{name}: {o.shape[0]} rays, {int(ref['samples'].sum())} samples composited of {int(ref['n_eff'].sum())} "
          f"marched; rays of > 64 samples {long}, of none {empty}, terminated {int(ref['terminated'].sum())}; "
          f"marched samples per mip {cen['mips']} (from dt alone {cen['mips_dt']})")
    assert long >= 1000 and empty >= 100
    if exp_step:
        assert sum(m > 0 for m in cen["mips"]) >= (3 if model.cascades > 2 else 2)
    assert int(ref["samples"].max()) <= 1024 and bool((ref["samples"] <= ref["n_eff"]).all())
    _assert_same(got, ref, name)
    # a ray with no sample is all zeros (the background blend happens in render_fused, after the kernel)
    none = ref["samples"] == 0
    assert not got["opacity"][none].any() and not got["depth"][none].any() and not got["rgb"][none].any()


# ---------------------------------------------------------------- 2. budget seams
BUDGETS = (1, 2, 3, 63, 64, 65, 1024)


def test_budget_seams(gpu):
    """Fully occupied grid, T_threshold = -1 (nothing terminates): a ray's result is its first `budget`
    samples, around the 64-sample chunk of the staged kernels."""
    model, o, d, exp_step = _config(gpu, "hash-rgb64")
    o, d = o[:257].contiguous(), d[:257].contiguous()
    saved = model.density_bitfield.clone()
    try:
        model.density_bitfield.fill_(255)
        whole = RR.staged_whole_rays(model, o, d, 1024, -1.0, exp_step)
        n_eff = whole["n_eff"]
        print(f"budget seams: rays of > 65 samples {int((n_eff > 65).sum())} of 257, longest {int(n_eff.max())}")
        assert int((n_eff > 65).sum()) >= 200 and not whole["terminated"].any()
        for budget in BUDGETS:
            ref = whole if budget == 1024 else RR.staged_whole_rays(model, o, d, budget, -1.0, exp_step)
            got = _fused(model, o, d, exp_step, budget=budget, thr=-1.0)
            assert torch.equal(got["samples"], n_eff.clamp(max=budget)), budget
            _assert_same(got, ref, f"budget {budget}")
    finally:
        model.density_bitfield.copy_(saved)


# ---------------------------------------------------------------- 3. termination seams
@pytest.mark.parametrize("name", ["hash-rgb64", "scale16-rgb64"])
def test_termination_seams(gpu, name):
    model, o, d, exp_step = _config(gpu, name)
    o, d = o[:RR.N_BASE].contiguous(), d[:RR.N_BASE].contiguous()
    for thr in (1e-4, 1e-2, 0.5, 0.9):
        ref = RR.staged_whole_rays(model, o, d, 1024, thr, exp_step)
        hit = ref["samples"] > 0
        frac = float(ref["terminated"].sum()) / float(hit.sum())
        print(f"{name} T_threshold {thr}: {int(hit.sum())} rays hit, {frac:.3f} of them terminate inside the box; "
              f"samples composited {int(ref['samples'].sum())} of {int(ref['n_eff'].sum())}")
        if thr == 0.5:
            assert 0.1 <= frac <= 0.9
        got = _fused(model, o, d, exp_step, thr=thr)
        _assert_same(got, ref, f"{name} T_threshold {thr}")


# ---------------------------------------------------------------- 4. fp64 accuracy of the composited ray
@pytest.mark.parametrize("name", ALL)
def test_composited_rays_against_fp64(gpu, oracle, name):
    got, ref = _whole(gpu, name)
    sig, rgbs, dl, ts, n_eff = (ref[k].cpu() for k in ("sigmas", "rgbs", "deltas", "ts", "n_eff"))
    n = sig.shape[0]
    amb = RR.ambiguous(sig, dl, n_eff, 1e-4)
    print(f"{name}: ambiguous rays {int(amb.sum())} of {n}")
    assert int(amb.sum()) <= n // 100
    keep = ~amb
    O64, D64, C64, count = R.composite_test64(sig, rgbs, dl, ts, n_eff, 1e-4)
    assert torch.equal(got["samples"].cpu().long()[keep], count[keep])
    alive = torch.arange(n)
    op, de, col = torch.zeros(n), torch.zeros(n), torch.zeros(n, 3)
    oracle.composite_test_fw(sig, rgbs, dl, ts, None, alive, 1e-4, n_eff, op, de, col)
    worst = []
    for k, orc, want in (("opacity", op, O64), ("depth", de, D64), ("rgb", col, C64)):
        e_o, e_k = R.err(orc[keep], want[keep]), R.err(got[k].cpu()[keep], want[keep])
        print(f"    {name:21s} {k:9s} {e_o:.3e}  {8 * e_o:.3e}  {e_k:.3e}  {e_k / e_o:.2f}")
        if e_k > 8 * e_o:
            worst.append((k, e_k, e_o))
    assert not worst, worst


# ---------------------------------------------------------------- 5. queue seams
def _slots(width):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus * (3 if width == 64 else 2) * 128


def _queue_sizes(slots):
    return (slots - 1, slots, slots + 1, slots + 31, slots + 33, 2 * slots + RR.N_BASE, 3 * slots + slots // 3)


def _tiled(gpu, name, sizes, with_samples=True):
    model, o, d, exp_step = _config(gpu, name)
    base, _ = _whole(gpu, name)
    o, d = o[:RR.N_BASE], d[:RR.N_BASE]
    for n in sizes:
        idx = torch.arange(n, device=gpu) % RR.N_BASE
        got = _fused(model, o[idx].contiguous(), d[idx].contiguous(), exp_step, with_samples=with_samples)
        for k in KEYS[:3] + (("samples",) if with_samples else ()):
            same = got[k] == base[k][idx]
            same = same.all(1) if same.dim() > 1 else same
            assert bool(same.all()), (f"{name} n_rays {n}, {k}: {int((~same).sum())} rows differ from the base "
                                      f"block's, first row {int((~same).nonzero()[0])}")
        assert got["total"] == int(base["samples"][idx].sum())


@pytest.mark.parametrize("name", ["hash-rgb64", "mixedfeature-rgb128"])
def test_queue_seams(gpu, name):
    """rays[i] = base[i % 4099] for n_rays around one, two and three fills of the resident ray slots:
    row i is the base block's row i % 4099, bit for bit (test 1 holds the base block to the staged path)."""
    slots = _slots(_config(gpu, name)[0].rgb_width)
    print(f"{name}: {slots} ray slots; n_rays {_queue_sizes(slots)}")
    _tiled(gpu, name, _queue_sizes(slots))


def test_queue_seams_real_scene(gpu):
    _tiled(gpu, "scale16-rgb64", (2 * _slots(64) + RR.N_BASE,))


def test_queue_seams_without_samples_output(gpu):
    """samples = NULL through the ABI: the three float outputs are the same bits, total_samples the same count."""
    _tiled(gpu, "hash-rgb64", (_slots(64) + 33,), with_samples=False)
