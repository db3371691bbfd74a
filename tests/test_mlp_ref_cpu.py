"""tests/mlp_ref.py (the float64-accumulated restatement of csrc/mlp.hip) checked on the CPU, and the
precondition of every input of tests/test_gpu_mlp_seams.py.

1. With every fp16 rounding replaced by the identity, the reference backward is torch's float64
   autograd of the reference forward (rtol 1e-12): the formulas are right.
2. The reference forward is tests/test_gpu_tcnn.py's mlp16 on the same inputs.
3. order_sensitivity < field_ref.ORDER_LIMIT (2e-4) for every (n, seed, config, region) the GPU file
   runs: the GPU file compares kernels with this reference at max error / max reference < 2e-3, which
   only means something where the reference is not itself deciding an fp16 rounding or a ReLU gate by
   its summation order.  A seed that breaks this fails here, naming the case, not on the GPU.
4. The launch and region tables cross the seams they are named after: which dW chunk, 32-sample tile
   and grid trip each [lo, hi) falls in.
"""
import pytest
import torch

import field_ref
import mlp_ref as R

CFG_IDS = [f"{W}-{NH}-{OA}" for W, NH, OA in R.CONFIGS]


@pytest.mark.parametrize("cfg", R.CONFIGS, ids=CFG_IDS)
def test_backward_is_autograd_of_forward_without_rounding(cfg):
    W, NH, OA = cfg
    x, params, dout = R.seam_inputs(173, 2, W, NH, OA)
    x64 = x.double().requires_grad_(True)
    p64 = params.double().requires_grad_(True)
    ident = lambda t: t  # noqa: E731
    y, acts = R.forward(x64, p64, W, NH, OA, rnd=ident)
    (y * dout.double()).sum().backward()
    with torch.no_grad():
        dx, dWs = R.backward(acts, dout, rnd=ident)
    # autograd sums in another order, so an element that cancels to near zero carries the float64
    # rounding of its terms: 1e-12 of each output's maximum (the GPU file's measure), not of the element
    def rel(got, ref):
        assert float(ref.abs().max()) > 0
        return float((got - ref).abs().max() / ref.abs().max())

    assert rel(dx, x64.grad) < 1e-12
    for l, (got, ref) in enumerate(zip(dWs, R.split(p64.grad, W, NH))):
        assert rel(got, ref) < 1e-12, l
    assert rel(R.flat(dWs), p64.grad) < 1e-12  # flat() is the parameter layout


@pytest.mark.parametrize("cfg", R.CONFIGS, ids=CFG_IDS)
def test_forward_is_mlp16(cfg):
    from test_gpu_tcnn import mlp16
    W, NH, OA = cfg
    x, params, _ = R.seam_inputs(173, 3, W, NH, OA)
    y, acts = R.forward(x, params, W, NH, OA)
    assert y.dtype == torch.float64 and y.shape == (173, 16)
    assert len(acts["a"]) == NH + 1 and len(acts["Ws"]) == NH + 1
    for n_out in (3, 16):
        ref = mlp16(x, params, R.shapes_of(W, NH), n_out, OA)
        assert torch.allclose(y[:, :n_out], ref, rtol=1e-12, atol=0)


def test_inputs():
    for W, NH, OA in R.CONFIGS:
        x, params, dout = R.seam_inputs(33, 1, W, NH, OA)
        n_out = R.n_out_of(NH, OA)
        assert n_out == (16 if (NH, OA) == (1, "None") else 3)
        assert x.dtype == torch.float16 and x.shape == (33, 32) and float(x.abs().max()) <= 0.5
        assert params.shape == (R.n_params(W, NH),) == (W * 32 + (NH - 1) * W * W + 16 * W,)
        assert dout.dtype == torch.float16 and dout.shape == (33, 16)
        assert float(dout[:, n_out:].abs().max() if n_out < 16 else 0) == 0 and float(dout[:, :n_out].abs().min()) > 0
    assert set(R.BW_TRIP_CONFIGS) <= set(R.CONFIGS) and set(R.SAT_CONFIGS) <= set(R.CONFIGS)
    assert torch.equal(R.tile_rows(R.BASE_N + 2), torch.cat([torch.arange(R.BASE_N), torch.arange(2)]))


def test_region_reference_is_the_masked_sum():
    """backward(take(acts, idx), dout[idx]) is the weight gradient of the whole block with dout zeroed
    outside idx (what the spotlight cases launch), and its dx the rows idx."""
    W, NH, OA = 64, 2, "Sigmoid"
    x, params, dout = R.seam_inputs(300, 3, W, NH, OA)
    _, acts = R.forward(x, params, W, NH, OA)
    idx = torch.arange(130, 177)
    masked = torch.zeros_like(dout)
    masked[idx] = dout[idx]
    full = R.backward(acts, masked)
    part = R.backward(R.take(acts, idx), dout[idx])
    assert torch.allclose(full[0][idx], part[0], rtol=1e-12, atol=0)
    rest = torch.ones(300, dtype=torch.bool)
    rest[idx] = False
    assert float(full[0][rest].abs().max()) == 0
    for a, b in zip(full[1], part[1]):
        assert float(b.abs().max()) > 0 and torch.allclose(a, b, rtol=1e-12, atol=0)


def test_constants_restate_the_launch_arithmetic():
    assert (R.TILE, R.WG, R.CH, R.TRIP) == (32, 128, 1024, 524288)
    assert R.WG == 4 * R.TILE and R.CH % R.WG == 0 and R.TRIP % R.CH == 0
    assert R.BASE_N < R.TRIP and R.BASE_N % R.TILE != 0
    # the small launches: below, at and above one tile (32) and one workgroup of 4 waves (128)
    assert set(R.SMALL_NS) >= {1, R.TILE - 1, R.TILE, R.TILE + 1, R.WG - 1, R.WG + 1, 173}
    # 127: one workgroup, its last tile ragged; 129: a second workgroup with one live sample and three idle waves
    assert -(-127 // R.WG) == 1 and -(-129 // R.WG) == 2 and -(-129 // R.TILE) == 5
    # the chunk seams: ld = ceil32(n) against CH
    ld = lambda n: -(-n // R.TILE) * R.TILE  # noqa: E731
    chunks = lambda n: -(-ld(n) // R.CH)     # noqa: E731
    assert [(ld(n), chunks(n)) for n in R.CHUNK_NS] == [(1024, 1), (1024, 1), (1056, 2), (2080, 3)]
    assert ld(1025) - R.CH == 32  # the second chunk: 32 rows, 1 of them live
    # the base block: five chunks, the last one 928 rows of a 5024-row ld
    assert ld(R.BASE_N) == 5024 and chunks(R.BASE_N) == 5 and ld(R.BASE_N) - 4 * R.CH == 928
    assert ld(R.SAT_N) == R.SAT_N and chunks(R.SAT_N) == 4


def test_regions_are_the_designed_seams():
    n = R.launch_sizes()
    assert n == {"two_trip": R.TRIP + 173, "base": R.BASE_N, "exact": R.TRIP, "exact_plus_1": R.TRIP + 1}
    reg = {r[0]: r for r in R.regions()}
    assert set(reg) == {"second_trip", "ragged_tile", "trip_boundary", "chunk_boundary", "last_chunk", "single_sample"}
    for name, launch, lo, hi, start in reg.values():
        assert 0 <= start <= lo < hi <= n[launch], name
        assert start % R.CH == 0 and lo - start < R.CH, name  # the multiple of CH at or below lo
    tile, chunk, trip = (lambda s: s // R.TILE), (lambda s: s // R.CH), (lambda s: s // R.TRIP)
    # a launch takes a second trip exactly when it has more than 4096 workgroups' worth of tiles
    wgs = lambda m: min(-(-m // R.WG), 4096)  # noqa: E731
    assert wgs(n["exact"]) * R.WG == n["exact"] and wgs(n["two_trip"]) * R.WG < n["two_trip"]
    assert wgs(n["base"]) * R.WG >= n["base"]
    _, _, lo, hi, _ = reg["second_trip"]
    assert (trip(lo), trip(hi - 1)) == (1, 1) and lo == R.TRIP and hi - lo == 173
    _, _, lo, hi, _ = reg["ragged_tile"]  # 13 samples: tile 5 of the second trip, workgroup 1's second wave
    assert hi - lo == 13 and tile(lo) == tile(hi - 1) == R.TRIP // R.TILE + 5 and lo % R.TILE == 0
    assert hi == n["two_trip"] and trip(lo) == 1
    _, _, lo, hi, start = reg["trip_boundary"]  # the first trip's last workgroup | the second trip's first
    assert (trip(lo), trip(hi - 1)) == (0, 1) and (lo, hi) == (R.TRIP - R.WG, R.TRIP + R.WG)
    assert chunk(lo) + 1 == chunk(hi - 1) == R.TRIP // R.CH and start == R.TRIP - R.CH
    _, _, lo, hi, start = reg["chunk_boundary"]  # one tile either side of chunks 2 | 3
    assert (chunk(lo), chunk(hi - 1)) == (2, 3) and tile(hi - 1) - tile(lo) == 1 and start == 2 * R.CH
    assert hi < n["base"] - R.CH  # chunk 4, after the region, holds zeros only
    _, _, lo, hi, start = reg["last_chunk"]  # the last chunk of a launch that ends on the trip: no pad rows
    assert chunk(lo) == chunk(hi - 1) == R.TRIP // R.CH - 1 and hi == n["exact"] and trip(hi - 1) == 0
    _, _, lo, hi, start = reg["single_sample"]  # one live sample in a 32-row chunk, in the second trip
    assert hi - lo == 1 and trip(lo) == 1 and chunk(lo) == R.TRIP // R.CH and lo == start


@pytest.mark.parametrize("cfg", R.CONFIGS, ids=CFG_IDS)
def test_order_sensitivity_of_every_gpu_input(cfg):
    worst = R.worst_sensitivities(cfg, R.SMALL_SEED[cfg], R.BASE_SEED[cfg])
    expected = ({f"small_{n}" for n in R.SMALL_NS} | {f"chunk_{n}" for n in R.CHUNK_NS}
                | {"base_block", "sample_1024"} | {r[0] for r in R.regions()})
    assert set(worst) == expected
    for case, sens in worst.items():
        assert len(sens) == cfg[1] + 2
        print(f"{cfg} {case}: order sensitivity dx {sens[0]:.2e} dW " + " ".join(f"{s:.2e}" for s in sens[1:]))
    for case, sens in worst.items():
        assert max(sens) < field_ref.ORDER_LIMIT, (cfg, case, sens)


@pytest.mark.parametrize("cfg", R.SAT_CONFIGS, ids=[f"{W}-{NH}-{OA}" for W, NH, OA in R.SAT_CONFIGS])
def test_saturation_inputs(cfg):
    W = cfg[0]
    for case in ("bounds", "overflow"):
        share, lo, hi = R.saturation_stats(W, case)
        fw, bw = R.saturation_sensitivity(W, case)
        print(f"{cfg} saturation, {case}: {share:.3f} of the logits beyond +-15, range [{lo:.1f}, {hi:.1f}], order "
              f"sensitivity forward {fw:.2e} backward " + " ".join(f"{s:.2e}" for s in bw))
        assert share >= 0.10, (cfg, case, "saturation share", share)
        if case == "bounds":
            assert max(bw) < field_ref.ORDER_LIMIT, (cfg, "saturation", bw)
            assert fw <= R.FW_ORDER_LIMIT, (cfg, "saturation, forward", fw)
        else:  # exp(-z) is inf in fp32 past z = -88.7: the kernel's sigmoid must take that to 0, not to NaN
            assert lo < -88.8 and hi > 88.8, (cfg, "overflow range", lo, hi)


def test_saturation_scale_amplifies_the_summation_order():
    """Why the bounds are not asserted at the overflow scale: there the float32 and float64
    restatements themselves differ by more than the forward bound (a hidden activation's fp16
    rounding, amplified by the scaled W_out)."""
    for W in (64, 128):
        x, params, _ = R.saturation_inputs(W, "overflow")
        assert R.forward_sensitivity(x, params, W, 2, "Sigmoid") > 2e-3


def test_order_sensitivity_sees_a_bad_seed():
    """The measure is not vacuous: seed 1 at (128, 2, Sigmoid) flips a ReLU gate between float32 and
    float64 accumulation in the base block (found by the seed search)."""
    cfg = (128, 2, "Sigmoid")
    assert max(R.order_sensitivity(*R.seam_inputs(R.BASE_N, 1, *cfg), *cfg)) > 10 * field_ref.ORDER_LIMIT
