"""The standalone FullyFusedMLP kernels (csrc/mlp.hip: mlp_fw_kernel, mlp_bw_kernel, mlp_dw_kernel,
mlp_dw_reduce_kernel) at the seams of their tiles, chunks and grid-stride loops, against the
float64-accumulated reference of tests/mlp_ref.py, over the C ABI (mfnerf_mlp_fw / mfnerf_mlp_bw).

A wave takes a 32-sample tile, a workgroup four of them; the grid is capped at 4096 workgroups, so the
grid-stride loop takes a second trip only past TRIP = 524288 samples.  The backward writes the layer
inputs and pre-activation gradients transposed, padded with zero rows to ld = ceil32(n); the weight
gradients are split-K GEMMs over chunks of CH = 1024 of those ld rows, summed in chunk order and
ADDED into grad.  tests/test_gpu_tcnn.py's test_fully_fused_mlp_vs_fp16_oracle is the one-trip,
one-chunk case.  Here, for (W, NH, OA) in {64, 128} x {1, 2} x {None, Sigmoid}:

  (1) test_small_n              n in {1, 31, 32, 33, 127, 129, 173}: forward and backward
  (2) test_chunk_seams          n in {1023, 1024, 1025, 2049}; at 1025 also sample 1024 alone (the
                                second chunk: 32 rows, 1 live)
  (3) test_base_block           n = 4999: five chunks, the last one 928 rows; a second call into the
                                same grad doubles it
  (4) test_fw_two_trips         n = TRIP + 173
  (5) test_bw_two_trips         n = TRIP + 173, full dout: dx of every row (five configs)
  (6) test_bw_spotlight         dout zero outside a region: second_trip, ragged_tile, trip_boundary
                                of TRIP + 173; chunk_boundary of 4999; last_chunk of TRIP;
                                single_sample of TRIP + 1 (five configs)
  (7) test_sigmoid_saturation   W_out scaled until a third of the logits lie beyond +-15, at the scale
                                where the CPU preconditions still hold
      test_sigmoid_overflow     W_out scaled until the logits pass -88.7, where exp(-z) is inf in fp32:
                                everything finite, and the saturated outputs and samples compared
  (8) test_module_*             through mfnerf.tcnn.Network: padded output rows, the pack cache after
                                in-place updates, n = 0, argument errors

Every backward runs with dx and the whole workspace (transposed buffers and slab) filled with NaN: an
unwritten pad row or slab entry shows as NaN in grad.  dx and the forward's out carry 32 sentinel
rows past n that must come back untouched.

Inputs.  Every launch above 173 samples tiles one base block of 4999 samples (mlp_ref.BASE_N, sample
i = base sample i mod 4999): a sample recurs at other lane, wave, workgroup, chunk and trip positions
and the reference is computed on the base block alone, once per config.  With gradients tiled like
that a dropped tile moves a weight gradient by a few 1e-5, below any tolerance, hence the spotlights:
the weight gradients of a launch whose dout is zero outside a region are the region's own, compared
with the reference summed over the region.

Tolerances (no new numbers).  Backward: max|got - ref| / max|ref| < 2e-3 for dx and for each layer's
dW separately, test_field_bw's measure and bound (the same MFMA instruction, fp16 points and fp32
accumulation).  Forward: test_fully_fused_mlp_vs_fp16_oracle's 2e-3 * max(1, max|ref|).  The measure
means something only where the reference does not decide an fp16 rounding by its summation order:
mlp_ref.order_sensitivity < 2e-4 for every (n, seed, config, region) used here, asserted on the CPU
by tests/test_mlp_ref_cpu.py.

Bit-equalities, derived from the code: a sample's outputs depend on no other sample and not on its
position (the MFMA column is the sample; no cross-lane reduction on the data path), and a region
launched on its own from a multiple of CH has the chunk and in-chunk order of the full launch, the
other chunks adding exact zeros.

Saturation.  A hidden activation whose fp16 rounding falls the other way moves a logit by ulp(a) *
|W_out|, so scaling W_out carries the summation order into the output: at the scale that reaches
the fp32 overflow of exp(-z) (256) the float32 and float64 restatements themselves differ by 2e-3 ..
9e-3 in y, and the kernel measured 3.9e-3 | 3.7e-3 (width 64 | 128) against this reference there.
test_sigmoid_saturation therefore runs at the scale (64 | 96) where order_sensitivity < 2e-4 and the
forward's own sensitivity <= 2^-10 hold (tests/test_mlp_ref_cpu.py), and test_sigmoid_overflow
compares at scale 256 only what the order cannot move.

Measured on an MI355X (every test prints its figures), `kernel | CPU order sensitivity`, the worst
of dx and each layer's dW against the bound 2e-3; the forward as error / max(1, max|ref|) against 2e-3:
    backward                 64, 1, None       64, 1, Sigmoid    64, 2, None       64, 2, Sigmoid
    small n (7 sizes)        1.3e-05 | 3.8e-05 3.4e-07 | 3.4e-07 5.1e-05 | 3.7e-05 5.9e-06 | 2.8e-05
    chunk seams (4 sizes)    3.6e-05 | 4.2e-05 1.6e-05 | 1.1e-05 7.7e-05 | 4.1e-05 1.8e-04 | 2.6e-05
    sample 1024 alone        6.5e-08 | 7.8e-08 8.5e-08 | 8.3e-08 2.9e-08 | 7.3e-08 6.9e-08 | 8.3e-08
    base block               6.3e-05 | 3.3e-05 1.2e-05 | 1.6e-05 5.7e-05 | 3.1e-05 1.5e-04 | 2.2e-05
    two trips, dx            6.3e-05 | 3.3e-05    -                 -              1.5e-04 | 2.2e-05
    second_trip              1.5e-07 | 1.7e-05    -                 -              8.4e-06 | 3.1e-05
    ragged_tile              6.9e-08 | 2.2e-07    -                 -              6.5e-08 | 8.1e-07
    trip_boundary            3.9e-05 | 3.9e-05    -                 -              9.6e-06 | 2.9e-05
    chunk_boundary           8.0e-08 | 1.4e-07    -                 -              3.3e-06 | 1.0e-06
    last_chunk               6.5e-05 | 3.4e-05    -                 -              2.5e-05 | 2.0e-05
    single_sample            8.3e-08 | 1.1e-07    -                 -              7.8e-08 | 7.8e-08
    saturation                  -                 -                 -              7.6e-05 | 7.6e-05
    forward
    small n (7 sizes)        1.9e-06           0                 2.4e-04           0
    base block, two trips    2.4e-04           4.9e-04           4.9e-04           4.9e-04
    saturation                  -                 -                 -              1.1e-03 | 9.8e-04

    backward                 128, 1, None      128, 1, Sigmoid   128, 2, None      128, 2, Sigmoid
    small n (7 sizes)        4.3e-05 | 4.3e-05 5.2e-06 | 1.1e-05 9.1e-05 | 6.0e-05 3.1e-05 | 4.7e-05
    chunk seams (4 sizes)    3.5e-05 | 4.9e-05 1.8e-05 | 2.5e-05 3.8e-05 | 4.1e-05 4.1e-05 | 4.1e-05
    sample 1024 alone        3.9e-08 | 9.3e-08 6.1e-08 | 1.5e-07 4.8e-08 | 2.4e-07 7.2e-08 | 8.0e-08
    base block               5.3e-05 | 4.9e-05 9.9e-06 | 1.9e-05 6.8e-05 | 6.6e-05 7.6e-05 | 7.2e-05
    two trips, dx            5.3e-05 | 4.9e-05    -              6.8e-05 | 6.6e-05 7.6e-05 | 7.2e-05
    second_trip              1.4e-07 | 1.0e-05    -              2.9e-05 | 5.7e-05 2.5e-05 | 5.0e-05
    ragged_tile              9.6e-08 | 4.0e-06    -              1.3e-07 | 1.5e-07 5.2e-05 | 1.8e-07
    trip_boundary            5.1e-07 | 2.6e-06    -              2.6e-05 | 5.3e-05 2.6e-05 | 5.2e-05
    chunk_boundary           5.0e-06 | 4.0e-06    -              4.4e-06 | 4.4e-06 4.1e-06 | 2.5e-06
    last_chunk               6.9e-05 | 4.0e-05    -              3.5e-05 | 5.7e-05 6.9e-05 | 4.7e-05
    single_sample            6.5e-08 | 1.4e-07    -              1.1e-07 | 3.1e-07 1.3e-07 | 8.8e-08
    saturation                  -                 -                 -              1.8e-04 | 1.8e-04
    forward
    small n (7 sizes)        3.8e-06           0                 6.1e-05           2.4e-04
    base block, two trips    1.2e-04           4.9e-04           2.4e-04           4.9e-04
    saturation                  -                 -                 -              7.3e-04 | 7.3e-04
(`-`: the case does not run that config.)  test_sigmoid_overflow: every output finite; the saturated
outputs exact, dx of the saturated samples within 2.3e-7 of the reference's maximum.
Every bit-equality asserted here held for every config: out and dx of a sample at any position of the
two-trip launch against the one-trip launch of the base block; dx of the chunk-seam prefixes against
the base block's; dx and grad of each of the 30 (config, region) spotlights launched on their own from
a multiple of CH against the spotlight launch; grad of a repeated call.
"""
import functools
import types

import pytest
import torch

import mlp_ref as R
from mfnerf import tcnn
from mfnerf._lib import call, load, ptr, stream

pytestmark = pytest.mark.gpu

TOL = 2e-3      # test_field_bw: max error / max reference
FW_TOL = 2e-3   # test_fully_fused_mlp_vs_fp16_oracle: x max(1, max|ref|)
NAN = float("nan")
SENTINEL = -7.0
GUARD = 32      # sentinel rows past n in out and dx
REGIONS = tuple(r[0] for r in R.regions())


def _id(cfg):
    return f"{cfg[0]}-{cfg[1]}-{cfg[2]}"


ALL = [pytest.param(c, id=_id(c)) for c in R.CONFIGS]
TRIP_CFGS = [pytest.param(c, id=_id(c)) for c in R.BW_TRIP_CONFIGS]
SAT_CFGS = [pytest.param(c, id=_id(c)) for c in R.SAT_CONFIGS]


def _net(cfg, dev, params):
    """A config's C-ABI arguments and the MFMA fragment blob of `params`."""
    W, NH, OA = cfg
    n_out = R.n_out_of(NH, OA)
    assert load().mfnerf_mlp_n_params(32, W, NH, n_out) == R.n_params(W, NH) == params.numel()
    nb = load().mfnerf_mlp_packed_bytes(32, W, NH, n_out)
    assert nb > 0
    packed = torch.empty(nb // 2, dtype=torch.float16, device=dev)
    call("mfnerf_mlp_pack", ptr(params.to(dev).float().contiguous()), 32, W, NH, n_out, ptr(packed), stream())
    return types.SimpleNamespace(cfg=cfg, W=W, NH=NH, OA=OA, n_out=n_out, sig=int(OA == "Sigmoid"), dev=dev,
                                 packed=packed, n_params=params.numel())


def _fw(c, x, n):
    """mfnerf_mlp_fw into a NaN-filled out with GUARD sentinel rows past n."""
    out = torch.full((n + GUARD, 16), NAN, dtype=torch.float16, device=c.dev)
    out[n:] = SENTINEL
    call("mfnerf_mlp_fw", ptr(x), n, ptr(c.packed), 32, c.W, c.NH, c.n_out, c.sig, ptr(out), stream())
    torch.cuda.synchronize()
    assert bool((out[n:] == SENTINEL).all()), "the forward wrote past row n"
    return out[:n]


def _bw(c, x, n, dout, grad=None):
    """mfnerf_mlp_bw with dx and the workspace NaN-filled (0x7fff halves: NaN as f16 and, in pairs,
    as f32), GUARD sentinel rows past n in dx, and grad zero unless given.  Returns dx (n, 32), grad."""
    dx = torch.full((n + GUARD, 32), NAN, device=c.dev)
    dx[n:] = SENTINEL
    if grad is None:
        grad = torch.zeros(c.n_params, device=c.dev)
    nb = load().mfnerf_mlp_bw_workspace(n, 32, c.W, c.NH, c.n_out)
    assert nb > 0 and nb % 4 == 0
    ws = torch.full((nb // 2,), 0x7FFF, dtype=torch.int16, device=c.dev)
    call("mfnerf_mlp_bw", ptr(x), n, ptr(c.packed), 32, c.W, c.NH, c.n_out, c.sig, ptr(dout), ptr(dx), ptr(grad),
         ptr(ws), stream())
    torch.cuda.synchronize()
    assert bool((dx[n:] == SENTINEL).all()), "the backward wrote dx past row n"
    return dx[:n], grad


def _err(got, ref):
    ref = ref.to(got.device)
    m = float(ref.abs().max())
    assert m > 0
    return float((got.double() - ref).abs().max()) / m


def _check(what, got, ref):
    err = _err(got, ref)
    print(f"{what}: max error / max reference {err:.3e}")
    assert err < TOL, (what, err)


def _check_bw(what, c, dx, grad, ref):
    """dx and every layer's dW against the reference (dx, [dW_l]); everything finite."""
    assert torch.isfinite(dx).all(), f"{what}: a row of dx was not written"
    assert torch.isfinite(grad).all(), f"{what}: an unwritten pad row or slab entry reached grad"
    _check(f"{what} dx", dx, ref[0])
    for l, (got, r) in enumerate(zip(R.split(grad, c.W, c.NH), ref[1])):
        _check(f"{what} dW_{l}", got, r)


def _check_fw(what, out, y_ref):
    ref = y_ref.half().double().to(out.device)
    assert torch.isfinite(out).all(), f"{what}: a row of out was not written"
    err, scale = float((out.double() - ref).abs().max()), max(1.0, float(ref.abs().max()))
    print(f"{what} forward: max error / max(1, max reference) {err / scale:.3e}")
    assert err <= FW_TOL * scale, (what, err)


@functools.lru_cache(maxsize=None)
def _ctx(cfg):
    """Per config: the base block on the device, its packed weights, its reference (computed once)."""
    dev = torch.device("cuda:0")
    b = R.base_block(cfg)
    x, params, dout = b["inputs"]
    c = _net(cfg, dev, params)
    c.base, c.cpu = b, (x, dout)
    c.x, c.dout = x.to(dev), dout.to(dev)
    dx, dWs = R.backward(b["a64"], dout)
    c.ref_dx, c.ref_dW = dx.to(dev), dWs
    c.ref_y16 = b["y"].half().to(dev)
    c.sizes = R.launch_sizes()
    c.regions = {r[0]: r for r in R.regions()}
    return c


@functools.lru_cache(maxsize=None)
def _launch(cfg, n):
    """(x, dout) of a launch of n samples tiling the base block, built on the device, and the base rows."""
    c = _ctx(cfg)
    rows = R.tile_rows(n).to(c.dev)
    return c.x[rows].contiguous(), c.dout[rows].contiguous(), rows


@functools.lru_cache(maxsize=None)
def _base_bw(cfg):
    """The one-trip backward of the base block alone: dx (4999, 32) and grad."""
    c = _ctx(cfg)
    return _bw(c, c.x, R.BASE_N, c.dout)


# ------------------------------------------------------------------------------------------- (1)
@pytest.mark.parametrize("n", R.SMALL_NS)
@pytest.mark.parametrize("cfg", ALL)
def test_small_n(gpu, cfg, n):
    x, params, dout = R.seam_inputs(n, R.SMALL_SEED[cfg], *cfg)
    c = _net(cfg, gpu, params)
    y, acts = R.forward(x, params, *cfg)
    what = f"{_id(cfg)} n={n}"
    _check_fw(what, _fw(c, x.to(gpu), n), y)
    dx, grad = _bw(c, x.to(gpu), n, dout.to(gpu))
    _check_bw(what, c, dx, grad, R.backward(acts, dout))


# ------------------------------------------------------------------------------------------- (2)
@pytest.mark.parametrize("n", R.CHUNK_NS)
@pytest.mark.parametrize("cfg", ALL)
def test_chunk_seams(gpu, cfg, n):
    c = _ctx(cfg)
    x, dout = c.x[:n], c.dout[:n]
    acts = R.take(c.base["a64"], torch.arange(n))
    what = f"{_id(cfg)} n={n}"
    dx, grad = _bw(c, x, n, dout)
    _check_bw(what, c, dx, grad, R.backward(acts, c.cpu[1][:n]))
    assert torch.equal(dx, _base_bw(cfg)[0][:n]), "dx of a sample depends on the launch's length"
    if n == 1025:
        # sample 1024 alone: the second chunk's one live row; dW is that sample's outer products
        one = torch.zeros_like(dout)
        one[1024] = dout[1024]
        dx1, g1 = _bw(c, x, n, one)
        ref = R.backward(R.take(c.base["a64"], torch.arange(1024, 1025)), c.cpu[1][1024:1025])
        _check_bw(f"{what} sample 1024 alone", c, dx1[1024:], g1, ref)
        assert bool((dx1[:1024] == 0).all())
        assert torch.equal(dx1[1024], dx[1024])


# ------------------------------------------------------------------------------------------- (3)
@pytest.mark.parametrize("cfg", ALL)
def test_base_block(gpu, cfg):
    c = _ctx(cfg)
    dx, grad = _base_bw(cfg)
    _check_bw(f"{_id(cfg)} n={R.BASE_N}", c, dx, grad, (c.ref_dx, c.ref_dW))
    # grad is added into, not stored: a second call into the same buffer gives twice the sums
    _, twice = _bw(c, c.x, R.BASE_N, c.dout, grad=grad.clone())
    assert float(grad.abs().max()) > 0
    assert torch.allclose(twice, 2 * grad, rtol=1e-6, atol=0)
    # deterministic: chunks are summed in a fixed order
    assert torch.equal(_bw(c, c.x, R.BASE_N, c.dout)[1], grad)


# ------------------------------------------------------------------------------------------- (4)
@pytest.mark.parametrize("cfg", ALL)
def test_fw_two_trips(gpu, cfg):
    c = _ctx(cfg)
    n = c.sizes["two_trip"]
    assert n == R.TRIP + 173
    x, _, rows = _launch(cfg, n)
    out = _fw(c, x, n)
    assert torch.isfinite(out).all(), "a row of out was not written"
    ref = c.ref_y16.double()
    err = (out.double() - ref[rows]).abs().amax(1)
    scale = max(1.0, float(ref.abs().max()))
    print(f"{_id(cfg)} n={n} forward: max error / max(1, max reference) {float(err.max()) / scale:.3e} "
          f"(second trip {float(err[R.TRIP:].max()) / scale:.3e})")
    assert float(err.max()) <= FW_TOL * scale, (float(err.max()), int(err.argmax()))
    # the same sample at any lane, wave, workgroup and trip: the bits of the one-trip launch of the
    # base block alone
    one = _fw(c, c.x, R.BASE_N)
    _check_fw(f"{_id(cfg)} n={R.BASE_N}", one, c.base["y"])
    diff = (out != one[rows]).any(1)
    assert not bool(diff.any()), (int(diff.sum()), int(diff.nonzero()[0]))


# ------------------------------------------------------------------------------------------- (5)
@pytest.mark.parametrize("cfg", TRIP_CFGS)
def test_bw_two_trips(gpu, cfg):
    c = _ctx(cfg)
    n = c.sizes["two_trip"]
    x, dout, rows = _launch(cfg, n)
    dx, grad = _bw(c, x, n, dout)
    assert torch.isfinite(dx).all(), "a row of dx was not written"
    assert torch.isfinite(grad).all(), "an unwritten pad row or slab entry reached grad"
    err = (dx.double() - c.ref_dx[rows]).abs().amax(1) / c.ref_dx.abs().max()
    print(f"{_id(cfg)} n={n} dx: max error / max reference {float(err.max()):.3e} "
          f"(second trip {float(err[R.TRIP:].max()):.3e})")
    assert float(err.max()) < TOL, (float(err.max()), int(err.argmax()))
    diff = (dx != _base_bw(cfg)[0][rows]).any(1)
    assert not bool(diff.any()), (int(diff.sum()), int(diff.nonzero()[0]))


# ------------------------------------------------------------------------------------------- (6)
@pytest.mark.parametrize("region", REGIONS)
@pytest.mark.parametrize("cfg", TRIP_CFGS)
def test_bw_spotlight(gpu, cfg, region):
    c = _ctx(cfg)
    name, launch, lo, hi, start = c.regions[region]
    n = c.sizes[launch]
    x, dout, rows = _launch(cfg, n)
    masked = torch.zeros_like(dout)
    masked[lo:hi] = dout[lo:hi]
    dx, grad = _bw(c, x, n, masked)
    base_rows = rows[lo:hi].cpu()
    ref = R.backward(R.take(c.base["a64"], base_rows), c.cpu[1][base_rows])
    assert torch.allclose(ref[0], c.ref_dx[rows[lo:hi]].cpu(), rtol=1e-12, atol=0)  # (a sample's rows depend on no other)
    assert torch.isfinite(dx).all(), "a row of dx was not written"
    _check_bw(f"{_id(cfg)} {region} [{lo},{hi}) of {n}", c, dx[lo:hi], grad, ref)
    # rows outside the region: written, and exactly zero (no gradient reaches them)
    outside = torch.ones(n, dtype=torch.bool, device=gpu)
    outside[lo:hi] = False
    assert bool((dx[outside] == 0).all())
    # the region's samples launched on their own from a multiple of CH: the same chunks, the same
    # order inside each chunk, the other chunks of the full launch adding exact zeros
    m = hi - start
    dx_a, grad_a = _bw(c, x[start:hi], m, masked[start:hi])
    same_dx, same_grad = torch.equal(dx_a, dx[start:hi]), torch.equal(grad_a, grad)
    print(f"{_id(cfg)} {region}: launched alone, dx bit-equal {same_dx}, grad bit-equal {same_grad}")
    assert same_dx
    assert same_grad, int((grad_a != grad).sum())


# ------------------------------------------------------------------------------------------- (7)
@pytest.mark.parametrize("cfg", SAT_CFGS)
def test_sigmoid_saturation(gpu, cfg):
    W = cfg[0]
    x, params, dout = R.saturation_inputs(W, "bounds")
    n = R.SAT_N
    c = _net(cfg, gpu, params)
    y, acts = R.forward(x, params, *cfg)
    z = acts["z"][:, :3]
    share = float((z.abs() > 15).double().mean())
    print(f"{_id(cfg)} saturation: {share:.3f} of the logits beyond +-15, range [{float(z.min()):.1f}, {float(z.max()):.1f}]")
    assert share >= 0.10
    what = f"{_id(cfg)} saturated n={n}"
    _check_fw(what, _fw(c, x.to(gpu), n), y)
    dx, grad = _bw(c, x.to(gpu), n, dout.to(gpu))
    _check_bw(what, c, dx, grad, R.backward(acts, dout))


@pytest.mark.parametrize("cfg", SAT_CFGS)
def test_sigmoid_overflow(gpu, cfg):
    """Logits past -88.7, where __expf(-z) is inf: y must come out 0 (and 1 - y, y (1 - y) finite), not
    NaN.  At the scale that reaches this the reference's own unsaturated outputs move with its
    summation order by more than the bounds (tests/test_mlp_ref_cpu.py), so only what the order cannot
    move is compared: outputs whose logit lies beyond +-15 (the sigmoid's slope there is below 3.1e-7)
    and dx of the samples whose three live logits all do."""
    W = cfg[0]
    x, params, dout = R.saturation_inputs(W, "overflow")
    n = R.SAT_N
    c = _net(cfg, gpu, params)
    y, acts = R.forward(x, params, *cfg)
    z = acts["z"]
    assert float(z[:, :3].min()) < -88.8 and float(z[:, :3].max()) > 88.8
    out = _fw(c, x.to(gpu), n)
    dx, grad = _bw(c, x.to(gpu), n, dout.to(gpu))
    assert torch.isfinite(out).all() and torch.isfinite(dx).all() and torch.isfinite(grad).all()
    flat = z.abs() > 15
    assert float(flat[:, :3].double().mean()) >= 0.10
    err = float((out.double().cpu() - y.half().double())[flat].abs().max())
    rows = flat[:, :3].all(1)
    ref_dx = R.backward(acts, dout)[0]
    err_dx = float((dx.double().cpu() - ref_dx)[rows].abs().max() / ref_dx.abs().max())
    print(f"{_id(cfg)} overflow n={n}: saturated outputs max error {err:.3e}; dx of the {int(rows.sum())} saturated "
          f"samples max error / max reference {err_dx:.3e}")
    assert int(rows.sum()) > n // 10
    assert err <= FW_TOL and err_dx < TOL


# ------------------------------------------------------------------------------------------- (8)
def _module(gpu, width=64, depth=2, n_in=32, n_out=3, act="Sigmoid", seed=3):
    return tcnn.Network(n_in, n_out, {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": act,
                                      "n_neurons": width, "n_hidden_layers": depth}, seed=seed).to(gpu)


def _module_x(gpu, n=173, n_in=32):
    g = torch.Generator().manual_seed(17)
    return (torch.rand(n, n_in, generator=g) - 0.5).half().to(gpu)


@pytest.mark.parametrize("width,depth,act", [(64, 2, "Sigmoid"), (128, 2, "None")])
def test_module_padded_output_rows_get_no_gradient(gpu, width, depth, act):
    net = _module(gpu, width, depth, act=act)
    x = _module_x(gpu).requires_grad_(True)
    g = torch.Generator().manual_seed(18)
    y = net(x)
    assert y.shape == (173, 3) and y.dtype == torch.float16
    (y.float() * (torch.randn(173, 3, generator=g) * 1e-2).to(gpu)).sum().backward()
    w_out = net.params.grad[-16 * width:].view(16, width)
    assert float(w_out[:3].abs().min(1).values.max()) > 0 and torch.isfinite(net.params.grad).all()
    assert bool((w_out[3:] == 0).all()), "rows 3..15 of the W_out gradient must be exactly zero"
    assert torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0


@pytest.mark.parametrize("update", ["mul_", "adam_step"])
def test_module_repacks_after_an_in_place_update(gpu, update):
    net = _module(gpu)
    x = _module_x(gpu)
    before = net(x).detach().clone()
    if update == "mul_":
        with torch.no_grad():
            net.params.mul_(2)
    else:
        opt = torch.optim.Adam(net.parameters(), lr=1e-2)
        net(x).float().sum().backward()
        opt.step()
    after = net(x).detach()
    fresh = _module(gpu, seed=99)
    with torch.no_grad():
        fresh.params.copy_(net.params)
    assert not torch.equal(after, before), "the forward ran on the stale packed weights"
    assert torch.equal(after, fresh(x).detach())


def test_module_n_zero(gpu):
    net = _module(gpu)
    x = torch.empty(0, 32, dtype=torch.float16, device=gpu, requires_grad=True)
    y = net(x)
    assert y.shape == (0, 3) and y.dtype == torch.float16
    y.float().sum().backward()
    assert net.params.grad is not None and bool((net.params.grad == 0).all())
    assert x.grad.shape == (0, 32)


BAD_NETWORKS = [("width 96", dict(width=96), "width=96"), ("three hidden layers", dict(depth=3), "n_hidden_layers=3"),
                ("n_in 16", dict(n_in=16), "n_in=16"), ("n_out 17", dict(n_out=17), "n_out=17")]


@pytest.mark.parametrize("name,kw,named", BAD_NETWORKS, ids=[b[0].replace(" ", "_") for b in BAD_NETWORKS])
def test_argument_errors_name_the_unsupported_network(gpu, name, kw, named):
    # the module route
    net = _module(gpu, act="None", **kw)
    with pytest.raises(RuntimeError, match="unsupported network|outside MF-NeRF's configuration"):
        net(_module_x(gpu, 33, kw.get("n_in", 32)))
    # the C ABI: refused before anything is launched
    a = dict(n_in=32, width=64, depth=2, n_out=3)
    a.update(kw)
    x = _module_x(gpu, 33, 32)
    buf = torch.zeros(1 << 20, dtype=torch.float16, device=gpu)
    out = torch.full((33, 16), SENTINEL, dtype=torch.float16, device=gpu)
    net_args = (a["n_in"], a["width"], a["depth"], a["n_out"])
    for fn, args in (("mfnerf_mlp_pack", (ptr(buf.float()), *net_args, ptr(buf), stream())),
                     ("mfnerf_mlp_fw", (ptr(x), 33, ptr(buf), *net_args, 0, ptr(out), stream())),
                     ("mfnerf_mlp_bw", (ptr(x), 33, ptr(buf), *net_args, 0, ptr(out), ptr(buf.float()), ptr(buf.float()),
                                        ptr(buf), stream()))):
        with pytest.raises(RuntimeError, match="unsupported network") as e:
            call(fn, *args)
        assert named in str(e.value), str(e.value)
    assert load().mfnerf_mlp_n_params(*net_args) == -1 and load().mfnerf_mlp_packed_bytes(*net_args) == -1
    assert load().mfnerf_mlp_bw_workspace(33, *net_args) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def test_misaligned_dx_is_refused(gpu):
    cfg = (64, 2, "Sigmoid")
    c = _ctx(cfg)
    n = 33
    buf = torch.full((n * 32 + 4,), SENTINEL, device=gpu)
    dx = buf[1:1 + n * 32]
    assert dx.data_ptr() % 16 == 4
    grad = torch.zeros(c.n_params, device=gpu)
    ws = torch.zeros(load().mfnerf_mlp_bw_workspace(n, 32, c.W, c.NH, c.n_out), dtype=torch.uint8, device=gpu)
    with pytest.raises(RuntimeError, match="misaligned buffer"):
        call("mfnerf_mlp_bw", ptr(c.x), n, ptr(c.packed), 32, c.W, c.NH, c.n_out, c.sig, ptr(c.dout), ptr(dx), ptr(grad),
             ptr(ws), stream())
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()) and bool((grad == 0).all())
