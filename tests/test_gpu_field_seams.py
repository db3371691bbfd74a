"""The fused field MLP kernels (csrc/field_fw.hip: field_fw_kernel; csrc/field_bw.hip: field_bw_coop_kernel +
slab_reduce_kernel) at the seams of their persistent loops, against the float64-accumulated reference
of tests/field_ref.py.

The cooperative backward launches G = mfnerf_field_bw_slab_rows(width) workgroups; each takes the
128-sample group g, then g + G, ...  tests/test_gpu_field.py's test_field_bw is the one-pass case.  Here:

  (a) test_bw_small_n           N in {1, 31, 32, 33, 173} against the reference, the slab NaN-filled
  (b) test_bw_two_passes        N2 = G * 128 + 173: the second trip holds a full group (workgroup 0)
                                and, in workgroup 1, a full tile, a 13-sample tile and two idle waves
  (c) test_bw_spotlight         gradients zero outside a region: second_pass, ragged_tile,
                                pass_boundary (groups G - 1 | G); width 128 also third_pass
  (d) test_bw_spotlight         last_group of N = G * 128, last_group_p1 and single_sample of G * 128 + 1
  (e) test_bw_live_count, test_fw_live_count     n_dev < n, NaN in every input past the count
  (f) test_bw_level_l1          the 16 sums mfnerf_field_bw adds into level_l1
  (g) test_bw_as_the_training_step_calls_it      planar features, n_dev, level_l1, device-side scale
  (h) test_fw_two_trips         N = 2048 * 128 + 173: the forward's grid-stride loop repeats

Inputs.  Every launch above 173 samples tiles one base block of 4999 samples (field_ref.BASE_N,
sample i = base sample i mod 4999): a sample recurs at other lane, wave, workgroup and pass
positions and the reference is computed on the base block alone.  With gradients tiled like that a
dropped or doubled group moves a weight gradient by ~0.2 %, below any tolerance, hence the
spotlights: the weight gradients of a launch whose incoming gradients are zero outside a region are
the region's own, compared with the reference summed over the region.

Tolerances (no new numbers).  Against the reference: max|got - ref| / max|ref| < 2e-3, test_field_bw's
measure and bound; forward: test_field_fw's rtol / atol.  The measure means something only where
the reference does not decide an fp16 rounding by its summation order: field_ref.order_sensitivity <
2e-4 for every (N, seed, width, region) used here, asserted on the CPU by tests/test_field_ref_cpu.py.
level_l1: rtol 1e-5 (test_level_l1_any_level_count).  Planar against row-major weight gradients:
rtol 1e-5, atol 1e-6 max (test_planar_encode_and_field_match_row_major).

Bit-equalities, derived from the code: a sample's outputs depend on no other sample and not on its
position (the MFMA column is the sample; no cross-lane reduction on the data path), and a region
launched on its own from a multiple of 128 has the group, wave and lane assignment of the full
launch, the other trips adding exact zeros.  Whether each held on an MI355X is recorded with the
measured errors at the end of this docstring.

Measured on an MI355X (every test prints its figures; order sensitivities from the CPU test):
    case                                   worst of dL_dfeat, gx, gr    order sensitivity
    small N (1, 31, 32, 33; 173)           <= 3.7e-5; 5.3e-5 | 1.2e-4   <= 3.7e-5; 5.3e-5 | 7.6e-5
    two passes, dL_dfeat of every sample   1.7e-4 | 1.7e-4              1.1e-4 | 1.0e-4 (base block)
    second_pass                            1.2e-5 | 3.3e-5              1.2e-5 | 1.2e-4
    ragged_tile                            6.2e-8 | 7.0e-7              1.3e-7 | 2.0e-7
    pass_boundary                          1.2e-5 | 8.6e-5              2.4e-5 | 9.5e-5
    last_group, last_group_p1              3.6e-6 | 8.6e-5              2.8e-5 | 8.6e-5
    single_sample                          7.8e-8 | 1.0e-7              8.8e-8 | 7.6e-8
    third_pass (width 128)                 4.8e-5                       7.3e-5
(width 64 | 128, against the bound 2e-3), level_l1 within 6.9e-7 of the float64 sums (bound 1e-5).
Every bit-equality asserted here held at both widths: dL_dfeat of a sample at any position of the
two-pass launch against the one-pass launch of the base block; gx, gr and dL_dfeat of each region
launched on its own against the spotlight launch; dL_dfeat, gx, gr under a live count against the
launch of the live samples; planar / device-scale dL_dfeat against row-major / host-scale; the
forward's second trip, its live-count call and density_only against the one-trip launch.
"""
import functools
import types

import pytest
import torch

import field_ref as R
from mfnerf import field as FLD
from mfnerf._lib import call, load, ptr, stream
from oracle import field_oracle as FO

pytestmark = pytest.mark.gpu

WIDTHS = (64, 128)
TOL = 2e-3           # test_field_bw: max error / max reference
L1_RTOL = 1e-5       # test_level_l1_any_level_count
NAN = float("nan")
REGIONS = ("second_pass", "ragged_tile", "pass_boundary", "last_group", "last_group_p1", "single_sample")
SPOTLIGHTS = [(w, r) for w in WIDTHS for r in REGIONS] + [(128, "third_pass")]


@functools.lru_cache(maxsize=None)
def _ctx(width):
    """Per width: G, the base block on the device, its packed weights, its reference (computed once)."""
    dev = torch.device("cuda:0")
    G = load().mfnerf_field_bw_slab_rows(width)
    assert G > 0
    b = R.base_block(width)
    feat, dirs, px, pr, dsig, drgb = b["inputs"]
    c = types.SimpleNamespace(width=width, G=G, dev=dev, base=b, cpu=(feat, dirs, dsig, drgb),
                              packed=FLD.pack_field_weights(px.to(dev), pr.to(dev), width),
                              gpu=tuple(t.to(dev) for t in (feat, dirs, dsig, drgb)),
                              ref=R.backward(b["a64"], dsig, drgb), sizes=R.launch_sizes(G, width),
                              regions={r[0]: r for r in R.regions(G, width)})
    return c


@functools.lru_cache(maxsize=None)
def _launch(width, n):
    """(feat, dirs, dL_dsigma, dL_drgb) of a launch of n samples tiling the base block, and the base rows."""
    c = _ctx(width)
    rows = R.tile_rows(n).to(c.dev)
    return tuple(t[rows].contiguous() for t in c.gpu), rows


def _amp(dev, scale=R.S):
    """A zeroed mfnerf_amp_state (8 words) with `scale` set; word 0 is the non-finite flag."""
    amp = torch.zeros(8, dtype=torch.int32, device=dev)
    amp[2:3].view(torch.float32).fill_(scale)
    return amp


def _bw(c, feat, dirs, n, dsig, drgb, n_dev=None, level_l1=None, stride=0, device_scale=False):
    """mfnerf_field_bw over the C ABI with a NaN-filled dL_dfeat and slab: an unwritten row of
    either shows (an idle workgroup must still write its slab row, or the fold turns gx / gr NaN)."""
    dfeat = torch.full((n, 32), NAN, device=c.dev)
    gx, gr = torch.zeros(3072, device=c.dev), torch.zeros(R.rgb_net_params(c.width), device=c.dev)
    ws = FLD.field_bw_workspace(n, c.width, c.dev).fill_(NAN)
    amp = _amp(c.dev)
    call("mfnerf_field_bw", ptr(feat), stride, ptr(dirs), n, ptr(n_dev), ptr(c.packed), c.width, ptr(dsig), ptr(drgb),
         0.0 if device_scale else R.S, ptr(dfeat), ptr(gx), ptr(gr), ptr(ws), ptr(amp), ptr(level_l1), stream())
    torch.cuda.synchronize()
    return dfeat, gx, gr, int(amp[0])


def _err(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


def _check(what, got, ref):
    err = _err(got, ref)
    print(f"{what}: max error / max reference {err:.3e}")
    assert err < TOL, (what, err)


# ------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("N", R.SMALL_NS)
@pytest.mark.parametrize("width", WIDTHS)
def test_bw_small_n(gpu, width, N):
    c = _ctx(width)
    feat, dirs, px, pr, dsig, drgb = R.seam_inputs(N, R.SMALL_SEED[width], width)
    _, _, acts = R.forward(feat, dirs, px, pr, width)
    ref = R.backward(acts, dsig, drgb)
    c1 = types.SimpleNamespace(width=width, dev=gpu, packed=FLD.pack_field_weights(px.to(gpu), pr.to(gpu), width))
    dfeat, gx, gr, flag = _bw(c1, feat.to(gpu), dirs.to(gpu), N, dsig.to(gpu), drgb.to(gpu))
    assert flag == 0 and c.G * 128 > N
    for name, got, r in zip(("dL_dfeat", "gx", "gr"), (dfeat, gx, gr), ref):
        assert torch.isfinite(got).all(), name
        _check(f"W={width} N={N} {name}", got, r)


# ------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("width", WIDTHS)
def test_bw_two_passes(gpu, width):
    c = _ctx(width)
    n = c.sizes["two_pass"]
    assert n == c.G * 128 + 173
    (feat, dirs, dsig, drgb), rows = _launch(width, n)
    dfeat, gx, gr, flag = _bw(c, feat, dirs, n, dsig, drgb)
    assert flag == 0
    assert torch.isfinite(dfeat).all(), "a row of dL_dfeat was not written"
    assert torch.isfinite(gx).all() and torch.isfinite(gr).all()
    ref = c.ref[0]
    err = (dfeat.double().cpu() - ref[rows.cpu()]).abs().amax(1) / ref.abs().max()
    second = err[c.G * 128:]
    print(f"W={width} N={n} dL_dfeat: max error / max reference {float(err.max()):.3e} "
          f"(second pass {float(second.max()):.3e})")
    assert float(err.max()) < TOL, (float(err.max()), int(err.argmax()))
    # the same sample at any lane, wave, workgroup and pass: the bits of the one-pass launch of the
    # base block alone
    one = _bw(c, *c.gpu[:2], R.BASE_N, *c.gpu[2:])[0]
    diff = (dfeat != one[rows]).any(1)
    assert not bool(diff.any()), (int(diff.sum()), int(diff.nonzero()[0]))


# -------------------------------------------------------------------------------------- (c), (d)
@pytest.mark.parametrize("width,region", SPOTLIGHTS)
def test_bw_spotlight(gpu, width, region):
    c = _ctx(width)
    name, launch, lo, hi, start = c.regions[region]
    n = c.sizes[launch]
    (feat, dirs, dsig, drgb), rows = _launch(width, n)
    ms, mc = torch.zeros_like(dsig), torch.zeros_like(drgb)
    ms[lo:hi], mc[lo:hi] = dsig[lo:hi], drgb[lo:hi]
    dfeat, gx, gr, flag = _bw(c, feat, dirs, n, ms, mc)
    assert flag == 0
    base_rows = rows[lo:hi].cpu()
    cf, cd, cs, cc = c.cpu
    ref = R.backward(R.take(c.base["a64"], base_rows), cs[base_rows], cc[base_rows])
    assert torch.allclose(ref[0], c.ref[0][base_rows], rtol=1e-12, atol=0)  # (a sample's rows depend on no other)
    _check(f"W={width} {region} [{lo},{hi}) of {n} dL_dfeat", dfeat[lo:hi], ref[0])
    _check(f"W={width} {region} [{lo},{hi}) of {n} gx", gx, ref[1])
    _check(f"W={width} {region} [{lo},{hi}) of {n} gr", gr, ref[2])
    # rows outside the region: written, and exactly zero (no gradient reaches them)
    outside = torch.ones(n, dtype=torch.bool, device=gpu)
    outside[lo:hi] = False
    assert bool((dfeat[outside] == 0).all())
    # the region's samples launched on their own from a multiple of 128: the same groups, waves and
    # lanes, the same slab rows' worth of non-zero partials folded in the same fixed order
    m = hi - start
    alone = _bw(c, feat[start:hi], dirs[start:hi], m, ms[start:hi], mc[start:hi])
    assert alone[3] == 0
    assert torch.equal(alone[0], dfeat[start:hi])
    assert torch.equal(alone[1], gx), int((alone[1] != gx).sum())
    assert torch.equal(alone[2], gr), int((alone[2] != gr).sum())


# ------------------------------------------------------------------------------------------- (e)
def _poisoned(t, k):
    t = t.clone()
    t[k:] = NAN
    return t


@pytest.mark.parametrize("width", WIDTHS)
def test_bw_live_count(gpu, width):
    c = _ctx(width)
    n = c.sizes["two_pass"]
    k = n - 77
    (feat, dirs, dsig, drgb), _ = _launch(width, n)
    n_dev = torch.tensor([k], dtype=torch.int32, device=gpu)
    l1 = torch.zeros(16, device=gpu)
    dfeat, gx, gr, flag = _bw(c, _poisoned(feat, k), _poisoned(dirs, k), n, _poisoned(dsig, k), _poisoned(drgb, k),
                              n_dev=n_dev, level_l1=l1)
    assert flag == 0, "a sample past the live count reached the non-finite flag"
    assert bool(torch.isnan(dfeat[k:]).all()), "dL_dfeat written past the live count"
    assert torch.isfinite(dfeat[:k]).all()
    l1b = torch.zeros(16, device=gpu)
    live = _bw(c, feat[:k], dirs[:k], k, dsig[:k], drgb[:k], level_l1=l1b)
    assert torch.equal(dfeat[:k], live[0])
    assert torch.equal(gx, live[1]) and torch.equal(gr, live[2])
    assert float(l1.min()) > 0 and torch.allclose(l1, l1b, rtol=L1_RTOL, atol=0)


@pytest.mark.parametrize("width", WIDTHS)
def test_fw_live_count(gpu, width):
    c = _ctx(width)
    n, k = 173, 100
    feat, dirs = c.gpu[0][:n].contiguous(), c.gpu[1][:n].contiguous()
    s0, c0 = FLD.field_fw(feat, dirs, n, c.packed, width)
    n_dev = torch.tensor([k], dtype=torch.int32, device=gpu)
    fp, dp = _poisoned(feat, k), _poisoned(dirs, k)
    s1, c1 = FLD.field_fw(fp, dp, n, c.packed, width, n_dev=n_dev, sigma=torch.full((n,), -7.0, device=gpu),
                          rgb=torch.full((n, 3), -7.0, device=gpu))
    sd, _ = FLD.field_fw(fp, None, n, c.packed, width, density_only=True, n_dev=n_dev,
                         sigma=torch.full((n,), -7.0, device=gpu))
    torch.cuda.synchronize()
    assert bool((s1[k:] == -7.0).all()) and bool((c1[k:] == -7.0).all()) and bool((sd[k:] == -7.0).all())
    assert torch.equal(s1[:k], s0[:k]) and torch.equal(c1[:k], c0[:k]) and torch.equal(sd[:k], s0[:k])
    assert torch.isfinite(s0).all() and torch.isfinite(c0).all()


# ------------------------------------------------------------------------------------------- (f)
@pytest.mark.parametrize("case", ["n33", "two_pass_live_count"])
@pytest.mark.parametrize("width", WIDTHS)
def test_bw_level_l1(gpu, width, case):
    c = _ctx(width)
    if case == "n33":
        n = k = 33
        feat, dirs, dsig, drgb = (t[:n].contiguous() for t in c.gpu)
        n_dev = None
    else:
        n = c.sizes["two_pass"]
        k = n - 77
        (feat, dirs, dsig, drgb), _ = _launch(width, n)
        n_dev = torch.tensor([k], dtype=torch.int32, device=gpu)
    l1 = torch.zeros(16, device=gpu)
    dfeat, _, _, flag = _bw(c, feat, dirs, n, dsig, drgb, n_dev=n_dev, level_l1=l1)
    assert flag == 0
    ref = R.level_l1_ref(dfeat[:k].cpu())
    assert float(ref.min()) > 0
    got = l1.double().cpu()
    print(f"W={width} {case}: level_l1 max relative error {float(((got - ref).abs() / ref).max()):.3e}")
    assert torch.allclose(got, ref, rtol=L1_RTOL, atol=0)
    # mfnerf_grid_level_l1 of the buffer the call wrote (the step's other way to the same 16 sums)
    sep = torch.zeros(16, device=gpu)
    call("mfnerf_grid_level_l1", ptr(dfeat), n, ptr(n_dev), 16, ptr(sep), stream())
    torch.cuda.synchronize()
    assert torch.allclose(sep.double().cpu(), ref, rtol=L1_RTOL, atol=0)
    assert torch.allclose(l1, sep, rtol=L1_RTOL, atol=0)
    # level_l1 is added into, not stored: a second call without zeroing gives twice the sums
    _bw(c, feat, dirs, n, dsig, drgb, n_dev=n_dev, level_l1=l1)
    assert torch.allclose(l1.double().cpu(), 2 * ref, rtol=L1_RTOL, atol=0)


# ------------------------------------------------------------------------------------------- (g)
@pytest.mark.parametrize("width", WIDTHS)
def test_bw_as_the_training_step_calls_it(gpu, width):
    """Planar features (plane stride cap > n), the device live count, level_l1 and the loss scale read
    from the amp state, together, at two passes -- against the row-major call with the host's scale."""
    c = _ctx(width)
    n = c.sizes["two_pass"]
    k, cap = n - 77, n + 51
    (feat, dirs, dsig, drgb), _ = _launch(width, n)
    planes = torch.full((16, cap, 2), NAN, dtype=torch.float16, device=gpu)
    planes[:, :n] = feat.view(n, 16, 2).permute(1, 0, 2)
    n_dev = torch.tensor([k], dtype=torch.int32, device=gpu)
    l1r, l1p = torch.zeros(16, device=gpu), torch.zeros(16, device=gpu)
    row = _bw(c, feat, dirs, n, dsig, drgb, n_dev=n_dev, level_l1=l1r)
    pla = _bw(c, planes, dirs, n, dsig, drgb, n_dev=n_dev, level_l1=l1p, stride=cap, device_scale=True)
    assert row[3] == 0 and pla[3] == 0
    assert torch.isfinite(row[0][:k]).all()
    assert torch.equal(pla[0][:k], row[0][:k])
    assert bool(torch.isnan(pla[0][k:]).all()) and bool(torch.isnan(row[0][k:]).all())
    for a, b in zip(pla[1:3], row[1:3]):
        assert float(b.abs().max()) > 0
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6 * float(b.abs().max()))
    assert float(l1r.min()) > 0 and torch.allclose(l1p, l1r, rtol=L1_RTOL, atol=0)


# ------------------------------------------------------------------------------------------- (h)
@pytest.mark.parametrize("width", WIDTHS)
def test_fw_two_trips(gpu, width):
    c = _ctx(width)
    # launch_fw (csrc/field_fw.hip) caps the grid at 2048 workgroups of 4 tiles of 32 samples: the
    # grid-stride loop of field_fw_kernel takes a second trip only past 2048 * 128 samples
    n = 2048 * 128 + 173
    rows = R.tile_rows(n).to(gpu)
    feat, dirs = c.gpu[0][rows].contiguous(), c.gpu[1][rows].contiguous()
    s, col = FLD.field_fw(feat, dirs, n, c.packed, width, sigma=torch.full((n,), NAN, device=gpu),
                          rgb=torch.full((n, 3), NAN, device=gpu))
    bf, bd, px, pr = c.base["inputs"][:4]
    s_ref, c_ref, _ = FO.ngp_field_fw16(bf, bd, px, pr, width)
    r = rows.cpu()
    # test_field_fw's bounds
    assert torch.allclose(s.cpu(), s_ref[r], rtol=4e-3, atol=1e-6)
    assert torch.allclose(col.cpu(), c_ref[r], atol=2e-3, rtol=0)
    s1, c1 = FLD.field_fw(c.gpu[0], c.gpu[1], R.BASE_N, c.packed, width)
    assert torch.equal(s, s1[rows]) and torch.equal(col, c1[rows])
    sd, _ = FLD.field_fw(feat, None, n, c.packed, width, density_only=True, sigma=torch.full((n,), NAN, device=gpu))
    assert torch.equal(sd, s)
