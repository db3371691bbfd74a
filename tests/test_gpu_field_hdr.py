"""The field kernels without the output sigmoid (csrc/field_fw.hip's and field_bw.hip's LOGRAD instantiations:
mfnerf_field_fw_lograd, mfnerf_field_bw_lograd, mfnerf_field_bw_inputs_lograd) against the float64
reference tests/field_hdr_ref.py, at both widths, with row-major and with planar features.

Forward: N in {1, 31, 32, 33, 173} and a live count below N (NaN in every input past it, the sentinel
past it preserved).  sigma is torch.equal to mfnerf_field_fw's on the same inputs (the code is shared up
to the epilogue); the log-radiance is within test_field_fw's atol / rtol (2e-3 / 0) of the reference.
Backward: the same small N with a NaN-filled slab; one two-pass launch G * 128 + 173 tiling the
4999-sample base block; the ragged_tile and pass_boundary spotlights; the live count.  Against the
reference: max|got - ref| / max|ref| < 2e-3, test_field_bw's measure and bound; dL_ddirs of the _inputs
form under the same measure and bound (tests/test_gpu_input_grad.py).  The measure's precondition (the
reference decides no fp16 rounding by its summation order) is asserted for every input used here by
tests/test_field_hdr_ref_cpu.py.  Bit-equalities are test_gpu_field_seams.py's, for the same reasons.

Measured on an MI355X (every test prints its figures), width 64 | 128, row-major = planar to the bit:
log-radiance error 0 | <= 1.5e-5 (N = 173) at |log-radiance| <= 0.51; backward, worst of dL_dfeat, gx,
gr: small N <= 3.8e-5; two passes 8.3e-5 | 2.1e-4; ragged_tile 3.8e-4 | 9.4e-8; pass_boundary 3.0e-5 |
4.0e-5; dL_ddirs <= 6.0e-7 -- against the bound 2e-3.  Every bit-equality asserted here held.
"""
import functools
import types

import pytest
import torch

import field_hdr_ref as H
import field_ref as R
import input_grad_ref as IR
from mfnerf import field as FLD
from mfnerf._lib import call, load, ptr, stream

pytestmark = pytest.mark.gpu

WIDTHS = (64, 128)
LAYOUTS = ("rows", "planar")
TOL = 2e-3           # test_field_bw / test_field_bw_inputs: max error / max reference
NAN = float("nan")
PAD = 51             # planar: the plane stride exceeds n by this


def _features(feat, layout):
    """(buffer, plane stride) of (n,32) f16 features: row-major, or level planes (16, n + PAD) half2
    with NaN in the padding."""
    if layout == "rows":
        return feat.contiguous(), 0
    n = feat.shape[0]
    planes = torch.full((16, n + PAD, 2), NAN, dtype=torch.float16, device=feat.device)
    planes[:, :n] = feat.view(n, 16, 2).permute(1, 0, 2)
    return planes, n + PAD


@functools.lru_cache(maxsize=None)
def _ctx(width):
    dev = torch.device("cuda:0")
    G = load().mfnerf_field_bw_slab_rows(width)
    b = H.base_block(width)
    feat, dirs, px, pr, dsig, dlog = b["inputs"]
    return types.SimpleNamespace(width=width, G=G, dev=dev, base=b, cpu=(feat, dirs, dsig, dlog),
                                 packed=FLD.pack_field_weights(px.to(dev), pr.to(dev), width),
                                 gpu=tuple(t.to(dev) for t in (feat, dirs, dsig, dlog)),
                                 ref=H.backward(b["a64"], dsig, dlog), n2=R.launch_sizes(G, width)["two_pass"],
                                 regions={r[0]: r for r in R.regions(G, width)})


@functools.lru_cache(maxsize=None)
def _launch(width, n):
    c = _ctx(width)
    rows = R.tile_rows(n).to(c.dev)
    return tuple(t[rows].contiguous() for t in c.gpu), rows


def _amp(dev, scale=R.S):
    amp = torch.zeros(8, dtype=torch.int32, device=dev)
    amp[2:3].view(torch.float32).fill_(scale)
    return amp


def _bw(c, feat, dirs, n, dsig, dlog, n_dev=None, layout="rows", ddirs=False):
    """mfnerf_field_bw_lograd (or the _inputs form) with NaN-filled dL_dfeat, dL_ddirs and slab."""
    buf, stride = _features(feat, layout)
    dfeat = torch.full((n, 32), NAN, device=c.dev)
    gx, gr = torch.zeros(3072, device=c.dev), torch.zeros(R.rgb_net_params(c.width), device=c.dev)
    ws = FLD.field_bw_workspace(n, c.width, c.dev).fill_(NAN)
    amp = _amp(c.dev)
    args = (ptr(buf), stride, ptr(dirs), n, ptr(n_dev), ptr(c.packed), c.width, ptr(dsig), ptr(dlog), R.S, ptr(dfeat),
            ptr(gx), ptr(gr), ptr(ws), ptr(amp), None)
    dd = None
    if ddirs:
        dd = torch.full((n, 3), NAN, device=c.dev)
        call("mfnerf_field_bw_inputs_lograd", *args, ptr(dd), stream())
    else:
        call("mfnerf_field_bw_lograd", *args, stream())
    torch.cuda.synchronize()
    return dfeat, gx, gr, int(amp[0]), dd


def _check(what, got, ref):
    err = float((got.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"{what}: max error / max reference {err:.3e}")
    assert err < TOL, (what, err)


def _small(width, N, dev):
    feat, dirs, px, pr, dsig, dlog = R.seam_inputs(N, H.SMALL_SEED[width], width)
    c = types.SimpleNamespace(width=width, dev=dev, packed=FLD.pack_field_weights(px.to(dev), pr.to(dev), width))
    return c, (feat, dirs, px, pr, dsig, dlog)


# ---------------------------------------------------------------------------- forward
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("N", R.SMALL_NS)
@pytest.mark.parametrize("width", WIDTHS)
def test_fw_small_n(gpu, width, N, layout):
    c, (feat, dirs, px, pr, _, _) = _small(width, N, gpu)
    s_ref, l_ref, _ = H.forward(feat, dirs, px, pr, width)
    buf, stride = _features(feat.to(gpu), layout)
    s, lg = FLD.field_fw_lograd(buf, dirs.to(gpu), N, c.packed, width, plane_stride=stride)
    assert lg.dtype == torch.float16 and lg.shape == (N, 3)
    s0, _ = FLD.field_fw(feat.to(gpu), dirs.to(gpu), N, c.packed, width)
    assert torch.equal(s, s0), "sigma differs from mfnerf_field_fw's"
    # test_field_fw's bounds
    assert torch.allclose(s.cpu().double(), s_ref, rtol=4e-3, atol=1e-6)
    err = float((lg.cpu().double() - l_ref).abs().max())
    print(f"W={width} N={N} {layout}: log-radiance max error {err:.3e} (max |ref| {float(l_ref.abs().max()):.3f})")
    assert torch.allclose(lg.cpu().double(), l_ref, atol=2e-3, rtol=0)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("width", WIDTHS)
def test_fw_live_count(gpu, width, layout):
    c = _ctx(width)
    n, k = 173, 100
    feat, dirs = c.gpu[0][:n].contiguous(), c.gpu[1][:n].contiguous()
    s0, l0 = FLD.field_fw_lograd(feat, dirs, n, c.packed, width)
    fp, dp = feat.clone(), dirs.clone()
    fp[k:], dp[k:] = NAN, NAN
    buf, stride = _features(fp, layout)
    n_dev = torch.tensor([k], dtype=torch.int32, device=gpu)
    s1, l1 = FLD.field_fw_lograd(buf, dp, n, c.packed, width, n_dev=n_dev, plane_stride=stride,
                                 sigma=torch.full((n,), -7.0, device=gpu),
                                 lograd=torch.full((n, 3), -7.0, dtype=torch.float16, device=gpu))
    torch.cuda.synchronize()
    assert bool((s1[k:] == -7.0).all()) and bool((l1[k:] == -7.0).all()), "written past the live count"
    assert torch.equal(s1[:k], s0[:k]) and torch.equal(l1[:k], l0[:k])
    assert torch.isfinite(s0).all() and torch.isfinite(l0.float()).all()
    assert torch.allclose(l0.cpu().double(), c.base["lograd"][:n], atol=2e-3, rtol=0)


# ---------------------------------------------------------------------------- backward
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("N", R.SMALL_NS)
@pytest.mark.parametrize("width", WIDTHS)
def test_bw_small_n(gpu, width, N, layout):
    c, (feat, dirs, px, pr, dsig, dlog) = _small(width, N, gpu)
    _, _, acts = H.forward(feat, dirs, px, pr, width)
    ref = H.backward(acts, dsig, dlog)
    dd_ref = IR.ddirs_from_dsh(dirs, H.dsh(acts, dlog))
    a = (feat.to(gpu), dirs.to(gpu), N, dsig.to(gpu), dlog.to(gpu))
    dfeat, gx, gr, flag, _ = _bw(c, *a, layout=layout)
    assert flag == 0
    for name, got, r in zip(("dL_dfeat", "gx", "gr"), (dfeat, gx, gr), ref):
        assert torch.isfinite(got).all(), name
        _check(f"W={width} N={N} {layout} {name}", got, r)
    # the _inputs form: everything above bit for bit, and the direction gradient
    dfeat2, gx2, gr2, flag2, dd = _bw(c, *a, layout=layout, ddirs=True)
    assert flag2 == 0 and torch.equal(dfeat2, dfeat) and torch.equal(gx2, gx) and torch.equal(gr2, gr)
    assert torch.isfinite(dd).all()
    _check(f"W={width} N={N} {layout} dL_ddirs", dd, dd_ref)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("width", WIDTHS)
def test_bw_two_passes(gpu, width, layout):
    c = _ctx(width)
    n = c.n2
    assert n == c.G * 128 + 173
    (feat, dirs, dsig, dlog), rows = _launch(width, n)
    dfeat, gx, gr, flag, _ = _bw(c, feat, dirs, n, dsig, dlog, layout=layout)
    assert flag == 0
    assert torch.isfinite(dfeat).all(), "a row of dL_dfeat was not written"
    assert torch.isfinite(gx).all() and torch.isfinite(gr).all()
    ref = c.ref[0]
    err = (dfeat.double().cpu() - ref[rows.cpu()]).abs().amax(1) / ref.abs().max()
    print(f"W={width} N={n} {layout} dL_dfeat: max error / max reference {float(err.max()):.3e} "
          f"(second pass {float(err[c.G * 128:].max()):.3e})")
    assert float(err.max()) < TOL, (float(err.max()), int(err.argmax()))
    # the same sample at any lane, wave, workgroup and pass: the bits of the one-pass launch of the base block
    one = _bw(c, *c.gpu[:2], R.BASE_N, *c.gpu[2:])[0]
    assert torch.equal(dfeat, one[rows])


@pytest.mark.parametrize("region", H.REGIONS)
@pytest.mark.parametrize("width", WIDTHS)
def test_bw_spotlight(gpu, width, region):
    c = _ctx(width)
    _, launch, lo, hi, start = c.regions[region]
    assert launch == "two_pass"
    n = c.n2
    (feat, dirs, dsig, dlog), rows = _launch(width, n)
    ms, mc = torch.zeros_like(dsig), torch.zeros_like(dlog)
    ms[lo:hi], mc[lo:hi] = dsig[lo:hi], dlog[lo:hi]
    dfeat, gx, gr, flag, _ = _bw(c, feat, dirs, n, ms, mc)
    assert flag == 0
    base_rows = rows[lo:hi].cpu()
    _, _, cs, cc = c.cpu
    ref = H.backward(R.take(c.base["a64"], base_rows), cs[base_rows], cc[base_rows])
    _check(f"W={width} {region} [{lo},{hi}) of {n} dL_dfeat", dfeat[lo:hi], ref[0])
    _check(f"W={width} {region} [{lo},{hi}) of {n} gx", gx, ref[1])
    _check(f"W={width} {region} [{lo},{hi}) of {n} gr", gr, ref[2])
    outside = torch.ones(n, dtype=torch.bool, device=gpu)
    outside[lo:hi] = False
    assert bool((dfeat[outside] == 0).all())
    # the region launched on its own from a multiple of 128: the same groups, waves, lanes and fold
    alone = _bw(c, feat[start:hi], dirs[start:hi], hi - start, ms[start:hi], mc[start:hi])
    assert alone[3] == 0 and torch.equal(alone[0], dfeat[start:hi])
    assert torch.equal(alone[1], gx) and torch.equal(alone[2], gr)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("width", WIDTHS)
def test_bw_live_count(gpu, width, layout):
    c = _ctx(width)
    n = c.n2
    k = n - 77
    (feat, dirs, dsig, dlog), _ = _launch(width, n)

    def poisoned(t):
        t = t.clone()
        t[k:] = NAN
        return t
    n_dev = torch.tensor([k], dtype=torch.int32, device=gpu)
    dfeat, gx, gr, flag, dd = _bw(c, poisoned(feat), poisoned(dirs), n, poisoned(dsig), poisoned(dlog), n_dev=n_dev,
                                  layout=layout, ddirs=True)
    assert flag == 0, "a sample past the live count reached the non-finite flag"
    assert bool(torch.isnan(dfeat[k:]).all()) and bool(torch.isnan(dd[k:]).all()), "written past the live count"
    live = _bw(c, feat[:k], dirs[:k], k, dsig[:k], dlog[:k], layout=layout, ddirs=True)
    assert torch.equal(dfeat[:k], live[0]) and torch.equal(dd[:k], live[4])
    assert torch.equal(gx, live[1]) and torch.equal(gr, live[2])
