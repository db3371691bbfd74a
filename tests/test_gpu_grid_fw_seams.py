"""The hash-grid forward (csrc/grid_fw.hip: grid_fw_kernel and grid_fw_planar_kernel) at its gather
seams, to one fp16 rounding: every output inside [rn16(ref - e), rn16(ref + e)] of the fp64 reference
with e = 12 x 2^-24 x sum |w f| (tests/grid_fw_ref.py derives it; nothing is measured, nothing is
scaled by a tensor's maximum).  tests/test_grid_fw_ref_cpu.py proves on the host that a faithful fp32
emulation of the kernels lies inside this bound, that four wrong kernels lie outside it, and that the
inputs used here reach every class of row planar_gather distinguishes.

Every comparison runs the row-major and the planar kernel, asserts their outputs equal bit for bit,
checks the bound, and asserts that everything past the live count -- rows of the row-major output,
entries [live, plane_stride) of every plane -- still holds the NaN bits it was filled with.

On an MI355X, per case as check() prints them (the host emulation gives the same figures; the
grid-stride case's are identical to five digits):
  * outputs bit-equal to rn16(ref): 0.99963 .. 0.99990 on the U(-0.5, 0.5) table at >= 4000 outputs
    (0.99901 .. 0.99952 at the 1008 .. 2080 outputs of the 63 .. 65-point cases: one or two outputs),
    0.99979 .. 0.99988 on the wide-range table, 0.99995 .. 0.99999 on the initial table;
  * outputs whose interval holds more than one fp16 value: 1.4 % .. 2.4 % on the U(-0.5, 0.5) table
    (1.557 % of the grid-stride case's 16,785,504), 0.8 % .. 0.9 % on the wide-range table, 0.11 % ..
    0.15 % on the initial table;
  * the initial table: 62,008 .. 62,307 of 65,584 (L = 8) and 124,513 .. 124,673 of 131,168 (L = 16)
    outputs are non-zero fp16 subnormals with a one-value interval, every one returned bit for bit.
Nothing failed on the first run: no kernel change came out of this suite.
"""
import ctypes

import numpy as np
import pytest
import torch

import grid_fw_ref as FW
import grid_seam_ref as GS
import input_grad_ref as IG
from mfnerf._lib import load, ptr, stream

pytestmark = pytest.mark.gpu

OK, INVALID = 0, 1
_GEO, _REF = {}, {}


def _ref(name, olay, x01, table, tag, kind):
    """(ref, A) of a case, the geometry computed once per (layout, points) and shared by its tables."""
    if (name, tag) not in _GEO:
        _GEO[name, tag] = FW.geometry(olay, x01)
    if (name, tag, kind) not in _REF:
        _REF[name, tag, kind] = FW.forward_ref(x01, table, olay, _GEO[name, tag])
    return _REF[name, tag, kind]


def _fill_kept(t):
    return bool((t.view(torch.int16) == FW.NAN16).all())


def _run(gpu, lay, x, t16, n_dev=None, x_min=0.0, x_range=1.0, stride=None, desc=None):
    """Both kernels over the cap = x.shape[0] points, the live count min(cap, n_dev) read from the
    device where given -> the live rows (live, L*F) f16 on the host.  The outputs are NaN-filled first,
    the row-major one four rows longer than cap, the planes plane_stride > cap apart."""
    cap, L = x.shape[0], lay.L
    live = cap if n_dev is None else min(cap, n_dev)
    stride = stride or (cap + 127) // 128 * 128 + 128
    assert stride > cap
    desc = desc or lay.desc()
    xg, tg = x.to(gpu).contiguous(), t16.to(gpu)
    nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=gpu)
    out = torch.full((cap + 4, 2 * L), float("nan"), dtype=torch.float16, device=gpu)
    planes = torch.full((L, stride, 2), float("nan"), dtype=torch.float16, device=gpu)
    lib = load()
    st = lib.mfnerf_grid_encode_fw(ptr(xg), cap, ptr(nd), x_min, x_range, desc, ptr(tg), ptr(out), stream())
    assert st == OK, lib.mfnerf_last_error()
    st = lib.mfnerf_grid_encode_fw_planar(ptr(xg), cap, ptr(nd), x_min, x_range, desc, ptr(tg), ptr(planes), stride,
                                          stream())
    assert st == OK, lib.mfnerf_last_error()
    torch.cuda.synchronize()
    assert _fill_kept(out[live:]), "row-major: rows past the live count written"
    assert _fill_kept(planes[:, live:]), "planar: plane entries past the live count written"
    row = out[:live]
    pl = planes[:, :live].permute(1, 0, 2).reshape(live, 2 * L)
    if not torch.equal(row.view(torch.int16), pl.view(torch.int16)):
        bad = torch.nonzero(row.view(torch.int16) != pl.view(torch.int16))
        i, j = (int(v) for v in bad[0])
        raise AssertionError(f"planar != row-major at {bad.shape[0]} outputs; first: sample {i} level {j // 2} feature "
                             f"{j % 2} planar {float(pl[i, j])!r} row-major {float(row[i, j])!r}")
    return row.cpu()


def _compare(gpu, name, x, kind, tag, what, n_dev=None, x_min=0.0, x_range=1.0, stride=None, seed=31):
    lay, olay = FW.layouts(name)
    table = FW.table16(kind, lay.n_params, seed=seed)
    x01 = IG.normalise(x, x_min, x_range)
    assert float(x01.min()) >= 0.0 and float(x01.max()) <= 1.0
    ref, A = _ref(name, olay, x01, table, tag, kind)
    got = _run(gpu, lay, x, table, n_dev=n_dev, x_min=x_min, x_range=x_range, stride=stride)
    live = got.shape[0]
    FW.check(got, ref[:live], A[:live], what, olay, x01)
    return got.numpy(), ref[:live], A[:live]


# ------------------------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("kind", FW.TABLES)
@pytest.mark.parametrize("name", FW.LAYOUT_CASES)
def test_layouts(gpu, name, kind):
    """4099 points with the cube's corners on the suite's real-scene layouts and on odd_tables (tables
    of 67 .. 1021, 2 and 3 entries at odd entry offsets: the clamped load, i0 == i1), with tables of
    U(-0.5, 0.5), tcnn's initial U(-1e-4, 1e-4) and randn x 2^[-8, 4].  The initial table's outputs lie at
    and below fp16's smallest normal: subnormal outputs must come out as the reference's, not as zeros."""
    got, ref, A = _compare(gpu, name, FW.layout_points(), kind, "layout", f"layout {name} {kind}")
    if kind != "init":
        return
    lo, hi, _ = FW.interval(ref, A)
    r16 = ref.astype(np.float16)
    sub = (r16 != 0) & (np.abs(r16.astype(np.float32)) < 2.0 ** -14) & (lo == hi)
    print(f"layout {name} init: {int(sub.sum())} of {sub.size} outputs are non-zero fp16 subnormals")
    assert int(sub.sum()) > 0
    assert bool((got[sub] != 0).all()), "subnormal outputs flushed to zero"
    assert np.array_equal(got[sub].view(np.int16), r16[sub].view(np.int16))


# ---------------------------------------------------------------------------------------- spotlights
@pytest.mark.parametrize("name", ["C", "D", "E", "F", "G", "H"])
def test_spotlights(gpu, name):
    """The table-gradient suite's spotlight points (the 2^k - 1 cells, the canonical steps 1, 2 and 3 of
    the shared tables, resolutions above 1025) through the forward."""
    _compare(gpu, name, GS.spot_case(name).x, "unit", "spot", f"spotlights {name}")


# -------------------------------------------------------------------------------------- level counts
@pytest.mark.parametrize("name", FW.LEVEL_CASES)
def test_level_counts(gpu, name):
    """L = 4, 8, 12, 20 and 32 at N = 1027: the planar kernel's la / 15 - grp pairing without a level b
    (L = 4, 8; 12 on four groups) and its second j iteration (20, 32) store every level exactly once --
    a plane left untouched would still hold NaN and fail the bound."""
    x = GS.random_points(1027, seed=9)
    got, _, _ = _compare(gpu, name, x, "unit", "levels", f"levels {name}")
    assert not np.isnan(got).any()


# -------------------------------------------------------------------------------------------- counts
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("name", ["small_T", "G"])
def test_counts(gpu, name, N):
    """Point counts around a wave and a block."""
    _compare(gpu, name, GS.random_points(257, seed=10)[:N].contiguous(), "unit", f"count{N}", f"count {name} {N}")


@pytest.mark.parametrize("n_dev", [0, 1, 257, 1024, 5000])
@pytest.mark.parametrize("name", ["small_T", "G"])
def test_live_count_from_the_device(gpu, name, n_dev):
    """Capacity 1024 with the live count on the device: above n it clamps to n, at 0 nothing is written;
    the planes are 1152 apart, so a kernel that mixed n, the live count and the stride up would write
    where the fill is checked."""
    got, _, _ = _compare(gpu, name, GS.random_points(1024, seed=12), "unit", "ndev", f"n_dev {n_dev} {name}",
                         n_dev=n_dev, stride=1152)
    assert got.shape[0] == min(n_dev, 1024)


# --------------------------------------------------------------------------------------- grid stride
def test_grid_stride(gpu):
    """lego, N = 524,288 + 256 + 3: the row-major kernel's 8192 blocks and the planar kernel's 2048
    blocks per level group both take a second grid-stride iteration that ends in a partial block.
    x[i] = base[i % 8191] (8191 prime, 524,288 % 8191 = 64): a sample read or stored one stride off is
    another point.  The reference is computed for the 8191 points and tiled."""
    lay, olay = FW.layouts("lego")
    N, p = FW.STRIDE_N, FW.STRIDE_PERIOD
    base = FW.stride_base()
    table = FW.table16("unit", lay.n_params, seed=33)
    ref, A = FW.forward_ref(base, table, olay)
    reps = (N + p - 1) // p
    x = base.repeat(reps, 1)[:N].contiguous()
    got = _run(gpu, lay, x, table)
    FW.check(got, np.tile(ref, (reps, 1))[:N], np.tile(A, (reps, 1))[:N], "grid stride lego", olay, x)


# ------------------------------------------------------------------------------------- normalisation
@pytest.mark.parametrize("x_min,x_range", [(-0.5, 1.0), (-1.0, 2.0), (-16.0, 32.0), (-1.5, 3.0)])
def test_normalisation(gpu, x_min, x_range):
    """x' = (x - x_min) / x_range in both kernels against torch's fp32 division.  The first three
    divide exactly; (-1.5, 3) needs the correctly rounded fp32 division the build's -fno-fast-math and
    hipcc's default give (a reciprocal-multiply would move pos by an fp32 ulp of x': visible at the
    finest levels first)."""
    u = GS.random_points(2053, seed=14)
    x = (u * x_range + x_min).float()
    _compare(gpu, "lego", x, "unit", f"norm{x_min}", f"normalisation ({x_min}, {x_range})", x_min=x_min,
             x_range=x_range)


# ------------------------------------------------------------------------------------- error returns
def test_error_returns_launch_nothing(gpu):
    """Bad arguments are MFN_ERR_INVALID before any launch (the outputs keep their fill); n = 0 is MFN_OK
    and writes nothing.  A level of one entry: the planar forward refuses it (its 8-byte load would
    read past the table), the row-major forward takes it."""
    lay, olay = FW.layouts("small_T")
    lib = load()
    n, stride = 64, 128
    x = GS.random_points(n, seed=15).to(gpu)
    t16 = FW.table16("unit", lay.n_params, seed=34).to(gpu)
    out = torch.full((n, 2 * lay.L), float("nan"), dtype=torch.float16, device=gpu)
    planes = torch.full((lay.L, stride, 2), float("nan"), dtype=torch.float16, device=gpu)
    null = ctypes.c_void_p(0)

    def desc(**kw):
        d = lay.desc()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def planar(n=n, stride=stride, d=None, table=ptr(t16), xs=ptr(x)):
        return lib.mfnerf_grid_encode_fw_planar(xs, n, null, 0.0, 1.0, d or lay.desc(), table, ptr(planes), stride,
                                                stream())

    def row(n=n, d=None, table=ptr(t16)):
        return lib.mfnerf_grid_encode_fw(ptr(x), n, null, 0.0, 1.0, d or lay.desc(), table, ptr(out), stream())

    one = lay.desc()
    one.size[lay.L - 1] = 1
    assert planar(n=-1) == INVALID and row(n=-1) == INVALID
    assert planar(stride=n - 1) == INVALID
    assert planar(d=desc(n_levels=6)) == INVALID and row(d=desc(n_levels=6)) == INVALID
    assert planar(d=desc(n_features=4)) == INVALID and row(d=desc(n_features=4)) == INVALID
    assert planar(table=null) == INVALID and row(table=null) == INVALID
    assert planar(d=one) == INVALID
    assert b"needs >= 2" in lib.mfnerf_last_error()
    assert planar(n=0) == OK and row(n=0) == OK
    assert planar(n=0, table=null, xs=null) == OK
    torch.cuda.synchronize()
    assert _fill_kept(out) and _fill_kept(planes)
    # the row-major kernel on the one-entry level: every corner is entry 0 of that level
    assert row(d=one) == OK
    torch.cuda.synchronize()
    olay.sizes[lay.L - 1] = 1
    ref, A = FW.forward_ref(x.cpu(), t16.cpu(), olay)
    FW.check(out.cpu(), ref, A, "row-major, a level of one entry")
