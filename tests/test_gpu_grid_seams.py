"""The table-gradient scatter (csrc/grid_bw_binned.hip, grid_records.hpp, grid_bw_atomic.hip) at its
seams: every bin_scatter_kernel instantiation, real-scene layouts (Hash grids up to res 131072,
MixedFeature tables that are no power of two), the record kinds at the cells where they change, runs
across the 16- and 64-sample chunks, live counts around a chunk, the PAIR kernel's second tile, the
accumulate's stage chunks and the fused Adam tail -- against the fp64 oracle under the per-entry
bound of tests/grid_seam_ref.py (nothing in it is scaled by a region's largest entry).

Every comparison runs the fixed-point atomic path once and the partitioned path twice, asserts the
partitioned bits equal and the private copies left zero.  tests/test_grid_plan_cpu.py proves which
kernel each layout runs; tests/test_grid_seam_ref_cpu.py that the inputs cross the seams named here."""
import numpy as np
import pytest
import torch

import grid_fw_ref as FW
import grid_plan_ref as GP
import grid_seam_ref as GS
import input_grad_ref as IG
from mfnerf import engine, synthetic
from mfnerf import field as FLD
from mfnerf._lib import call, load, ptr, stream
from oracle import field_oracle as FO

pytestmark = pytest.mark.gpu


def _scatter(gpu, lay, x, dy, n_dev=None, n_slots=0):
    """(atomic fixed-point gradient, partitioned gradient, its workspace), the first two f64 on the host."""
    desc, N = lay.desc(), x.shape[0]
    xg, dyg = x.to(gpu).contiguous(), dy.to(gpu).contiguous()
    nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=gpu)
    nc = load().mfnerf_grid_encode_bw_workspace(desc) // 4
    ws = FLD.grid_bw_workspace(desc, gpu)
    fx = torch.zeros(lay.n_params, device=gpu)
    FLD.grid_encode_bw(xg, N, dyg, fx, lay, desc, n_dev=nd, workspace=ws, fixed_point=True)
    assert not bool(ws.any()), "atomic path: private copies not left zero"
    bn = []
    for _ in range(2):
        ws = FLD.grid_bw_binned_workspace(desc, n_slots or N, gpu)
        gt = torch.zeros(lay.n_params, device=gpu)
        FLD.grid_encode_bw(xg, N, dyg, gt, lay, desc, n_dev=nd, workspace=ws, binned=True, n_slots=n_slots)
        assert not bool(ws[:nc].any()), "partitioned path: private copies not left zero"
        bn.append(gt)
    assert torch.equal(bn[0], bn[1]), f"partitioned path not reproducible: {int((bn[0] != bn[1]).sum())} values"
    return fx.cpu().double(), bn[1].cpu().double(), ws


def _check(got, T, lay, what, spots=None):
    """|got - ref| <= the per-entry bound, table region by table region."""
    bound = T.bound
    worst = 0.0
    for a, b in GS.table_regions(lay):
        err = (got[a:b] - T.ref[a:b]).abs()
        excess = err - bound[a:b]
        worst = max(worst, float((err / bound[a:b]).max()))
        if float(excess.max()) > 0:
            p = a + int(excess.argmax())
            who = spots.describe(p // 2) if spots is not None else ""
            raise AssertionError(f"{what}: value {p} (table at {a}) got {float(got[p])!r} ref {float(T.ref[p])!r} "
                                 f"bound {float(bound[p])!r}, {int((excess > 0).sum())} values out {who}")
    print(f"{what}: max |got - ref| / bound = {worst:.3f}")


def _compare(gpu, lay, olay, x, dy, what, spots=None, n_dev=None, n_slots=0):
    m = x.shape[0] if n_dev is None else n_dev
    T = GS.entry_terms(x[:m], dy[:m], lay, olay)
    fx, bn, ws = _scatter(gpu, lay, x, dy, n_dev=n_dev, n_slots=n_slots)
    assert float(T.ref.abs().max()) > 0 or m == 0
    _check(fx, T, lay, what + " (fixed-point atomics)", spots)
    _check(bn, T, lay, what + " (partitioned)", spots)
    return ws


def _dy(n, lay, seed, mag=1e-3):
    return torch.randn(n, 2 * lay.L, generator=torch.Generator().manual_seed(seed)) * mag


# ------------------------------------------------------------------------------------------ spotlights
@pytest.mark.parametrize("name", ["C", "D", "E", "F", "G", "H"])
def test_spotlights(gpu, name):
    """A few hundred sparse points aimed at the x cells where a record changes kind (2^k - 1 for every
    k, the cells around m 2^shift - 1, the canonical steps 1 / 2 / 3 of a shared table), each with a
    gradient at its own level only: every one of their contributions is more than 4x the bound at its
    entry (test_grid_seam_ref_cpu.py), so a dropped or misrouted record fails here, and the failure
    names the class, level and cell."""
    lay, olay = GS.layouts(name)
    sp = GS.spot_case(name)
    _compare(gpu, lay, olay, sp.x, sp.dy, f"spotlights {name}", spots=sp)
    if name not in ("D", "E"):
        return
    # the forward (row-major and planar) and the input gradient at res > 1025, on the same points
    N = sp.x.shape[0]
    g = torch.Generator().manual_seed(7)
    table = (torch.rand(lay.n_params, generator=g) - 0.5).half()
    ref = FO.grid_encode(sp.x, table.float(), olay)
    desc, xg, t16 = lay.desc(), sp.x.to(gpu), table.to(gpu)
    out = FLD.grid_encode_fw(xg, N, t16, lay, desc)
    # fp32 accumulation of fp16 corners, one fp16 rounding of the output: <= 1 fp16 ulp (|y| < 1)
    assert torch.allclose(out.float().cpu(), ref, atol=1e-3, rtol=0)
    ref64, A = FW.forward_ref(sp.x, table, olay)  # ... and to that one rounding (tests/grid_fw_ref.py)
    FW.check(out.cpu(), ref64, A, f"spotlights {name}, row-major forward", olay, sp.x)
    cap = (N + 127) // 128 * 128
    xp = torch.zeros(cap, 3, device=gpu)
    xp[:N] = xg
    planes = torch.full((lay.L, cap, 2), float("nan"), dtype=torch.float16, device=gpu)
    n_dev = torch.tensor([N], dtype=torch.int32, device=gpu)
    call("mfnerf_grid_encode_fw_planar", ptr(xp), cap, ptr(n_dev), 0.0, 1.0, desc, ptr(t16), ptr(planes), cap, stream())
    torch.cuda.synchronize()
    pl = planes[:, :N].permute(1, 0, 2).reshape(N, -1)
    assert torch.allclose(pl.float().cpu(), ref, atol=1e-3, rtol=0)
    FW.check(pl.cpu(), ref64, A, f"spotlights {name}, planar forward", olay, sp.x)
    dyf = torch.randn(N, 2 * lay.L, generator=g)
    dref, A = IG.dx_ref(sp.x, table, dyf, olay)
    got = FLD.grid_encode_bw_input(xg, N, t16, dyf.to(gpu), desc).cpu()
    err = (got.double() - dref).abs()
    print(f"input gradient {name}: max err / A = {float((err / A.clamp_min(1e-300)).max()):.3e}")
    assert torch.isfinite(got).all() and bool((err <= 2.0 ** -15 * A).all())


# ---------------------------------------------------------------------------------- every instantiation
@pytest.mark.parametrize("name,inst", [("A", (12, True)), ("B", (16, True)), ("C", (8, False)), ("G", (12, False)),
                                       ("lego", (10, True)), ("small_T", (8, True)), ("H", (16, False))])
def test_every_instantiation(gpu, name, inst):
    """bin_scatter_kernel<MAXB, PAIR> for all seven (MAXB, PAIR): <12, PAIR> and <16, PAIR> take the
    run-time level select, <16, PAIR> alone stores one record per thread and pass; 4099 random points
    with the cube's corners."""
    lay, olay = GS.layouts(name)
    assert GP.bin_plan(lay).instantiation == inst
    N = 4099
    _compare(gpu, lay, olay, GS.random_points(N, seed=2), _dy(N, lay, 3), f"instantiation {name} {inst}")


# ------------------------------------------------------------------------------------------------ runs
RUN_CASE = GS.RUN_LENGTHS + GS.RUN_LENGTHS[::-1] + (16, 16, 7)


@pytest.mark.parametrize("name", ["H", "G", "lego"])
def test_runs(gpu, name):
    """'Rays' of 1, 2, 15, 16, 17, 33 and 200 identical or nearly identical samples (the merged
    records' and the dense kernel's runs across the 16- and 64-sample chunks), a zero-gradient sample
    in the middle of the long ones, the last run ending on a partial chunk."""
    lay, olay = GS.layouts(name)
    x, dy = GS.run_case(lay, RUN_CASE, seed=2)
    _compare(gpu, lay, olay, x, dy, f"runs {name}")


def test_dense_kernel_runs_across_window_chunks(gpu):
    """Above 131,072 live samples a wave of the dense-level kernel takes a window of two 64-sample
    chunks and carries the run open at the first one's end into the second: runs of identical samples
    across a chunk boundary inside a window, across a window boundary (issued twice, never carried),
    and a 200-sample run across both.  Only the dense levels' gradient is non-zero."""
    lay, olay = GS.layouts("lego")
    x, dy = GS.dense_window_case(lay)
    assert x.shape[0] > 64 * GP.DENSE_WAVES
    _compare(gpu, lay, olay, x, dy, "dense window")


# ---------------------------------------------------------------------------------------------- counts
@pytest.mark.parametrize("N", [1, 15, 16, 17, 4095, 4096, 4097])
@pytest.mark.parametrize("name", ["small_T", "G"])
def test_counts(gpu, name, N):
    """Live counts around one 16-sample chunk and around 256 units x 16 samples."""
    lay, olay = GS.layouts(name)
    _compare(gpu, lay, olay, GS.ray_points(N, seed=N), _dy(N, lay, N + 1), f"count {name} {N}")


@pytest.mark.parametrize("name", ["small_T", "G"])
def test_live_count_from_the_device(gpu, name):
    lay, olay = GS.layouts(name)
    n = 6000
    x, dy = GS.ray_points(n, seed=5), _dy(n, lay, 6)
    _compare(gpu, lay, olay, x, dy, f"n_dev 4099 of 6000 {name}", n_dev=4099)
    # a live count of 0: the partitioned region is overwritten with zeros, the rest stays zero
    desc = lay.desc()
    first = load().mfnerf_grid_binned_first_value(desc)
    assert 0 < first < lay.n_params
    gt = torch.zeros(lay.n_params, device=gpu)
    gt[first:] = 7.0
    ws = FLD.grid_bw_binned_workspace(desc, n, gpu)
    zero = torch.zeros(1, dtype=torch.int32, device=gpu)
    FLD.grid_encode_bw(x.to(gpu), n, dy.to(gpu), gt, lay, desc, n_dev=zero, workspace=ws, binned=True)
    assert not bool(gt.any())
    assert not bool(ws[:load().mfnerf_grid_encode_bw_workspace(desc) // 4].any())
    _compare(gpu, lay, olay, x, dy, f"n_dev 0 of 6000 {name}", n_dev=0)


# ------------------------------------------------------------------------- the PAIR kernel's second tile
def test_pair_kernel_second_tile(gpu):
    """A unit of the PAIR kernel holds 2 x 1024 samples per tile: 524,288 + 16 + 7 samples give unit 0
    a second tile of 16 samples, unit 1 one of 7, the other units none.  Only the four binned levels'
    gradient is non-zero (the oracle's cost; the dense levels have their own test above)."""
    lay, olay = GS.layouts("small_T")
    P = GP.bin_plan(lay)
    N = 2 * GP.SC_THREADS * GP.UNITS + 16 + 7
    per_unit = np.bincount(GP.unit_of_sample(np.arange(N)), minlength=GP.UNITS)
    assert per_unit[0] == 2048 + 16 and per_unit[1] == 2048 + 7 and (per_unit[2:] == 2048).all()
    x = torch.rand(N, 3, generator=torch.Generator().manual_seed(8))
    dy = _dy(N, lay, 9)
    dy[:, :2 * P.level[0]] = 0.0
    _compare(gpu, lay, olay, x, dy, "PAIR second tile")


# ------------------------------------------------------------------------------------- accumulate chunks
@pytest.mark.parametrize("k", [0, 1, 2], ids=[f"N{n}" for n in GS.ACCUM_N])
def test_accumulate_chunks(gpu, k):
    """Every sample at one interior point of the small-T layout: a partition's compacted record count
    T (every unit's count rounded up to even) is exactly one stage chunk of ACC_RB = 4096 records, just
    above it, and above two chunks; an odd unit count makes a pad record."""
    lay, olay = GS.layouts("small_T")
    P = GP.bin_plan(lay)
    n, x, counts, slot, T = GS.accum_chunk_cases(lay, olay, P)[k]
    assert int(counts.max()) <= slot
    if n == 4096:
        assert (T == GP.ACC_RB).any()
    elif n == 4099:
        assert ((T > GP.ACC_RB) & (T <= GP.ACC_RB + 32)).any() and (counts % 2 == 1).any()
    else:
        assert (T > 2 * GP.ACC_RB).any() and (counts % 2 == 1).any()
    dy = _dy(n, lay, 11 + k)
    assert bool((dy != 0).all())
    _compare(gpu, lay, olay, x, dy, f"accumulate chunks N={n}")


def test_overflowing_slots_and_a_partial_last_partition(gpu):
    """Layout G (tables of 21,840 entries: a last partition of 80), every sample at one of two points
    with a corner in such a partition, the slots sized for N / 16: they overflow, and the partial
    partition sums its records and its overflow words."""
    lay, olay = GS.layouts("G")
    P = GP.bin_plan(lay)
    assert all(P.last_partition_entries(t) == 80 for t in range(P.n_tables))
    pts = GS.points_in_last_partition(lay, olay, P, 2)
    N = 40000
    x = pts[torch.randint(0, 2, (N,), generator=torch.Generator().manual_seed(12))].contiguous()
    ws = _compare(gpu, lay, olay, x, _dy(N, lay, 13), "overflow G", n_slots=N // 16)
    ovf = load().mfnerf_grid_encode_bw_binned_flag_offset(lay.desc(), N // 16) // 4
    assert int(ws[ovf].view(torch.int32)) > 0, "no slot overflowed"


# ------------------------------------------------------------------------------------------- fused tail
FUSED_RAYS = 32  # the smallest count tried (32 .. 256) still marches samples: ~2300 at G, ~700 at E


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("name,kw", [("G", {"grid": "MixedFeature", "N_tables": 3, "log2_T": 16}),
                                     ("E", {"scale": 16.0, "log2_T": 19})])
def test_fused_adam_tail_on_the_new_layouts(gpu, name, kw, skip):
    """mfnerf_grid_encode_bw_binned_adam + mfnerf_adam_step_fixed_partial == mfnerf_grid_encode_bw_binned
    + mfnerf_adam_step_fixed, bit for bit, as test_partitioned_accumulate_with_fused_adam_matches_unfused
    drives them -- on G (the last partition's 80 of 256 entries: the clamped state load) and on E (the
    real-scene Hash layout)."""
    st = engine.TrainStep(engine.StepConfig(n_rays=FUSED_RAYS, n_parts=1, **kw), device=gpu, seed=0)
    lay, _ = GS.layouts(name)
    assert (st.layout.sizes, st.layout.offsets, st.layout.res) == (lay.sizes, lay.offsets, lay.res)
    st.set_occupancy(synthetic.ball_density_grid(cascades=st.cascades, scale=st.cfg.scale))
    assert st._fused_adam_ok()
    batches = st.make_batches(2, seed=5)
    st.run(batches[0])  # m, v non-zero
    mb, nomark = st.mbuf[0], (lambda name: None)
    st._use(mb)
    st._march(batches[1], mb, nomark)
    st._chain(batches[1], mb, 0, nomark)
    if skip:
        st.finite_status[0] = 1
    torch.cuda.synchronize()
    assert int(mb.counters[0, 0]) > 0, "the step marched no samples"
    names = ("params", "grads", "m", "v", "p16", "step_dev", "finite_status", "_level_l1")
    snap = {k: getattr(st, k).clone() for k in names}
    ws = st.parts[0].grid_ws
    snap_ws = ws.clone()
    st._grid_bw(mb, 0)
    st._finish_update()
    torch.cuda.synchronize()
    ref = {k: getattr(st, k).clone() for k in names}
    ref_ws = ws.clone()
    for k in names:
        getattr(st, k).copy_(snap[k])
    ws.copy_(snap_ws)
    st._grid_bw(mb, 0, fuse_adam=True)
    st._finish_update(partial=True)
    torch.cuda.synchronize()
    for k in names:
        got = getattr(st, k)
        if not torch.equal(got, ref[k]):
            d = (got.float() - ref[k].float()).abs()
            bad = torch.nonzero(d.flatten() > 0).flatten()
            raise AssertionError(f"{k}: {bad.numel()} values differ, first {bad[:8].tolist()}, max {float(d.max())}, "
                                 f"off_table {st.off_table}, first partitioned value "
                                 f"{st.off_table + load().mfnerf_grid_binned_first_value(st.desc)}")
    nc = load().mfnerf_grid_encode_bw_workspace(st.desc) // 4  # the private copies: zeroed by both
    assert not bool(ws[:nc].any()) and not bool(ref_ws[:nc].any()) and not bool(st.grads.any())
    if not skip:
        assert not torch.equal(st.params, snap["params"])
