"""The host mirror of the partitioned scatter's plan (tests/grid_plan_ref.py) against the library's
own host queries -- the library loads without a GPU -- and the coverage claim of
tests/test_gpu_grid_seams.py: which bin_scatter_kernel instantiation, partition size and record
kinds each of its layouts runs."""
import pytest

import grid_plan_ref as GP
import grid_seam_ref as GS
from mfnerf._lib import load
from mfnerf.grid import GridLayout
from test_gpu_field import LEGO_B, _layouts

# every layout the suite's table-gradient tests use, and the seam suite's own
NAMED = dict(
    [(n, a) for n, a in _layouts()] +
    [("hash_T14", (16, 2, 14, 16, LEGO_B, "Hash", 1)), ("hash_T12", (16, 2, 12, 16, LEGO_B, "Hash", 1)),
     ("mixed_T20x8", (16, 2, 20, 16, LEGO_B, "MixedFeature", 8)),
     ("hash_scale4", (16, 2, 20, 16, GP.b_of(8192), "Hash", 1)),
     ("hash_scale16", (16, 2, 20, 16, GP.b_of(32768), "Hash", 1)),
     ("hash_scale64", (16, 2, 20, 16, GP.b_of(131072), "Hash", 1))] +
    list(GS.SUITE_LAYOUTS.items()))


@pytest.mark.parametrize("name", sorted(NAMED))
def test_mirror_matches_the_library(name):
    lay = GridLayout(*NAMED[name])
    lib, desc = load(), lay.desc()
    for n in (1, 4099, 300000):  # the byte count depends on n_bins, pair_ok and n_binned (slot_size)
        assert lib.mfnerf_grid_encode_bw_binned_workspace(desc, n) == GP.workspace_bytes(lay, n), n
    assert lib.mfnerf_grid_binned_first_value(desc) == GP.first_value(lay)
    assert lib.mfnerf_grid_dense_values(desc) == GP.dense_values(lay)
    assert lib.mfnerf_grid_encode_bw_workspace(desc) == GP.GRAD_COPIES * GP.dense_entries(lay) * 8
    W = GP.workspace_layout(lay, 4099)
    assert lib.mfnerf_grid_encode_bw_binned_flag_offset(desc, 4099) == W["ovf"]


def test_mixedfeature_at_scale_64_is_rejected():
    """(res + 2) canon_res >= 2^31: check_desc refuses the layout, and so does the mirror."""
    lay = GridLayout(16, 2, 20, 16, GP.b_of(131072), "MixedFeature", 8)
    assert not GP.check_desc(lay)
    assert load().mfnerf_grid_encode_bw_binned_workspace(lay.desc(), 4099) == -1 == GP.workspace_bytes(lay, 4099)


# name: ((MAXB, PAIR), shift, partitions, finest res)
TABLE = {"A": ((12, True), 11, 1408, 1025), "B": ((16, True), 11, 1920, 1024), "C": ((8, False), 8, 448, 2048),
         "D": ((16, False), 8, 960, 32768), "E": ((12, False), 11, 3072, 32768), "F": ((16, False), 8, 960, 131072),
         "G": ((12, False), 8, 258, 1025), "H": ((16, False), 8, 256, 32768),
         "lego": ((10, True), 11, 2560, 1025), "small_T": ((8, True), 8, 16, 32)}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_suite_layouts_run_the_kernels_they_are_there_for(name):
    lay = GridLayout(*GS.SUITE_LAYOUTS[name])
    P = GP.bin_plan(lay)
    assert (P.instantiation, P.shift, P.n_bins, lay.res[-1]) == TABLE[name]


def test_suite_covers_every_instantiation_and_record_kind():
    plans = {n: (GridLayout(*a), GP.bin_plan(GridLayout(*a))) for n, a in GS.SUITE_LAYOUTS.items()}
    inst = {P.instantiation for _, P in plans.values()}
    assert inst == {(8, True), (10, True), (12, True), (16, True), (8, False), (12, False), (16, False)}
    assert {P.shift for _, P in plans.values()} == {8, 11}
    # an own-table pair level in the single-record kernel (pair records beside straddling singles)
    assert any(not P.pair_ok and any(P.pairable[l] for l in P.level) for _, P in plans.values())
    # the real-scene Hash layout: finest res 32768 in partitions of 2^11
    layE, PE = plans["E"]
    assert layE.res[-1] == 32768 and PE.shift == 11 and not PE.pair_ok and all(PE.pairable[l] for l in PE.level)
    # MixedFeature levels of canonical step 1, 2 (pair records with s = 0 / 1) and >= 3 (merged), in
    # power-of-two shared tables (H), and shared tables that are no power of two (G: `% size`)
    layH, PH = plans["H"]
    steps = {int(PH.canon_step[l]) for l in PH.level if not PH.merge[l]}
    assert steps == {1, 2} and any(PH.merge[l] for l in PH.level)
    assert [l for l in PH.level if PH.merge[l]] == list(range(2, 13))
    assert all(s & (s - 1) == 0 for s in PH.t_size)
    layG, PG = plans["G"]
    assert PG.t_size == [21840] * 3 and any(PG.merge[l] for l in PG.level) and not all(PG.merge[l] for l in PG.level)
    # a table whose last partition is partial (the fused Adam's clamped state load)
    assert [PG.last_partition_entries(t) for t in range(3)] == [80, 80, 80] and 80 < 1 << PG.shift
    # each spotlit layout's record classes, from its plan (test_grid_seam_ref_cpu.py: none is empty)
    want = {"C": {"pair", "straddle single"},
            "D": {"pair", "straddle single", "cut single", "mask-past-table single"},
            "E": {"pair", "straddle single", "cut single"},
            "F": {"pair", "straddle single", "cut single", "mask-past-table single"},
            "G": {"single", "merged"},
            "H": {"pair", "straddle single", "cut single", "mask-past-table single", "merged", "single"}}
    for n, w in want.items():
        assert GS.expected_classes(*plans[n]) == w, n
    assert set().union(*want.values()) == set(GS.CLASSES)
