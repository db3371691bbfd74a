"""The inputs of tests/test_gpu_grid_seams.py, checked on the host: the spotlight points reach the
cells and record classes they are aimed at, a lost or misrouted contribution of any of them would
break the per-entry bound, and the run / count / chunk cases cross the seams they are named for."""
import collections

import numpy as np
import pytest
import torch

import grid_plan_ref as GP
import grid_seam_ref as GS
from oracle import field_oracle as FO
from test_gpu_field import _abs_grad

SPOT_LAYOUTS = ["C", "D", "E", "F", "G", "H"]


@pytest.mark.parametrize("name", SPOT_LAYOUTS)
def test_spotlights_reach_every_class_and_stay_visible(name):
    lay, olay = GS.layouts(name)
    P = GP.bin_plan(lay)
    sp = GS.spot_case(name)
    S = len(sp.cls)
    print(name, S, "spotlights,", sp.dropped, "dropped:", dict(collections.Counter(sp.cls)))
    assert 100 <= S <= 1000 and sp.dropped <= 0.06 * (S + sp.dropped)
    # the oracle's cell formula puts every point where it was aimed, inside the unit cube
    assert bool(((sp.x >= 0) & (sp.x <= 1)).all())
    for k in range(S):
        pos = np.float32(np.float64(sp.x[k, 0]) * float(olay.scales[sp.level[k]]) + 0.5)
        assert int(np.floor(pos)) == sp.cell[k, 0]
    # every class the layout's plan can produce is hit; all three x fractions survive
    assert set(sp.cls) == GS.expected_classes(lay, P)
    assert set(np.round(sp.f, 6)) == set(np.round(GS.SPOT_F, 6))
    assert set(sp.level) == set(P.level)
    # the record format against the oracle's indices: a pair record's second entry is the first one
    # XOR ((2 << ones) - 1) << s inside one partition; the single kinds are single for their reason
    emask = (1 << P.shift) - 1
    for k in range(S):
        l, size = int(sp.level[k]), lay.sizes[sp.level[k]]
        mask = ((2 << int(sp.ones[k])) - 1) << int(sp.s[k])
        rel = sp.entries[k] - lay.offsets[l]
        for yz in range(4):
            i0, i1 = int(rel[2 * yz]), int(rel[2 * yz + 1])
            if sp.cls[k] == "pair" and not P.pair_ok:
                assert i0 >> P.shift == i1 >> P.shift and (i0 & emask) ^ mask == i1 & emask, (k, yz)
            elif sp.cls[k] == "pair":  # the PAIR kernel clamps ones below shift
                assert (i0 & emask) ^ ((2 << min(int(sp.ones[k]), P.shift - 1)) - 1) == i1 & emask
            elif sp.cls[k] == "straddle single":
                assert i0 >> P.shift != i1 >> P.shift and mask < size and sp.ones[k] < 15
            elif sp.cls[k] == "cut single":
                assert sp.ones[k] >= 15
            elif sp.cls[k] == "mask-past-table single":
                assert mask >= size and sp.ones[k] < 15
    # a lost contribution must be visible: each of the eight, for both features, > 4 x the bound
    bound = GS.entry_terms(sp.x, sp.dy, lay, olay).bound.numpy()
    mag = np.abs(sp.dy.double().numpy()[np.arange(S)[:, None], 2 * sp.level[:, None] + np.arange(2)[None]])
    assert float(mag.min()) >= 0.5 and float(mag.max()) <= 2.0
    assert int((sp.dy != 0).sum()) == 2 * S  # non-zero only at the spotlight's level
    contrib = sp.weights[:, :, None] * mag[:, None, :]
    b = bound[2 * sp.entries[:, :, None] + np.arange(2)[None, None]]
    worst = float((contrib / b).min())
    print(name, "smallest contribution / bound:", worst)
    assert worst > 4.0


def test_spotlight_trailing_ones_reach_the_cut():
    """2^k - 1 for every k inside the grid: up to 15 at res 32768 (14 pairs or straddles, 15 is cut), up
    to 17 at res 131072; in H's shared tables of 2^14 the pair mask reaches past the table from ones = 13."""
    for name, top in (("D", 15), ("E", 15), ("F", 17)):
        sp = GS.spot_case(name)
        finest = sp.level == sp.level.max()
        assert set(sp.ones[finest]) >= set(range(top + 1)), name
        cut = [k for k in range(len(sp.cls)) if sp.cls[k] == "cut single"]
        assert {int(sp.ones[k]) for k in cut} == set(range(15, top + 1))
    sp = GS.spot_case("H")
    past = [k for k in range(len(sp.cls)) if sp.cls[k] == "mask-past-table single"]
    # ((2 << ones) - 1) << s >= 2^14: from ones = 14 on a step-1 cell (13 on a step-2 cell, s = 1, which
    # no cell of H's two step-2 levels has)
    assert {(int(sp.ones[k]), int(sp.s[k])) for k in past} >= {(14, 0)}
    assert all(((2 << int(sp.ones[k])) - 1) << int(sp.s[k]) >= 1 << 14 for k in past)
    steps = collections.Counter()
    lay, _ = GS.layouts("H")
    P = GP.bin_plan(lay)
    for k in range(len(sp.cls)):
        if not P.merge[int(sp.level[k])]:
            steps[GS.x_pair(lay, P, int(sp.level[k]), int(sp.cell[k, 0]))[0]] += 1
    assert set(steps) == {1, 2, 3}  # c(x + 1) - c(x)


def test_entry_terms_agree_with_the_oracle():
    """The fp64 sums of the bound against the oracle's own autograd gradient (fp32 weights)."""
    lay, olay = GS.layouts("H")
    x = GS.random_points(700, seed=3)
    dy = torch.randn(700, 32, generator=torch.Generator().manual_seed(4))
    T = GS.entry_terms(x, dy, lay, olay)
    tp = torch.zeros(lay.n_params).requires_grad_(True)
    (FO.grid_encode(x, tp, olay).double() * dy.double()).sum().backward()
    gabs = _abs_grad(x, dy, olay)
    assert float(((T.ref - tp.grad.double()).abs() - 1e-6 * gabs - 1e-12).max()) <= 0
    assert torch.allclose(T.gabs, gabs, rtol=1e-6, atol=1e-12)
    assert bool((T.rrow >= T.gabs * (1 - 1e-12)).all()) and bool((T.cnt[T.gabs > 0] >= 1).all())
    # the unit: 2^-30 of the power of two above the table's L1 (test_gpu_field._table_unit_bound's)
    for a, b in GS.table_regions(lay):
        assert len(set(T.unit[a:b].tolist())) == 1


def test_run_cases_cross_the_chunks():
    lengths = GS.RUN_LENGTHS + GS.RUN_LENGTHS[::-1] + (16, 16, 7)
    lay, _ = GS.layouts("H")
    x, dy = GS.run_case(lay, lengths, seed=2)
    N = x.shape[0]
    assert N == sum(lengths) and N % 16 == 15  # the last run ends on a partial 16-sample chunk
    _, starts = GS.run_points(lengths, seed=2)
    for s0, m in zip(starts, lengths):
        same = bool((x[s0:s0 + m] == x[s0]).all())
        assert same or float((x[s0:s0 + m] - x[s0]).abs().max()) < 1e-4
        if m >= 15:
            assert bool((dy[s0 + m // 2] == 0).all()) and bool((dy[s0 + m // 2 - 1] != 0).all())
    assert any(s0 // 16 != (s0 + m - 1) // 16 for s0, m in zip(starts, lengths))
    # the dense-level kernel's window: two chunks of 64 above 131,072 live samples
    win = -(-GS.DENSE_N // (64 * GP.DENSE_WAVES))
    assert win == 2 and GS.DENSE_N % 16 and GS.DENSE_N % 64
    s0, m = GS.DENSE_RUNS["chunk boundary inside a window"]
    assert s0 // 128 == (s0 + m - 1) // 128 and s0 // 64 != (s0 + m - 1) // 64
    s0, m = GS.DENSE_RUNS["window boundary"]
    assert s0 // 128 + 1 == (s0 + m - 1) // 128 and (s0 + m - 1) % 128 < 64 and s0 % 128 >= 64
    s0, m = GS.DENSE_RUNS["chunk+window+chunk"]
    assert m == 200 and (s0 + m - 1) // 64 - s0 // 64 == 3
    lego, _ = GS.layouts("lego")
    xd, dyd = GS.dense_window_case(lego)
    first = GP.first_binned_level(lego)
    assert first == 6 and bool((dyd[:, 2 * first:] == 0).all()) and bool((dyd[:5, :2 * first] != 0).all())
    for s0, m in GS.DENSE_RUNS.values():
        assert bool((xd[s0:s0 + m] == xd[s0]).all()) and not bool((xd[s0 - 1] == xd[s0]).all())


def test_accumulate_chunk_cases_hit_the_stage_sizes():
    """ACC_RB = 4096 records per stage chunk: a partition at exactly one chunk, one just above it (a
    last chunk of <= 32 records), one of more than two chunks; a unit with an odd count (a pad
    record); no slot overflows (the records take the compacted path)."""
    lay, olay = GS.layouts("small_T")
    P = GP.bin_plan(lay)
    cases = GS.accum_chunk_cases(lay, olay, P)
    Ts = np.concatenate([T for *_, T in cases])
    assert (Ts == GP.ACC_RB).any()
    assert ((Ts > GP.ACC_RB) & (Ts <= GP.ACC_RB + 32)).any()
    assert (Ts > 2 * GP.ACC_RB).any()
    assert any((counts % 2 == 1).any() for _, _, counts, _, _ in cases)
    for n, x, counts, slot, T in cases:
        assert x.shape == (n, 3) and int(counts.max()) <= slot
        assert np.array_equal(counts, GS.pair_record_counts(lay, olay, P, x))
    # G's overflow case: two points with a corner in a table's last (80-entry) partition
    layG, olayG = GS.layouts("G")
    PG = GP.bin_plan(layG)
    pts = GS.points_in_last_partition(layG, olayG, PG, 2)
    assert pts.shape == (2, 3)
