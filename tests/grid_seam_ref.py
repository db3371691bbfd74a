"""Inputs and the per-entry bound of the table-gradient seam tests (test infrastructure, no test in
here).  Everything is fp64 / int64 on the CPU; the corner indices are the oracle's
(oracle.field_oracle.grid_index), the cell and weights come from the fp32 pos the kernels take
(input_grad_ref._geo).

THE BOUND.  For a table value (entry e, feature f), with the oracle's corner indices:
    gabs = sum of |wx wy wz dy_f| over the contributions to e          (the existing record bound's sum)
    rrow = sum of |wy wz dy_f| over every corner contribution to e, the x weight left out
    cnt  = number of contributions to e (samples whose dy at the level is non-zero, per corner)
    unit = the table's int32 fixed-point unit 2^(e - 30), the table's L1 of dy < 2^e
    |got - ref| <= 2^-11 1.0001 gabs + 2^-15 rrow + 1e-5 gabs + unit ((0.5 + 2^-10) cnt + 0.5)
Term by term (csrc/grid_records.hpp, grid_bw_binned.hip):
  * a record carries wy wz dy_f (in table units, times 2^-15) as fp16: one rounding to 11 significant
    bits, <= 2^-11 of the value, times the x weight <= 2^-11 of the contribution;
  * the x weight is the 15-bit fxq = min(32767, rint(32768 wx)): off by <= 2^-16, and by <= 2^-15
    where it is clipped; it multiplies wy wz dy_f for the x corner (1 - fxq) and the x+1 corner (fxq).
    (Both corners of one row falling on ONE entry count twice in rrow: each carries the weight's error.)
  * fp32 products (wy wz, times dy, times the weight; the merged records' run sums of <= 16 values)
    against fp64: a few 2^-24 each, 1e-5 as the ragged-ray test already allows;
  * every contribution is rounded once to an integer at the table's unit or finer (0.5 unit; the
    dense-level kernel and the atomic path round each sample or run the same way), an fp16 record
    value below 2^-14 is subnormal (spacing 2^-24 x 2^15 units: 2^-10 unit), and the partition's sum
    is rounded once back to the table's unit (0.5 unit).
Nothing in it is scaled by a region's largest entry.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

import grid_plan_ref as GP
from input_grad_ref import _geo
from oracle import field_oracle as FO

REC_REL = 2.0 ** -11
FX_ABS = 2.0 ** -15
FP32_REL = 1e-5
SPOT_F = (2.0 ** -7, 0.5, 1.0 - 2.0 ** -7)
RUN_LENGTHS = (1, 2, 15, 16, 17, 33, 200)
CLASSES = ("pair", "straddle single", "cut single", "mask-past-table single", "merged", "single")


def _corner(olay, l, g, w, c):
    """(absolute entry (n,) i64 numpy, [wx, wy, wz] f64 numpy) of corner c of level l."""
    bit = [(c >> d) & 1 for d in range(3)]
    idx = FO.grid_index(olay, l, g[:, 0] + bit[0], g[:, 1] + bit[1], g[:, 2] + bit[2]) + olay.offsets[l]
    wt = [(w[:, d] if bit[d] else 1 - w[:, d]).numpy() for d in range(3)]
    return idx.numpy(), wt


@dataclass
class Terms:
    ref: torch.Tensor    # (n_params,) f64 the gradient
    gabs: torch.Tensor   # (n_params,)
    rrow: torch.Tensor   # (n_params,)
    cnt: torch.Tensor    # (n_params,) the entry's count, repeated per feature
    unit: torch.Tensor   # (n_params,)

    @property
    def bound(self):
        return (REC_REL * 1.0001 * self.gabs + FX_ABS * self.rrow + FP32_REL * self.gabs +
                self.unit * ((0.5 + 2.0 ** -10) * self.cnt + 0.5))


def entry_terms(x, dy, lay, olay):
    """The fp64 table gradient of dy at the points x and the bound's per-entry sums (levels whose dy
    is all zero are skipped: they contribute nothing to any of them)."""
    n, L = x.shape[0], lay.L
    d_all = dy.double().view(n, L, 2).numpy()
    ne = olay.n_entries
    ref, gabs, rrow = np.zeros((ne, 2)), np.zeros((ne, 2)), np.zeros((ne, 2))
    cnt = np.zeros(ne)
    l1 = np.abs(d_all).sum((0, 2))
    for l in range(L):
        live = (d_all[:, l] != 0).any(1)
        if not live.any():
            continue
        sel = torch.from_numpy(np.nonzero(live)[0])
        d = d_all[live, l]
        g, w = _geo(olay, l, x[sel])
        a, m = lay.offsets[l], lay.sizes[l]  # the level's table: entries [a, a + m)
        for c in range(8):
            idx, wt = _corner(olay, l, g, w, c)
            idx = idx - a
            wyz = wt[1] * wt[2]
            for f in range(2):
                v = wt[0] * wyz * d[:, f]
                ref[a:a + m, f] += np.bincount(idx, v, m)
                gabs[a:a + m, f] += np.bincount(idx, np.abs(v), m)
                rrow[a:a + m, f] += np.bincount(idx, np.abs(wyz * d[:, f]), m)
            cnt[a:a + m] += np.bincount(idx, minlength=m)
    unit = np.zeros(ne)
    for l in range(L):
        t_l1 = float(sum(l1[k] for k in range(L) if lay.offsets[k] == lay.offsets[l]))
        if t_l1 > 0:
            unit[lay.offsets[l]:lay.offsets[l] + lay.sizes[l]] = 2.0 ** (math.frexp(t_l1)[1] - 30)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1))  # noqa: E731
    return Terms(t(ref), t(gabs), t(rrow), t(np.repeat(cnt, 2)), t(np.repeat(unit, 2)))


def table_regions(lay):
    """[(first value, end value)] of every table (a MixedFeature table shared by levels once)."""
    return sorted({(2 * lay.offsets[l], 2 * (lay.offsets[l] + lay.sizes[l])) for l in range(lay.L)})


# ------------------------------------------------------------------ the record a cell's x-pair becomes
def _ctz_not(v):
    """Trailing ones of v (32-bit)."""
    k = 0
    while k < 32 and (v >> k) & 1:
        k += 1
    return k


def x_pair(lay, P, l, gx):
    """(canonical step, ones, s) of the x-pair (gx, gx + 1) at binned level l as level_records_geo
    takes them: an own table steps by 1 in x itself; a shared power-of-two table in canon_coord."""
    size = lay.sizes[l]
    if lay.kind[l] == 1 and size & (size - 1) == 0:
        c0, c1 = gx * lay.canon_res // lay.res[l], (gx + 1) * lay.canon_res // lay.res[l]
        step = c1 - c0
        return step, _ctz_not(c0 >> 1 if step == 2 else c0), int(step == 2)
    if lay.kind[l] == 1:
        return (gx + 1) * lay.canon_res // lay.res[l] - gx * lay.canon_res // lay.res[l], _ctz_not(gx), 0
    return 1, _ctz_not(gx), 0


def record_class(lay, olay, P, l, g):
    """The class of the records cell g = (gx, gy, gz) of binned level l becomes, with (ones, s)."""
    step, ones, s = x_pair(lay, P, l, g[0])
    if P.pair_ok:
        return "pair", ones, s
    if P.merge[l]:
        return "merged", ones, s
    size = lay.sizes[l]
    pow2 = size & (size - 1) == 0
    if not (P.pairable[l] or (lay.kind[l] == 1 and pow2 and step in (1, 2))):
        return "single", ones, s
    if ones >= 15:
        return "cut single", ones, s
    if ((2 << ones) - 1) << s >= size:
        return "mask-past-table single", ones, s
    for yz in range(4):
        gy, gz = torch.tensor([g[1] + (yz & 1)]), torch.tensor([g[2] + (yz >> 1)])
        i0 = int(FO.grid_index(olay, l, torch.tensor([g[0]]), gy, gz))
        i1 = int(FO.grid_index(olay, l, torch.tensor([g[0] + 1]), gy, gz))
        if i0 >> P.shift != i1 >> P.shift:
            return "straddle single", ones, s
    return "pair", ones, s


def _level_x_pairs(lay, P, l):
    """(step, s, ones) of every x cell 0 .. res - 1 of binned level l (x_pair, vectorised)."""
    res = lay.res[l]
    g = np.arange(res, dtype=np.int64)
    if lay.kind[l] == 1:
        c0, c1 = g * lay.canon_res // res, (g + 1) * lay.canon_res // res
    else:
        c0, c1 = g, g + 1
    step = c1 - c0
    pow2 = lay.sizes[l] & (lay.sizes[l] - 1) == 0
    s = ((step == 2) & (lay.kind[l] == 1) & pow2).astype(np.int64)
    cs = np.where(s == 1, c0 >> 1, c0) if (lay.kind[l] == 0 or pow2) else g
    ones = np.zeros_like(cs)
    m = cs.copy()
    for _ in range(32):
        on = (m & 1) == 1
        ones += on
        m = np.where(on, m >> 1, 0)
    return step, s, ones


def expected_classes(lay, P):
    """The classes a layout's records can fall in: level_records_geo's decisions over EVERY x cell a
    point of [0, 1] can lie in (cell g needs g + 2^-7 - 0.5 <= scale), not only the spotlit ones.  Both
    x corners of a row differ by the mask ((2 << ones) - 1) << s, so they straddle two partitions
    exactly when ones + s >= shift (in a table of more than one partition)."""
    if P.pair_ok:
        return {"pair"}
    out = set()
    for l in P.level:
        if P.merge[l]:
            out.add("merged")
            continue
        size = lay.sizes[l]
        pow2 = size & (size - 1) == 0
        step, s, ones = _level_x_pairs(lay, P, l)
        n = min(lay.res[l], int(math.floor(lay.scales[l] + 0.5 - 2.0 ** -7)) + 1)
        step, s, ones = step[:n], s[:n], ones[:n]
        base = np.full(n, bool(P.pairable[l])) | ((lay.kind[l] == 1) & pow2 & ((step == 1) | (step == 2)))
        cut = base & (ones >= 15)
        past = base & ~cut & ((((2 << np.minimum(ones, 40)) - 1) << s) >= size)
        straddle = base & ~cut & ~past & (ones + s >= P.shift) & (size > 1 << P.shift)
        pair = base & ~cut & ~past & ~straddle
        for name, m in (("single", ~base), ("cut single", cut), ("mask-past-table single", past),
                        ("straddle single", straddle), ("pair", pair)):
            if m.any():
                out.add(name)
    return out


def target_cells(lay, P, l):
    """x cells of binned level l to spotlight: the first cell of every (canonical step, s, trailing
    ones) the level has -- on an own table that is 2^k - 1 for every k --, the cells at and around
    m 2^shift - 1, and one ordinary cell."""
    res = lay.res[l]
    if P.merge[l]:
        return sorted({1, res // 3, res // 2})
    cells, seen = {res // 3}, set()
    step, s, ones = _level_x_pairs(lay, P, l)
    for k in range(res):
        key = (min(int(step[k]), 3), int(s[k]), int(ones[k]))
        if key not in seen:
            seen.add(key)
            cells.add(k)
    if lay.kind[l] == 0:
        for mm in (1, 2, 3):
            for d in (-2, -1, 0):
                c = (mm << P.shift) + d
                if 0 <= c < res:
                    cells.add(c)
    return sorted(cells)


# ------------------------------------------------------------------------------------ spotlight points
@dataclass
class Spotlights:
    x: torch.Tensor       # (S, 3) f32
    dy: torch.Tensor      # (S, 2 L) f32, non-zero only at the spotlight's level
    level: np.ndarray     # (S,)
    cell: np.ndarray      # (S, 3) the cell the oracle puts the point in at its level
    f: np.ndarray         # (S,) the x fraction asked for
    cls: list             # (S,) record class
    ones: np.ndarray      # (S,) trailing ones the record would carry
    s: np.ndarray         # (S,) the pair mask's shift
    entries: np.ndarray   # (S, 8) absolute entries of the 8 corners (corner c: bit 0 = x)
    weights: np.ndarray   # (S, 8) f64 trilinear weights
    dropped: int          # candidates that missed their cell or stayed invisible

    def describe(self, entry):
        """The spotlights with a corner at `entry`: 'class level cell' for a failure message."""
        rows = np.nonzero((self.entries == entry).any(1))[0]
        return [f"{self.cls[k]} level {self.level[k]} cell {tuple(int(v) for v in self.cell[k])} f {self.f[k]:.4f}"
                for k in rows[:4]]


def _spot_corners(olay, x, level):
    S = x.shape[0]
    ent, wts, cell = np.zeros((S, 8), np.int64), np.zeros((S, 8)), np.zeros((S, 3), np.int64)
    for l in sorted(set(level.tolist())):
        sel = np.nonzero(level == l)[0]
        g, w = _geo(olay, l, x[torch.from_numpy(sel)])
        cell[sel] = g.numpy()
        for c in range(8):
            idx, wt = _corner(olay, l, g, w, c)
            ent[sel, c] = idx
            wts[sel, c] = wt[0] * wt[1] * wt[2]
    return ent, wts, cell


def _invisible(x, dy, level, lay, olay):
    """Spotlights with a corner contribution (either feature) <= 4 x the bound at its entry."""
    bound = entry_terms(x, dy, lay, olay).bound.numpy()
    ent, wts, _ = _spot_corners(olay, x, level)
    mag = np.abs(dy.double().numpy()[np.arange(len(level))[:, None], 2 * level[:, None] + np.arange(2)[None]])  # (S,2)
    contrib = wts[:, :, None] * mag[:, None, :]                      # (S, 8, 2)
    b = bound[2 * ent[:, :, None] + np.arange(2)[None, None]]      # (S, 8, 2)
    return ~(contrib > 4 * b).all((1, 2))


def spotlights(lay, olay, seed=0):
    """Sparse points aimed at chosen x cells of every binned level (module docstring of the tests):
    x = (g0 + f - 0.5) / scale_l in fp32 for f in SPOT_F, y and z in a random cell with weights in
    [0.25, 0.75], dy non-zero (magnitude in [0.5, 2]) only at the level.  A point whose fp32 pos does
    not land in cell g0 (or outside [0, 1]) is dropped; one whose eight contributions are not all above
    4 x the bound at their entries gets new y, z (five rounds), then is dropped too."""
    P = GP.bin_plan(lay)
    rng = np.random.default_rng(seed)
    lv, g0, ff = [], [], []
    for l in P.level:
        for c in target_cells(lay, P, l):
            for f in SPOT_F:
                lv.append(l); g0.append(c); ff.append(f)
    lv, g0, ff = np.array(lv), np.array(g0, np.int64), np.array(ff)
    S = len(lv)
    scale = np.array([lay.scales[l] for l in lv], np.float64)
    res = np.array([lay.res[l] for l in lv], np.int64)

    def draw_yz(k):
        cells = rng.integers(1, np.maximum(res[k] - 2, 2))[:, None] * np.ones((1, 2), np.int64)
        cells[:, 1] = rng.integers(1, np.maximum(res[k] - 2, 2))
        return ((cells + rng.uniform(0.25, 0.75, (len(k), 2)) - 0.5) / scale[k, None]).astype(np.float32)

    x = np.zeros((S, 3), np.float32)
    x[:, 0] = ((g0 + ff - 0.5) / scale).astype(np.float32)
    x[:, 1:] = draw_yz(np.arange(S))
    dy = np.zeros((S, 2 * lay.L), np.float32)
    mag = rng.uniform(0.5, 2.0, (S, 2)) * rng.choice([-1.0, 1.0], (S, 2))
    dy[np.arange(S), 2 * lv] = mag[:, 0]
    dy[np.arange(S), 2 * lv + 1] = mag[:, 1]
    xt = torch.from_numpy(x)
    _, _, cell = _spot_corners(olay, xt, lv)
    keep = (cell[:, 0] == g0) & (x >= 0).all(1) & (x <= 1).all(1)
    for rnd in range(6):
        idx = np.nonzero(keep)[0]
        bad = _invisible(torch.from_numpy(x[idx]), torch.from_numpy(dy[idx]), lv[idx], lay, olay)
        if not bad.any():
            break
        if rnd == 5:
            keep[idx[bad]] = False
        else:
            x[idx[bad], 1:] = draw_yz(idx[bad])
    idx = np.nonzero(keep)[0]
    xt, dyt, lv, ff = torch.from_numpy(x[idx].copy()), torch.from_numpy(dy[idx].copy()), lv[idx], ff[idx]
    ent, wts, cell = _spot_corners(olay, xt, lv)
    info = [record_class(lay, olay, P, int(lv[k]), [int(v) for v in cell[k]]) for k in range(len(idx))]
    return Spotlights(xt, dyt, lv, cell, ff, [i[0] for i in info], np.array([i[1] for i in info]),
                      np.array([i[2] for i in info]), ent, wts, S - len(idx))


# ------------------------------------------------------------------------------------------------ runs
def run_points(lengths, seed=0, near=2.0 ** -22, lo=0.2, hi=0.8):
    """'Rays' of consecutive samples in one cell: run k is lengths[k] copies of a random point --
    identical for even k, each 2^-22 further along a random direction for odd k (the coarse levels'
    cell stays, the finest levels' changes now and then).  -> (x (N,3) f32, run starts)."""
    rng = np.random.default_rng(seed)
    xs, starts, n = [], [], 0
    for k, m in enumerate(lengths):
        p = rng.uniform(lo, hi, 3)
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        t = np.arange(m)[:, None] * (near if k % 2 else 0.0)
        xs.append(p[None] + t * d[None])
        starts.append(n)
        n += m
    return torch.from_numpy(np.concatenate(xs).astype(np.float32)), starts


def run_case(lay, lengths, seed=0, levels=None, mag=1e-3):
    """(x, dy) of run_points with a random dy (only `levels` non-zero where given), one zero-gradient
    sample in the middle of every run of >= 15 samples."""
    x, starts = run_points(lengths, seed)
    g = torch.Generator().manual_seed(seed + 1)
    dy = torch.randn(x.shape[0], 2 * lay.L, generator=g) * mag
    if levels is not None:
        keep = torch.zeros(2 * lay.L)
        for l in levels:
            keep[2 * l:2 * l + 2] = 1.0
        dy = dy * keep
    for s0, m in zip(starts, lengths):
        if m >= 15:
            dy[s0 + m // 2] = 0.0
    return x, dy


# --------------------------------------------------------------------- record counts of the PAIR layout
def pair_record_counts(lay, olay, P, x):
    """(n_bins, UNITS) records per (partition, scatter unit) of a PAIR layout (one record per sample,
    binned level and (y,z) row, in the partition of the row's x corner; every dy non-zero)."""
    assert P.pair_ok
    n = x.shape[0]
    unit = (np.arange(n) // 16) % GP.UNITS
    counts = np.zeros((P.n_bins, GP.UNITS), np.int64)
    for l in P.level:
        g, _ = _geo(olay, l, x)
        for yz in range(4):
            i0 = FO.grid_index(olay, l, g[:, 0], g[:, 1] + (yz & 1), g[:, 2] + (yz >> 1)).numpy()
            np.add.at(counts, (P.t_bin0[P.table_of[l]] + (i0 >> P.shift), unit), 1)
    return counts


def point_with_single_row_partition(lay, olay, P, seed=0):
    """An interior point some partition of which receives exactly ONE (level, row) record per sample
    (so N samples at it give that partition N records) and another two, as a (1,3) f32 tensor."""
    rng = np.random.default_rng(seed)
    for _ in range(200):
        x = torch.from_numpy(rng.uniform(0.3, 0.7, (1, 3)).astype(np.float32))
        c = pair_record_counts(lay, olay, P, x).sum(1)
        if (c == 1).any() and (c == 2).any():
            return x
    raise AssertionError("no such point")


def points_in_last_partition(lay, olay, P, n, seed=0):
    """n points of [0.2, 0.8]^3 with a corner of a binned level in the LAST partition of its table."""
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.uniform(0.2, 0.8, (4000, 3)).astype(np.float32))
    hit = np.zeros(x.shape[0], bool)
    for l in P.level:
        t = P.table_of[l]
        first = ((P.t_bin0[t + 1] - P.t_bin0[t] - 1) << P.shift) + olay.offsets[l]
        g, w = _geo(olay, l, x)
        for c in range(8):
            hit |= _corner(olay, l, g, w, c)[0] >= first
    assert hit.sum() >= n
    return x[torch.from_numpy(np.nonzero(hit)[0][:n])]


# ------------------------------------------------------------------------------------- the suite's cases
LEGO = (16, 2, 19, 16, GP.b_of(1024), "Hash", 1)
SMALL_T = (8, 2, 10, 4, 8 ** (1 / 7), "Hash", 1)
SUITE_LAYOUTS = dict(GP.SEAM_LAYOUTS, lego=LEGO, small_T=SMALL_T)  # every layout test_gpu_grid_seams.py runs


def layouts(name):
    """(library layout, oracle layout) of a suite layout."""
    from mfnerf.grid import GridLayout
    return GridLayout(*SUITE_LAYOUTS[name]), FO.GridLayout(*SUITE_LAYOUTS[name])


def ray_points(n, seed=0, S=64):
    """n training-shaped points: rays of S consecutive samples, sqrt(3) / 1024 apart."""
    g = torch.Generator().manual_seed(seed)
    R = (n + S - 1) // S
    o = torch.rand(R, 1, 3, generator=g) * 0.6 + 0.2
    d = torch.nn.functional.normalize(torch.randn(R, 1, 3, generator=g), dim=-1)
    x = (o + d * (torch.arange(S).view(1, S, 1) * (3 ** 0.5 / 1024))).clamp(0, 1).reshape(-1, 3)
    return x[:n].contiguous()


def random_points(n, seed=0):
    """n uniform points with the unit cube's eight corners first."""
    x = torch.rand(n, 3, generator=torch.Generator().manual_seed(seed))
    k = min(n, 8)
    x[:k] = torch.tensor([[(c >> d) & 1 for d in range(3)] for c in range(8)], dtype=torch.float32)[:k]
    return x


# The dense-level kernel gives a wave a window of ceil(n / (64 DENSE_WAVES)) chunks of 64 samples and
# carries the run open at a chunk's end into the window's next chunk.  Above 131,072 live samples the
# window holds two chunks (128 samples).  Runs of identical samples as (first sample, length):
DENSE_N = 131072 + 9000 + 5
DENSE_RUNS = {"chunk+window+chunk": (128 * 100 + 30, 200),  # samples 30 .. 229 of the windows from 100 on
              "chunk boundary inside a window": (128 * 300 + 44, 40),
              "window boundary": (128 * 500 + 108, 40)}


def dense_window_case(lay, seed=0):
    """(x, dy) for the dense-level kernel's carried run: DENSE_N ray-shaped samples with DENSE_RUNS
    written over them, dy non-zero only at the dense levels (those before the first binned one), one
    zero-gradient sample inside the 200-sample run."""
    x = ray_points(DENSE_N, seed)
    rng = np.random.default_rng(seed)
    for s0, m in DENSE_RUNS.values():
        x[s0:s0 + m] = torch.from_numpy(rng.uniform(0.3, 0.7, (1, 3)).astype(np.float32))
    dy = torch.randn(DENSE_N, 2 * lay.L, generator=torch.Generator().manual_seed(seed + 1)) * 1e-3
    dy[:, 2 * GP.first_binned_level(lay):] = 0.0
    dy[DENSE_RUNS["chunk+window+chunk"][0] + 77] = 0.0
    return x, dy


# Accumulate chunks: every sample at ONE interior point of the small-T (PAIR) layout, so a partition
# that one (level, row) of the point falls in receives exactly one record per sample.
ACCUM_N = (4096, 4099, 12293)


def accum_chunk_cases(lay, olay, P, seed=0):
    """[(N, x (N,3), counts (n_bins, UNITS), slot, T (n_bins,))] for ACCUM_N samples at one point."""
    p = point_with_single_row_partition(lay, olay, P, seed)
    rows = pair_record_counts(lay, olay, P, p).sum(1)  # (level, row) records per sample and partition
    out = []
    for n in ACCUM_N:
        per_unit = np.bincount((np.arange(n) // 16) % GP.UNITS, minlength=GP.UNITS)
        counts = rows[:, None] * per_unit[None]
        slot = GP.slot_size(n, P)
        out.append((n, p.repeat(n, 1).contiguous(), counts, slot, GP.partition_record_counts(counts, slot)))
    return out


_SPOTS = {}


def spot_case(name):
    """The suite's spotlights of a layout (built once per process)."""
    if name not in _SPOTS:
        _SPOTS[name] = spotlights(*layouts(name), seed=1)
    return _SPOTS[name]
