"""The hash-grid forward (csrc/grid_fw.hip) against fp64 under a derived bound of one fp16 rounding,
the kernel restated in fp32 numpy with four wrong variants, the census of what planar_gather does
per (level, (y,z) row), and the layouts of tests/test_gpu_grid_fw_seams.py (test infrastructure, no
test in here).  Everything is numpy on the CPU; the corner indices are the oracle's
(oracle.field_oracle.grid_index), the cell and weights come from the fp32 pos the kernels take
(input_grad_ref._geo); the library is not imported for any arithmetic.

THE BOUND.  For an output (sample, level, feature) with the 8 corners' weights w_c and fp16 table
values f_c, ref = sum_c w_c f_c in fp64 and A = sum_c |w_c f_c|.
  * w = pos - floor(pos) is exact in fp32, and for pos >= 0.5 (x01 >= 0) a multiple of 2^-24, so 1 - w
    is exact too; counted as one rounding all the same.  corner_weight multiplies three factors: two
    rounded products.  A corner weight is rounded at most 3 times, each by <= 2^-24 of its value;
  * the 8 fmas (exact product, one rounding of the running sum) round 8 times, each by <= 2^-24 of a
    partial sum <= A;
so |acc32 - ref| <= 11 x 2^-24 x A, and e = 12 x 2^-24 x A covers the second-order terms.  The output
is ONE round-to-nearest-even fp16 conversion of acc32, and rounding is monotonic:
    rn16(ref - e) <= got <= rn16(ref + e)
with rn16 numpy's float64 -> float16 cast (a single rounding; torch's CPU cast goes through fp32).
For ~98.5 % of the outputs both ends are the same fp16 value: the kernel must hit rn16(ref) exactly.
Nothing in this is measured and nothing is scaled by a tensor's maximum.
"""
import collections
from dataclasses import dataclass

import numpy as np
import torch

import grid_plan_ref as GP
import grid_seam_ref as GS
from input_grad_ref import _geo
from oracle import field_oracle as FO

E_REL = 12 * 2.0 ** -24
VARIANTS = ("kernel", "no_fma_pos", "truncate_f16", "half_accumulate", "swap_x_corner_on_odd_rows")
NAN16 = 0x7E00  # the bits torch.full(..., nan, dtype=float16) writes

# ------------------------------------------------------------------------------------------- layouts
LEVEL_LAYOUTS = {
    "L4": (4, 2, 12, 8, 2.0, "Hash", 1),
    "L12": (12, 2, 14, 16, GP.b_of(512, 16, 12), "Hash", 1),
    "L20": (20, 2, 14, 16, GP.b_of(4096, 16, 20), "MixedFeature", 3),
    "L32": (32, 2, 12, 16, GP.b_of(2048, 16, 32), "Hash", 1),
}
ODD_SIZES = [67, 216, 515, 1001, 1021, 2, 3, 1000]
ODD_RES = [4, 6, 8, 10, 14, 18, 24, 32]


def odd_tables():
    """(library layout, oracle layout) of the small-T layout with hand-patched tables: sizes ODD_SIZES,
    offsets their running sum (odd at levels 1, 2, 4 and 7).  Levels 0-3 stay dense (res^3 <= size); 4-7 are
    hashed with an odd, a 2-entry, a 3-entry and an even non-power-of-two table.  No layout GridLayout
    builds has these; check_desc accepts them through the C ABI."""
    from mfnerf.grid import GridLayout
    lay, olay = GridLayout(*GS.SMALL_T), FO.GridLayout(*GS.SMALL_T)
    assert lay.res == ODD_RES and olay.res == ODD_RES
    offs = [int(v) for v in np.cumsum([0] + ODD_SIZES[:-1])]
    for o in (lay, olay):
        o.sizes, o.offsets = list(ODD_SIZES), list(offs)
        o.n_entries = sum(ODD_SIZES)
        o.n_params = 2 * o.n_entries
    return lay, olay


def layouts(name):
    """(library layout, oracle layout) of a suite layout, a level-count layout or odd_tables."""
    if name == "odd_tables":
        return odd_tables()
    if name in LEVEL_LAYOUTS:
        from mfnerf.grid import GridLayout
        return GridLayout(*LEVEL_LAYOUTS[name]), FO.GridLayout(*LEVEL_LAYOUTS[name])
    return GS.layouts(name)


TABLES = ("unit", "init", "wide")


def table16(kind, n_params, seed=0):
    """An fp16 table (n_params,): 'unit' U(-0.5, 0.5) as every other test; 'init' tcnn's U(-1e-4, 1e-4)
    (at and below fp16's smallest normal 6.1e-5); 'wide' randn x 2^randint(-8, 4)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "unit":
        t = torch.rand(n_params, generator=g) - 0.5
    elif kind == "init":
        t = (torch.rand(n_params, generator=g) - 0.5) * 2e-4
    elif kind == "wide":
        t = torch.randn(n_params, generator=g) * torch.exp2(torch.randint(-8, 5, (n_params,), generator=g).float())
    else:
        raise ValueError(kind)
    return t.half()


LAYOUT_CASES = ("lego", "small_T", "E", "F", "G", "H", "odd_tables")
LEVEL_CASES = ("L4", "small_T", "L12", "L20", "L32")


def layout_points():
    """The 4099 points of the layout cases: uniform, the unit cube's eight corners first."""
    return GS.random_points(4099, seed=4)


# The grid-stride case: the row-major kernel strides above 8192 blocks of 256 threads, L / 4 threads a
# point; the planar kernel above 2048 blocks of 256 samples per level group.
STRIDE_N = 524288 + 256 + 3
STRIDE_PERIOD = 8191  # prime, 524288 % 8191 == 64: a sample read one stride off is another point


def stride_base():
    """The STRIDE_PERIOD distinct points the grid-stride case repeats: x[i] = base[i % STRIDE_PERIOD]."""
    return GS.random_points(STRIDE_PERIOD, seed=6)


# ------------------------------------------------------------------------------------------ geometry
@dataclass
class Geo:
    w: np.ndarray    # (L, n, 3) f32  pos - floor(pos)
    idx: np.ndarray  # (L, 8, n) i64  absolute entry of corner c (bit 0 = x, 1 = y, 2 = z)


def _np(t, dtype=None):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a if dtype is None else a.astype(dtype)


def geometry(olay, x01, fma=True):
    """The cells, weights and oracle corner indices of every level.  fma: pos = fmaf(scale, x, 0.5)
    (evaluated in fp64, rounded once: input_grad_ref._geo); else scale * x rounded, then + 0.5 rounded."""
    x01 = torch.as_tensor(x01, dtype=torch.float32)
    n, L = x01.shape[0], olay.L
    w = np.zeros((L, n, 3), np.float32)
    idx = np.zeros((L, 8, n), np.int64)
    for l in range(L):
        if fma:
            g, wl = _geo(olay, l, x01)
            w[l] = wl.numpy().astype(np.float32)  # exact: pos - floor(pos) of an fp32 pos
        else:
            pos = x01.numpy() * np.float32(olay.scales[l]) + np.float32(0.5)
            assert pos.dtype == np.float32
            fl = np.floor(pos)
            w[l] = pos - fl
            g = torch.from_numpy(fl.astype(np.int64))
        for c in range(8):
            idx[l, c] = FO.grid_index(olay, l, g[:, 0] + (c & 1), g[:, 1] + ((c >> 1) & 1),
                                      g[:, 2] + ((c >> 2) & 1)).numpy() + olay.offsets[l]
    return Geo(w, idx)


def forward_ref(x01, table16, olay, geo=None):
    """(ref, A), both (n, L*F) f64 numpy: the encoding of x01 (normalised: input_grad_ref.normalise)
    with the products and the sum in fp64, and the sum of the 8 terms' absolute values."""
    geo = geo or geometry(olay, x01)
    L, _, n = geo.idx.shape
    tab = _np(table16)
    assert tab.dtype == np.float16
    tab = tab.reshape(-1, 2)
    ref, A = np.zeros((n, 2 * L)), np.zeros((n, 2 * L))
    for l in range(L):
        w = geo.w[l].astype(np.float64)
        for c in range(8):
            wt = np.ones(n)
            for d in range(3):
                wt = wt * (w[:, d] if (c >> d) & 1 else 1.0 - w[:, d])
            term = wt[:, None] * tab[geo.idx[l, c]].astype(np.float64)
            ref[:, 2 * l:2 * l + 2] += term
            A[:, 2 * l:2 * l + 2] += np.abs(term)
    return ref, A


# --------------------------------------------------------------------------------------- the bound
def interval(ref, A):
    """(rn16(ref - e), rn16(ref + e), e): the fp16 values a correct kernel can return."""
    e = E_REL * A
    with np.errstate(over="ignore"):
        return (ref - e).astype(np.float16), (ref + e).astype(np.float16), e


def outside(got16, ref, A):
    """Boolean (n, L*F): outputs outside [rn16(ref - e), rn16(ref + e)] (a NaN is outside)."""
    lo, hi, _ = interval(ref, A)
    got = _np(got16).astype(np.float32)
    return ~((got >= lo.astype(np.float32)) & (got <= hi.astype(np.float32)))


def check(got16, ref, A, what, olay=None, x01=None):
    """Assert the bound on every output; print the share of outputs bit-equal to rn16(ref) and the
    share whose interval holds more than one fp16 value.  A failure names the sample, the level, the
    feature, got, ref, e and (given olay and x01) the gather classes of the sample's rows at the level.
    -> {'n', 'exact', 'multi'}."""
    got = _np(got16)
    assert got.dtype == np.float16 and got.shape == ref.shape == A.shape, (got.dtype, got.shape, ref.shape)
    lo, hi, e = interval(ref, A)
    bad = outside(got, ref, A)
    with np.errstate(over="ignore"):
        r16 = ref.astype(np.float16)
    n = max(got.size, 1)
    stats = {"n": got.size, "exact": float((got.view(np.int16) == r16.view(np.int16)).sum()) / n,
             "multi": float((lo != hi).sum()) / n}
    print(f"{what}: {got.size} outputs, bit-equal to rn16(ref) {stats['exact']:.5f}, "
          f"interval of more than one fp16 value {stats['multi']:.5f}")
    if bad.any():
        i, j = (int(v) for v in np.argwhere(bad)[0])
        l, f = j // 2, j % 2
        rows = ""
        if olay is not None and x01 is not None:
            rc = row_classes(olay, torch.as_tensor(x01, dtype=torch.float32)[i:i + 1])
            rows = f", level kind {rc.kind[l]}, rows {[flag_name(int(v)) for v in rc.flags[l, 0]]}"
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.size} outputs outside the bound; first: sample {i} "
                             f"level {l} feature {f} got {float(got[i, j])!r} ref {float(ref[i, j])!r} "
                             f"e {float(e[i, j])!r} allowed [{float(lo[i, j])!r}, {float(hi[i, j])!r}]{rows}")
    return stats


# ------------------------------------------------------------------------ what planar_gather does per row
CLAMPED, X_IN_UY, IN_U, X1_NOT_A, SAME = 1, 2, 4, 8, 16  # raw != a, i0 != a, in_u, i1 != a, i0 == i1


def flag_name(f):
    s = ("clamped " if f & CLAMPED else "") + ("x in u.y" if f & X_IN_UY else "x in u.x")
    s += (", x+1 in u" + (".x" if not f & X1_NOT_A else ".y")) if f & IN_U else ", x+1 single"
    return s + (", i0 == i1" if f & SAME else "")


def level_kind(olay, l):
    """(table, size class): dense / hashed (own table) / MixedFeature x pow2 / even / odd."""
    size, res = olay.sizes[l], olay.res[l]
    table = "MixedFeature" if olay.table_of_level[l] >= 0 else "dense" if res ** 3 <= size else "hashed"
    return table, "pow2" if size & (size - 1) == 0 else "even" if size % 2 == 0 else "odd"


@dataclass
class Rows:
    kind: list         # per level: level_kind
    flags: np.ndarray  # (L, n, 4) u8: the row yz = (y bit) + 2 (z bit) of every sample

    def census(self):
        """Counter of (table, size class, flags) over every (level, sample, row)."""
        c = collections.Counter()
        for l, k in enumerate(self.kind):
            v, m = np.unique(self.flags[l], return_counts=True)
            for f, cnt in zip(v, m):
                c[k + (int(f),)] += int(cnt)
        return c


def row_classes(olay, x01, geo=None):
    """planar_gather's decisions restated from the oracle's indices: per (level, row) the 8-byte load
    starts at a = min(dense ? i0 : i0 & ~1, size - 2); the x corner is u.y where i0 != a; the x+1
    corner is in u where i1 - a < 2 (as u.y where i1 != a), else loaded singly."""
    geo = geo or geometry(olay, x01)
    L, _, n = geo.idx.shape
    flags = np.zeros((L, n, 4), np.uint8)
    for l in range(L):
        size = olay.sizes[l]
        assert size >= 2
        dense = level_kind(olay, l)[0] == "dense"
        for yz in range(4):
            i0, i1 = geo.idx[l, 2 * yz] - olay.offsets[l], geo.idx[l, 2 * yz + 1] - olay.offsets[l]
            raw = i0 if dense else i0 & ~1
            a = np.minimum(raw, size - 2)
            in_u = (i1 == a) | (i1 == a + 1)
            flags[l, :, yz] = (CLAMPED * (raw != a) + X_IN_UY * (i0 != a) + IN_U * in_u + X1_NOT_A * (i1 != a) +
                               SAME * (i0 == i1))
    return Rows([level_kind(olay, l) for l in range(olay.L)], flags)


# Predicates over a census key (table, size class, flags): the classes the GPU tests' inputs must reach.
DENSE_CLASSES = {
    "dense ordinary": lambda t, s, f: t == "dense" and f & (CLAMPED | X_IN_UY | IN_U | X1_NOT_A) == IN_U | X1_NOT_A,
    "dense last entry (clamped, x+1 single)": lambda t, s, f: t == "dense" and f & CLAMPED and not f & IN_U,
}
EVEN_CLASSES = {
    f"{t} {'x in u.y' if uy else 'x in u.x'}, {'x+1 in u' if iu else 'x+1 single'}":
        (lambda t, uy, iu: lambda tt, s, f: tt == t and s != "odd" and not f & CLAMPED and
         bool(f & X_IN_UY) == uy and bool(f & IN_U) == iu)(t, uy, iu)
    for t in ("hashed", "MixedFeature") for uy in (False, True) for iu in (False, True)
}
ODD_CLASSES = {
    "clamped single": lambda t, s, f: t == "hashed" and f & CLAMPED and not f & IN_U,
    "clamped pair (i1 == a)": lambda t, s, f: t == "hashed" and f & CLAMPED and f & IN_U and not f & X1_NOT_A,
    "i0 == i1": lambda t, s, f: bool(f & SAME),
}


def class_counts(census, classes):
    """{class name: rows of the census in it}."""
    return {name: sum(cnt for key, cnt in census.items() if pred(*key)) for name, pred in classes.items()}


# ------------------------------------------------------------------------- the kernel in fp32 numpy
def emulate_fw(x01, table16, olay, variant="kernel", geo=None):
    """grid_fw_kernel / grid_fw_planar_kernel restated in fp32 numpy -> (n, L*F) f16 numpy: the
    corners in order 0..7, the weight ((1 or 1 - w_x) * y factor) * z factor with every product rounded
    to fp32, each fmaf an exact product (fp64 holds it) plus one rounding of the sum, one
    round-to-nearest fp16 conversion at the end.  (The fp64 sum under an fmaf rounds once more before
    the fp32 rounding: a double rounding that moves a result by one fp32 ulp once in ~2^29 operations.)
    variant:
      kernel                     the kernel
      no_fma_pos                 pos = scale * x rounded, + 0.5 rounded
      truncate_f16               the fp16 conversion truncates
      half_accumulate            tcnn's own accumulation: the weight rounded to fp16, fp16 fmas
      swap_x_corner_on_odd_rows  the x and x+1 words of a row exchanged where i0 != a (the u.y rows)"""
    assert variant in VARIANTS, variant
    geo = geo or geometry(olay, x01, fma=variant != "no_fma_pos")
    L, _, n = geo.idx.shape
    tab = _np(table16)
    assert tab.dtype == np.float16
    tab = tab.reshape(-1, 2)
    swap = row_classes(olay, x01, geo).flags & X_IN_UY if variant == "swap_x_corner_on_odd_rows" else None
    half = variant == "half_accumulate"
    out = np.zeros((n, 2 * L), np.float16)
    for l in range(L):
        w = geo.w[l]
        omw = np.float32(1.0) - w
        acc = np.zeros((n, 2), np.float16 if half else np.float32)
        for c in range(8):
            idx = geo.idx[l, c]
            if swap is not None:
                idx = np.where(swap[l, :, c >> 1] != 0, geo.idx[l, c ^ 1], idx)
            wt = w[:, 0] if c & 1 else omw[:, 0]
            wt = wt * (w[:, 1] if c & 2 else omw[:, 1])
            wt = wt * (w[:, 2] if c & 4 else omw[:, 2])
            assert wt.dtype == np.float32
            if half:
                wt = wt.astype(np.float16)
            acc = (wt.astype(np.float64)[:, None] * tab[idx].astype(np.float64) + acc.astype(np.float64)).astype(acc.dtype)
        h = acc.astype(np.float16)
        if variant == "truncate_f16":
            over = np.abs(h.astype(np.float32)) > np.abs(acc)
            h[over] = np.nextafter(h[over], np.float16(0))
        out[:, 2 * l:2 * l + 2] = h
    return out
