"""Host mirror of the partitioned table-gradient scatter's plan (test infrastructure, no test in here).

A Python restatement of csrc/grid_bw_binned.hip's first_binned_level, bin_plan, slot_size and
binned_workspace_layout, of grid_common.hpp's check_desc and dense_entries_of, and of the template
choice binned_impl makes, for a mfnerf.grid.GridLayout.  tests/test_grid_plan_cpu.py proves it
against the library's own host queries; the GPU seam tests use it to say which kernel a layout runs
and to size their inputs (slots, record counts per partition).
"""
import math
from dataclasses import dataclass, field

MIN_BIN_SHIFT, MAX_BIN_SHIFT = 8, 11
UNITS = 256          # scatter workgroups
MAX_TBINS = 1024     # partitions of one table
MAX_BINS = 16384
MAX_BINNED = 16
GRAD_COPIES = 8      # private copies of the dense levels
ACC_RB = 4096        # records per stage chunk of the accumulate
SC_THREADS = 1024    # the scatter workgroup: a tile is SC_THREADS x (2 if PAIR else 1) samples per unit
DENSE_WAVES = 2048   # grid_bw_dense_kernel: a wave's window is ceil(n / (64 * DENSE_WAVES)) chunks of 64


def b_of(N, N_min=16, L=16):
    """The per-level scale whose finest level has (about) N cells: exp(log(N / N_min) / (L - 1))."""
    return math.exp(math.log(N / N_min) / (L - 1))


# GridLayout(L, F, log2_T, N_min, b, kind, n_tables) of the layouts the seam suite adds
SEAM_LAYOUTS = {
    "A": (16, 2, 18, 16, b_of(1024), "Hash", 1),
    "B": (16, 2, 18, 64, b_of(1024, 64), "Hash", 1),
    "C": (8, 2, 14, 16, b_of(2048, 16, 8), "Hash", 1),
    "D": (16, 2, 14, 16, b_of(32768), "Hash", 1),
    "E": (16, 2, 19, 16, b_of(32768), "Hash", 1),
    "F": (16, 2, 14, 16, b_of(131072), "Hash", 1),
    "G": (16, 2, 16, 16, b_of(1024), "MixedFeature", 3),
    "H": (16, 2, 16, 16, b_of(32768), "MixedFeature", 4),
}


@dataclass
class Plan:
    n_binned: int = 0
    n_bins: int = 0
    n_tables: int = 0
    shift: int = 0
    pair_ok: int = 1
    level: list = field(default_factory=list)      # the binned levels
    pairable: dict = field(default_factory=dict)   # per binned level
    merge: dict = field(default_factory=dict)      # per binned level
    table_of: dict = field(default_factory=dict)   # per binned level: its table
    t_offset: list = field(default_factory=list)   # per table (entries)
    t_size: list = field(default_factory=list)
    t_bin0: list = field(default_factory=list)     # first partition of each table; [n_tables] = n_bins
    t_level: list = field(default_factory=list)
    canon_step: dict = field(default_factory=dict)  # per binned level of a shared table: canon_res / res

    @property
    def instantiation(self):
        """(MAXB, PAIR) of the bin_scatter_kernel binned_impl launches."""
        if self.pair_ok:
            return (8 if self.n_binned <= 8 else 10 if self.n_binned <= 10 else 12 if self.n_binned <= 12
                    else MAX_BINNED), True
        return (8 if self.n_binned <= 8 else 12 if self.n_binned <= 12 else MAX_BINNED), False

    @property
    def first_value(self):
        """mfnerf_grid_binned_first_value: the first value (2 per entry) of the partitioned tables."""
        return 2 * self.t_offset[0] if self.n_bins > 0 else -1

    def last_partition_entries(self, t):
        """Entries of table t's last partition (n_e of bin_accum_kernel; < 2^shift: partial)."""
        return self.t_size[t] - ((self.t_bin0[t + 1] - self.t_bin0[t] - 1) << self.shift)


def check_desc(lay):
    if lay.F != 2 or lay.L <= 0 or lay.L > 32 or lay.L % 4:
        return False
    for l in range(lay.L):
        if lay.sizes[l] == 0 or lay.res[l] == 0:
            return False
        if lay.kind[l] == 1 and (lay.res[l] + 2) * lay.canon_res >= 1 << 31:
            return False
    return True


def dense_entries(lay):
    e = 0
    for l in range(lay.L):
        if lay.kind[l] != 0 or lay.res[l] ** 3 > lay.sizes[l] or lay.offsets[l] != e:
            break
        e += lay.sizes[l]
    return e


def first_binned_level(lay):
    first_hashed = lay.L
    for l in range(lay.L):
        if not (lay.kind[l] == 0 and lay.res[l] ** 3 <= lay.sizes[l]):
            first_hashed = l
            break
    l0 = first_hashed
    moved = True
    while moved:
        moved = False
        for a in range(first_hashed, l0):
            for b in range(l0, lay.L):
                if lay.offsets[a] == lay.offsets[b]:
                    l0, moved = a, True
                    break
            if moved:
                break
    return l0


def bin_plan(lay):
    """The Plan of a layout, or None where bin_plan() returns -1."""
    P = Plan()
    entries, max_x = 0, 0
    for l in range(first_binned_level(lay), lay.L):
        if lay.offsets[l] in P.t_offset:
            t = P.t_offset.index(lay.offsets[l])
        else:
            t = P.n_tables
            P.t_offset.append(lay.offsets[l])
            P.t_size.append(lay.sizes[l])
            P.t_level.append(l)
            P.n_tables += 1
            entries += lay.sizes[l]
        pow2 = lay.sizes[l] & (lay.sizes[l] - 1) == 0
        P.table_of[l] = t
        P.pairable[l] = int(lay.kind[l] == 0 and pow2)
        P.merge[l] = int(lay.canon_res >= 3 * lay.res[l]) if lay.kind[l] == 1 else int(not P.pairable[l])
        if lay.kind[l] == 1:
            P.canon_step[l] = lay.canon_res / lay.res[l]
        P.level.append(l)
        max_x = max(max_x, lay.canon_res if lay.kind[l] == 1 else lay.res[l])
    P.n_binned = len(P.level)
    if any(s == 0 for s in P.t_size):
        return None
    P.shift = MAX_BIN_SHIFT
    while P.shift > MIN_BIN_SHIFT and (entries >> P.shift) < 1024:
        P.shift -= 1
    nb = 0
    for t in range(P.n_tables):
        P.t_bin0.append(nb)
        nb += (P.t_size[t] + (1 << P.shift) - 1) >> P.shift
        if P.t_size[t] & (P.t_size[t] - 1) or max_x >= 1 << P.shift:
            P.pair_ok = 0
    if not all(P.pairable[l] for l in P.level):
        P.pair_ok = 0
    P.t_bin0.append(nb)
    P.n_bins = nb
    if P.n_binned > MAX_BINNED:
        return None
    if any(P.level[j] != P.level[0] + j for j in range(P.n_binned)):
        return None
    if any(P.t_bin0[t + 1] - P.t_bin0[t] > MAX_TBINS for t in range(P.n_tables)):
        return None
    return None if nb > MAX_BINS else P


def slot_size(nn, P):
    """Records per (partition, unit) slot at live count nn."""
    recs = nn * P.n_binned * (4 if P.pair_ok else 8)
    s = 3 * ((recs + P.n_bins * UNITS - 1) // (P.n_bins * UNITS)) + 96
    return (s + 15) // 16 * 16


def _align256(b):
    return (b + 255) // 256 * 256


def workspace_layout(lay, n_max):
    """Byte offsets {priv, ovw, scnt, smax, ovf, rec, end} of binned_workspace_layout, or None (-1)."""
    if not check_desc(lay) or n_max < 0:
        return None
    P = bin_plan(lay)
    if P is None:
        return None
    W = {"priv": 0}
    off = _align256(GRAD_COPIES * dense_entries(lay) * 2 * 4)
    W["ovw"] = off
    off += _align256(sum(P.t_size) * 8)
    nb = P.n_bins if P.n_bins > 0 else 1
    W["scnt"] = off
    off += _align256(nb * UNITS * 4)
    W["smax"] = off
    off += _align256(UNITS * 4)
    W["ovf"] = off
    off += 256
    W["rec"] = off
    if nb * UNITS * slot_size(n_max, P) >= 1 << 31:
        return None
    off += _align256(nb * UNITS * slot_size(n_max, P) * 8)
    W["end"] = off
    return W


def workspace_bytes(lay, n_max):
    W = workspace_layout(lay, n_max)
    return -1 if W is None else W["end"]


def dense_values(lay):
    return 2 * dense_entries(lay) if check_desc(lay) else -1


def first_value(lay):
    if not check_desc(lay):
        return -1
    P = bin_plan(lay)
    return P.first_value if P is not None and P.n_bins > 0 else -1


def unit_of_sample(i):
    """The scatter unit (workgroup) that owns sample i: 16-sample chunk i // 16 goes to unit chunk % UNITS."""
    return (i // 16) % UNITS


def partition_record_counts(counts, slot):
    """The accumulate's compacted record count T per partition from the (n_bins, UNITS) record counts:
    every slot's count capped at the slot and rounded up to even."""
    import numpy as np
    c = np.minimum(np.asarray(counts, np.int64), slot)
    return ((c + 1) & ~1).sum(1)
