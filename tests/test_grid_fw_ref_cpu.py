"""tests/grid_fw_ref.py proven on the host: the faithful fp32 emulation of the forward kernels lies
inside the derived bound on every layout and table, each wrong variant lies outside it (two of them
inside the suite's old atol=1e-3), the inputs of tests/test_gpu_grid_fw_seams.py reach every gather
class of planar_gather, and the grid-stride case crosses both kernels' block caps."""
import numpy as np
import pytest
import torch

import grid_fw_ref as FW
import grid_seam_ref as GS

BOUND_LAYOUTS = ["lego", "E", "F", "G", "H", "odd_tables"]
_CASE = {}


def _case(name):
    """(oracle layout, x01, {fma: Geo}, {table kind: (table, ref, A)}) of 6000 random points, built once."""
    if name not in _CASE:
        _, olay = FW.layouts(name)
        x = GS.random_points(6000)
        geos = {True: FW.geometry(olay, x), False: FW.geometry(olay, x, fma=False)}
        tabs = {}
        for k, kind in enumerate(FW.TABLES):
            t = FW.table16(kind, olay.n_params, seed=20 + k)
            tabs[kind] = (t,) + FW.forward_ref(x, t, olay, geos[True])
        _CASE[name] = (olay, x, geos, tabs)
    return _CASE[name]


def _emulate(name, kind, variant):
    olay, x, geos, tabs = _case(name)
    return FW.emulate_fw(x, tabs[kind][0], olay, variant, geos[variant != "no_fma_pos"])


@pytest.mark.parametrize("name", BOUND_LAYOUTS)
def test_faithful_emulation_is_inside_the_bound(name):
    olay, x, geos, tabs = _case(name)
    for kind in FW.TABLES:
        t, ref, A = tabs[kind]
        got = _emulate(name, kind, "kernel")
        st = FW.check(got, ref, A, f"emulation {name} {kind}", olay, x)
        # the bound is not vacuous: nearly every interval is ONE fp16 value, which the emulation hits
        assert st["exact"] >= 0.999 and 0.0 < st["multi"] < 0.05
    assert float(np.abs(tabs["init"][1]).max()) < 2.0 ** -13  # the init table's outputs: at fp16's subnormals


@pytest.mark.parametrize("variant", FW.VARIANTS[1:])
@pytest.mark.parametrize("name", BOUND_LAYOUTS)
def test_wrong_variants_are_outside_the_bound(name, variant):
    olay, x, geos, tabs = _case(name)
    counts = {}
    for kind in FW.TABLES:
        t, ref, A = tabs[kind]
        counts[kind] = int(FW.outside(_emulate(name, kind, variant), ref, A).sum())
    print(f"{variant} {name}: outputs outside the bound of {ref.size}: {counts}")
    assert counts["unit"] > 0
    with pytest.raises(AssertionError, match="outside the bound"):
        FW.check(_emulate(name, "unit", variant), tabs["unit"][1], tabs["unit"][2], f"{variant} {name}", olay, x)


@pytest.mark.parametrize("variant", ["no_fma_pos", "truncate_f16"])
@pytest.mark.parametrize("name", BOUND_LAYOUTS)
def test_the_old_tolerance_accepts_two_wrong_kernels(name, variant):
    """atol=1e-3 on |y| < 0.5 (two to eight fp16 ulps) passes a kernel that truncates the fp16 conversion
    on every output of every layout (max error 2.44e-4: one ulp), and one without the fma in pos on
    every output of lego, F, G and odd_tables (max 1.2e-4 .. 3.5e-4).  At E and H (res 32768: pos moves
    by up to 2^-9) ONE output of 192,000 of that kernel is past 1e-3 (1.04e-3, 1.15e-3, level 14) --
    the old tolerance sees 1 where the bound sees 45 to 50."""
    t, ref, A = _case(name)[3]["unit"]
    got = torch.from_numpy(_emulate(name, "unit", variant).astype(np.float32))
    n_out = int(FW.outside(got.numpy().astype(np.float16), ref, A).sum())
    if variant == "no_fma_pos" and name in ("E", "H"):
        over = int(((got.double() - torch.from_numpy(ref)).abs() > 1e-3).sum())
        print(f"{variant} {name}: {over} outputs past atol=1e-3, {n_out} outside the bound")
        assert over <= 1 and n_out >= 30
        return
    assert torch.allclose(got, torch.from_numpy(ref).float(), atol=1e-3, rtol=0)
    assert n_out > 0


def _census(name, x):
    _, olay = FW.layouts(name)
    return FW.row_classes(olay, x).census()


@pytest.mark.parametrize("name", FW.LAYOUT_CASES)
def test_the_layout_points_reach_every_gather_class(name):
    """The 4099 points of test_layouts: both dense classes, the four classes of every hashed /
    MixedFeature level kind the layout has, and on odd_tables the three the clamp and tiny tables add."""
    _, olay = FW.layouts(name)
    cen = _census(name, FW.layout_points())
    want = dict(FW.DENSE_CLASSES)
    tables = {FW.level_kind(olay, l)[0] for l in range(olay.L)}
    want.update({k: v for k, v in FW.EVEN_CLASSES.items() if k.split()[0] in tables})
    if name == "odd_tables":
        want.update(FW.ODD_CLASSES)
        assert {FW.level_kind(olay, l) for l in range(olay.L)} >= {("dense", "odd"), ("dense", "even"),
                                                                  ("hashed", "odd"), ("hashed", "pow2"),
                                                                  ("hashed", "even")}
    counts = FW.class_counts(cen, want)
    print(name, counts)
    print(name, {k[:2] + (FW.flag_name(k[2]),): v for k, v in sorted(cen.items())})
    assert all(v > 0 for v in counts.values()), counts


@pytest.mark.parametrize("name", ["C", "D", "E", "F", "G", "H"])
def test_the_spotlights_reach_the_hashed_classes(name):
    _, olay = FW.layouts(name)
    cen = _census(name, GS.spot_case(name).x)
    tables = {FW.level_kind(olay, l)[0] for l in range(olay.L)} - {"dense"}
    counts = FW.class_counts(cen, {k: v for k, v in FW.EVEN_CLASSES.items() if k.split()[0] in tables})
    print(name, counts)
    assert all(v > 0 for v in counts.values()), counts


def test_level_count_layouts():
    """L = 4, 8, 12, 20, 32: has_b == false on every group (4, 8), on some (12), and the second j
    iteration of the planar kernel (20: without lb, 32: with)."""
    Ls = {name: FW.layouts(name)[0].L for name in FW.LEVEL_CASES}
    assert sorted(Ls.values()) == [4, 8, 12, 20, 32]
    for name in FW.LEVEL_CASES:
        lay, olay = FW.layouts(name)
        assert (lay.sizes, lay.offsets, lay.res, lay.scales) == (olay.sizes, olay.offsets, olay.res, olay.scales)
        assert min(lay.sizes) >= 2
        # every level is stored by exactly one (group, j, a / b) of grid_fw_planar_kernel
        stored = []
        for grp in range(8):
            for m in range((lay.L + 15) // 16):
                la, lb = 16 * m + grp, 16 * m + 15 - grp
                if la < lay.L:
                    stored.append(la)
                    if lb < lay.L:
                        stored.append(lb)
        assert sorted(stored) == list(range(lay.L))
    assert FW.layouts("L20")[0].kind.count(1) > 0  # MixedFeature levels in the second j iteration too
    assert FW.layouts("L20")[0].kind[16:] == [1, 1, 1, 1]


def test_odd_tables_patch_both_layouts_identically():
    lay, olay = FW.odd_tables()
    assert lay.sizes == olay.sizes == FW.ODD_SIZES and lay.offsets == olay.offsets
    assert lay.n_entries == olay.n_entries == 3825 and lay.n_params == olay.n_params == 7650
    assert lay.offsets == [0, 67, 283, 798, 1799, 2820, 2822, 2825]
    # odd entry offsets (8-byte loads at 4-byte alignment whatever the index) on dense and hashed levels
    assert [l for l in range(8) if lay.offsets[l] % 2] == [1, 2, 4, 7]
    d = lay.desc()
    assert list(d.size[:8]) == FW.ODD_SIZES and list(d.offset[:8]) == lay.offsets
    kinds = [FW.level_kind(olay, l) for l in range(8)]
    assert [k[0] for k in kinds] == ["dense"] * 4 + ["hashed"] * 4
    assert [k[1] for k in kinds[4:]] == ["odd", "pow2", "odd", "even"]


def test_the_stride_case_crosses_both_block_caps():
    lay, _ = FW.layouts("lego")
    N = FW.STRIDE_N
    assert N * (lay.L // 4) > 8192 * 256 and N > 8192 * 256 // (lay.L // 4)  # row-major: threads past the cap
    assert N > 2048 * 256                                                    # planar: samples per group
    assert N % 256 != 0 and (N * (lay.L // 4)) % 256 != 0                    # both end in a partial block
    p = FW.STRIDE_PERIOD
    assert all(p % k for k in range(2, int(p ** 0.5) + 1)) and 524288 % p == 64
    # a sample read one stride off (either kernel: 524,288 samples) is another point of the base
    base = FW.stride_base()
    assert base.shape == (p, 3) and len({tuple(r) for r in base.tolist()}) == p
    i = np.arange(N - 524288)
    assert ((i + 524288) % p != i % p).all()


def test_forward_entry_points_refuse_before_the_device():
    """The forward entry points' argument checks come before any HIP call (as tests/test_field_abi_cpu.py
    shows for the field head): refused calls need no GPU.  A level of one entry is refused by the planar
    forward alone -- its 8-byte load at min(idx, size - 2) would wrap and read past the table."""
    import ctypes

    from mfnerf import _lib
    lib = _lib.load()
    lay, _ = FW.layouts("small_T")
    mem = ctypes.create_string_buffer(64)
    some, null = ctypes.c_void_p(ctypes.addressof(mem)), ctypes.c_void_p(0)

    def planar(n=8, stride=8, d=None, table=some):
        return lib.mfnerf_grid_encode_fw_planar(some, n, null, 0.0, 1.0, d or lay.desc(), table, some, stride, null)

    def row(n=8, d=None, table=some):
        return lib.mfnerf_grid_encode_fw(some, n, null, 0.0, 1.0, d or lay.desc(), table, some, null)

    def desc(**kw):
        d = lay.desc()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for level in (0, 3, 7):
        one = lay.desc()
        one.size[level] = 1
        assert planar(d=one) == 1
        assert lib.mfnerf_last_error().decode() == (f"grid_encode_fw_planar: level {level} has 1 entries, the planar "
                                                    f"forward needs >= 2")
        assert planar(d=one, n=0) == 1  # a property of the layout, whatever n
        assert row(d=one, n=0) == 0
    assert planar(n=-1) == 1 and row(n=-1) == 1 and planar(n=8, stride=7) == 1
    assert planar(d=desc(n_levels=6)) == 1 and row(d=desc(n_levels=6)) == 1
    assert planar(d=desc(n_features=4)) == 1 and row(d=desc(n_features=4)) == 1
    assert planar(table=null) == 1 and row(table=null) == 1
    assert planar(n=0, table=null) == 0 and row(n=0, table=null) == 0
    two = lay.desc()
    two.size[7] = 2
    assert planar(d=two, n=0) == 0
