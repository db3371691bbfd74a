"""Mesh cleaning without a GPU: the numpy restatement (mesh_clean_ref.py, the specification the kernels
of csrc/mesh_clean.hip match) against known answers and against its second statement, the closedness
of what it keeps, its behaviour under a renaming of the vertices; and, on the host, the C ABI
declarations, their ctypes signatures, the argument checks and the export tool's flags."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import mesh_clean_ref as C
import mesh_ref as M
from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def meshes():
    return C.input_meshes()


def _counts(m):
    """Face counts of the components with a face, by label."""
    labels, counts = C.components(m["vertices"].shape[0], m["faces"])
    return labels, counts, {int(r): int(counts[r]) for r in np.flatnonzero(counts > 0)}


# ------------------------------------------------------------------------------- known answers
def test_two_spheres_tie(meshes):
    m = meshes["two_spheres"]
    assert m["vertices"].shape[0] == 956 and m["faces"].shape[0] == 1904
    labels, counts, table = _counts(m)
    assert sorted(table.values()) == [952, 952] and 0 in table
    one = C.clean(m, largest_only=True)
    assert one["components"] == (2, 1) and one["faces"].shape[0] == 952
    # the tie goes to the smallest label: the kept vertices are those labelled 0, in order
    assert np.array_equal(one["vertices"], m["vertices"][labels == 0])
    both = C.clean(m, min_fraction=1.0)
    assert both["components"] == (2, 2)
    for k in ("vertices", "normals", "colors", "faces"):
        assert np.array_equal(both[k], m[k])


def test_torus_is_one_component_and_cleaning_is_the_identity(meshes):
    m = meshes["torus"]
    _, _, table = _counts(m)
    assert table == {0: 3512}
    for kw in ({}, {"min_faces": 25}, {"min_fraction": 1.0}, {"largest_only": True}):
        out = C.clean(m, **kw)
        assert out["components"] == (1, 1)
        for k in ("vertices", "normals", "colors", "faces"):
            assert np.array_equal(out[k], m[k]) and out[k].dtype == m[k].dtype


def test_hollow_shell_has_two_surface_components(meshes):
    """The inner wall of a shell is a component of its own: these are components of the SURFACE."""
    m = meshes["shell"]
    _, _, table = _counts(m)
    assert sorted(table.values()) == [2156, 6488]
    out = C.clean(m, largest_only=True)
    assert out["components"] == (2, 1) and out["faces"].shape[0] == 6488
    _, uses, balance = M.edge_table(out["faces"])
    assert (uses == 2).all() and (balance == 0).all()
    assert M.euler_characteristic(out["vertices"].shape[0], out["faces"]) == 2


def test_noise_components(meshes):
    m = meshes["noise"]
    assert m["faces"].shape[0] == 7618
    _, _, table = _counts(m)
    sizes = sorted(table.values())
    assert len(sizes) == 7 and sizes[-1] == 7520 and sizes[:2] == [4, 4]
    m = meshes["sparse_noise"]
    _, _, table = _counts(m)
    assert len(table) == 60 and max(table.values()) == 628


def test_specks_are_24_faces_and_min_faces_25_removes_them(meshes):
    m = meshes["specks"]
    _, _, table = _counts(m)
    sizes = sorted(table.values())
    assert sizes[:-1] == [24] * len(C.SPECKS)
    sphere = C.input_lattices()["specks"]
    plain = M.extract(M.sphere_field(*M.lattice_xyz(C.R_INPUT)).astype(np.float32), sphere[1])
    assert sizes[-1] == plain["faces"].shape[0]
    out = C.clean(m, min_faces=25)
    assert out["components"] == (len(C.SPECKS) + 1, 1)
    assert np.array_equal(out["faces"], plain["faces"]) and np.array_equal(out["vertices"], plain["vertices"])
    assert C.clean(m, min_faces=24)["components"] == (len(C.SPECKS) + 1, len(C.SPECKS) + 1)


# ------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("name", sorted(C.input_lattices()))
def test_union_find_and_breadth_first_search_agree(meshes, name):
    m = meshes[name]
    V = m["vertices"].shape[0]
    a, b = C.components(V, m["faces"]), C.components_bfs(V, m["faces"])
    assert a[0].dtype == np.int32 and a[1].dtype == np.int32
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    labels, counts = a
    assert (labels <= np.arange(V)).all() and np.array_equal(labels[labels], labels)
    assert int(counts.sum()) == m["faces"].shape[0] and (counts[labels != np.arange(V)] == 0).all()
    assert (labels[m["faces"]] == labels[m["faces"][:, :1]]).all()


@pytest.mark.parametrize("kw", [{}, {"min_faces": 25}, {"min_fraction": 0.3}, {"largest_only": True}], ids=str)
@pytest.mark.parametrize("name", C.CLOSED_INPUTS)
def test_kept_components_stay_closed(meshes, name, kw):
    m = meshes[name]
    before = {r: chi for r, _, _, chi in C.component_table(m["vertices"].shape[0], m["faces"])}
    out = C.clean(m, **kw)
    V = out["vertices"].shape[0]
    assert np.array_equal(np.unique(out["faces"]), np.arange(V)), "a kept vertex no face uses"
    _, uses, balance = M.edge_table(out["faces"])
    assert (uses == 2).all() and (balance == 0).all()
    after = C.component_table(V, out["faces"])
    assert len(after) == out["components"][1]
    assert all(chi == 2 or name == "torus" for _, _, _, chi in after)
    assert M.euler_characteristic(V, out["faces"]) == sum(chi for _, _, _, chi in after)
    assert sum(chi for _, _, _, chi in after) <= sum(before.values())
    if not kw:
        assert sum(chi for _, _, _, chi in after) == sum(before.values())


@pytest.mark.parametrize("name", sorted(C.input_lattices()))
def test_renamed_vertices_give_the_renamed_partition(meshes, name):
    m = meshes[name]
    V = m["vertices"].shape[0]
    labels, counts = C.components(V, m["faces"])
    p, perm = C.permuted(m, seed=3)
    plabels, pcounts = C.components(V, p["faces"])
    # the same classes: vertex v became perm[v]
    same = plabels[perm]
    assert np.array_equal(same[:, None] == same[None, :], labels[:, None] == labels[None, :]) if V < 3000 else True
    for r in np.flatnonzero(labels == np.arange(V)):
        members = perm[labels == r]
        assert (plabels[members] == members.min()).all()
        assert pcounts[members.min()] == counts[r]
    assert sorted(pcounts[pcounts > 0].tolist()) == sorted(counts[counts > 0].tolist())
    # cleaning commutes with the renaming up to the order of the vertices
    a, b = C.clean(m, min_faces=25), C.clean(p, min_faces=25)
    assert a["components"] == b["components"] and a["faces"].shape == b["faces"].shape
    assert np.array_equal(a["vertices"][a["faces"]], b["vertices"][b["faces"]])
    assert np.array_equal(a["colors"][a["faces"]], b["colors"][b["faces"]])


def test_unreferenced_vertices_and_bad_faces():
    v = np.arange(18, dtype=np.float32).reshape(6, 3)
    mesh = {"vertices": v, "normals": -v, "faces": np.asarray([[4, 2, 5], [1, 6, 2], [0, -1, 4]], np.int32)}
    labels, counts = C.components(6, mesh["faces"])
    assert labels.tolist() == [0, 1, 2, 3, 2, 2] and counts.tolist() == [0, 0, 1, 0, 0, 0]
    assert np.array_equal(C.components_bfs(6, mesh["faces"])[0], labels)
    out = C.clean(mesh)
    assert out["components"] == (4, 1) and out["faces"].tolist() == [[1, 0, 2]]
    assert np.array_equal(out["vertices"], v[[2, 4, 5]]) and "colors" not in out
    empty = C.clean({"vertices": v[:0], "normals": v[:0], "faces": np.zeros((0, 3), np.int32)})
    assert empty["components"] == (0, 0) and empty["faces"].shape == (0, 3)


def test_min_fraction_is_rounded_to_fp32_and_compared_in_fp64():
    labels = np.asarray([0, 0, 0, 3, 3, 3], np.int32)
    counts = np.asarray([10, 0, 0, 1, 0, 0], np.int32)
    # float32(0.1) > 0.1: 1 >= 0.1 * 10 holds for the double 0.1, but not for the fraction rounded to fp32
    assert 0.1 * 10.0 == 1.0 and np.float64(np.float32(0.1)) * 10.0 > 1.0
    assert C.select(labels, counts, min_fraction=0.1).tolist() == [True, False, False, False, False, False]
    assert C.select(labels, counts, min_fraction=0.0625).tolist() == [True, False, False, True, False, False]


def test_occupancy_mask_restatement():
    """One cascade, G = 4: bit (morton) of the cell decides; outside the box is cleared."""
    G, scale = 4, 0.5
    bits = np.zeros(G ** 3 // 8, np.uint8)
    # cell (x, y, z) = (3, 0, 2): morton = x bits at 0,3; y at 1,4; z at 2,5 -> 1 + 8 + 32
    m = 1 + 8 + 32
    bits[m >> 3] |= 1 << (m & 7)
    lo, hi = (-0.4, -0.45, -0.7), (0.45, 0.4, 0.7)
    mask = C.occupancy_mask(lo, hi, (17, 17, 7), bits, 1, scale, G)
    x, y, z = C.lattice_positions(lo, hi, (17, 17, 7))
    want = (x >= 0.25) & (x <= 0.5) & (y < -0.25) & (z >= 0.0) & (z < 0.25)
    assert want.any() and np.array_equal(mask, want)
    assert not mask[np.abs(z) > 0.5].any()
    assert C.occupancy_mask(lo, hi, (17, 17, 7), ~np.zeros_like(bits), 1, scale, G).sum() == (np.abs(z) <= 0.5).sum()


# ------------------------------------------------------------------------------- C ABI, bindings
ENTRY_POINTS = {"mfnerf_mesh_components": 6, "mfnerf_mesh_select": 12, "mfnerf_mesh_compact": 15,
                "mfnerf_mesh_occupancy_mask": 12}


def _declared(name):
    src = open(os.path.join(ROOT, "include", "mfnerf.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+" + name + r"\s*\((.*?)\)\s*;", src, re.S)
    assert m, f"{name} is not declared (with a comment) in include/mfnerf.h"
    return m.group(1), [a.strip() for a in m.group(2).split(",")]


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_header_and_signature_agree(name):
    from mfnerf import _lib
    comment, args = _declared(name)
    assert "test.ipynb" in comment and "mesh cell" in comment
    res, argtypes = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == len(argtypes) == ENTRY_POINTS[name]
    for decl, ty in zip(args, argtypes):
        if "*" in decl or "mfnerf_stream_t" in decl:
            assert ty is ctypes.c_void_p, decl
        elif decl.startswith("int64_t"):
            assert ty is ctypes.c_int64, decl
        else:
            assert decl.startswith("float") and ty is ctypes.c_float, decl
    assert "mfnerf_stream_t" in args[-1]


def test_header_cites_the_tuning_it_replaces():
    src = open(os.path.join(ROOT, "include", "mfnerf.h")).read()
    assert "little noise" in src


def test_library_exports_the_entry_points_at_abi_2():
    from mfnerf import _lib
    assert os.path.exists(_lib.LIB_PATH), "build libmfnerf_hip.so first (__graft_entry__.build())"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert _lib.load().mfnerf_abi_version() == 2


def test_entry_points_refuse_bad_sizes_without_a_device():
    """The size checks come first and touch no device: 2^31 elements, negative sizes, null pointers,
    bad selection arguments, a bitfield too small -> MFN_ERR_INVALID (1) with a message."""
    from mfnerf import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    f3 = (ctypes.c_float * 3)(0.0, 0.0, 0.0)

    def refused(status, word):
        assert status == 1
        assert word in lib.mfnerf_last_error().decode(), lib.mfnerf_last_error().decode()

    for V, F, word in [(1 << 31, 4, "2^31"), (4, 1 << 31, "2^31"), (1 << 40, 1 << 40, "2^31"), (-1, 4, "negative"),
                       (4, -7, "negative"), (4, 4, "null"), (0, 0, "null")]:
        refused(lib.mfnerf_mesh_components(null, V, F, null, null, null), word)
        refused(lib.mfnerf_mesh_select(null, V, F, null, null, 0, 0.0, 0, null, null, null, null), word)
        refused(lib.mfnerf_mesh_compact(null, null, null, null, V, F, null, null, null, null, null, null, null, null,
                                        null), word)
    refused(lib.mfnerf_mesh_select(null, 4, 4, null, null, -1, 0.0, 0, null, null, null, null), "min_faces")
    for fraction in (-0.5, 1.5, float("nan")):
        refused(lib.mfnerf_mesh_select(null, 4, 4, null, null, 0, fraction, 0, null, null, null, null), "min_fraction")
    mask = lib.mfnerf_mesh_occupancy_mask
    for dims in [(1 << 11, 1 << 10, 1 << 10), (1 << 40, 2, 2), (46341, 46341, 2)]:
        refused(mask(null, f3, f3, *dims, null, 1 << 18, 1, 128, 0.5, null), "2^31")
    for dims in [(1, 2, 2), (2, 0, 2), (2, 2, -3)]:
        refused(mask(null, f3, f3, *dims, null, 1 << 18, 1, 128, 0.5, null), "resolution")
    for cascades, G in [(0, 128), (33, 128), (1, 0), (1, 100), (1, 2048), (16, 1024)]:
        refused(mask(null, f3, f3, 2, 2, 2, null, 1 << 40, cascades, G, 0.5, null), "grid_size")
    refused(mask(null, f3, f3, 2, 2, 2, null, (1 << 18) - 1, 1, 128, 0.5, null), "bytes")
    refused(mask(null, f3, f3, 2, 2, 2, null, 3 << 18, 4, 128, 0.5, null), "bytes")
    refused(mask(null, f3, f3, 2, 2, 2, null, 1 << 18, 1, 128, 0.0, null), "scale")
    refused(mask(null, f3, f3, 2, 2, 2, null, 1 << 18, 1, 128, 0.5, null), "null")
    refused(mask(null, None, f3, 2, 2, 2, null, 1 << 18, 1, 128, 0.5, null), "null")


def test_build_lists_the_new_unit():
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bmesh_clean\.hip\b", mk, re.M)
    assert re.search(r"^resource:.*\bmesh_clean\.hip\b", mk, re.M)
    # (one rule compiles every unit of that list: the list is handed on, and the rule reports a unit)
    assert re.search(r"^resource:.*\n\t.*\$\(\^:%\.hip=resource-%\)", mk, re.M)
    assert re.search(r"^resource-%: %\.hip\n\t.*kernel-resource-usage -c \$<", mk, re.M)
    # the sizes the GPU tests place their edge cases around
    src = open(os.path.join(PKG, "csrc", "mesh_clean.hip")).read()
    assert re.search(r"constexpr int CLEAN_BLOCK = 256;", src) and re.search(r"constexpr int ITEMS = 16;", src)


def _host_mesh(V=4, F=2):
    return {"vertices": torch.zeros(V, 3), "normals": torch.zeros(V, 3), "faces": torch.zeros(F, 3, dtype=torch.int32)}


def test_wrappers_refuse_bad_arguments_before_the_device():
    from mfnerf import mesh
    for fn in (mesh.components, mesh.clean_mesh):
        with pytest.raises(RuntimeError, match="dict"):
            fn({"vertices": torch.zeros(4, 3)})
        with pytest.raises(RuntimeError, match="int32"):
            fn(dict(_host_mesh(), faces=torch.zeros(2, 3, dtype=torch.int64)))
        with pytest.raises(RuntimeError, match="float32"):
            fn(dict(_host_mesh(), normals=torch.zeros(4, 3, dtype=torch.float64)))
        with pytest.raises(RuntimeError, match=r"\(n, 3\)"):
            fn(dict(_host_mesh(), faces=torch.zeros(6, dtype=torch.int32)))
        with pytest.raises(RuntimeError, match=r"\(n, 3\)"):
            fn(dict(_host_mesh(), vertices=torch.zeros(4, 4)))
        with pytest.raises(RuntimeError, match="contiguous"):
            fn(dict(_host_mesh(), vertices=torch.zeros(3, 4).t()))
        with pytest.raises(RuntimeError, match="one row per vertex"):
            fn(dict(_host_mesh(), normals=torch.zeros(5, 3)))
        with pytest.raises(RuntimeError, match="one row per vertex"):
            fn(dict(_host_mesh(), colors=torch.zeros(3, 3)))
        with pytest.raises(RuntimeError, match="CUDA"):
            fn(_host_mesh())
    with pytest.raises(RuntimeError, match="min_faces"):
        mesh.clean_mesh(_host_mesh(), min_faces=-1)
    with pytest.raises(RuntimeError, match="min_faces"):
        mesh.clean_mesh(_host_mesh(), min_faces=2.5)
    for fraction in (-0.1, 1.01, float("nan")):
        with pytest.raises(RuntimeError, match="min_fraction"):
            mesh.clean_mesh(_host_mesh(), min_fraction=fraction)
    with pytest.raises(RuntimeError, match="uint8"):
        mesh.occupancy_mask(torch.zeros(3, 3, 3), -1, 1, torch.zeros(8), 1, 0.5, 128)
    with pytest.raises(RuntimeError, match="float32"):
        mesh.occupancy_mask(torch.zeros(3, 3, 3, dtype=torch.float64), -1, 1, torch.zeros(8, dtype=torch.uint8), 1, 0.5,
                            128)
    with pytest.raises(RuntimeError, match="CUDA"):
        mesh.occupancy_mask(torch.zeros(3, 3, 3), -1, 1, torch.zeros(8, dtype=torch.uint8), 1, 0.5, 128)


class _NoModel:
    """Stands in for a model where the call must be refused before anything looks at it."""
    scale = 0.5

    def __getattr__(self, name):
        raise AssertionError(f"the model's {name} was used")


@pytest.mark.parametrize("threshold", [0, 0.0, -1.0, float("nan")])
def test_occupancy_needs_a_positive_threshold(threshold):
    from mfnerf import mesh
    with pytest.raises(RuntimeError, match="sigma_threshold > 0"):
        mesh.extract_mesh(_NoModel(), 8, sigma_threshold=threshold, occupancy=True)


def test_extract_mesh_checks_the_cleaning_arguments_first():
    from mfnerf import mesh
    with pytest.raises(RuntimeError, match="min_fraction"):
        mesh.extract_mesh(_NoModel(), 8, clean={"min_fraction": 2.0})
    with pytest.raises(TypeError):
        mesh.extract_mesh(_NoModel(), 8, clean={"min_area": 2.0})


# ------------------------------------------------------------------------------- the export tool
def _export_tool():
    saved = dict(os.environ)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import export_mesh
    finally:
        sys.path.pop(0)
        os.environ.clear()
        os.environ.update(saved)  # the tool sets a runtime variable for its own process
    return export_mesh


def test_export_tool_flags():
    ap = _export_tool().build_parser()
    old = ap.parse_args([])
    assert (old.occupancy, old.min_faces, old.min_fraction, old.largest_only) == (False, 0, 0.0, False)
    assert not _export_tool().cleaning_requested(old)
    assert (old.steps, old.resolution, old.threshold, old.out, old.reps, old.no_colors) == \
        (30000, [256], 20.0, "mesh.ply", 5, False)
    new = ap.parse_args(["--resolution", "256", "512", "--occupancy", "--min-faces", "25", "--min-fraction", "0.01",
                         "--largest-only"])
    assert (new.occupancy, new.min_faces, new.min_fraction, new.largest_only) == (True, 25, 0.01, True)
    assert new.resolution == [256, 512] and _export_tool().cleaning_requested(new)
    for flags in (["--occupancy"], ["--min-faces", "1"], ["--min-fraction", "0.5"], ["--largest-only"]):
        assert _export_tool().cleaning_requested(ap.parse_args(flags)), flags
