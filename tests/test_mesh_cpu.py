"""Mesh extraction without a GPU: the numpy restatement (mesh_ref.py, the specification the kernels
of csrc/mesh.hip match) is checked for topology, enclosed volume, orientation, normals and case
coverage; the generated case table, the C ABI declarations, their ctypes signatures and the PLY
writer are checked on the host."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import mesh_ref as M
from conftest import PKG, ROOT

R = 32  # the table of the closed-surface checks below was measured at this resolution


def _field(fn, R=R, **kw):
    X, Y, Z = M.lattice_xyz(R)
    return fn(X, Y, Z, **kw).astype(np.float32)


@pytest.fixture(scope="module")
def meshes():
    return {"sphere": M.extract(_field(M.sphere_field), M.SPHERE_THR),
            "torus": M.extract(_field(M.torus_field), M.TORUS_THR),
            "two": M.extract(_field(M.two_spheres_field), -0.15)}


# (chi, analytic volume); the prototype's volume errors at R = 32: -0.54 %, -1.6 %, -2.2 %
CLOSED = {"sphere": (2, 4.0 / 3.0 * math.pi * M.SPHERE_R ** 3),
          "torus": (0, 2.0 * math.pi ** 2 * M.TORUS_MAJOR * M.TORUS_MINOR ** 2),
          "two": (4, 2 * 4.0 / 3.0 * math.pi * 0.15 ** 3)}


# ------------------------------------------------------------------------------- the case table
def test_kuhn_split_and_table_shape():
    assert M.TETS == ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))
    assert M.TRI_COUNT == [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]
    types = set()
    for t in range(6):
        for case in range(16):
            for tri in M.TABLE[t][case]:
                assert len(tri) == 3 and len(set(tri)) == 3
                for u, d in tri:
                    assert 0 <= u <= 6 and 1 <= d <= 7 and u & d == 0
                    # the edge joins an inside and an outside corner of the tetrahedron
                    a, b = M.TETS[t].index(u), M.TETS[t].index(u | d)
                    assert (case >> a & 1) != (case >> b & 1)
                    types.add(d)
    assert types == set(range(1, 8))  # 3 axis edges, 3 face diagonals, the body diagonal


def test_table_header_regenerates_byte_for_byte():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_mesh_table
    finally:
        sys.path.pop(0)
    committed = open(os.path.join(PKG, "csrc", "mesh_table.hpp")).read()
    assert gen_mesh_table.render() == committed, "run tools/gen_mesh_table.py"


# ------------------------------------------------------------------------------- topology, volume
def _open_edges_lie_on_a_boundary_plane(vertices, edges, lo=-0.5, hi=0.5):
    """Both ends of every given edge on one common face of the lattice's box."""
    v = vertices.astype(np.float64)
    planes = np.concatenate([np.abs(v - lo) <= 1e-6, np.abs(v - hi) <= 1e-6], 1)  # (V, 6)
    return bool((planes[edges[:, 0]] & planes[edges[:, 1]]).any(1).all())


@pytest.mark.parametrize("name", sorted(CLOSED))
def test_closed_surfaces(meshes, name):
    m = meshes[name]
    chi, volume = CLOSED[name]
    V, faces = m["vertices"].shape[0], m["faces"]
    assert faces.min() >= 0 and faces.max() == V - 1
    assert np.array_equal(np.unique(faces), np.arange(V)), "a vertex no face uses"
    _, uses, balance = M.edge_table(faces)
    # closed: every edge in exactly two faces, once in each direction
    assert (uses == 2).all() and (balance == 0).all()
    got = M.euler_characteristic(V, faces)
    err = M.signed_volume(m["vertices"], faces) / volume - 1.0
    print(f"{name}: V {V} F {faces.shape[0]} chi {got} volume error {100 * err:+.2f} %")
    assert got == chi
    # positive: normals point outwards; one-sided: the mesh is inscribed in the convex cross-sections
    assert -0.03 <= err <= 0.0


def test_surface_cut_by_the_lattice_boundary():
    X, Y, Z = M.lattice_xyz(R)
    m = M.extract(M.sphere_field(X, Y, Z, (0.4, 0.0, 0.0)).astype(np.float32), -0.3)
    V, faces = m["vertices"].shape[0], m["faces"]
    edges, uses, balance = M.edge_table(faces)
    assert uses.max() == 2 and (balance[uses == 2] == 0).all()
    single = edges[uses == 1]
    print(f"cut sphere: chi {M.euler_characteristic(V, faces)}, {single.shape[0]} single-face edges")
    assert M.euler_characteristic(V, faces) == 1
    assert single.shape[0] > 0
    assert _open_edges_lie_on_a_boundary_plane(m["vertices"], single), "an open edge away from the lattice boundary"


def test_noise_is_manifold_and_reaches_every_case():
    """A 10^3 lattice of uniform noise: all 14 non-trivial cases of each of the six tetrahedra occur,
    and even there no edge lies in more than two faces and interior edges are matched."""
    rng = np.random.default_rng(0)
    m = M.extract(rng.random((10, 10, 10), dtype=np.float32), 0.5)
    assert (m["cases"][:, 1:15] > 0).all(), m["cases"]
    assert m["cases"].sum() == 6 * 9 ** 3
    assert m["faces"].shape[0] == int(m["tcount"].sum()) == int((m["cases"] * np.asarray(M.TRI_COUNT)).sum())
    assert m["vertices"].shape[0] == int(m["vcount"].sum())
    edges, uses, balance = M.edge_table(m["faces"])
    assert uses.max() == 2 and (balance[uses == 2] == 0).all()
    assert _open_edges_lie_on_a_boundary_plane(m["vertices"], edges[uses == 1])


def test_anisotropic_lattice_strides():
    """(Rx, Ry, Rz) = (7, 3, 12) with its own bounds: a closed ellipsoid, positions inside the box."""
    lo, hi = (-0.4, -0.2, -0.7), (0.5, 0.3, 0.6)
    X, Y, Z = M.lattice_xyz((7, 3, 12), lo, hi)
    s = -np.sqrt(((X - 0.05) / 0.3) ** 2 + ((Y - 0.04) / 0.2) ** 2 + ((Z + 0.03) / 0.5) ** 2).astype(np.float32)
    assert s.shape == (13, 4, 8)
    m = M.extract(s, -1.0, lo, hi)
    _, uses, balance = M.edge_table(m["faces"])
    assert (uses == 2).all() and (balance == 0).all()
    assert M.euler_characteristic(m["vertices"].shape[0], m["faces"]) == 2
    assert M.signed_volume(m["vertices"], m["faces"]) > 0
    assert (m["vertices"] >= np.asarray(lo, np.float32)).all() and (m["vertices"] <= np.asarray(hi, np.float32)).all()


# ------------------------------------------------------------------------------- normals, edge rules
@pytest.mark.parametrize("name,outward", [("sphere", M.sphere_outward), ("torus", M.torus_outward)])
def test_normals_point_outwards(meshes, name, outward):
    m = meshes[name]
    n = m["normals"]
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-12)
    dots = (n * outward(m["vertices"])).sum(1)
    print(f"{name}: min normal . outward = {dots.min():.4f}")
    assert (dots > 0).all()
    # the faces' own normals agree with them
    v = m["vertices"].astype(np.float64)
    f = m["faces"]
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert ((fn * n[f[:, 0]]).sum(1) > 0).all()


def test_inside_is_strict_and_nonfinite_values():
    s = np.zeros((2, 2, 2), np.float32)
    assert M.extract(s, 0.0)["faces"].shape[0] == 0  # sigma == thr is outside
    s[0, 0, 0] = 1.0
    m = M.extract(s, 0.0)
    assert m["vertices"].shape[0] == 7 and m["faces"].shape[0] == 6  # corner 0 lies in all six tetrahedra
    assert np.array_equal(m["t"], np.ones(7, np.float32))            # (0 - 1)/(0 - 1): at the far ends
    s[0, 0, 0] = np.inf
    m = M.extract(s, 0.0)
    assert m["vertices"].shape[0] == 7 and np.array_equal(m["t"], np.full(7, 0.5, np.float32))
    s[0, 0, 0] = np.nan
    assert M.extract(s, 0.0)["vertices"].shape[0] == 0               # NaN is outside
    s[:] = 1.0
    s[0, 0, 0] = np.nan
    m = M.extract(s, 0.0)
    assert m["vertices"].shape[0] == 7 and np.array_equal(m["t"], np.full(7, 0.5, np.float32))
    assert np.array_equal(m["normals"], np.zeros((7, 3)))            # a non-finite gradient


# ------------------------------------------------------------------------------- C ABI, bindings
ENTRY_POINTS = {"mfnerf_mesh_lattice_points": 9, "mfnerf_mesh_count": 8, "mfnerf_mesh_emit": 13}


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


def test_library_exports_the_entry_points_at_abi_2():
    from mfnerf import _lib
    assert os.path.exists(_lib.LIB_PATH), "build libmfnerf_hip.so first (__graft_entry__.build())"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert _lib.load().mfnerf_abi_version() == 2


def test_entry_points_refuse_bad_sizes_without_a_device():
    """The size checks come first and touch no device: 2^31 points, a resolution of 0, null pointers,
    a slab outside the lattice -> MFN_ERR_INVALID (1) with a message."""
    from mfnerf import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    f3 = (ctypes.c_float * 3)(0.0, 0.0, 0.0)

    def refused(status, word):
        assert status == 1
        assert word in lib.mfnerf_last_error().decode()

    for dims in [(1 << 11, 1 << 10, 1 << 10), (1 << 40, 2, 2), (1 << 21, 1 << 21, 1 << 21), (46341, 46341, 2)]:
        refused(lib.mfnerf_mesh_count(null, *dims, 0.5, null, null, null), "2^31")
        refused(lib.mfnerf_mesh_emit(null, *dims, 0.5, null, null, f3, f3, null, null, null, null), "2^31")
        refused(lib.mfnerf_mesh_lattice_points(f3, f3, *dims, 0, 1, null, null), "2^31")
    for dims in [(1, 2, 2), (2, 1, 2), (2, 2, 1), (2, 0, 2)]:
        refused(lib.mfnerf_mesh_count(null, *dims, 0.5, null, null, null), "resolution")
        refused(lib.mfnerf_mesh_emit(null, *dims, 0.5, null, null, f3, f3, null, null, null, null), "resolution")
        refused(lib.mfnerf_mesh_lattice_points(f3, f3, *dims, 0, 1, null, null), "resolution")
    refused(lib.mfnerf_mesh_count(null, 2, 2, 2, 0.5, null, null, null), "null")
    refused(lib.mfnerf_mesh_emit(null, 2, 2, 2, 0.5, null, null, f3, f3, null, null, null, null), "null")
    refused(lib.mfnerf_mesh_emit(null, 2, 2, 2, 0.5, null, null, null, f3, null, null, null, null), "null")
    refused(lib.mfnerf_mesh_lattice_points(f3, f3, 2, 2, 2, 0, 8, null, null), "null")
    refused(lib.mfnerf_mesh_lattice_points(f3, f3, 2, 2, 2, 0, 9, null, null), "outside")
    refused(lib.mfnerf_mesh_lattice_points(f3, f3, 2, 2, 2, -1, 2, null, null), "outside")


def test_build_lists_the_new_unit():
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bmesh\.hip\b", mk, re.M)
    assert re.search(r"^resource:.*\bmesh\.hip\b", mk, re.M)
    assert re.search(r"^HDRS :=[^\n]*(\\\n[^\n]*)*\bmesh_table\.hpp\b", mk, re.M)


def test_wrappers_refuse_bad_arguments_before_the_device():
    from mfnerf import mesh
    with pytest.raises(RuntimeError, match="float32"):
        mesh.mesh_from_lattice(torch.zeros(3, 3, 3, dtype=torch.float64), 0.0, -1, 1)
    with pytest.raises(RuntimeError, match=r"\(nz, ny, nx\)"):
        mesh.mesh_from_lattice(torch.zeros(27), 0.0, -1, 1)
    with pytest.raises(RuntimeError, match="contiguous"):
        mesh.mesh_from_lattice(torch.zeros(3, 3, 4).transpose(0, 2), 0.0, -1, 1)
    with pytest.raises(RuntimeError, match="resolution must be >= 1"):
        mesh.mesh_from_lattice(torch.zeros(3, 1, 3), 0.0, -1, 1)
    with pytest.raises(RuntimeError, match="CUDA"):
        mesh.mesh_from_lattice(torch.zeros(3, 3, 3), 0.0, -1, 1)
    with pytest.raises(RuntimeError, match="resolution must be >= 1"):
        mesh._resolution3((4, 0, 4))
    with pytest.raises(RuntimeError, match="2\\^31"):
        mesh._resolution3(1290)
    assert mesh._resolution3(1024) == (1024, 1024, 1024) and mesh._resolution3((7, 3, 12)) == (7, 3, 12)
    from mfnerf.trainer import Trainer
    assert callable(Trainer.extract_mesh)


# ------------------------------------------------------------------------------- PLY
def _read_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elements, props = [], {}
    for line in lines[2:]:
        w = line.split()
        if w[:1] == ["element"]:
            elements.append((w[1], int(w[2])))
            props[w[1]] = []
        elif w[:1] == ["property"]:
            props[elements[-1][0]].append(w[1:])
    assert [e[0] for e in elements] == ["vertex", "face"]
    np_type = {"float": "<f4", "uchar": "u1"}
    vdt = np.dtype([(p[1], np_type[p[0]]) for p in props["vertex"]])
    nv, nf = elements[0][1], elements[1][1]
    verts = np.frombuffer(raw, vdt, nv, end)
    assert props["face"] == [["list", "uchar", "int", "vertex_indices"]]
    fdt = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    faces = np.frombuffer(raw, fdt, nf, end + nv * vdt.itemsize)
    assert end + nv * vdt.itemsize + nf * fdt.itemsize == len(raw)
    return verts, faces


@pytest.mark.parametrize("colors", [False, True])
def test_save_ply_round_trips(tmp_path, meshes, colors):
    from mfnerf.mesh import save_ply
    m = meshes["two"]
    mesh = {"vertices": torch.from_numpy(m["vertices"]), "normals": torch.from_numpy(m["normals"].astype(np.float32)),
            "faces": torch.from_numpy(m["faces"])}
    rng = np.random.default_rng(1)
    if colors:
        mesh["colors"] = torch.from_numpy(rng.random(m["vertices"].shape, dtype=np.float32))
    path = tmp_path / "m.ply"
    save_ply(path, mesh)
    verts, faces = _read_ply(path)
    names = ["x", "y", "z", "nx", "ny", "nz"] + (["red", "green", "blue"] if colors else [])
    assert list(verts.dtype.names) == names
    assert np.array_equal(np.stack([verts[k] for k in "xyz"], 1), m["vertices"])
    assert np.array_equal(np.stack([verts["n" + k] for k in "xyz"], 1), m["normals"].astype(np.float32))
    if colors:
        want = np.rint(mesh["colors"].numpy() * 255).astype(np.uint8)
        assert np.array_equal(np.stack([verts[k] for k in ("red", "green", "blue")], 1), want)
    assert (faces["n"] == 3).all() and np.array_equal(faces["v"], m["faces"])


def test_save_ply_empty_mesh(tmp_path):
    from mfnerf.mesh import save_ply
    empty = {"vertices": np.zeros((0, 3), np.float32), "normals": np.zeros((0, 3), np.float32),
             "faces": np.zeros((0, 3), np.int32), "colors": np.zeros((0, 3), np.float32)}
    path = tmp_path / "empty.ply"
    save_ply(path, empty)
    verts, faces = _read_ply(path)
    assert verts.shape == (0,) and faces.shape == (0,) and len(verts.dtype.names) == 9
