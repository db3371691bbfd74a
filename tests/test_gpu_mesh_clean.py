"""Mesh cleaning on the GPU (csrc/mesh_clean.hip, mfnerf/mesh.py) against the numpy restatement
(mesh_clean_ref.py).  Everything is specified exactly, so every comparison is ==: labels, face counts,
the cleaned arrays bit for bit, the culled lattice.  Each input comes as extracted (vertices ordered
by lattice point, unions mostly between near indices) and with its vertex indices randomly renamed."""
import math

import numpy as np
import pytest
import torch

import mesh_clean_ref as C
from mfnerf import mesh

pytestmark = pytest.mark.gpu

NAMES = sorted(C.input_lattices())
FORMS = ["extracted", "permuted"]
BLOCK = 256  # CLEAN_BLOCK of csrc/mesh_clean.hip
BLOCK_ITEMS = 16 * BLOCK  # elements per workgroup of its kernels that take ITEMS = 16 per thread

_REF = {}


def _input(name, form):
    """(mesh of arrays, labels, face counts): computed once, shared, read-only."""
    key = (name, form)
    if key not in _REF:
        m = C.input_meshes()[name]
        if form == "permuted":
            m, _ = C.permuted(m, seed=5)
        labels, counts = C.components(m["vertices"].shape[0], m["faces"])
        for a in (*m.values(), labels, counts):
            a.setflags(write=False)
        _REF[key] = (m, labels, counts)
    return _REF[key]


def _device(m, gpu):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for k, v in m.items()}


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_same_mesh(got, want):
    assert set(got) == set(want)
    assert got["components"] == want["components"]
    for k in ("vertices", "normals", "colors", "faces"):
        if k in want:
            assert got[k].dtype == (torch.int32 if k == "faces" else torch.float32)
            assert tuple(got[k].shape) == want[k].shape, k
            assert np.array_equal(_bits(got[k]), _bits(want[k])), k


def _strip_mesh(faces, V, gpu):
    """A mesh around a face list: the positions carry the vertex index, so a misplaced row shows."""
    v = np.arange(3 * V, dtype=np.float32).reshape(V, 3)
    return _device({"vertices": v, "normals": -v, "faces": np.ascontiguousarray(faces, dtype=np.int32)}, gpu)


# ------------------------------------------------------------------------------- labels, cleaning
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_components_match_the_restatement(gpu, name, form):
    m, labels, counts = _input(name, form)
    got = mesh.components(_device(m, gpu))
    assert got["labels"].dtype == torch.int32 and got["face_counts"].dtype == torch.int32
    assert got["labels"].is_cuda and got["face_counts"].is_cuda
    assert np.array_equal(got["labels"].cpu().numpy(), labels)
    assert np.array_equal(got["face_counts"].cpu().numpy(), counts)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_clean_mesh_matches_the_restatement(gpu, name, form):
    m, _, _ = _input(name, form)
    d = _device(m, gpu)
    before = {k: v.clone() for k, v in d.items()}
    for min_faces in (0, 5, 25):
        for min_fraction in (0.0, 0.01, 1.0):
            kw = {"min_faces": min_faces, "min_fraction": min_fraction}
            _assert_same_mesh(mesh.clean_mesh(d, **kw), C.clean(m, **kw))
    _assert_same_mesh(mesh.clean_mesh(d, largest_only=True), C.clean(m, largest_only=True))
    no_colors = {k: v for k, v in d.items() if k != "colors"}
    _assert_same_mesh(mesh.clean_mesh(no_colors, min_faces=25),
                      C.clean({k: v for k, v in m.items() if k != "colors"}, min_faces=25))
    for k in d:
        assert torch.equal(d[k], before[k]), f"clean_mesh modified its input's {k}"


@pytest.mark.parametrize("form", FORMS)
def test_largest_only_on_the_tie_keeps_label_zero(gpu, form):
    m, labels, counts = _input("two_spheres", form)
    assert sorted(counts[counts > 0].tolist()) == [952, 952] and counts[0] == 952
    got = mesh.clean_mesh(_device(m, gpu), largest_only=True)
    assert got["components"] == (2, 1) and got["faces"].shape[0] == 952
    assert np.array_equal(_bits(got["vertices"]), _bits(m["vertices"][labels == 0]))


def test_sigma_is_passed_through(gpu):
    m, _, _ = _input("specks", "extracted")
    d = _device(m, gpu)
    d["sigma"] = torch.zeros(2, 2, 2, device=gpu)
    out = mesh.clean_mesh(d, min_faces=25)
    assert out["sigma"] is d["sigma"] and out["components"] == (len(C.SPECKS) + 1, 1)


# ------------------------------------------------------------------------------- adversarial shapes
def _bit_reversal(n_bits):
    i = np.arange(1 << n_bits, dtype=np.int64)
    r = np.zeros_like(i)
    for b in range(n_bits):
        r |= (i >> b & 1) << (n_bits - 1 - b)
    return r


STRIP_F = 1 << 17


def _strip(order):
    """A triangle strip of 2^17 faces over 2^17 + 2 vertices: face i = (i, i+1, i+2), renamed."""
    V = STRIP_F + 2
    i = np.arange(STRIP_F, dtype=np.int64)
    faces = np.stack([i, i + 1, i + 2], 1)
    if order == "reversed":  # the minimum index sits at the far end
        faces = V - 1 - faces
    elif order == "bit-reversed":  # neighbours in the strip are far apart as indices
        rename = np.concatenate([_bit_reversal(17), [STRIP_F, STRIP_F + 1]])
        faces = rename[faces]
    return faces, V


@pytest.mark.parametrize("order", ["forward", "reversed", "bit-reversed"])
def test_long_strip_is_one_component(gpu, order):
    """Spans 512 workgroups and builds deep trees before the flatten."""
    faces, V = _strip(order)
    d = _strip_mesh(faces, V, gpu)
    got = mesh.components(d)
    assert int(got["labels"].max()) == 0 and int(got["labels"].min()) == 0
    counts = got["face_counts"]
    assert int(counts[0]) == STRIP_F and int(counts[1:].max()) == 0
    out = mesh.clean_mesh(d, min_fraction=1.0)
    assert out["components"] == (1, 1)
    for k in ("vertices", "normals", "faces"):
        assert torch.equal(out[k], d[k]), k


def test_many_tiny_components_and_unreferenced_vertices(gpu):
    T, U = 1 << 15, 1000
    V = 3 * T + U
    rng = np.random.default_rng(2)
    unref = np.zeros(V, dtype=bool)
    unref[rng.choice(V, U, replace=False)] = True
    used = np.flatnonzero(~unref)
    faces = used.reshape(T, 3)[:, [1, 2, 0]]  # the label is not the face's first vertex
    d = _strip_mesh(faces, V, gpu)
    got = mesh.components(d)
    want_labels = np.arange(V)
    want_labels[used] = np.repeat(used.reshape(T, 3)[:, 0], 3)
    want_counts = np.zeros(V, dtype=np.int32)
    want_counts[used.reshape(T, 3)[:, 0]] = 1
    assert np.array_equal(got["labels"].cpu().numpy(), want_labels)
    assert np.array_equal(got["face_counts"].cpu().numpy(), want_counts)
    out = mesh.clean_mesh(d)
    assert out["components"] == (T + U, T)
    assert out["vertices"].shape[0] == 3 * T and out["faces"].shape[0] == T
    assert torch.equal(out["vertices"], d["vertices"][torch.from_numpy(~unref).to(gpu)])
    want_faces = (np.arange(3 * T).reshape(T, 3)[:, [1, 2, 0]]).astype(np.int32)
    assert np.array_equal(out["faces"].cpu().numpy(), want_faces)
    assert mesh.clean_mesh(d, min_faces=2)["components"] == (T + U, 0)


def test_two_tetrahedra_sharing_one_vertex_are_one_component(gpu):
    tet = np.asarray([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]])
    second = np.asarray([3, 4, 5, 6])[tet]  # shares vertex 3 only
    d = _strip_mesh(np.concatenate([second, tet]), 7, gpu)
    got = mesh.components(d)
    assert got["labels"].tolist() == [0] * 7 and got["face_counts"].tolist() == [8, 0, 0, 0, 0, 0, 0]
    apart = _strip_mesh(np.concatenate([np.asarray([7, 4, 5, 6])[tet], tet]), 8, gpu)
    got = mesh.components(apart)
    assert got["labels"].tolist() == [0, 0, 0, 0, 4, 4, 4, 4] and got["face_counts"].tolist() == [4, 0, 0, 0, 4, 0, 0, 0]


def test_faces_with_indices_out_of_range_are_ignored(gpu):
    """The guard of every kernel: a face holding V and one holding -1 join nothing, count nowhere and
    are removed; everything else is as without them."""
    m, _, _ = _input("sparse_noise", "extracted")
    V, F = m["vertices"].shape[0], m["faces"].shape[0]
    faces = m["faces"].copy()
    bad = np.asarray([[faces[10, 0], V, faces[900, 1]], [-1, faces[20, 1], faces[2000, 2]]], np.int32)
    with_bad = dict(m, faces=np.concatenate([faces[:100], bad[:1], faces[100:], bad[1:]]))
    ref_labels, ref_counts = C.components(V, m["faces"])
    d = _device(with_bad, gpu)
    got = mesh.components(d)
    assert np.array_equal(got["labels"].cpu().numpy(), ref_labels)
    assert np.array_equal(got["face_counts"].cpu().numpy(), ref_counts)
    for kw in ({}, {"min_faces": 25}, {"largest_only": True}):
        _assert_same_mesh(mesh.clean_mesh(d, **kw), C.clean(m, **kw))
        _assert_same_mesh(mesh.clean_mesh(d, **kw), C.clean(with_bad, **kw))
    only_bad = _strip_mesh(bad, V, gpu)
    assert mesh.clean_mesh(only_bad)["components"] == (V, 0)
    assert mesh.components(only_bad)["labels"].tolist() == list(range(V))


@pytest.mark.parametrize("n", [1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1,
                               BLOCK_ITEMS - 1, BLOCK_ITEMS, BLOCK_ITEMS + 1])
def test_sizes_around_the_block(gpu, n):
    """F = n faces over V = n + 2, max(n, 3) and 3 n + 1 vertices: the last workgroup is empty but for
    one thread, full, or one short, for faces and for vertices, in the kernels that take one element
    per thread and in those that take 16."""
    rng = np.random.default_rng(n)
    for V in (n + 2, max(n, 3), 3 * n + 1):
        faces = rng.integers(0, V, (n, 3)).astype(np.int32)
        faces[:, 1] = (faces[:, 0] + 1 + rng.integers(0, 3, n)) % V  # short edges: more than one component
        faces[:, 2] = (faces[:, 0] + 1 + rng.integers(0, 3, n)) % V
        v = rng.random((V, 3), dtype=np.float32)
        m = {"vertices": v, "normals": rng.random((V, 3), dtype=np.float32), "faces": faces}
        labels, counts = C.components(V, faces)
        d = _device(m, gpu)
        got = mesh.components(d)
        assert np.array_equal(got["labels"].cpu().numpy(), labels)
        assert np.array_equal(got["face_counts"].cpu().numpy(), counts)
        for kw in ({}, {"min_faces": 3}, {"min_fraction": 0.5}, {"largest_only": True}):
            _assert_same_mesh(mesh.clean_mesh(d, **kw), C.clean(m, **kw))


@pytest.mark.parametrize("V,F", [(0, 0), (5, 0)])
def test_empty_input_makes_no_launch(gpu, monkeypatch, V, F):
    calls = []
    real = mesh.call
    monkeypatch.setattr(mesh, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    d = {"vertices": torch.zeros(V, 3, device=gpu), "normals": torch.zeros(V, 3, device=gpu),
         "colors": torch.zeros(V, 3, device=gpu), "faces": torch.zeros(F, 3, dtype=torch.int32, device=gpu)}
    out = mesh.clean_mesh(d)
    comp = mesh.components(d)
    torch.cuda.synchronize()
    assert calls == []
    assert out["components"] == (V, 0)
    for k in ("vertices", "normals", "colors"):
        assert tuple(out[k].shape) == (0, 3) and out[k].dtype == torch.float32 and out[k].is_cuda
    assert tuple(out["faces"].shape) == (0, 3) and out["faces"].dtype == torch.int32
    assert comp["labels"].tolist() == list(range(V)) and comp["face_counts"].tolist() == [0] * V


def test_nothing_kept_makes_no_compact_launch(gpu, monkeypatch):
    m, _, _ = _input("sparse_noise", "extracted")
    calls = []
    real = mesh.call
    monkeypatch.setattr(mesh, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    out = mesh.clean_mesh(_device(m, gpu), min_faces=10 ** 6)
    assert calls == ["mfnerf_mesh_components", "mfnerf_mesh_select"]
    assert out["components"] == (60, 0) and out["vertices"].shape[0] == 0 and out["faces"].shape[0] == 0


def test_two_runs_are_bit_identical(gpu):
    m, _, _ = _input("noise", "permuted")
    d = _device(m, gpu)
    a, b = mesh.clean_mesh(d, min_faces=5), mesh.clean_mesh(d, min_faces=5)
    ca, cb = mesh.components(d), mesh.components(d)
    assert a["components"] == b["components"]
    for k in ("vertices", "normals", "colors"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert torch.equal(a["faces"], b["faces"])
    assert torch.equal(ca["labels"], cb["labels"]) and torch.equal(ca["face_counts"], cb["face_counts"])


# ------------------------------------------------------------------------------- occupancy
def _model(scale, gpu):
    """As test_gpu_mesh.py's `model`, with the occupancy bitfield drawn at random."""
    from mfnerf.field import XYZ_NET_PARAMS
    from mfnerf.networks import NGP
    from mfnerf.trainer import HParams
    m = NGP(scale=scale, hparams=HParams(T=16)).to(gpu)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        table = m.xyz_encoder.params[XYZ_NET_PARAMS:]
        table.copy_((torch.rand(table.numel(), generator=g) - 0.5).to(gpu))
        m.density_bitfield.copy_(torch.randint(0, 256, (m.density_bitfield.numel(),), generator=g,
                                               dtype=torch.uint8).to(gpu))
    return m


@pytest.fixture(scope="module")
def model(gpu):
    return _model(0.5, gpu)


def _assert_rounding_cannot_decide(lo, hi, R, cascades, scale, G):
    """In fp64: no in-box lattice point within 1e-3 cells of a cell boundary of its cascade, no
    point's largest |coordinate| within 1e-5 of a power of two or of scale.  fp32 evaluates the cell
    coordinate 0.5 * (x / bound + 1) * G <= 128 to within a few 2^-24 * 128 < 1e-4, so the fp32 kernel
    and the fp64 restatement then take every decision alike."""
    cell_margin, mip_margin = C.rounding_margins(lo, hi, R, cascades, scale, G)
    print(f"R {R}: {cell_margin:.5f} cells from a cell boundary, {mip_margin:.2e} from a cascade boundary")
    assert cell_margin > 1e-3 and mip_margin > 1e-5


# (scale, cascades, R): bounds (-0.97, 0.99) * scale, chosen on the CPU for the margins asserted above
@pytest.mark.parametrize("scale,cascades,R", [(0.5, 1, 27), (2.0, 3, 27)])
def test_density_lattice_occupancy_matches_the_restatement(gpu, model, scale, cascades, R):
    m = model if scale == 0.5 else _model(scale, gpu)
    assert m.cascades == cascades and m.grid_size == 128
    lo, hi = -0.97 * scale, 0.99 * scale
    _assert_rounding_cannot_decide(lo, hi, R, cascades, scale, m.grid_size)
    keep = C.occupancy_mask(lo, hi, R, m.density_bitfield.cpu().numpy(), cascades, scale, m.grid_size)
    assert 0.3 < keep.mean() < 0.7
    plain = mesh.density_lattice(m, R, lo, hi)
    got = mesh.density_lattice(m, R, lo, hi, occupancy=True)
    assert torch.equal(mesh.density_lattice(m, R, lo, hi, occupancy=False), plain)
    want = torch.where(torch.from_numpy(keep).to(gpu), plain, torch.zeros_like(plain))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    if cascades > 1:  # every cascade decides somewhere
        _, mip, _, _ = C._cells(lo, hi, R, cascades, scale, m.grid_size)
        assert set(np.unique(mip)) == set(range(cascades))


@pytest.mark.parametrize("scale,cascades", [(0.5, 1), (2.0, 3)])
def test_occupancy_mask_on_an_anisotropic_lattice_reaching_outside_the_box(gpu, scale, cascades):
    """Its own resolution and bounds per axis, a third of the points outside [-scale, scale]^3: those
    are cleared whatever the bitfield says.  Values of every kind; the ones that stay keep their bits."""
    G, R = 128, (17, 11, 23)
    lo = tuple(v * scale for v in (-0.91, -1.23, -0.83))
    hi = tuple(v * scale for v in (1.17, 0.89, 1.29))
    _assert_rounding_cannot_decide(lo, hi, R, cascades, scale, G)
    rng = np.random.default_rng(4)
    bits = rng.integers(0, 256, cascades * G ** 3 // 8, dtype=np.uint8)
    keep = C.occupancy_mask(lo, hi, R, bits, cascades, scale, G)
    x, y, z = C.lattice_positions(lo, hi, R)
    outside = (np.abs(x) > scale) | (np.abs(y) > scale) | (np.abs(z) > scale)
    assert 0.2 < outside.mean() < 0.5 and not keep[outside].any() and keep[~outside].any()
    sigma = rng.standard_normal(keep.shape).astype(np.float32) * 50
    kind = rng.random(keep.shape)
    sigma[kind < 0.05] = np.inf
    sigma[(kind >= 0.05) & (kind < 0.1)] = np.nan
    sigma[(kind >= 0.1) & (kind < 0.15)] = -0.0
    s = torch.from_numpy(sigma).to(gpu)
    out = mesh.occupancy_mask(s, lo, hi, torch.from_numpy(bits).to(gpu), cascades, scale, G)
    assert out is s  # in place
    want = np.where(keep, sigma, np.float32(0.0))
    assert np.array_equal(s.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # an all-set bitfield clears exactly the outside
    s = torch.from_numpy(sigma).to(gpu)
    mesh.occupancy_mask(s, lo, hi, torch.full((bits.size,), 255, dtype=torch.uint8, device=gpu), cascades, scale, G)
    want = np.where(outside, np.float32(0.0), sigma)
    assert np.array_equal(s.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------- on a model
RES = (20, 17, 23)
BOUNDS = ((-0.45, -0.3, -0.5), (0.4, 0.5, 0.35))


def _positive_threshold(model):
    sigma = mesh.density_lattice(model, RES, *BOUNDS, occupancy=True)
    thr = float(sigma[sigma > 0].median())
    assert math.isfinite(thr) and thr > 0
    return thr


def test_extract_mesh_cleans_the_culled_lattice(gpu, model):
    thr = _positive_threshold(model)
    kw = {"min_faces": 25, "min_fraction": 0.01}
    got = mesh.extract_mesh(model, RES, thr, bounds=BOUNDS, occupancy=True, clean=kw, return_sigma=True)
    assert set(got) == {"vertices", "normals", "faces", "colors", "components", "sigma"}
    sigma = mesh.density_lattice(model, RES, *BOUNDS, occupancy=True)
    assert torch.equal(got["sigma"].view(torch.int32), sigma.view(torch.int32))
    raw = mesh.mesh_from_lattice(sigma, thr, *BOUNDS)
    want = mesh.clean_mesh(raw, **kw)
    total, kept = want["components"]
    assert got["components"] == (total, kept) and 0 < kept < total, (total, kept)
    assert 0 < want["faces"].shape[0] < raw["faces"].shape[0]
    for k in ("vertices", "normals", "faces"):
        assert torch.equal(got[k], want[k]), k
    assert got["colors"].shape == got["vertices"].shape
    assert torch.equal(got["colors"], mesh.vertex_colors(model, want))
    # the device result is the restatement's cleaning of the same raw mesh
    host = {k: raw[k].cpu().numpy() for k in ("vertices", "normals", "faces")}
    _assert_same_mesh({k: v for k, v in want.items()}, C.clean(host, **kw))
    # each argument alone
    only_cull = mesh.extract_mesh(model, RES, thr, bounds=BOUNDS, occupancy=True, colors=False)
    assert set(only_cull) == {"vertices", "normals", "faces"}
    for k in only_cull:
        assert torch.equal(only_cull[k], raw[k]), k
    only_clean = mesh.extract_mesh(model, RES, thr, bounds=BOUNDS, clean={"largest_only": True}, colors=False)
    unculled = mesh.mesh_from_lattice(mesh.density_lattice(model, RES, *BOUNDS), thr, *BOUNDS)
    _assert_same_mesh(only_clean, {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v)
                                   for k, v in mesh.clean_mesh(unculled, largest_only=True).items()})
    assert only_clean["components"][1] == 1


def test_extract_mesh_defaults_are_unchanged(gpu, model):
    thr = _positive_threshold(model)
    got = mesh.extract_mesh(model, RES, thr, bounds=BOUNDS, return_sigma=True)
    explicit = mesh.extract_mesh(model, RES, thr, bounds=BOUNDS, return_sigma=True, occupancy=False, clean=None)
    assert set(got) == set(explicit) == {"vertices", "normals", "faces", "colors", "sigma"}
    sigma = mesh.density_lattice(model, RES, *BOUNDS)
    want = mesh.mesh_from_lattice(sigma, thr, *BOUNDS)
    assert torch.equal(got["sigma"].view(torch.int32), sigma.view(torch.int32))
    for k in ("vertices", "normals", "faces"):
        assert torch.equal(got[k], want[k]) and torch.equal(explicit[k], want[k]), k
    assert torch.equal(got["colors"], mesh.vertex_colors(model, want))
    assert torch.equal(explicit["colors"], got["colors"])


def test_trainer_extract_mesh_cleans(gpu):
    from mfnerf import data
    from mfnerf.trainer import HParams, Trainer
    W = 32
    focal = 0.5 * W / math.tan(0.5 * 0.6911112)
    imgs, poses, dirs, K = data.ball_scene_views(data.BallScene(n_balls=6, seed=1), 8, W, focal, seed=0)
    ds = data.DeviceDataset(imgs, poses, dirs, K=K, img_wh=(W, W), device=gpu, seed=5)
    tr = Trainer(HParams(batch_size=1024, T=16), ds, device=gpu)
    tr.fit(steps=32, log_every=0)
    sigma = tr.extract_mesh(resolution=8, colors=False, return_sigma=True)["sigma"]
    thr = max(float(sigma.median()), 1e-3)
    kw = dict(resolution=(24, 20, 16), sigma_threshold=thr, bounds=((-0.5, -0.4, -0.3), (0.5, 0.45, 0.4)),
              return_sigma=True, occupancy=True, clean={"min_faces": 5})
    a = tr.extract_mesh(**kw)
    b = mesh.extract_mesh(tr.to_ngp(), **kw)
    assert set(a) == set(b) == {"vertices", "normals", "faces", "colors", "sigma", "components"}
    assert a["components"] == b["components"]
    for k in ("vertices", "normals", "faces", "colors", "sigma"):
        assert torch.equal(a[k], b[k]), k
