"""Mesh extraction on the GPU (csrc/mesh.hip, mfnerf/mesh.py) against the numpy restatement
(mesh_ref.py): faces identical as integers, vertices within 1e-6 * (hi - lo) per axis, normals within
1 - 1e-5 of the fp64 restatement on the smooth fields; the C ABI's limits; determinism; and
extract_mesh / Trainer.extract_mesh on a model."""
import ctypes
import math

import numpy as np
import pytest
import torch

import mesh_ref as M
from mfnerf import _lib, mesh

pytestmark = pytest.mark.gpu

# one cell; two; no multiple of a block edge; across 32 and 64 points per row; unequal extents
SHAPES = [1, 2, 5, 13, 33, 64, (7, 3, 12)]
FIELDS = ["noise", "sphere", "torus", "integers", "nonfinite"]
LO, HI = -0.5, 0.5


def _r3(R):
    return (R, R, R) if isinstance(R, int) else R


def _lattice(field, R, seed=0):
    """(sigma (nz, ny, nx) f32, threshold)."""
    Rx, Ry, Rz = _r3(R)
    shape = (Rz + 1, Ry + 1, Rx + 1)
    rng = np.random.default_rng(seed + 1000 * Rx + Rz)
    if field == "noise":
        return rng.random(shape, dtype=np.float32), 0.5
    if field == "sphere":
        return M.sphere_field(*M.lattice_xyz(_r3(R), LO, HI)).astype(np.float32), M.SPHERE_THR
    if field == "torus":
        return M.torus_field(*M.lattice_xyz(_r3(R), LO, HI)).astype(np.float32), M.TORUS_THR
    if field == "integers":  # many exact equalities with the threshold and t = 0 / t = 1 vertices
        return rng.integers(0, 3, shape).astype(np.float32), 1.0
    s = rng.random(shape, dtype=np.float32)
    kind = rng.random(shape)
    s[kind < 0.08] = np.inf
    s[(kind >= 0.08) & (kind < 0.16)] = np.nan
    s[(kind >= 0.16) & (kind < 0.2)] = -np.inf
    return s, 0.5


_REF = {}


def _reference(field, R):
    """The restatement's mesh of a lattice: computed once, shared, never modified."""
    key = (field, R)
    if key not in _REF:
        sigma, thr = _lattice(field, R)
        ref = M.extract(sigma, thr, LO, HI)
        for a in ref.values():
            a.setflags(write=False)
        sigma.setflags(write=False)
        _REF[key] = (sigma, thr, ref)
    return _REF[key]


def _host(m):
    return {k: v.cpu().numpy() for k, v in m.items()}


def _assert_matches(got, ref, lo, hi, normals):
    span = np.asarray(hi, np.float64) - np.asarray(lo, np.float64)
    assert got["faces"].dtype == np.int32 and got["vertices"].dtype == np.float32
    assert got["vertices"].shape == ref["vertices"].shape and got["faces"].shape == ref["faces"].shape
    assert got["normals"].shape == ref["vertices"].shape
    assert np.array_equal(got["faces"], ref["faces"])
    if ref["vertices"].shape[0] == 0:
        return
    dv = np.abs(got["vertices"].astype(np.float64) - ref["vertices"].astype(np.float64)).max(0)
    print(f"V {ref['vertices'].shape[0]} F {ref['faces'].shape[0]} max |dv| / span {dv / span}")
    assert (dv <= 1e-6 * span).all()
    if normals:
        dots = (got["normals"].astype(np.float64) * ref["normals"]).sum(1)
        print(f"min normal dot {dots.min():.9f}")
        assert (dots >= 1.0 - 1e-5).all()
    else:  # unit or exactly zero, never NaN
        length = np.linalg.norm(got["normals"].astype(np.float64), axis=1)
        assert np.isfinite(got["normals"]).all()
        assert (np.abs(length - 1.0) <= 1e-5)[length != 0].all()


@pytest.mark.parametrize("R", SHAPES, ids=str)
@pytest.mark.parametrize("field", FIELDS)
def test_kernels_match_the_restatement(gpu, field, R):
    sigma, thr, ref = _reference(field, R)
    got = _host(mesh.mesh_from_lattice(torch.from_numpy(sigma).to(gpu), thr, LO, HI))
    _assert_matches(got, ref, (LO,) * 3, (HI,) * 3, normals=field in ("sphere", "torus"))


def test_counts_match_the_restatement(gpu):
    """mfnerf_mesh_count's two outputs and the scans, on noise with non-finite entries."""
    sigma, thr, ref = _reference("nonfinite", (7, 3, 12))
    s = torch.from_numpy(sigma).to(gpu)
    nz, ny, nx = s.shape
    vcount = torch.full((nx * ny * nz,), 99, dtype=torch.uint8, device=gpu)
    tcount = torch.full(((nx - 1) * (ny - 1) * (nz - 1),), 99, dtype=torch.uint8, device=gpu)
    _lib.call("mfnerf_mesh_count", _lib.ptr(s), nx, ny, nz, thr, _lib.ptr(vcount), _lib.ptr(tcount), _lib.stream())
    assert np.array_equal(vcount.cpu().numpy(), ref["vcount"])
    assert np.array_equal(tcount.cpu().numpy(), ref["tcount"])
    voff, toff, totals = mesh.count_and_scan(s, thr)
    assert voff.dtype == torch.int32 and toff.dtype == torch.int32
    assert totals.tolist() == [int(ref["vcount"].sum()), int(ref["tcount"].sum())]
    assert np.array_equal(voff.cpu().numpy(), np.cumsum(ref["vcount"], dtype=np.int64) - ref["vcount"])
    assert np.array_equal(toff.cpu().numpy(), np.cumsum(ref["tcount"], dtype=np.int64) - ref["tcount"])


def test_chunked_scan_carries_across_chunks(gpu, monkeypatch):
    monkeypatch.setattr(mesh, "_SCAN_CHUNK", 1000)
    c = torch.randint(0, 13, (4321,), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(gpu)
    out, total = mesh._exclusive_scan(c)
    want = torch.cumsum(c.long(), 0) - c
    assert torch.equal(out.long(), want) and int(total) == int(c.long().sum())


@pytest.mark.parametrize("value", [0.0, 1.0], ids=["all-below", "all-above"])
@pytest.mark.parametrize("R", [1, 13, (7, 3, 12)], ids=str)
def test_empty_result_makes_no_emit_launch(gpu, monkeypatch, value, R):
    Rx, Ry, Rz = _r3(R)
    calls = []
    real = mesh.call
    monkeypatch.setattr(mesh, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    m = mesh.mesh_from_lattice(torch.full((Rz + 1, Ry + 1, Rx + 1), value, device=gpu), 0.5, LO, HI)
    torch.cuda.synchronize()
    assert calls == ["mfnerf_mesh_count"]
    assert tuple(m["vertices"].shape) == (0, 3) and tuple(m["normals"].shape) == (0, 3)
    assert tuple(m["faces"].shape) == (0, 3) and m["faces"].dtype == torch.int32
    assert m["vertices"].device.type == "cuda"


def test_limits_are_refused_before_any_launch(gpu):
    """Straight through the C ABI, tiny buffers and absurd sizes: MFN_ERR_INVALID with a message, and
    the buffers keep their contents."""
    lib = _lib.load()
    P, NULL = _lib.ptr, ctypes.c_void_p(0)
    f3 = lambda *v: (ctypes.c_float * 3)(*v)  # noqa: E731
    lo, hi = f3(-1, -1, -1), f3(1, 1, 1)
    sigma = torch.zeros(8, device=gpu)
    sigma[0] = 1.0
    b8 = torch.full((64,), 7, dtype=torch.uint8, device=gpu)
    c8 = torch.full((64,), 7, dtype=torch.uint8, device=gpu)
    i32 = torch.full((64,), 7, dtype=torch.int32, device=gpu)
    j32 = torch.full((64,), 7, dtype=torch.int32, device=gpu)
    f32 = torch.full((64,), 7.0, device=gpu)
    g32 = torch.full((64,), 7.0, device=gpu)
    st = _lib.stream()

    def refused(status, word):
        assert status == 1, status  # MFN_ERR_INVALID
        msg = lib.mfnerf_last_error().decode()
        assert word in msg, msg

    big = [(1 << 11, 1 << 10, 1 << 10), (1 << 31, 2, 2), (2, 1 << 40, 2), (1 << 21, 1 << 21, 1 << 21),
           (46341, 46341, 2), (1291, 1291, 1291)]
    for nx, ny, nz in big:
        refused(lib.mfnerf_mesh_count(P(sigma), nx, ny, nz, 0.5, P(b8), P(c8), st), "2^31")
        refused(lib.mfnerf_mesh_emit(P(sigma), nx, ny, nz, 0.5, P(i32), P(j32), lo, hi, P(f32), P(g32), P(i32), st),
                "2^31")
        refused(lib.mfnerf_mesh_lattice_points(lo, hi, nx, ny, nz, 0, 4, P(f32), st), "2^31")
    for nx, ny, nz in [(1, 2, 2), (2, 1, 2), (2, 2, 1), (0, 2, 2), (2, 2, -5)]:  # some R = 0 (or worse)
        refused(lib.mfnerf_mesh_count(P(sigma), nx, ny, nz, 0.5, P(b8), P(c8), st), "resolution")
        refused(lib.mfnerf_mesh_emit(P(sigma), nx, ny, nz, 0.5, P(i32), P(j32), lo, hi, P(f32), P(g32), P(i32), st),
                "resolution")
        refused(lib.mfnerf_mesh_lattice_points(lo, hi, nx, ny, nz, 0, 1, P(f32), st), "resolution")
    # null pointers, one at a time
    count_args = [P(sigma), 2, 2, 2, 0.5, P(b8), P(c8), st]
    for k in (0, 5, 6):
        refused(lib.mfnerf_mesh_count(*[NULL if i == k else a for i, a in enumerate(count_args)]), "null")
    emit_args = [P(sigma), 2, 2, 2, 0.5, P(i32), P(j32), lo, hi, P(f32), P(g32), P(i32), st]
    for k in (0, 5, 6, 7, 8, 9, 10, 11):
        refused(lib.mfnerf_mesh_emit(*[NULL if i == k else a for i, a in enumerate(emit_args)]), "null")
    refused(lib.mfnerf_mesh_lattice_points(lo, hi, 2, 2, 2, 0, 8, NULL, st), "null")
    refused(lib.mfnerf_mesh_lattice_points(None, hi, 2, 2, 2, 0, 8, P(f32), st), "null")
    # a slab outside the lattice
    for first, count in [(0, 9), (8, 1), (-1, 2), (3, -1), (1 << 40, 1), (1, 1 << 62)]:
        refused(lib.mfnerf_mesh_lattice_points(lo, hi, 2, 2, 2, first, count, P(f32), st), "outside")
    assert lib.mfnerf_mesh_lattice_points(lo, hi, 2, 2, 2, 8, 0, P(f32), st) == 0  # an empty slab is fine
    torch.cuda.synchronize()
    for t in (b8, c8, i32, j32, f32, g32):
        assert bool((t == 7).all()), "a refused call wrote to its buffers"
    # Python refuses V or F beyond int32 before the emit launch
    with pytest.raises(RuntimeError, match="2\\^31"):
        mesh.emit(sigma.view(2, 2, 2), 0.5, -1, 1, i32, j32, 1 << 31, 5)
    with pytest.raises(RuntimeError, match="2\\^31"):
        mesh.emit(sigma.view(2, 2, 2), 0.5, -1, 1, i32, j32, 5, 1 << 31)


def test_lattice_points_slabs(gpu):
    """Any slab of the lattice equals the torch-computed points, bit for bit, unequal extents."""
    lo, hi = (-0.4, -0.2, -0.7), (0.5, 0.3, 0.6)
    nx, ny, nz = 8, 4, 13
    want = _torch_lattice_points(lo, hi, (nx - 1, ny - 1, nz - 1), gpu)
    n = nx * ny * nz
    lo3, hi3 = (ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*hi)
    for first, count in [(0, n), (0, 1), (n - 1, 1), (37, 301), (255, 161)]:
        out = torch.full((count + 2, 3), -9.0, device=gpu)
        _lib.call("mfnerf_mesh_lattice_points", lo3, hi3, nx, ny, nz, first, count, _lib.ptr(out[1:]), _lib.stream())
        assert torch.equal(out[1:count + 1], want[first:first + count])
        assert bool((out[0] == -9).all()) and bool((out[-1] == -9).all())


def test_two_runs_are_bit_identical(gpu):
    sigma, thr, _ = _reference("noise", 33)
    s = torch.from_numpy(sigma).to(gpu)
    a = mesh.mesh_from_lattice(s, thr, LO, HI)
    b = mesh.mesh_from_lattice(s, thr, LO, HI)
    for k in ("vertices", "normals", "faces"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


# ------------------------------------------------------------------------------- on a model
def _torch_lattice_points(lo, hi, R, dev):
    """(n, 3) f32 lattice points in linear-index order, from torch ops: lo + i * ((hi - lo) / R)."""
    ax = []
    for k in range(3):
        l, h = torch.tensor(lo[k], dtype=torch.float32), torch.tensor(hi[k], dtype=torch.float32)
        step = ((h - l) / torch.tensor(float(R[k]), dtype=torch.float32)).to(dev)  # one IEEE fp32 division
        ax.append(l.to(dev) + torch.arange(R[k] + 1, dtype=torch.float32, device=dev) * step)
    z, y, x = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return torch.stack([x, y, z], -1).reshape(-1, 3).contiguous()


@pytest.fixture(scope="module")
def model(gpu):
    from mfnerf.field import XYZ_NET_PARAMS
    from mfnerf.networks import NGP
    from mfnerf.trainer import HParams
    m = NGP(scale=0.5, hparams=HParams(T=16)).to(gpu)  # the Lego layout at T = 2^16
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        table = m.xyz_encoder.params[XYZ_NET_PARAMS:]
        table.copy_((torch.rand(table.numel(), generator=g) - 0.5).to(gpu))  # re-drawn U(-0.5, 0.5)
    return m


RES = (20, 17, 23)
BOUNDS = ((-0.45, -0.3, -0.5), (0.4, 0.5, 0.35))


def test_extract_mesh_on_a_model(gpu, model):
    lo, hi = BOUNDS
    n = (RES[0] + 1) * (RES[1] + 1) * (RES[2] + 1)
    with torch.no_grad():
        want_sigma = model.density(_torch_lattice_points(lo, hi, RES, gpu)).view(RES[2] + 1, RES[1] + 1, RES[0] + 1)
    thr = float(want_sigma.median())
    assert math.isfinite(thr) and float(want_sigma.min()) < thr < float(want_sigma.max())
    # the lattice does not depend on the slab size: whole, dividing (n = 9072 = 9 * 1008) and not
    assert n == 9 * 1008
    for chunk in (1 << 22, 1008, 4536, 1000, 4099):
        m = mesh.extract_mesh(model, RES, thr, bounds=BOUNDS, colors=False, chunk=chunk, return_sigma=True)
        assert torch.equal(m["sigma"], want_sigma), f"chunk {chunk}"
    m = mesh.extract_mesh(model, RES, thr, bounds=BOUNDS, return_sigma=True)
    assert set(m) == {"vertices", "normals", "faces", "colors", "sigma"}
    ref = M.extract(want_sigma.cpu().numpy(), thr, lo, hi)
    assert ref["vertices"].shape[0] > 1000
    _assert_matches(_host({k: m[k] for k in ("vertices", "normals", "faces")}), ref, lo, hi, normals=False)
    with torch.no_grad():
        zero = (m["normals"] == 0).all(1, keepdim=True)
        dirs = torch.where(zero, torch.tensor([0.0, 0.0, 1.0], device=gpu), -m["normals"])
        want_rgb = model(m["vertices"], dirs)[1]
    assert m["colors"].dtype == torch.float32 and torch.equal(m["colors"], want_rgb)
    # defaults: the scene box, threshold 20 (test.ipynb), colours on
    d = mesh.extract_mesh(model, 6)
    whole = mesh.extract_mesh(model, 6, 20.0, bounds=(-0.5, 0.5), colors=True)
    for k in ("vertices", "normals", "faces", "colors"):
        assert torch.equal(d[k], whole[k])
    assert "sigma" not in d


def test_vertex_colors_of_zero_normals(gpu, model):
    v = torch.tensor([[0.1, 0.2, -0.1], [0.0, 0.3, 0.2]], device=gpu)
    nrm = torch.tensor([[0.0, 0.0, 0.0], [0.6, 0.0, 0.8]], device=gpu)
    got = mesh.vertex_colors(model, {"vertices": v, "normals": nrm})
    dirs = torch.tensor([[0.0, 0.0, 1.0], [-0.6, 0.0, -0.8]], device=gpu)
    with torch.no_grad():
        assert torch.equal(got, model(v, dirs)[1])


def test_trainer_extract_mesh(gpu):
    from mfnerf import data
    from mfnerf.trainer import HParams, Trainer
    W = 32
    focal = 0.5 * W / math.tan(0.5 * 0.6911112)
    imgs, poses, dirs, K = data.ball_scene_views(data.BallScene(n_balls=6, seed=1), 8, W, focal, seed=0)
    ds = data.DeviceDataset(imgs, poses, dirs, K=K, img_wh=(W, W), device=gpu, seed=5)
    tr = Trainer(HParams(batch_size=1024, T=16), ds, device=gpu)
    tr.fit(steps=32, log_every=0)
    sigma = tr.extract_mesh(resolution=8, colors=False, return_sigma=True)["sigma"]
    thr = float(sigma.median())
    kw = dict(resolution=(24, 20, 16), sigma_threshold=thr, bounds=((-0.5, -0.4, -0.3), (0.5, 0.45, 0.4)),
              return_sigma=True)
    a = tr.extract_mesh(**kw)
    b = mesh.extract_mesh(tr.to_ngp(), **kw)
    assert set(a) == set(b) == {"vertices", "normals", "faces", "colors", "sigma"}
    assert a["vertices"].shape[0] > 0 and a["faces"].shape[0] > 0
    for k in a:
        assert torch.equal(a[k], b[k]), k
