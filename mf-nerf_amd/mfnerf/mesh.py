"""A triangle mesh of the density field, extracted on the device (the reference's test.ipynb "mesh"
cell: model.density on an N^3 lattice, a host copy, mcubes.marching_cubes(sigma, sigma_threshold)
with sigma_threshold = 20).

    mesh = extract_mesh(model, resolution=256)        # or trainer.extract_mesh(resolution=256)
    save_ply("mesh.ply", mesh)

The lattice is filled slab by slab with the existing density kernels, classified and emitted by
csrc/mesh.hip (marching tetrahedra on the Kuhn split: the same iso-surface as marching cubes,
triangulated differently, watertight without an ambiguity table; specification: tests/mesh_ref.py).
Everything stays on the device; the vertex and face totals are read back once to size the outputs:
ONE host synchronisation per mesh.

Floaters (csrc/mesh_clean.hip; specification: tests/mesh_clean_ref.py): extract_mesh(occupancy=True)
clears the lattice where the renderer never samples, and clean_mesh / extract_mesh(clean={...})
removes small connected components, with one more synchronisation to size the cleaned mesh.
"""
import ctypes

import numpy as np
import torch

from ._lib import call, ptr, stream

_SCAN_CHUNK = 1 << 24  # elements per cumsum: bounds the scan's temporaries (12 * 2^24 < 2^31)
_LIMIT = 1 << 31


def _f3(v, name):
    a = [float(x) for x in (v if hasattr(v, "__len__") else (v, v, v))]
    if len(a) != 3:
        raise ValueError(f"{name} must be a number or three numbers")
    return (ctypes.c_float * 3)(*a)


def _exclusive_scan(counts):
    """uint8 counts (n,) -> (exclusive prefix sum (n,) int32, total () int64), on the device with no
    host read.  torch.cumsum in chunks, the carry a device scalar: beyond `counts` and the result the
    scan holds only chunk-sized temporaries."""
    n = counts.numel()
    out = torch.empty(n, dtype=torch.int32, device=counts.device)
    total = torch.zeros((), dtype=torch.int64, device=counts.device)
    for i in range(0, n, _SCAN_CHUNK):
        c = counts[i:i + _SCAN_CHUNK]
        inc = torch.cumsum(c, 0, dtype=torch.int32)
        # wraps only when the total reaches 2^31, which the caller refuses before anything reads `out`
        out[i:i + _SCAN_CHUNK] = (inc - c + total).to(torch.int32)
        total = total + inc[-1]
    return out, total


def _check_lattice(sigma):
    if not isinstance(sigma, torch.Tensor) or sigma.dim() != 3:
        raise RuntimeError("sigma must be a (nz, ny, nx) tensor")
    if sigma.dtype != torch.float32:
        raise RuntimeError(f"sigma must be {torch.float32}, got {sigma.dtype}")
    if not sigma.is_contiguous():
        raise RuntimeError("sigma must be contiguous")
    nz, ny, nx = sigma.shape
    if min(nx, ny, nz) < 2:
        raise RuntimeError(f"every resolution must be >= 1 (lattice {nx} x {ny} x {nz} points)")
    if nx * ny * nz >= _LIMIT:
        raise RuntimeError(f"the lattice must have fewer than 2^31 points ({nx} x {ny} x {nz})")
    if not sigma.is_cuda:
        raise RuntimeError("sigma must be a CUDA tensor")
    return nx, ny, nz


def count(sigma, threshold):
    """First pass (mfnerf_mesh_count): (vcount (n,) u8: the crossing edges each lattice point owns,
    tcount (cells,) u8: the triangles of each cell)."""
    nx, ny, nz = _check_lattice(sigma)
    vcount = torch.empty(nx * ny * nz, dtype=torch.uint8, device=sigma.device)
    tcount = torch.empty((nx - 1) * (ny - 1) * (nz - 1), dtype=torch.uint8, device=sigma.device)
    call("mfnerf_mesh_count", ptr(sigma), nx, ny, nz, float(threshold), ptr(vcount), ptr(tcount), stream())
    return vcount, tcount


def count_and_scan(sigma, threshold):
    """The first pass and the two scans: (voff (n,) i32, toff (cells,) i32, totals (2,) i64 on the
    device = [V, F]).  No host read.  Workspace: 1 + 1 + 4 + 4 bytes per lattice point."""
    vcount, tcount = count(sigma, threshold)
    voff, V = _exclusive_scan(vcount)
    del vcount
    toff, F = _exclusive_scan(tcount)
    return voff, toff, torch.stack([V, F])


def emit(sigma, threshold, lo, hi, voff, toff, V, F):
    """Second pass (mfnerf_mesh_emit) into freshly sized outputs; V == 0 makes no launch."""
    nx, ny, nz = _check_lattice(sigma)
    dev = sigma.device
    if V >= _LIMIT or F >= _LIMIT:
        raise RuntimeError(f"the mesh must have fewer than 2^31 vertices and faces (got {V} and {F}): lower the "
                           "resolution")
    mesh = {"vertices": torch.empty(V, 3, dtype=torch.float32, device=dev),
            "normals": torch.empty(V, 3, dtype=torch.float32, device=dev),
            "faces": torch.empty(F, 3, dtype=torch.int32, device=dev)}
    if V > 0:  # no crossing edge: no triangle either
        call("mfnerf_mesh_emit", ptr(sigma), nx, ny, nz, float(threshold), ptr(voff), ptr(toff), _f3(lo, "lo"),
             _f3(hi, "hi"), ptr(mesh["vertices"]), ptr(mesh["normals"]), ptr(mesh["faces"]), stream())
    return mesh


@torch.no_grad()
def mesh_from_lattice(sigma, threshold, lo, hi):
    """The iso-surface sigma = threshold of a lattice of values as an indexed triangle mesh.

    sigma: (nz, ny, nx) float32 CUDA tensor, point (x, y, z) at world position lo + i*(hi - lo)/(n - 1)
    per axis (lo, hi: a number or three).  Inside is sigma > threshold.  Returns {"vertices" (V,3) f32,
    "normals" (V,3) f32, "faces" (F,3) i32}, all on sigma's device: normals are -grad sigma (unit, or
    zero where the gradient vanishes), triangles are wound so that their normal points out of the
    inside region.  Deterministic: the same bits on every run.

    One host synchronisation: V and F are read back to size the outputs.  An empty result gives
    (0,3) tensors and launches no emit."""
    voff, toff, totals = count_and_scan(sigma, threshold)
    V, F = (int(v) for v in totals.cpu())  # the one read
    return emit(sigma, threshold, lo, hi, voff, toff, V, F)


def _resolution3(resolution):
    r = tuple(int(v) for v in resolution) if hasattr(resolution, "__len__") else (int(resolution),) * 3
    if len(r) != 3:
        raise ValueError("resolution must be an int or (Rx, Ry, Rz)")
    if min(r) < 1:
        raise RuntimeError(f"every resolution must be >= 1, got {r}")
    if (r[0] + 1) * (r[1] + 1) * (r[2] + 1) >= _LIMIT:
        raise RuntimeError(f"the lattice must have fewer than 2^31 points, got resolution {r}")
    return r


@torch.no_grad()
def density_lattice(model, resolution, lo, hi, chunk=1 << 22, occupancy=False):
    """model.density on the lattice of `resolution` cells spanning [lo, hi] -> sigma (nz, ny, nx) f32.
    Slab by slab (mfnerf_mesh_lattice_points -> grid encode -> field_fw density_only) through two
    chunk-sized buffers, with no host synchronisation; the values do not depend on `chunk`.
    occupancy=True then clears (occupancy_mask) the points the renderer never samples."""
    from . import field
    Rx, Ry, Rz = _resolution3(resolution)
    nx, ny, nz = Rx + 1, Ry + 1, Rz + 1
    n = nx * ny * nz
    chunk = max(1, min(int(chunk), n))
    dev = model.xyz_encoder.params.device
    packed, table16 = field.field_weights(model.xyz_encoder.params, model.rgb_net.params, model.rgb_width)
    lo3, hi3 = _f3(lo, "lo"), _f3(hi, "hi")
    sigma = torch.empty(n, dtype=torch.float32, device=dev)
    xyz = torch.empty(chunk, 3, dtype=torch.float32, device=dev)
    feat = torch.empty(chunk, model.layout.L * model.layout.F, dtype=torch.float16, device=dev)
    for first in range(0, n, chunk):
        cnt = min(chunk, n - first)
        call("mfnerf_mesh_lattice_points", lo3, hi3, nx, ny, nz, first, cnt, ptr(xyz), stream())
        field.grid_encode_fw(xyz, cnt, table16, model.layout, model.desc, model._x_min, model._x_range, out=feat)
        field.field_fw(feat, None, cnt, packed, model.rgb_width, density_only=True, sigma=sigma[first:first + cnt])
    sigma = sigma.view(nz, ny, nx)
    if occupancy:
        occupancy_mask(sigma, lo, hi, model.density_bitfield, model.cascades, model.scale, model.grid_size)
    return sigma


def occupancy_mask(sigma, lo, hi, density_bitfield, cascades, scale, grid_size):
    """Clear IN PLACE (mfnerf_mesh_occupancy_mask) the lattice values the renderer never samples:
    points outside the scene box [-scale, scale]^3 and points whose cell of their own cascade has a
    clear bit in density_bitfield (uint8, packbits' layout).  Cleared means 0.0; the other values
    keep their bits.  The density there was never trained and may exceed any threshold."""
    if not isinstance(density_bitfield, torch.Tensor) or density_bitfield.dtype != torch.uint8:
        raise RuntimeError("density_bitfield must be a uint8 tensor")
    if not density_bitfield.is_contiguous():
        raise RuntimeError("density_bitfield must be contiguous")
    nx, ny, nz = _check_lattice(sigma)
    if not density_bitfield.is_cuda:
        raise RuntimeError("density_bitfield must be a CUDA tensor")
    call("mfnerf_mesh_occupancy_mask", ptr(sigma), _f3(lo, "lo"), _f3(hi, "hi"), nx, ny, nz, ptr(density_bitfield),
         density_bitfield.numel(), int(cascades), int(grid_size), float(scale), stream())
    return sigma


@torch.no_grad()
def vertex_colors(model, mesh):
    """model(vertices, -normals)'s rgb (V,3) f32: each vertex seen along its inward normal, from
    (0, 0, 1) where the normal is zero."""
    v, nrm = mesh["vertices"], mesh["normals"]
    if v.shape[0] == 0:
        return torch.empty(0, 3, dtype=torch.float32, device=v.device)
    zero = (nrm == 0).all(1, keepdim=True)
    dirs = torch.where(zero, torch.tensor([0.0, 0.0, 1.0], device=v.device), -nrm)
    return model(v, dirs)[1].float()


@torch.no_grad()
def extract_mesh(model, resolution=256, sigma_threshold=20.0, bounds=None, colors=True, chunk=1 << 22,
                 return_sigma=False, occupancy=False, clean=None):
    """The surface sigma = sigma_threshold of an mfnerf.networks.NGP as a triangle mesh (test.ipynb's
    mesh cell, whose threshold of 20 is the default).

    resolution: cells per axis, an int or (Rx, Ry, Rz); bounds = (lo, hi) in world coordinates (each a
    number or three), default the scene box [-scale, scale]^3.  The density lattice is filled slab by
    slab (`chunk` points at a time, no host synchronisation inside the loop), then mesh_from_lattice
    extracts the surface with ONE host synchronisation (reading the vertex and face totals).

    Returns {"vertices", "normals", "faces"} as mesh_from_lattice; colors=True adds "colors" (V,3) f32 =
    model(vertices, -normals)'s rgb; return_sigma=True adds "sigma" (nz, ny, nx) f32.

    occupancy=True culls the lattice by the model's own occupancy bitfield first (occupancy_mask: the
    density was never trained where the renderer does not sample); it needs sigma_threshold > 0, since
    a cleared point holds 0.  clean = a dict of clean_mesh's keyword arguments removes small
    components (one more host synchronisation) and adds "components"; colours are computed afterwards,
    on the kept vertices only.  With both at their defaults nothing changes."""
    if occupancy and not sigma_threshold > 0:
        raise RuntimeError(f"occupancy=True needs sigma_threshold > 0 (got {sigma_threshold}): a culled lattice "
                           "point holds 0.0 and would lie inside the surface")
    if clean is not None:
        clean = dict(clean)
        _check_selection(**clean)
    if colors and getattr(model, "rgb_act", "Sigmoid") != "Sigmoid":
        raise NotImplementedError("extract_mesh(colors=True): vertex colours of an HDR/exposure model "
                                  "(rgb_act='None') need an exposure, which this call does not take; pass "
                                  "colors=False")
    lo, hi = (-float(model.scale), float(model.scale)) if bounds is None else bounds
    sigma = density_lattice(model, resolution, lo, hi, chunk, occupancy)
    mesh = mesh_from_lattice(sigma, sigma_threshold, lo, hi)
    if clean is not None:
        mesh = clean_mesh(mesh, **clean)
    if colors:
        mesh["colors"] = vertex_colors(model, mesh)
    if return_sigma:
        mesh["sigma"] = sigma
    return mesh


# ------------------------------------------------------------------------------- cleaning
def _check_mesh(mesh):
    """(V, F) of a mesh dict after the argument checks; touches no device."""
    if not isinstance(mesh, dict) or any(k not in mesh for k in ("vertices", "normals", "faces")):
        raise RuntimeError('mesh must be a dict with "vertices", "normals" and "faces"')
    names = [("vertices", torch.float32), ("normals", torch.float32), ("faces", torch.int32)]
    if mesh.get("colors") is not None:
        names.append(("colors", torch.float32))
    for name, dtype in names:
        t = mesh[name]
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 3:
            raise RuntimeError(f"{name} must be a (n, 3) tensor")
        if t.dtype != dtype:
            raise RuntimeError(f"{name} must be {dtype}, got {t.dtype}")
        if not t.is_contiguous():
            raise RuntimeError(f"{name} must be contiguous")
    V, F = mesh["vertices"].shape[0], mesh["faces"].shape[0]
    for name, _ in names:
        if name != "faces" and mesh[name].shape[0] != V:
            raise RuntimeError(f"{name} must have one row per vertex ({V}), got {mesh[name].shape[0]}")
    if V >= _LIMIT or F >= _LIMIT:
        raise RuntimeError(f"the mesh must have fewer than 2^31 vertices and faces (got {V} and {F})")
    for name, _ in names:
        if not mesh[name].is_cuda:
            raise RuntimeError(f"{name} must be a CUDA tensor")
    return V, F


def _check_selection(min_faces=0, min_fraction=0.0, largest_only=False):
    if int(min_faces) != min_faces or min_faces < 0:
        raise RuntimeError(f"min_faces must be an integer >= 0, got {min_faces}")
    if not 0.0 <= float(min_fraction) <= 1.0:
        raise RuntimeError(f"min_fraction must lie in [0, 1], got {min_fraction}")


def _components(faces, V):
    F = faces.shape[0]
    if V == 0 or F == 0:  # every vertex its own component, no launch of ours
        return (torch.arange(V, dtype=torch.int32, device=faces.device),
                torch.zeros(V, dtype=torch.int32, device=faces.device))
    labels = torch.empty(V, dtype=torch.int32, device=faces.device)
    face_counts = torch.empty(V, dtype=torch.int32, device=faces.device)
    call("mfnerf_mesh_components", ptr(faces), V, F, ptr(labels), ptr(face_counts), stream())
    return labels, face_counts


@torch.no_grad()
def components(mesh):
    """Connected components of a mesh (mfnerf_mesh_components): two vertices are connected when a face
    holds both.  Returns {"labels" (V,) i32: the smallest vertex index of each vertex's component,
    "face_counts" (V,) i32: at index r the faces of the component labelled r, 0 elsewhere}, device
    tensors, no host read; the same bits on every run.  Precondition: face indices in [0, V) (a face
    with an index outside is ignored: it connects nothing and counts nowhere)."""
    V, _ = _check_mesh(mesh)
    labels, face_counts = _components(mesh["faces"], V)
    return {"labels": labels, "face_counts": face_counts}


@torch.no_grad()
def clean_mesh(mesh, min_faces=0, min_fraction=0.0, largest_only=False):
    """A copy of `mesh` without its floaters.  A component (see `components`) is kept when its face
    count is >= min_faces and >= min_fraction (rounded to fp32) times the largest component's, the
    product and the comparison in fp64; largest_only keeps the largest alone, the one with the smallest
    label among equals.  A vertex no face uses is always dropped, and so is a face with an index
    outside [0, V) (indices in [0, V) are the precondition).

    The compaction is stable: kept vertices and faces keep their order, "vertices", "normals" and
    "colors" (if given) are copied bit for bit, face indices are renumbered.  Returns a new dict with
    those keys, "components": (total, kept) as ints and "sigma" passed through if present; the input
    is not modified.  Selection thresholds are computed on the device; ONE host synchronisation reads
    [V', F', total, kept] to size the outputs.  An empty mesh comes back empty without a launch."""
    _check_selection(min_faces, min_fraction, largest_only)
    V, F = _check_mesh(mesh)
    if V == 0 or F == 0:  # nothing is referenced: every vertex is a component of no face
        return compact(mesh, None, (0, 0, V, 0))
    labels, face_counts = _components(mesh["faces"], V)
    flags, sizes = select_and_scan(mesh, labels, face_counts, min_faces, min_fraction, largest_only)
    del labels, face_counts
    return compact(mesh, flags, sizes)


def select_and_scan(mesh, labels, face_counts, min_faces=0, min_fraction=0.0, largest_only=False):
    """clean_mesh's middle (mfnerf_mesh_select, two scans, the read): ((vkeep (V,) u8, voff (V,) i32,
    fkeep (F,) u8, foff (F,) i32), (V', F', components, components kept)).  V, F > 0."""
    V, F = mesh["vertices"].shape[0], mesh["faces"].shape[0]
    dev = mesh["vertices"].device
    vkeep = torch.empty(V, dtype=torch.uint8, device=dev)
    fkeep = torch.empty(F, dtype=torch.uint8, device=dev)
    stats = torch.empty(3, dtype=torch.int64, device=dev)
    call("mfnerf_mesh_select", ptr(mesh["faces"]), V, F, ptr(labels), ptr(face_counts), int(min_faces),
         float(min_fraction), int(bool(largest_only)), ptr(vkeep), ptr(fkeep), ptr(stats), stream())
    voff, Vk = _exclusive_scan(vkeep)
    foff, Fk = _exclusive_scan(fkeep)
    sizes = tuple(int(v) for v in torch.stack([Vk, Fk, stats[0], stats[1]]).cpu())  # the one read
    return (vkeep, voff, fkeep, foff), sizes


def compact(mesh, flags, sizes):
    """clean_mesh's end (mfnerf_mesh_compact) into freshly sized outputs; F' == 0 makes no launch."""
    Vk, Fk, total, kept = sizes
    if Vk >= _LIMIT or Fk >= _LIMIT:
        raise RuntimeError(f"the mesh must have fewer than 2^31 vertices and faces (got {Vk} and {Fk})")
    dev = mesh["vertices"].device
    has_colors = mesh.get("colors") is not None
    out = {k: torch.empty(Vk, 3, dtype=torch.float32, device=dev)
           for k in ["vertices", "normals"] + (["colors"] if has_colors else [])}
    out["faces"] = torch.empty(Fk, 3, dtype=torch.int32, device=dev)
    out["components"] = (total, kept)
    if "sigma" in mesh:
        out["sigma"] = mesh["sigma"]
    if Fk > 0:  # a kept face brings three kept vertices
        vkeep, voff, fkeep, foff = flags
        call("mfnerf_mesh_compact", ptr(mesh["vertices"]), ptr(mesh["normals"]),
             ptr(mesh["colors"] if has_colors else None), ptr(mesh["faces"]), mesh["vertices"].shape[0],
             mesh["faces"].shape[0], ptr(vkeep), ptr(voff), ptr(fkeep), ptr(foff), ptr(out["vertices"]),
             ptr(out["normals"]), ptr(out["colors"] if has_colors else None), ptr(out["faces"]), stream())
    return out


def save_ply(path, mesh):
    """Write a mesh (tensors or arrays) as binary little-endian PLY: float x y z nx ny nz per vertex,
    uchar red green blue when the mesh has "colors" (in [0, 1]), and int32 vertex-index face lists."""
    def host(a, dtype):
        if isinstance(a, torch.Tensor):
            a = a.detach().cpu().numpy()
        return np.ascontiguousarray(a, dtype=dtype)

    v = host(mesh["vertices"], "<f4").reshape(-1, 3)
    nrm = host(mesh["normals"], "<f4").reshape(-1, 3)
    f = host(mesh["faces"], "<i4").reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    has_colors = mesh.get("colors") is not None
    if has_colors:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    verts = np.empty(v.shape[0], dtype=fields)
    for k, name in enumerate(("x", "y", "z")):
        verts[name] = v[:, k]
        verts["n" + name] = nrm[:, k]
    if has_colors:
        c = np.rint(np.clip(host(mesh["colors"], "<f4").reshape(-1, 3), 0.0, 1.0) * 255.0).astype("u1")
        for k, name in enumerate(("red", "green", "blue")):
            verts[name] = c[:, k]
    face_rec = np.empty(f.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    face_rec["n"] = 3
    face_rec["v"] = f
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"]
    header += [f"property float {name}" for name in ("x", "y", "z", "nx", "ny", "nz")]
    if has_colors:
        header += [f"property uchar {name}" for name in ("red", "green", "blue")]
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(verts.tobytes())
        out.write(face_rec.tobytes())
