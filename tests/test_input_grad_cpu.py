"""CPU tests of the input-gradient feature: the three new entry points' header declarations against
their ctypes signatures, the tests' own fp64 reference of dL/dx against torch autograd, and the pose
helpers (mfnerf.pose).  No GPU compute."""
import ctypes
import os
import re

import pytest
import torch

import input_grad_ref as R
from conftest import ROOT

NEW_ENTRY_POINTS = ["mfnerf_grid_encode_bw_input", "mfnerf_field_bw_inputs", "mfnerf_rays_input_grad"]


def _declared_args(name):
    src = open(os.path.join(ROOT, "include", "mfnerf.h")).read()
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, re.M | re.S)
    assert m, f"{name} is not declared in include/mfnerf.h"
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


@pytest.mark.parametrize("name", NEW_ENTRY_POINTS)
def test_header_and_ctypes_signature_agree(name):
    from mfnerf import _lib
    args = _declared_args(name)
    assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    res, argtypes = _lib.SIGNATURES[name]
    assert res is ctypes.c_int
    assert len(args) == len(argtypes), (args, argtypes)
    for a, t in zip(args, argtypes):
        declared_ptr = "*" in a or a.startswith("mfnerf_stream_t")
        bound_ptr = t is ctypes.c_void_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer))
        assert declared_ptr == bound_ptr, (name, a, t)
        if not declared_ptr:  # scalars: the same C type
            want = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float}[a.split()[0]]
            assert t is want, (name, a, t)


def test_library_exports_the_new_entry_points():
    from mfnerf import _lib
    assert os.path.exists(_lib.LIB_PATH), "build libmfnerf_hip.so first (__graft_entry__.build())"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert _lib.load().mfnerf_abi_version() == 2


@pytest.mark.parametrize("kind,n_tables", R.KINDS)
def test_dx_reference_matches_autograd(kind, n_tables):
    """The formula evaluated term by term in fp64 (pos from the fp32 fma) against autograd through a
    differentiable fp64 restatement of the encode, at 2049 random points plus 0, 1 and
    (0.5, 0.25, 0.75); no point excluded.  Bound: 2e-4 of the largest component (measured 3.8e-5 Hash,
    3.1e-5 MixedFeature: the fp32 rounding of pos, <= 2^-24 * 1024 at the finest level)."""
    lay, _ = R.layouts(kind, n_tables)
    n = 2049 + 3
    x = R.points(n, seed=1)
    assert torch.equal(x[:3], torch.tensor([[0.0, 0, 0], [1.0, 1, 1], [0.5, 0.25, 0.75]]))
    table = R.random_table16(lay, seed=2)
    dy = torch.randn(n, lay.L * lay.F, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    ref, A = R.dx_ref(x, table, dy, lay)
    xv = x.double().requires_grad_(True)
    (R.encode64(xv, table, lay, x) * dy).sum().backward()
    err = (ref - xv.grad).abs().max().item()
    scale = ref.abs().max().item()
    print(f"{kind}: max |formula - autograd| / max |ref| = {err / scale:.3e}")
    assert scale > 0 and torch.isfinite(ref).all()
    assert err <= 2e-4 * scale
    assert (ref.abs() <= A * (1 + 1e-12)).all()


def test_axisangle_matches_matrix_exp():
    from mfnerf.pose import axisangle_to_R
    g = torch.Generator().manual_seed(0)
    v = torch.randn(17, 3, generator=g)
    v[0] = 0.0                      # the guarded |v| = 0
    v[1] *= 1e-4                    # a small angle
    v[2] = torch.tensor([0.0, 0.0, 3.0])
    Rb = axisangle_to_R(v)
    assert Rb.shape == (17, 3, 3) and Rb.dtype == torch.float32
    vx, vy, vz = v.double().unbind(-1)
    o = torch.zeros_like(vx)
    K = torch.stack([o, -vz, vy, vz, o, -vx, -vy, vx, o], -1).reshape(-1, 3, 3)
    ref = torch.matrix_exp(K)
    assert (Rb.double() - ref).abs().max().item() <= 1e-6
    assert torch.equal(axisangle_to_R(v[3]), Rb[3])  # an unbatched vector
    assert torch.equal(axisangle_to_R(torch.zeros(3)), torch.eye(3))


def test_pose_refiner_identity_and_gradients():
    from mfnerf import data, synthetic
    from mfnerf.pose import PoseRefiner
    poses = synthetic.camera_poses(n_cams=6)[:, :3].float()
    ref = PoseRefiner(len(poses))
    idx = torch.tensor([0, 3, 3, 5, 1])
    out = ref(poses[idx], idx)
    assert out.shape == (5, 3, 4)
    assert (out - poses[idx]).abs().max().item() <= 1e-7
    assert (ref.refined_poses(poses) - poses).abs().max().item() <= 1e-7
    assert not ref.refined_poses(poses).requires_grad
    # gradients reach dR / dT through get_rays, only on the images drawn
    dirs = torch.randn(5, 3, generator=torch.Generator().manual_seed(1))
    rays_o, rays_d = data.get_rays(dirs, out)
    wo = torch.randn(5, 3, generator=torch.Generator().manual_seed(2))
    wd = torch.randn(5, 3, generator=torch.Generator().manual_seed(3))
    ((rays_o * wo).sum() + (rays_d * wd).sum()).backward()
    assert ref.dR.grad is not None and ref.dT.grad is not None
    want_dT = torch.zeros(6, 3).index_add_(0, idx, wo)
    assert torch.allclose(ref.dT.grad, want_dT, atol=1e-6)
    assert ref.dR.grad[[0, 1, 3, 5]].abs().sum(1).min().item() > 0
    assert ref.dR.grad[[2, 4]].abs().max().item() == 0 and ref.dT.grad[[2, 4]].abs().max().item() == 0
    opt = ref.optimizer()
    assert isinstance(opt, torch.optim.Adam) and opt.param_groups[0]["lr"] == 1e-6
    opt.step()
    assert (ref.refined_poses(poses) - poses).abs().max().item() > 0
