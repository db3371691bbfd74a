"""CPU tests of pose refinement inside the fused step: the tests' own fp64 reference (pose_ref) against
autograd through the formula, the three new entry points' declarations against their ctypes
signatures, and the configuration surface (HParams.optimize_ext, StepConfig.refine_poses).  No GPU
compute."""
import ctypes
import os
import re

import pytest
import torch

import pose_ref as P
from conftest import ROOT

NEW_ENTRY_POINTS = ["mfnerf_pose_grad", "mfnerf_pose_step", "mfnerf_sample_rays_prep_idx"]


@pytest.mark.parametrize("length", [0.0, 1e-6, 1e-3, 0.1, 1.0])
def test_analytic_jt_g_matches_fp64_autograd(length):
    """pose_ref.jt_g against torch autograd through pose_ref.rotation (the reference's formula, guard
    included) in fp64, 64 random (axis, u, g) per |w|.  Bound 1e-8 |u||g|: autograd's own closed-form
    b' = sin t/t^2 - 2(1 - cos t)/t^3 loses up to 1e-16/t^3 * |w|^2 <= 1e-9 at t ~ 1e-6 and less
    elsewhere; a wrong term misses by O(|w|) or O(1).  At w = 0 both equal u x g."""
    g = torch.Generator().manual_seed(int(length * 1e7) + 1)
    ax = torch.randn(64, 3, generator=g, dtype=torch.float64)
    w = (ax / ax.norm(dim=1, keepdim=True) * length).requires_grad_(True)
    u = torch.randn(64, 3, generator=g, dtype=torch.float64)
    gr = torch.randn(64, 3, generator=g, dtype=torch.float64)
    (P.rotate(w, u) * gr).sum().backward()
    got = P.jt_g(w.detach(), u, gr)
    scale = u.norm(dim=1) * gr.norm(dim=1)
    ratio = float(((got - w.grad).abs().max(dim=1).values / scale).max())
    print(f"|w| = {length:g}: max |analytic - autograd| / (|u||g|) = {ratio:.3e}")
    assert torch.isfinite(got).all()
    assert ratio <= 1e-8
    if length == 0.0:
        # a = sin(1e-7)/1e-7 = 1 - 1.7e-15
        assert float((got - torch.linalg.cross(u, gr)).abs().max()) <= 1e-12 * float(scale.max())


def test_reference_composition_matches_pose_refiner():
    """pose_ref.compose is mfnerf.pose.PoseRefiner's forward in fp64."""
    from mfnerf import synthetic
    from mfnerf.pose import PoseRefiner
    poses = synthetic.camera_poses(n_cams=6)[:, :3].float()
    ref = PoseRefiner(6)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        ref.dR.copy_(torch.randn(6, 3, generator=g) * 0.05)
        ref.dT.copy_(torch.randn(6, 3, generator=g) * 0.05)
        ref.dR[0] = 0
    want = P.compose(poses, ref.dR.detach(), ref.dT.detach())
    assert float((ref.refined_poses(poses).double() - want).abs().max()) <= 1e-6


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
    scalars = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64}
    for a, t in zip(args, argtypes):
        declared_ptr = "*" in a or a.startswith("mfnerf_stream_t")
        assert declared_ptr == (t is ctypes.c_void_p), (name, a, t)
        if not declared_ptr:
            assert t is scalars[a.split()[0]], (name, a, t)


def test_library_exports_the_new_entry_points():
    from mfnerf import _lib
    assert os.path.exists(_lib.LIB_PATH), "build libmfnerf_hip.so first (__graft_entry__.build())"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert _lib.load().mfnerf_abi_version() == 2


def test_hparams_and_step_config_carry_the_option():
    from mfnerf.engine import StepConfig
    from mfnerf.trainer import HParams
    hp = HParams(optimize_ext=True)
    assert hp.pose_lr == 1e-6 and not HParams().optimize_ext
    c = StepConfig(refine_poses=True)
    assert c.ray_grads and c.pose_lr == 1e-6           # refine_poses implies ray_grads
    d = StepConfig()
    assert not d.refine_poses and not d.ray_grads


class _NoInit:
    """TrainStep's validation without a device: the checks read cfg, dataset and shard only."""

    def __new__(cls, cfg, dataset=None, shard=None):
        from mfnerf.engine import TrainStep
        st = object.__new__(TrainStep)
        st.cfg, st.dataset, st.shard = cfg, dataset, shard
        return st


def test_refine_poses_validation_messages():
    from mfnerf.engine import StepConfig, TrainStep
    from mfnerf.trainer import HParams, Trainer
    cfg = StepConfig(refine_poses=True)
    with pytest.raises(ValueError, match="attached dataset"):
        _NoInit(cfg)._check_refine()
    with pytest.raises(ValueError, match="data-parallel pose refinement is out of scope"):
        _NoInit(cfg, dataset=object(), shard=(0, 0, 1))._check_refine()
    with pytest.raises(ValueError, match="data-parallel pose refinement is out of scope"):
        _NoInit(cfg, dataset=object())._check_refine(exchange=lambda g: g)
    with pytest.raises(ValueError, match="sharded optimizer"):
        TrainStep.shard_optimizer(_NoInit(cfg), 0, 2)
    _NoInit(cfg, dataset=object())._check_refine()       # the supported combination passes
    _NoInit(StepConfig())._check_refine(exchange=lambda g: g)  # and the option off checks nothing
    with pytest.raises(ValueError, match="n_parts == 1"):
        TrainStep(StepConfig(refine_poses=True, n_parts=2), device="cpu")  # raised before any allocation
    with pytest.raises(NotImplementedError, match="optimize_ext"):
        Trainer(HParams(optimize_ext=True), train=None, device="cpu", world=2)
