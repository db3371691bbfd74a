"""Host side of the fused test-time renderer: the C ABI declaration and its ctypes signature agree,
the library exports it, and render_fused refuses host tensors like the vren ops.  No GPU compute."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT


def _declared_args(name):
    src = open(os.path.join(ROOT, "include", "mfnerf.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"^\s*int\s+" + name + r"\s*\((.*?)\)\s*;", src, re.M | re.S)
    assert m, f"{name} is not declared in include/mfnerf.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_and_signature_agree():
    from mfnerf import _lib
    args = _declared_args("mfnerf_render_test_fused")
    assert "mfnerf_render_test_fused" in _lib.SIGNATURES
    res, argtypes = _lib.SIGNATURES["mfnerf_render_test_fused"]
    assert res is ctypes.c_int
    assert len(argtypes) == len(args) == 26
    # every pointer argument of the declaration is a pointer in the binding, every scalar a scalar
    for decl, ty in zip(args, argtypes):
        is_ptr = "*" in decl or "mfnerf_stream_t" in decl
        assert is_ptr == (ty is ctypes.c_void_p or ty is ctypes.POINTER(_lib.GridDesc)), decl
    scalars = [(d.split()[-1], t) for d, t in zip(args, argtypes) if "*" not in d and "mfnerf_stream_t" not in d]
    kinds = {"n_rays": ctypes.c_int64, "cascades": ctypes.c_int, "scale": ctypes.c_float,
             "exp_step_factor": ctypes.c_float, "grid_size": ctypes.c_int, "max_samples_dt": ctypes.c_int,
             "ray_budget": ctypes.c_int, "T_threshold": ctypes.c_float, "x_min": ctypes.c_float,
             "x_range": ctypes.c_float, "rgb_width": ctypes.c_int}
    assert dict(scalars) == kinds


def test_library_exports_the_entry_point():
    from mfnerf import _lib
    assert os.path.exists(_lib.LIB_PATH), "build libmfnerf_hip.so first (__graft_entry__.build())"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mfnerf_render_test_fused")
    assert _lib.load().mfnerf_abi_version() == 2


def test_render_fused_rejects_cpu_tensors():
    from mfnerf import rendering
    o, d = torch.zeros(4, 3), torch.ones(4, 3)
    with pytest.raises(RuntimeError, match="CUDA"):
        rendering.render_fused(None, o, d)
