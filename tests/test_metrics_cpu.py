"""Host side of the validation metrics (mfnerf_image_metrics): the C ABI declaration and its ctypes
signature agree, the library exports both symbols at ABI version 2, the wrapper refuses bad
arguments, and the two restatements of the definition in metrics_ref.py check themselves and each
other.  No GPU compute."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import metrics_ref as R
from conftest import PKG, ROOT


def _declared(name):
    src = open(os.path.join(ROOT, "include", "mfnerf.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"^\s*(\w+)\s+" + name + r"\s*\((.*?)\)\s*;", src, re.M | re.S)
    assert m, f"{name} is not declared in include/mfnerf.h"
    return m.group(1), [a.strip() for a in m.group(2).split(",")]


def test_header_and_signature_agree():
    from mfnerf import _lib
    ret, args = _declared("mfnerf_image_metrics")
    res, argtypes = _lib.SIGNATURES["mfnerf_image_metrics"]
    assert ret == "int" and res is ctypes.c_int
    assert len(argtypes) == len(args) == 7
    # every pointer argument of the declaration is a pointer in the binding, every scalar a scalar
    for decl, ty in zip(args, argtypes):
        is_ptr = "*" in decl or "mfnerf_stream_t" in decl
        assert is_ptr == (ty is ctypes.c_void_p), decl
    scalars = [(d.split()[-1], t) for d, t in zip(args, argtypes) if "*" not in d and "mfnerf_stream_t" not in d]
    assert dict(scalars) == {"H": ctypes.c_int64, "W": ctypes.c_int64}
    assert args[4].startswith("double*") and args[4].split()[-1] == "out"

    ret, args = _declared("mfnerf_image_metrics_workspace")
    res, argtypes = _lib.SIGNATURES["mfnerf_image_metrics_workspace"]
    assert ret == "int64_t" and res is ctypes.c_int64
    assert [a.split()[0] for a in args] == ["int64_t", "int64_t"] and argtypes == [ctypes.c_int64] * 2


def test_library_exports_the_entry_points():
    from mfnerf import _lib
    assert os.path.exists(_lib.LIB_PATH), "build libmfnerf_hip.so first (__graft_entry__.build())"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mfnerf_image_metrics") and hasattr(lib, "mfnerf_image_metrics_workspace")
    assert _lib.load().mfnerf_abi_version() == 2


def test_workspace_query_and_tile_constants():
    """One pair of doubles per tile of the valid outputs; nothing for an image below one window.  The
    tile published by mfnerf/metrics.py is the kernel's (the sweep of the GPU tests is placed on it)."""
    from mfnerf import metrics
    src = open(os.path.join(PKG, "csrc", "metrics.hip")).read()
    m = re.search(r"constexpr int MT_TH = (\d+), MT_TW = (\d+);", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (metrics.TILE_H, metrics.TILE_W)
    assert f"static_assert(MT_TH == {metrics.TILE_H} && MT_TW == {metrics.TILE_W}" in src
    TH, TW = metrics.TILE_H, metrics.TILE_W
    assert metrics.workspace_bytes(11, 11) == 16
    assert metrics.workspace_bytes(TH + 10, TW + 10) == 16
    assert metrics.workspace_bytes(TH + 11, TW + 10) == 32
    assert metrics.workspace_bytes(TH + 11, 2 * TW + 11) == 2 * 3 * 16
    assert metrics.workspace_bytes(800, 800) == math.ceil(790 / TH) * math.ceil(790 / TW) * 16
    assert metrics.workspace_bytes(10, 800) == 0 and metrics.workspace_bytes(800, 10) == 0


def test_wrapper_rejects_bad_arguments():
    from mfnerf.metrics import image_metrics, psnr_from_mse
    H, W = 12, 13
    ok = torch.zeros(H * W, 3)
    with pytest.raises(RuntimeError, match="CUDA"):
        image_metrics(ok, ok, (W, H))
    with pytest.raises(RuntimeError, match="float32"):
        image_metrics(ok.double(), ok, (W, H))
    with pytest.raises(RuntimeError, match="float32"):
        image_metrics(ok, ok.half(), (W, H))
    with pytest.raises(RuntimeError, match="shape"):
        image_metrics(torch.zeros(H, W, 3), ok, (W, H))
    with pytest.raises(RuntimeError, match="shape"):
        image_metrics(ok, torch.zeros(H * W + 1, 3), (W, H))
    with pytest.raises(RuntimeError, match="shape"):
        image_metrics(torch.zeros(H * W, 4), ok, (W, H))
    with pytest.raises(RuntimeError, match="contiguous"):
        image_metrics(torch.zeros(3, H * W).t(), ok, (W, H))
    with pytest.raises(RuntimeError, match="at least 11"):
        image_metrics(torch.zeros(10 * W, 3), torch.zeros(10 * W, 3), (W, 10))
    with pytest.raises(RuntimeError, match="at least 11"):
        image_metrics(torch.zeros(H * 10, 3), torch.zeros(H * 10, 3), (10, H))
    with pytest.raises(RuntimeError, match="tensor"):
        image_metrics(np.zeros((H * W, 3), np.float32), ok, (W, H))
    mse = torch.tensor([1.0, 0.1, 1e-4], dtype=torch.float64)
    assert torch.allclose(psnr_from_mse(mse), torch.tensor([0.0, 10.0, 40.0], dtype=torch.float64), atol=1e-12)


# ---------------------------------------------------------------------------- the restatements
def test_reference_weights():
    g = R.weights()
    assert g.shape == (11,) and g.dtype == np.float64
    assert abs(math.fsum(g) - 1.0) <= 2.0 ** -52
    assert np.array_equal(g, g[::-1])
    assert abs(g[4] / g[5] - math.exp(-1 / 4.5)) <= 4 * 2.0 ** -53
    assert len(set(g.tolist())) == 6  # the six distinct values the kernel is handed


def test_reference_identical_images_give_exactly_one():
    for kind in R.KINDS:
        p, _ = R.image_pair(kind, 19, 23, seed=3)
        assert R.ssim64(p, p, 19, 23) == 1.0
        assert R.mse64(p, p) == 0.0


def test_reference_constant_images():
    H, W = 14, 12
    for a, b in ((0.25, 0.75), (0.9, 0.9), (0.0, 1.0), (0.5, 0.0)):
        p = np.full((H * W, 3), a, np.float32)
        t = np.full((H * W, 3), b, np.float32)
        a64, b64 = float(np.float32(a)), float(np.float32(b))
        want = (2 * a64 * b64 + R.C1) / (a64 * a64 + b64 * b64 + R.C1)
        assert abs(R.ssim64(p, t, H, W) - want) <= 1e-12
        assert abs(R.mse64(p, t) - (a64 - b64) ** 2) <= 1e-15


@pytest.mark.parametrize("H,W", [(12, 13), (43, 37), (75, 70)])
def test_restatements_agree_on_noise(H, W):
    """Pad-then-crop in fp32 against valid windows in fp64: fp32 rounding only, a few 1e-7 on noise
    (<= 3.5e-7 on these seeds); 5e-6 leaves room for another BLAS or convolution order."""
    for seed in range(3):
        p, t = R.image_pair("noise", H, W, seed)
        d = abs(R.ssim32_torchmetrics_form(p, t, H, W) - R.ssim64(p, t, H, W))
        print(f"noise {H}x{W} seed {seed}: |ssim32 - ssim64| = {d:.3g}")
        assert d <= 5e-6


def test_fp32_cancellation_is_reported_not_asserted():
    """Flat and smooth images: the fp32 form drifts from the fp64 value by E[x^2] - mu^2 cancelling
    (up to 3e-4 on one flat 11x11 view).  Printed, not bounded: it is why the kernel is fp64."""
    for kind in ("smooth", "flat"):
        for H, W in ((11, 11), (43, 37), (75, 70)):
            worst = 0.0
            for seed in range(3):
                p, t = R.image_pair(kind, H, W, seed)
                worst = max(worst, abs(R.ssim32_torchmetrics_form(p, t, H, W) - R.ssim64(p, t, H, W)))
            print(f"{kind} {H}x{W}: max |ssim32 - ssim64| over 3 seeds = {worst:.3g}")
            assert math.isfinite(worst)
