"""Host side of the viewer frame path (mfnerf.viewer, csrc/frame.hip): the orbit camera against the
scipy transcription of show_gui.py, the committed Turbo table against its generator, the C ABI
declarations against the ctypes signatures and the built library, and the HDR guard.  No GPU compute."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import frame_ref

NEW = {"mfnerf_camera_rays": (ctypes.c_int, 7), "mfnerf_frame_finish_workspace": (ctypes.c_int64, 0),
       "mfnerf_frame_finish": (ctypes.c_int, 10)}


class HP:  # the small hash-grid configuration of test_tonemap_cpu.py
    grid, L, F, T, N_min, N_max, N_tables, rgb_channels, rgb_layers = "Hash", 16, 2, 12, 4, 256, 1, 64, 2


def _script(seed=0, steps=300):
    """A scripted mouse session: drags of a few to a few hundred pixels, wheel clicks, pans."""
    g = np.random.default_rng(seed)
    for k in range(steps):
        kind = k % 5
        if kind in (0, 1, 3):
            yield "orbit", tuple(g.uniform(-300, 300, 2))
        elif kind == 2:
            yield "scale", (float(g.integers(-3, 4)),)
        else:
            yield "pan", tuple(g.uniform(-500, 500, 3 if k % 2 else 2))
    yield "orbit", (0.0, 0.0)  # a zero drag: the zero rotation vector


def test_orbit_camera_matches_the_scipy_transcription():
    """Both sides float64; Rodrigues' formula and scipy's quaternion route differ by rounding only, a
    few 2^-53 per call, carried through ~180 chained rotations: far below 1e-12."""
    pytest.importorskip("scipy")
    from mfnerf.viewer import OrbitCamera
    K = np.array([[1111.1, 0, 400.0], [0, 1111.1, 400.0], [0, 0, 1]])
    got, ref = OrbitCamera(K, (800, 600), r=2.5), frame_ref.OrbitCamera(K, (800, 600), r=2.5)
    assert (got.W, got.H, got.radius) == (800, 600, 2.5)
    assert np.array_equal(got.pose, ref.pose)
    worst = 0.0
    for name, args in _script():
        getattr(got, name)(*args)
        getattr(ref, name)(*args)
        assert got.pose.shape == (4, 4) and got.pose.dtype == np.float64
        worst = max(worst, float(np.abs(got.pose - ref.pose).max()))
    print("orbit camera: max |pose - scipy transcription| =", worst)
    assert worst <= 1e-12
    assert np.abs(got.rot @ got.rot.T - np.eye(3)).max() <= 1e-12  # still a rotation
    assert abs(got.radius - ref.radius) <= 1e-12 and got.radius != 2.5


def test_committed_turbo_table_is_the_generators():
    pytest.importorskip("matplotlib")
    gen = frame_ref.gen_turbo_table
    with open(gen.HEADER) as f:
        text = f.read()
    assert text == gen.render(), "csrc/turbo_table.hpp is stale: run tools/gen_turbo_table.py"
    t = gen.parse(text)
    assert t.shape == (256, 3) and t.dtype == np.uint8 and np.array_equal(t, gen.table())
    # Turbo's published end points: dark blue (48, 18, 59) to dark red (122, 4, 3)
    assert tuple(t[0]) == (48, 18, 59) and tuple(t[255]) == (122, 4, 3)


def _declared(name):
    src = open(os.path.join(ROOT, "include", "mfnerf.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"^\s*(int|int64_t)\s+" + name + r"\s*\((.*?)\)\s*;", src, re.M | re.S)
    assert m, f"{name} is not declared in include/mfnerf.h"
    args = [a.strip() for a in m.group(2).split(",")]
    return m.group(1), [] if args == ["void"] else args


def test_header_signatures_and_library_agree():
    from mfnerf import _lib
    assert os.path.exists(_lib.LIB_PATH), "build libmfnerf_hip.so first (__graft_entry__.build())"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, (res, n_args) in NEW.items():
        ret, args = _declared(name)
        assert hasattr(lib, name), f"{name} is not exported"
        got_res, argtypes = _lib.SIGNATURES[name]
        assert got_res is res and (ret == "int64_t") == (res is ctypes.c_int64)
        assert len(args) == len(argtypes) == n_args
        for decl, ty in zip(args, argtypes):
            assert ("*" in decl or "mfnerf_stream_t" in decl) == (ty is ctypes.c_void_p), decl
    scalars = {d.split()[-1]: t for d, t in zip(_declared("mfnerf_frame_finish")[1],
                                                _lib.SIGNATURES["mfnerf_frame_finish"][1]) if "*" not in d
               and "mfnerf_stream_t" not in d}
    assert scalars == {"n": ctypes.c_int64, "mode": ctypes.c_int, "bg": ctypes.c_float}
    assert _lib.load().mfnerf_frame_finish_workspace() > 0


def test_frame_renderer_names_the_hdr_gap():
    """The guard comes before any allocation: a CPU model is enough to reach it."""
    from mfnerf.networks import NGP
    from mfnerf.viewer import FrameRenderer
    K = np.array([[50.0, 0, 16], [0, 50.0, 16], [0, 0, 1]])
    with pytest.raises(NotImplementedError, match="HDR/exposure"):
        FrameRenderer(NGP(0.5, HP, rgb_act="None"), K, (32, 32))


def test_numpy_restatements_on_hand_values():
    """frame_ref itself, on values worked by hand (the GPU tests compare against it)."""
    f = np.float32
    c = np.array([0.0, 1.0, np.nextafter(f(1), f(2)), 0.5, -0.25, np.nan, 2.0, 254.5 / 255], f)
    assert frame_ref.colour_u8(c).tolist() == [0, 255, 255, 127, 0, 0, 255, 254]
    assert frame_ref.blend([0.0, 1.0, 0.25], np.full((3, 3), 0.5, f), 1.0)[:, 0].tolist() == [1.5, 0.5, 1.25]
    table = np.arange(768, dtype=np.int64).reshape(256, 3).astype(np.uint8)
    img = frame_ref.depth2img(np.array([2.0, 4.0, 3.0, 2.0], f), table)
    assert img[:, 0].tolist() == [table[0, 0], table[255, 0], table[127, 0], table[0, 0]]
    assert np.array_equal(frame_ref.depth2img(np.full(5, 3.0, f), table), np.tile(table[0], (5, 1)))
    o, d = frame_ref.camera_rays((2.0, 4.0, 1.0, 1.0), np.hstack([np.eye(3), [[1], [2], [3]]]), 2, 2)
    assert d.tolist() == [[-0.25, -0.125, 1], [0.25, -0.125, 1], [-0.25, 0.125, 1], [0.25, 0.125, 1]]
    assert o.tolist() == [[1, 2, 3]] * 4
