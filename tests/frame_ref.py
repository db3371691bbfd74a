"""Numpy restatements of the viewer frame path (mfnerf.viewer, csrc/frame.hip), written from the
reference's text and independent of the kernels' code:

* camera_rays        datasets/ray_utils.py:8-47 + :50-70 for one view, float64
* blend, colour_u8   rendering.py:93-94 and (rgb * 255).astype(uint8) of train.py:223, fp32
* depth2img          train.py:48-53 in fp32 with the committed Turbo table (RGB order)
* OrbitCamera        show_gui.py:19-51 transcribed with scipy.spatial.transform.Rotation
"""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_tool(name):
    """tools/<name>.py loaded by path: tools/ never enters sys.path, so none of its scripts can
    shadow a module of a later test."""
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen_turbo_table = _load_tool("gen_turbo_table")

F32 = np.float32


def lut():
    """The committed (256, 3) uint8 Turbo table of csrc/turbo_table.hpp."""
    return gen_turbo_table.committed()


def _pixels(W, H):
    i = np.arange(W * H)
    return (i % W).astype(np.float64), (i // W).astype(np.float64)


def camera_rays(K4, pose, W, H):
    """float64 (rays_o, rays_d), each (W*H, 3), of the fp32 inputs K4 = (fx, fy, cx, cy), pose (3, 4)."""
    fx, fy, cx, cy = (float(F32(k)) for k in K4)
    pose = np.asarray(pose, dtype=F32).astype(np.float64)
    u, v = _pixels(W, H)
    d = np.stack([(u - cx + 0.5) / fx, (v - cy + 0.5) / fy, np.ones_like(u)], -1)
    rays_d = d @ pose[:, :3].T
    rays_o = np.broadcast_to(pose[:, 3], rays_d.shape)
    return rays_o, rays_d


def camera_rays_bound(K4, pose, W, H):
    """Per-element error bound of fp32 rays_d against camera_rays(): 8 * 2^-24 * S with
    S[i, k] = (|u - cx| + 0.5)/fx |R_k0| + (|v - cy| + 0.5)/fy |R_k1| + |R_k2| -- at most three fp32
    roundings in each direction component plus at most three in the dot product, fused or not,
    i.e. 6 * 2^-24 * S to first order, rounded up."""
    fx, fy, cx, cy = (float(F32(k)) for k in K4)
    R = np.abs(np.asarray(pose, dtype=F32).astype(np.float64)[:, :3])
    u, v = _pixels(W, H)
    a = (np.abs(u - cx) + 0.5) / abs(fx)
    b = (np.abs(v - cy) + 0.5) / abs(fy)
    S = a[:, None] * R[None, :, 0] + b[:, None] * R[None, :, 1] + R[None, :, 2]
    return 8.0 * 2.0 ** -24 * S


def blend(opacity, rgb, bg):
    """rendering.py:93-94 in fp32: rgb + bg * (1 - opacity)."""
    opacity, rgb = np.asarray(opacity, F32), np.asarray(rgb, F32)
    with np.errstate(invalid="ignore"):
        return (rgb + F32(bg) * (F32(1) - opacity)[:, None]).astype(F32)


def colour_u8(c):
    """(c * 255).astype(uint8), train.py:223, where that cast is defined (the fp32 product in
    [0, 256): truncation); a product below 0 gives 0, one of 256 or more 255, NaN 0."""
    with np.errstate(invalid="ignore"):
        p = (np.asarray(c, F32) * F32(255)).astype(F32)
        inside = (p >= 0) & (p < 256)
        out = np.zeros(p.shape, np.uint8)
        out[inside] = p[inside].astype(np.uint8)
        out[p >= 256] = 255
    return out


def depth2img(depth, table=None):
    """train.py:48-53 in fp32, Turbo in RGB order: (n, 3) uint8.  A constant image (the reference
    divides 0 by 0) maps to entry 0."""
    table = lut() if table is None else table
    depth = np.asarray(depth, F32)
    mn, mx = depth.min(), depth.max()
    if mx == mn:
        k = np.zeros(depth.shape, np.uint8)
    else:
        x = ((depth - mn) / (mx - mn)).astype(F32)
        k = (x * F32(255)).astype(F32).astype(np.uint8)
    return table[k]


def depth_f32(frame_u8):
    """show_gui.py:99: depth2img(depth).astype(np.float32) / 255.0."""
    return (frame_u8.astype(F32) / F32(255.0)).astype(F32)


class OrbitCamera:
    """show_gui.py:19-51, transcribed (scipy's Rotation as there)."""

    def __init__(self, K, img_wh, r):
        self.K = K
        self.W, self.H = img_wh
        self.radius = r
        self.center = np.zeros(3)
        self.rot = np.eye(3)

    @property
    def pose(self):
        res = np.eye(4)
        res[2, 3] -= self.radius
        rot = np.eye(4)
        rot[:3, :3] = self.rot
        res = rot @ res
        res[:3, 3] -= self.center
        return res

    def orbit(self, dx, dy):
        from scipy.spatial.transform import Rotation as R
        rotvec_x = self.rot[:, 1] * np.radians(0.05 * dx)
        rotvec_y = self.rot[:, 0] * np.radians(-0.05 * dy)
        self.rot = R.from_rotvec(rotvec_y).as_matrix() @ R.from_rotvec(rotvec_x).as_matrix() @ self.rot

    def scale(self, delta):
        self.radius *= 1.1 ** (-delta)

    def pan(self, dx, dy, dz=0):
        self.center += 1e-4 * self.rot @ np.array([dx, dy, dz])
