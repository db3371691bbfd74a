"""The frame path of show_gui.py without its window: an orbit camera (show_gui.py:19-51) and a
renderer that turns its pose into an 8-bit colour or depth frame (render_cam, show_gui.py:72-99, and
the save branch of train.py:220-226) in one captured graph of three calls,

    mfnerf_camera_rays -> mfnerf_render_test_fused -> mfnerf_frame_finish

with every buffer allocated once and no wait for a render on the host (render()'s docstring has the
one bounded wait): the only per-frame traffic is the 48 pose bytes in and, if the caller asks
(to_host), the frame out.  The dearpygui window itself is not
here.
"""
import ctypes

import numpy as np
import torch

from .rendering import HDR_GAP, MAX_SAMPLES

MODES = {"rgb": 0, "depth": 1}
_POSE_SLOTS = 4  # pinned staging poses in flight before render() waits for the oldest copy


def _rotvec_matrix(rotvec):
    """scipy's Rotation.from_rotvec(rotvec).as_matrix(): Rodrigues' formula,
    R = I + sin(t) K + (1 - cos(t)) K^2 for the unit axis' cross-product matrix K."""
    rotvec = np.asarray(rotvec, dtype=np.float64)
    theta = float(np.linalg.norm(rotvec))
    if theta == 0.0:
        return np.eye(3)
    x, y, z = rotvec / theta
    K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return np.eye(3) + np.sin(theta) * K + (1.0 - np.cos(theta)) * (K @ K)


class OrbitCamera:
    """show_gui.py:19-51, same constants and multiplication order; the rotation vectors go through
    Rodrigues' formula in numpy instead of scipy."""

    def __init__(self, K, img_wh, r):
        self.K = K
        self.W, self.H = img_wh
        self.radius = r
        self.center = np.zeros(3)
        self.rot = np.eye(3)

    @property
    def pose(self):
        """(4, 4) float64 camera-to-world: back by the radius, rotate, translate."""
        res = np.eye(4)
        res[2, 3] -= self.radius
        rot = np.eye(4)
        rot[:3, :3] = self.rot
        res = rot @ res
        res[:3, 3] -= self.center
        return res

    def orbit(self, dx, dy):
        rotvec_x = self.rot[:, 1] * np.radians(0.05 * dx)
        rotvec_y = self.rot[:, 0] * np.radians(-0.05 * dy)
        self.rot = _rotvec_matrix(rotvec_y) @ _rotvec_matrix(rotvec_x) @ self.rot

    def scale(self, delta):
        self.radius *= 1.1 ** (-delta)

    def pan(self, dx, dy, dz=0):
        self.center += 1e-4 * self.rot @ np.array([dx, dy, dz])


def _k4(K):
    """(fx, fy, cx, cy) of a (3, 3) intrinsic matrix as the four host floats the C ABI takes."""
    K = K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else np.asarray(K)
    if K.shape != (3, 3):
        raise ValueError(f"K must be a (3, 3) intrinsic matrix, got {K.shape}")
    return (ctypes.c_float * 4)(float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))


def camera_rays(K, pose, img_wh, rays_o=None, rays_d=None):
    """mfnerf_camera_rays: one whole view's (rays_o, rays_d), each (W*H, 3) f32 -- get_ray_directions
    + get_rays (ray_utils.py:8-47, :50-70) in one launch.  pose: a DEVICE f32 tensor whose first
    twelve values are the row-major (3, 4) camera-to-world matrix (the kernel reads it, so a captured
    call follows the buffer's content); K (3, 3); img_wh = (W, H)."""
    from ._lib import call, check_input, ptr, stream
    W, H = int(img_wh[0]), int(img_wh[1])
    check_input("pose", pose, torch.float32)
    if pose.numel() < 12:
        raise RuntimeError("pose must hold the (3, 4) camera-to-world matrix")
    n = max(W * H, 0)
    rays_o = torch.empty(n, 3, device=pose.device) if rays_o is None else rays_o
    rays_d = torch.empty(n, 3, device=pose.device) if rays_d is None else rays_d
    for name, t in (("rays_o", rays_o), ("rays_d", rays_d)):
        check_input(name, t, torch.float32)
        if t.numel() != 3 * n:
            raise RuntimeError(f"{name} must be (W*H, 3)")
    call("mfnerf_camera_rays", _k4(K), ptr(pose), W, H, ptr(rays_o), ptr(rays_d), stream())
    return rays_o, rays_d


def finish_workspace(device):
    """The (uninitialised) workspace mfnerf_frame_finish takes."""
    from ._lib import load
    return torch.empty(int(load().mfnerf_frame_finish_workspace()), dtype=torch.uint8, device=device)


def frame_finish(opacity, depth, rgb, mode="rgb", bg=0.0, frame_u8=None, frame_f32=None, workspace=None,
                 want_f32=False):
    """mfnerf_frame_finish: the renderer's per-pixel sums to an (n, 3) uint8 frame (and, with
    want_f32 or a frame_f32 buffer, its float texture); returns (frame_u8, frame_f32 or None).
    mode "rgb": the blend rgb + bg * (1 - opacity) of rendering.py:93-94 and (c * 255).astype(uint8)
    (train.py:223) -- rgb is the UNBLENDED sum with bg = 1 or 0 as render() chooses, or an already
    blended image with bg = 0.  mode "depth": depth2img (train.py:48-53) with RGB Turbo."""
    from ._lib import call, check_input, ptr, stream
    if mode not in MODES:
        raise ValueError(f"unknown frame mode {mode!r} (one of {sorted(MODES)})")
    need = (("opacity", opacity), ("rgb", rgb)) if mode == "rgb" else (("depth", depth),)
    for name, t in need:
        check_input(name, t, torch.float32)
    lead = need[0][1]
    n, dev = lead.shape[0], lead.device
    if mode == "rgb" and (opacity.numel() != n or rgb.numel() != 3 * n):
        raise RuntimeError("opacity must be (n) and rgb (n, 3)")
    if mode == "depth" and depth.numel() != n:
        raise RuntimeError("depth must be (n)")
    if frame_u8 is None:
        frame_u8 = torch.empty(n, 3, dtype=torch.uint8, device=dev)
    if frame_f32 is None and want_f32:
        frame_f32 = torch.empty(n, 3, device=dev)
    check_input("frame_u8", frame_u8, torch.uint8)
    if frame_u8.numel() != 3 * n:
        raise RuntimeError("frame_u8 must be (n, 3)")
    if frame_f32 is not None:
        check_input("frame_f32", frame_f32, torch.float32)
        if frame_f32.numel() != 3 * n:
            raise RuntimeError("frame_f32 must be (n, 3)")
    if mode == "depth" and workspace is None:
        workspace = finish_workspace(dev)
    call("mfnerf_frame_finish", ptr(opacity if mode == "rgb" else None), ptr(depth if mode == "depth" else None),
         ptr(rgb if mode == "rgb" else None), int(n), MODES[mode], float(bg), ptr(workspace), ptr(frame_u8),
         ptr(frame_f32), stream())
    return frame_u8, frame_f32


class FrameRenderer:
    """render_cam (show_gui.py:72-99) for one model and one image size, every buffer preallocated:
    the device pose, the view's rays, the renderer's outputs and queue, the finish workspace, the
    uint8 and float frames and pinned host staging.  render(pose) copies the 3x4 pose to the device
    and replays ONE single-stream graph of camera_rays -> mfnerf_render_test_fused -> frame_finish
    (a linear chain; one graph per mode, captured on first use with torch.cuda.graph).  The defaults
    are render_cam's (show_gui.py:82-88).  As in render_fused, max_samples is a PER-RAY budget of
    evaluated samples, not the loop's cap on the sum of its rounds' chunk sizes.

    The field weights come from field.field_weights(...), and the graphs are captured again when the
    parameters' version counters change -- the rule field_weights caches by -- so a frame after an
    in-place parameter update shows the new weights.

    The tensors render(), frame_f32, rays() and results() return are the renderer's own buffers: the
    next render() overwrites them (in stream order)."""

    def __init__(self, model, K, img_wh, exp_step_factor=0.0, T_threshold=1e-2, max_samples=100, device=None):
        if getattr(model, "rgb_act", "Sigmoid") != "Sigmoid":
            raise NotImplementedError(HDR_GAP)
        W, H = int(img_wh[0]), int(img_wh[1])
        if W <= 0 or H <= 0:
            raise ValueError(f"img_wh must be positive, got {tuple(img_wh)}")
        self.model = model
        self.W, self.H = W, H
        self.K = K
        self._k4 = _k4(K)
        self.exp_step_factor = float(exp_step_factor)
        self.T_threshold = float(T_threshold)
        self.max_samples = int(max_samples)
        self.bg = 1.0 if self.exp_step_factor == 0 else 0.0  # rendering.py:93
        dev = self.device = torch.device(device) if device is not None else model.center.device
        if dev.type != "cuda":
            raise RuntimeError("FrameRenderer renders on the GPU; the model and device must be CUDA")
        n = self.n = W * H
        self._pose = torch.zeros(12, device=dev)
        self._pose_host = torch.zeros(_POSE_SLOTS, 12).pin_memory()
        self._pose_events = [torch.cuda.Event() for _ in range(_POSE_SLOTS)]
        self._pose_slot = 0
        self._rays_o = torch.empty(n, 3, device=dev)
        self._rays_d = torch.empty(n, 3, device=dev)
        self._opacity = torch.empty(n, device=dev)
        self._depth = torch.empty(n, device=dev)
        self._rgb = torch.empty(n, 3, device=dev)
        self._samples = torch.empty(n, dtype=torch.int32, device=dev)
        self._total = torch.zeros((), dtype=torch.int64, device=dev)
        self._queue = torch.empty(1, dtype=torch.int32, device=dev)
        self._ws = finish_workspace(dev)
        self._frame_u8 = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
        self._frame_f32 = torch.empty(H, W, 3, device=dev)
        self._host = {}     # dtype -> (pinned (H, W, 3) buffer, event)
        self._graphs = {}   # mode -> captured graph
        self._weights = None
        self._version = None

    # -- the three calls -------------------------------------------------------------------------
    def _refresh_weights(self):
        """The packed weights of the parameters as they are now; drops the graphs that baked older ones."""
        from . import field
        m = self.model
        ver = (m.xyz_encoder.params._version, m.rgb_net.params._version)
        if ver != self._version:
            self._weights = field.field_weights(m.xyz_encoder.params, m.rgb_net.params, m.rgb_width)
            self._version = ver
            self._graphs.clear()

    def _launch(self, mode):
        from ._lib import call, ptr, stream
        m = self.model
        packed, table16 = self._weights
        call("mfnerf_camera_rays", self._k4, ptr(self._pose), self.W, self.H, ptr(self._rays_o), ptr(self._rays_d),
             stream())
        call("mfnerf_render_test_fused", ptr(self._rays_o), ptr(self._rays_d), self.n, ptr(m.center),
             ptr(m.half_size), ptr(m.density_bitfield), int(m.cascades), float(m.scale), self.exp_step_factor,
             int(m.grid_size), MAX_SAMPLES, self.max_samples, self.T_threshold, float(m._x_min), float(m._x_range),
             m.desc, ptr(table16), ptr(packed), int(m.rgb_width), ptr(self._queue), ptr(self._opacity),
             ptr(self._depth), ptr(self._rgb), ptr(self._samples), ptr(self._total), stream())
        call("mfnerf_frame_finish", ptr(self._opacity), ptr(self._depth), ptr(self._rgb), self.n, MODES[mode],
             self.bg, ptr(self._ws), ptr(self._frame_u8), ptr(self._frame_f32), stream())

    def _set_pose(self, pose):
        """The 3x4 pose into the device buffer, through a pinned slot when it comes from the host."""
        if isinstance(pose, torch.Tensor) and pose.is_cuda:
            if pose.dim() != 2 or pose.shape[0] < 3 or pose.shape[1] != 4:
                raise ValueError(f"pose must be (3, 4) or (4, 4), got {tuple(pose.shape)}")
            self._pose.copy_(pose[:3].reshape(12))
            return
        p = np.asarray(pose.detach().cpu() if isinstance(pose, torch.Tensor) else pose, dtype=np.float32)
        if p.ndim != 2 or p.shape[0] < 3 or p.shape[1] != 4:
            raise ValueError(f"pose must be (3, 4) or (4, 4), got {p.shape}")
        k = self._pose_slot
        self._pose_slot = (k + 1) % _POSE_SLOTS
        self._pose_events[k].synchronize()  # the copy that last read this slot, _POSE_SLOTS frames ago
        self._pose_host[k].copy_(torch.from_numpy(np.ascontiguousarray(p[:3]).reshape(12)))
        self._pose.copy_(self._pose_host[k], non_blocking=True)
        self._pose_events[k].record()

    @torch.no_grad()
    def render(self, pose, mode="rgb", eager=False):
        """pose (3, 4) or (4, 4), numpy or tensor -> the (H, W, 3) uint8 device frame of `mode`
        ("rgb" or "depth"); frame_f32 holds its float texture.  Does not wait for the frame, nor
        for any render: the one wait a host pose can cause is for the 48-byte copy out of its pinned
        staging slot as used _POSE_SLOTS (4) frames earlier, so the host runs at most that many
        frames ahead of the device; a device pose waits for nothing.  eager=True issues the same
        three calls without a graph."""
        if mode not in MODES:
            raise ValueError(f"unknown frame mode {mode!r} (one of {sorted(MODES)})")
        with torch.cuda.device(self.device):
            self._refresh_weights()
            self._set_pose(pose)
            if eager:
                self._launch(mode)
                return self._frame_u8
            g = self._graphs.get(mode)
            if g is None:
                self._launch(mode)  # once outside capture: whatever a first launch loads is loaded
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._launch(mode)
                self._graphs[mode] = g
            g.replay()
        return self._frame_u8

    # -- the last frame ------------------------------------------------------------------------------
    @property
    def frame_f32(self):
        """(H, W, 3) f32: the blended colour ("rgb", the GUI's mvFormat_Float_rgb texture) or
        frame_u8 / 255 ("depth", show_gui.py:99) of the last frame."""
        return self._frame_f32

    def rays(self):
        """The last frame's (rays_o, rays_d), each (W*H, 3)."""
        return self._rays_o, self._rays_d

    def results(self):
        """The last frame's renderer outputs: opacity, depth, rgb BEFORE the background blend, the
        per-ray samples and their total (render_fused's keys)."""
        return {"opacity": self._opacity, "depth": self._depth, "rgb": self._rgb, "samples": self._samples,
                "total_samples": self._total}

    def mean_samples(self):
        """The GUI's "Samples/ray" (show_gui.py:94): total_samples / (W*H), a 0-d device tensor."""
        return self._total / self.n

    def to_host(self, frame):
        """An asynchronous copy of an (H, W, 3) frame into a pinned host buffer (one per dtype, reused
        by the next call): returns (host tensor, event); the tensor is valid once event.synchronize()
        returns."""
        hit = self._host.get(frame.dtype)
        if hit is None:
            hit = self._host[frame.dtype] = (torch.empty(self.H, self.W, 3, dtype=frame.dtype).pin_memory(),
                                             torch.cuda.Event())
        buf, ev = hit
        with torch.cuda.device(self.device):
            buf.copy_(frame.reshape(self.H, self.W, 3), non_blocking=True)
            ev.record()
        return buf, ev
