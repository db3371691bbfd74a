"""Frames per second from a camera pose to an 8-bit frame in host memory, along an orbit
(show_gui.py's render loop without its window), by two routes on the same poses:

  (a) mfnerf.viewer.FrameRenderer: pose -> one replayed graph (camera_rays, render_test_fused,
      frame_finish) -> an async copy of the uint8 frame into pinned memory, one event wait per frame;
  (b) what a caller had before it: torch get_ray_directions + get_rays per frame, render_fused with
      to_cpu / to_numpy (three float images over the bus), then numpy: (rgb * 255).astype(uint8), or
      depth2img with the same Turbo table.

Trains the field on the analytic ball scene (as tools/render_fps.py does) or loads --ckpt, then
orbits --frames poses with viewer.OrbitCamera.  Both routes run in one process, alternated round by
round after a warm-up; each round's rate is N frames over a host clock that stops when the last
frame is in host memory.  One JSON line on stdout (and --json PATH); --out DIR also writes route
(a)'s frames as PNGs (outside the timed rounds).

    python tools/orbit_frames.py [--train-steps 2000] [--width 800] [--frames 120] [--rounds 5]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mf-nerf_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-steps", type=int, default=2000)
    ap.add_argument("--ckpt", default=None, help="load this checkpoint instead of training")
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--frames", type=int, default=120, help="poses of one orbit = frames of one timed round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5, help="untimed frames per route and mode")
    ap.add_argument("--radius", type=float, default=1.5, help="orbit radius (the training views' distance)")
    ap.add_argument("--out", default=None, help="write route (a)'s frames here as PNGs")
    ap.add_argument("--json", default=None, help="also write the result line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("orbit_frames.py measures on the GPU; none is available")
    import gen_turbo_table
    from mfnerf import data
    from mfnerf.rendering import render_fused
    from mfnerf.trainer import HParams, Trainer
    from mfnerf.viewer import FrameRenderer, OrbitCamera

    dev = torch.device("cuda:0")
    W = H = args.width
    focal = 0.5 * W / math.tan(0.5 * 0.6911112)  # Lego field of view
    scene = data.BallScene.matching_grid(seed=0)
    n_views = 50 if args.ckpt is None else 2
    imgs, poses, dirs, K = data.ball_scene_views(scene, n_views, W, focal, seed=0, device=dev)
    ds = data.DeviceDataset(imgs, poses, dirs, K=K, img_wh=(W, H), device=dev, seed=1)
    del imgs
    tr = Trainer(HParams(batch_size=8192, num_epochs=1, steps_per_epoch=args.train_steps), ds, device=dev)
    if args.ckpt:
        tr.load(args.ckpt)
    else:
        tr.fit(log_every=0)
    model = tr.to_ngp()
    lut = gen_turbo_table.committed()

    cam = OrbitCamera(K, (W, H), r=args.radius)
    orbit = []
    for k in range(args.frames):  # one full turn, rising and falling by about 30 degrees (0.05 degrees per pixel)
        cam.orbit(360.0 / args.frames / 0.05,
                  30.0 * 2 * math.pi / args.frames / 0.05 * math.cos(2 * math.pi * k / args.frames))
        orbit.append(cam.pose.copy())

    kw = {"T_threshold": 1e-2, "max_samples": 100}  # render_cam's (show_gui.py:82-88)
    renderer = FrameRenderer(model, K, (W, H), **kw)

    def route_a(pose, mode):
        host, ev = renderer.to_host(renderer.render(pose, mode))
        ev.synchronize()
        return host.numpy()

    def route_b(pose, mode):
        directions = data.get_ray_directions(H, W, K, device=dev)
        o, d = data.get_rays(directions, torch.tensor(pose[:3], dtype=torch.float32, device=dev))
        res = render_fused(model, o, d, to_cpu=True, to_numpy=True, **kw)
        if mode == "rgb":
            return (res["rgb"].reshape(H, W, 3) * 255).astype(np.uint8)
        depth = res["depth"].reshape(H, W)
        depth = (depth - depth.min()) / (depth.max() - depth.min())
        return lut[(depth * 255).astype(np.uint8)]

    routes = {"frame_renderer": route_a, "host_route": route_b}
    result = {"metric": "orbit frames/s, pose -> uint8 frame in host memory", "width": W, "frames": args.frames,
              "rounds": args.rounds, "warmup": args.warmup, "radius": args.radius,
              "train_steps": None if args.ckpt else args.train_steps, "render_kwargs": kw}
    with torch.no_grad():
        for mode in ("rgb", "depth"):
            rates = {name: [] for name in routes}
            for name, fn in routes.items():
                for pose in orbit[:args.warmup]:
                    fn(pose, mode)
            # the two routes on one pose: the rays differ by fp32 rounding (one fused kernel against
            # torch's matmul), so a few bytes may differ by a quantisation step
            a, b = route_a(orbit[0], mode).astype(np.int16), route_b(orbit[0], mode).astype(np.int16)
            result[f"{mode}_bytes_differing"] = float((a != b).mean())
            result[f"{mode}_max_byte_difference"] = int(np.abs(a - b).max())
            for _ in range(args.rounds):
                for name, fn in routes.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for pose in orbit:
                        fn(pose, mode)
                    torch.cuda.synchronize()
                    rates[name].append(args.frames / (time.perf_counter() - t0))
            # route (a) without the copy out: pose -> device frame, by device events around one orbit
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for pose in orbit:
                renderer.render(pose, mode)
            e1.record()
            torch.cuda.synchronize()
            result[f"{mode}_frame_renderer_device_ms_per_frame"] = round(e0.elapsed_time(e1) / args.frames, 3)
            for name, r in rates.items():
                result[f"{mode}_{name}_fps"] = {"median": round(statistics.median(r), 2), "min": round(min(r), 2),
                                                "max": round(max(r), 2)}
            result[f"{mode}_speedup_median"] = round(statistics.median(rates["frame_renderer"])
                                                     / statistics.median(rates["host_route"]), 3)
        # the two frame kernels on their own: back-to-back calls on the last frame's buffers, by events
        # (an upper bound of each call's device time: it includes whatever gap separates the launches)
        from mfnerf import viewer
        res, (ro, rd) = renderer.results(), renderer.rays()
        pose_dev = torch.tensor(orbit[0][:3], dtype=torch.float32, device=dev).reshape(12)
        u8, f32, ws = renderer.render(orbit[0], "rgb"), renderer.frame_f32, viewer.finish_workspace(dev)
        alone = {"camera_rays": lambda: viewer.camera_rays(K, pose_dev, (W, H), rays_o=ro, rays_d=rd),
                 "frame_finish_rgb": lambda: viewer.frame_finish(res["opacity"], None, res["rgb"], "rgb", 1.0,
                                                                 frame_u8=u8, frame_f32=f32),
                 "frame_finish_depth": lambda: viewer.frame_finish(None, res["depth"], None, "depth", frame_u8=u8,
                                                                   frame_f32=f32, workspace=ws)}
        for name, fn in alone.items():
            for _ in range(20):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                fn()
            e1.record()
            torch.cuda.synchronize()
            result[f"{name}_us_per_call"] = round(e0.elapsed_time(e1) * 1e3 / 200, 2)
        renderer.render(orbit[0], "rgb")
        result["samples_per_ray"] = round(float(renderer.mean_samples()), 2)
        if args.out:
            from PIL import Image
            os.makedirs(args.out, exist_ok=True)
            for k, pose in enumerate(orbit):
                Image.fromarray(route_a(pose, "rgb").copy()).save(os.path.join(args.out, f"{k:03d}.png"))
                Image.fromarray(route_a(pose, "depth").copy()).save(os.path.join(args.out, f"{k:03d}_d.png"))
    result["data"] = "analytic 12-ball scene, Lego intrinsics (no dataset in the image)"
    line = json.dumps(result)
    print(line, flush=True)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
