"""Test-time rendering speed of the drop-in path (the reference's README.md:123
quotes 36.20 FPS for Lego 800x800 on an RTX 2080 Ti).

Trains the field on the analytic ball scene (mfnerf.data, Lego intrinsics) for --train-steps
steps with the fused trainer, then times mfnerf.rendering.render(test_time=True) -- the reference's
progressive test-time loop (rendering.py:46-118) over raymarching_test / composite_test_fw -- on
full 800x800 held-out views, and reports frames/s and PSNR.  One JSON line on stdout.

    python tools/render_fps.py [--train-steps 2000] [--views 5] [--fused]

--fused also times mfnerf.rendering.render_fused (the single-launch kernel) on the same frames and
adds its figures (fused_*) to the line, then times mfnerf.metrics.image_metrics alone on those frames
(device events, warmed up, --metric-calls calls: metrics_*) and Trainer.validate against
Trainer.evaluate(fused=True) per view (validate_* / evaluate_*).  SSIM (test/ssim, train.py:198-237)
is reported beside every PSNR.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mf-nerf_amd")]

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-steps", type=int, default=2000)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--fused", action="store_true", help="also time render_fused on the same frames")
    ap.add_argument("--metric-calls", type=int, default=200, help="timed image_metrics calls (--fused)")
    args = ap.parse_args()
    from mfnerf import data, synthetic
    from mfnerf.metrics import image_metrics, workspace_bytes
    from mfnerf.rendering import render, render_fused
    from mfnerf.trainer import HParams, Trainer

    dev = torch.device("cuda:0")
    W = args.width
    focal = 0.5 * W / math.tan(0.5 * 0.6911112)  # Lego field of view
    scene = data.BallScene.matching_grid(seed=0)
    imgs, poses, dirs, K = data.ball_scene_views(scene, 50, W, focal, seed=0, device=dev)
    ds = data.DeviceDataset(imgs, poses, dirs, K=K, img_wh=(W, W), device=dev, seed=1)
    del imgs
    hp = HParams(batch_size=8192, num_epochs=1, steps_per_epoch=args.train_steps)
    tr = Trainer(hp, ds, device=dev)
    t0 = time.time()
    tr.fit(log_every=0)
    torch.cuda.synchronize()
    train_s = time.time() - t0
    model = tr.to_ngp()
    t_imgs, t_poses, _, _ = data.ball_scene_views(scene, args.views, W, focal, seed=11, device=dev)
    dd = dirs.to(dev)
    times, psnrs, samples = [], [], []
    f_times, f_psnrs, f_samples = [], [], []
    ssims, f_ssims, f_frames = [], [], []
    m_out = torch.empty(2, dtype=torch.float64, device=dev)
    m_ws = torch.empty(workspace_bytes(W, W), dtype=torch.uint8, device=dev)
    with torch.no_grad():
        for i, (img, pose) in enumerate(zip(t_imgs, t_poses)):
            o, d = data.get_rays(dd, pose.to(dev))
            torch.cuda.synchronize()
            t = time.time()
            res = render(model, o, d, test_time=True)
            torch.cuda.synchronize()
            if i > 0 or args.views == 1:  # the first frame warms up allocations
                times.append(time.time() - t)
            psnrs.append(float(-10 * torch.log10(((res["rgb"].float() - img) ** 2).mean())))
            ssims.append(float(image_metrics(res["rgb"].float().contiguous(), img, (W, W), m_out, m_ws)[1]))
            samples.append(int(res["total_samples"]))
            if args.fused:
                torch.cuda.synchronize()
                t = time.time()
                res = render_fused(model, o, d)
                torch.cuda.synchronize()
                if i > 0 or args.views == 1:
                    f_times.append(time.time() - t)
                f_psnrs.append(float(-10 * torch.log10(((res["rgb"].float() - img) ** 2).mean())))
                f_frames.append(res["rgb"].float().contiguous())
                f_ssims.append(float(image_metrics(f_frames[-1], img, (W, W), m_out, m_ws)[1]))
                f_samples.append(int(res["total_samples"]))
    fps = len(times) / sum(times)
    fused = {}
    if args.fused:
        f_fps = len(f_times) / sum(f_times)
        fused = {"fused_fps": round(f_fps, 2), "fused_ms_per_frame": round(1e3 / f_fps, 2),
                 "fused_psnr": round(sum(f_psnrs) / len(f_psnrs), 2),
                 "fused_ssim": round(sum(f_ssims) / len(f_ssims), 4),
                 "fused_samples_per_ray": round(sum(f_samples) / len(f_samples) / (W * W), 2)}
        # image_metrics alone on the rendered frames: device events around the whole timed run
        calls = max(args.metric_calls, 1)
        for k in range(20):
            image_metrics(f_frames[k % len(f_frames)], t_imgs[k % len(f_frames)], (W, W), m_out, m_ws)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(calls):
            image_metrics(f_frames[k % len(f_frames)], t_imgs[k % len(f_frames)], (W, W), m_out, m_ws)
        e1.record()
        torch.cuda.synchronize()
        m_us = e0.elapsed_time(e1) * 1e3 / calls
        # the same calls replayed from one captured graph: the device time without the host's launch gaps
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for k in range(calls):
                image_metrics(f_frames[k % len(f_frames)], t_imgs[k % len(f_frames)], (W, W), m_out, m_ws)
        g.replay()
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        fused["metrics_us_per_call_graph"] = round(e0.elapsed_time(e1) * 1e3 / calls, 2)
        fused.update({"metrics_us_per_call": round(m_us, 2), "metrics_calls": calls,
                      "metrics_share_of_fused_frame": round(m_us * 1e-3 / (1e3 / f_fps), 5)})
        # the validation loop (one read at the end) against evaluate (one read per view), per view:
        # alternated, the fastest of three runs each (both include one to_ngp())
        loops = {"evaluate": lambda: tr.evaluate(t_imgs, t_poses, dirs, fused=True),
                 "validate": lambda: tr.validate(t_imgs, t_poses, dirs, fused=True)}
        best = {}
        for rep in range(4):  # the first round warms up
            for name, fn in loops.items():
                torch.cuda.synchronize()
                t = time.time()
                fn()
                torch.cuda.synchronize()
                if rep:
                    best[name] = min(best.get(name, float("inf")), time.time() - t)
        for name, v in best.items():
            fused[name + "_ms_per_view"] = round(v * 1e3 / args.views, 3)
    print(json.dumps({"metric": "test-time render frames/s (800x800)", "fps": round(fps, 2),
                      "ms_per_frame": round(1e3 / fps, 2), "psnr": round(sum(psnrs) / len(psnrs), 2),
                      "ssim": round(sum(ssims) / len(ssims), 4),
                      "samples_per_ray": round(sum(samples) / len(samples) / (W * W), 2), **fused,
                      "train_steps": args.train_steps, "train_s": round(train_s, 2), "views": args.views,
                      "reference": "36.20 FPS, RTX 2080 Ti, Lego (README.md:123)",
                      "data": "analytic 12-ball scene, Lego intrinsics (no dataset in the image)"}), flush=True)


if __name__ == "__main__":
    main()
