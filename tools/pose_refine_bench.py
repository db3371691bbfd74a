"""Measurements of pose refinement inside the fused step (StepConfig.refine_poses), one process, one
GPU; writes one JSON document.

    python tools/pose_refine_bench.py --out profiles/r09_pose_refine.json [--e2e] [--bench-lines DIR]

* the captured, replayed ray_grads step with refine_poses off and on, on bench.py's dataset (100
  analytic 800x800 views, 8192 rays, Lego config), the two alternated in blocks; ms per step by a host
  clock around synchronised blocks;
* mfnerf_pose_grad and mfnerf_pose_step alone on that step's buffers (device events around REPS
  launches, median / min over ROUNDS);
* --e2e: the end-to-end protocol of tests/test_gpu_pose_refine.py on both routes -- the eager one
  (PoseRefiner.optimizer(lr) + render(), frozen field) and the fused one (Trainer(optimize_ext)) -- and
  the ratio |dT[7] + offset| / |offset| each reaches;
* --bench-lines DIR: bench.py result lines saved as DIR/this_*.json and DIR/parent_*.json by a
  same-session run of this tree and of the parent commit, copied into the document.
"""
import argparse
import glob
import json
import math
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mf-nerf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from mfnerf import data, engine, synthetic  # noqa: E402
from mfnerf._lib import call, ptr, stream  # noqa: E402

ROUNDS, REPS = 15, 10


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / REPS  # us per call


def compare(variants):
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            t[k].append(timed(fn))
    return {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2)} for k, v in t.items()}


def bench_views(dev):
    scene = data.BallScene.matching_grid(seed=0)
    return data.ball_scene_views(scene, 100, synthetic.LEGO_W, synthetic.LEGO_F, seed=100, device=dev)


def make_step(dev, views, refine):
    imgs, poses, dirs, K = views
    st = engine.TrainStep(engine.StepConfig(ray_grads=True, refine_poses=refine), device=dev, seed=0)
    st.set_occupancy(synthetic.ball_density_grid())
    # the images are shared (already resident: DeviceDataset keeps the tensor it is given)
    st.attach_dataset(data.DeviceDataset(imgs, poses, dirs, K=K, img_wh=(synthetic.LEGO_W, synthetic.LEGO_H),
                                         device=dev, seed=7))
    for _ in range(6):
        st.run()
    torch.cuda.synchronize()
    return st


def step_timings(dev, views, out, steps=200):
    runs = {}
    for name, on in (("refine_poses_off", False), ("refine_poses_on", True)):
        st = make_step(dev, views, on)
        st.capture()
        st.replay()
        runs[name] = st
    t = {k: [] for k in runs}
    for _ in range(7):
        for name, st in runs.items():
            for _k in range(20):
                st.replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _k in range(steps):
                st.replay()
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) * 1e3 / steps)
    out["step_ms"] = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                          "max_ms": round(max(v), 4)} for k, v in t.items()}
    out["gate_timeouts"] = {k: st.gate_timeouts() for k, st in runs.items()}
    out["skipped_steps"] = {k: st.skipped_steps() for k, st in runs.items()}
    return runs["refine_poses_on"]


def kernel_timings(st, out):
    ds, t, mb, s = st.dataset, st.parts[0], st.state.march, stream()
    scratch = torch.empty_like(ds.poses)
    grads = torch.zeros_like(st.pose_grad)
    out["n_img"], out["rays"] = ds.n_img, st.cfg.n_rays
    # the update runs on copies: the step's own state is left as it is
    dR, dT, m, v, k = (x.clone() for x in (st.dR, st.dT, st.pose_m, st.pose_v, st.pose_step_dev))

    def pose_grad():
        call("mfnerf_pose_grad", ptr(t.dL_drays_o), ptr(t.dL_drays_d), ptr(mb.img_idx), ptr(mb.pix_idx), ptr(ds.poses),
             ptr(ds.directions), ptr(st.dR), st.cfg.n_rays, ds.n_img, ds.hw, ptr(grads[0]), ptr(grads[1]), None, s)

    def pose_step():
        call("mfnerf_pose_step", ptr(dR), ptr(dT), ptr(m), ptr(v), ptr(grads[0]), ptr(grads[1]), ptr(ds.poses),
             ds.n_img, 1e-6, 0.9, 0.999, 1e-8, ptr(k), None, None, ptr(scratch), s)

    out["kernels"] = compare({"pose_grad": pose_grad, "pose_step": pose_step})


# ---------------------------------------------------------------------------- end to end
def e2e(dev, out, steps, lr):
    from mfnerf.pose import PoseRefiner
    from mfnerf.rendering import render
    from mfnerf.trainer import HParams, Trainer
    W = 32
    focal = 0.5 * W / math.tan(0.5 * 0.6911112)
    imgs, poses, dirs, K = data.ball_scene_views(data.BallScene(n_balls=6, seed=1), 40, W, focal, seed=0)
    ds = data.DeviceDataset(imgs, poses, dirs, K=K, img_wh=(W, W), device=dev, seed=5)
    hp = HParams(batch_size=1024, T=14, num_epochs=1, steps_per_epoch=400)
    tr = Trainer(hp, ds, device=dev)
    tr.fit(log_every=0)
    ck = os.path.join(tempfile.mkdtemp(), "field.ckpt")
    tr.save(ck)
    offset = torch.tensor([0.03, -0.02, 0.025])
    moved = poses.clone()
    moved[7, :3, 3] += offset
    res = {"steps": steps, "pose_lr": lr, "offset": offset.tolist(), "image": 7, "rays_per_step": 1024}

    # the eager route: the trained field frozen, rays of random images / pixels from the refined poses
    model = tr.to_ngp()  # its parameters collect gradients nobody applies
    refiner = PoseRefiner(len(poses)).to(dev)
    opt = refiner.optimizer(lr)
    g = torch.Generator(device=dev).manual_seed(6)
    pg, dd, im = moved.float().to(dev), dirs.to(dev), imgs.to(dev)
    torch.manual_seed(0)
    t0 = time.perf_counter()
    for _ in range(steps):
        idx = torch.randint(0, len(poses), (1024,), generator=g, device=dev)
        pix = torch.randint(0, W * W, (1024,), generator=g, device=dev)
        rays_o, rays_d = data.get_rays(dd[pix], refiner(pg[idx], idx))
        r = render(model, rays_o, rays_d)
        o = r["opacity"] + 1e-10
        loss = ((r["rgb"] - im[idx, pix]) ** 2).mean() + 1e-3 * (-o * torch.log(o)).mean()
        opt.zero_grad(set_to_none=True)
        model.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    res["eager_ms_per_step"] = round((time.perf_counter() - t0) * 1e3 / steps, 3)
    res["rho_eager"] = float((refiner.dT[7].detach().cpu() + offset).norm() / offset.norm())

    # the fused route
    ds2 = data.DeviceDataset(imgs, moved, dirs, K=K, img_wh=(W, W), device=dev, seed=6)
    hp2 = HParams(batch_size=1024, T=14, num_epochs=1, steps_per_epoch=400, optimize_ext=True, pose_lr=lr)
    tr2 = Trainer(hp2, ds2, device=dev)
    tr2.load(ck)
    tr2.step.set_lr(0.0)
    tr2.training_step()  # eager + capture
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr2.training_step()
    torch.cuda.synchronize()
    res["fused_ms_per_step"] = round((time.perf_counter() - t0) * 1e3 / steps, 3)
    res["rho_fused"] = float((tr2.step.dT[7].cpu() + offset).norm() / offset.norm())
    res["fused_skipped_steps"] = tr2.step.skipped_steps()
    res["fused_gate_timeouts"] = tr2.step.gate_timeouts()
    os.remove(ck)
    out["e2e"] = res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--e2e-only", action="store_true")
    ap.add_argument("--e2e-steps", type=int, default=200)
    ap.add_argument("--e2e-lr", type=float, default=1e-3)
    ap.add_argument("--bench-lines", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_refine_bench: no GPU (a timing needs one)")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "reps_per_round": REPS,
           "config": "StepConfig defaults (8192 rays, Hash L16 F2 T2^19, ball-union occupancy), ray_grads on, "
                     "bench.py's dataset: 100 analytic 800x800 views drawn on the device"}
    if not a.e2e_only:
        st = step_timings(dev, bench_views(dev), out)
        kernel_timings(st, out)
    if a.e2e or a.e2e_only:
        e2e(dev, out, a.e2e_steps, a.e2e_lr)
    if a.bench_lines:
        lines = {}
        for path in sorted(glob.glob(os.path.join(a.bench_lines, "*.json"))):
            with open(path) as f:
                last = [ln for ln in f.read().splitlines() if ln.startswith("{")][-1]
            lines[os.path.splitext(os.path.basename(path))[0]] = json.loads(last)
        out["bench_py"] = lines
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
