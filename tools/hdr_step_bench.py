"""Measurements of the HDR/exposure model inside the fused step (StepConfig.hdr), one process, one GPU;
writes one JSON document.

    python tools/hdr_step_bench.py --out profiles/hdr_step.json [--bench-lines DIR]

* the captured, replayed step with hdr off and on at the Lego shape (bench.py's preset: 8192 rays,
  Hash, T 2^19, rgb 64; the calibrated ball occupancy): off trains on bench.py's dataset (100 analytic
  800x800 views), on on the same balls photographed at three exposures (34 poses x 3, mfnerf.data.
  hdr_ball_scene_views).  The two are alternated in blocks; ms per step by a host clock around
  synchronised blocks: median, min and max over the blocks, the on - off difference beside the off
  line's own spread, samples per ray, gate timeouts and skipped steps.  The models train while they
  are timed, so the workloads drift apart; the pair is therefore timed again with the learning rate 0
  after the same number of training steps (frozen field: the option's own cost at equal weights' age);
* the module route for the HDR model at the same shape and from the on step's weights: render() +
  NeRFLoss + the unit-exposure term, autograd under torch's GradScaler, torch Adam (what trained the
  model before this option), ms per step over synchronised blocks;
* --bench-lines DIR: bench.py result lines saved as DIR/this_*.json and DIR/parent_*.json by a
  same-session, alternated run of this tree and of a build of the parent commit, copied into the
  document with the this - parent difference of their step times beside each side's spread.
"""
import argparse
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mf-nerf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from mfnerf import data, engine, synthetic  # noqa: E402
from mfnerf.field import XYZ_NET_PARAMS  # noqa: E402

BLOCKS, SETTLE, STEPS = 7, 20, 200
MODULE_BLOCKS, MODULE_STEPS = 3, 20
LEGO = dict(n_rays=8192, log2_T=19, grid="Hash", N_tables=1, rgb_width=64, lr=1e-2)
WH = (synthetic.LEGO_W, synthetic.LEGO_H)


def datasets(dev):
    scene = data.BallScene.matching_grid(seed=0)
    imgs, poses, dirs, K = data.ball_scene_views(scene, 100, synthetic.LEGO_W, synthetic.LEGO_F, seed=100, device=dev)
    ldr = data.DeviceDataset(imgs, poses, dirs, K=K, img_wh=WH, device=dev, seed=7)
    himgs, hposes, _, _, exposure = data.hdr_ball_scene_views(scene, 34, synthetic.LEGO_W, synthetic.LEGO_F, seed=100,
                                                              device=dev)
    hdr = data.DeviceDataset(himgs, hposes, dirs, K=K, img_wh=WH, device=dev, seed=7, exposure=exposure,
                             unit_exposure_rgb=data.UNIT_EXPOSURE_RGB_SYNTHETIC)
    return ldr, hdr


def make_step(dev, ds, hdr):
    kw = dict(hdr=True, unit_exposure_rgb=ds.unit_exposure_rgb) if hdr else {}
    st = engine.TrainStep(engine.StepConfig(**LEGO, **kw), device=dev, seed=0)
    st.set_occupancy(synthetic.ball_density_grid())
    st.attach_dataset(ds)
    for _ in range(6):
        st.run()
    torch.cuda.synchronize()
    st.capture()
    st.replay()
    return st


def _stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "blocks_ms": [round(x, 4) for x in v]}


def alternate(runs):
    t = {k: [] for k in runs}
    for _ in range(BLOCKS):
        for name, st in runs.items():
            for _k in range(SETTLE):
                st.replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _k in range(STEPS):
                st.replay()
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) * 1e3 / STEPS)
    res = {"step_ms": {k: _stats(v) for k, v in t.items()}}
    off, on = res["step_ms"]["hdr_off"], res["step_ms"]["hdr_on"]
    res["on_minus_off_ms"] = round(on["median_ms"] - off["median_ms"], 4)
    res["off_spread_ms"] = round(off["max_ms"] - off["min_ms"], 4)
    res["samples_per_ray"] = {k: round(float(st.live_samples()) / st.cfg.n_rays, 1) for k, st in runs.items()}
    res["gate_timeouts"] = {k: st.gate_timeouts() for k, st in runs.items()}
    res["skipped_steps"] = {k: st.skipped_steps() for k, st in runs.items()}
    return res


def module_route(dev, st, ds):
    """render() + autograd + torch Adam for NGP('None') holding the on step's weights."""
    from mfnerf.losses import NeRFLoss
    from mfnerf.networks import NGP
    from mfnerf.rendering import render
    from mfnerf.trainer import HParams
    c = st.cfg
    model = NGP(scale=c.scale, hparams=HParams(T=c.log2_T, rgb_channels=c.rgb_width), rgb_act="None").to(dev)
    with torch.no_grad():
        p = st.params
        model.xyz_encoder.params.copy_(torch.cat([p[:XYZ_NET_PARAMS], p[st.off_table:st.n_params]]))
        model.rgb_net.params.copy_(p[st.off_rgb:st.off_table])
        model.density_grid.copy_(st.density_grid)
        model.density_bitfield.copy_(st.bitfield)
        for i in range(3):
            getattr(model, f"tonemapper_net_{i}").params.copy_(st.tm_params[i])
    opt = torch.optim.Adam([q for q in model.parameters() if q.numel()], lr=c.lr, eps=1e-15)
    loss_fn = NeRFLoss(lambda_distortion=0)
    scaler = torch.amp.GradScaler("cuda")  # PL precision=16 (train.py:287)
    N = c.n_rays
    buf = torch.empty(3, N, 3, device=dev)
    ii, pp = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    u = ds.unit_exposure_rgb

    def one():
        ds.sample(buf, ii, pp)
        res = render(model, buf[0], buf[1], exposure=ds.exposure[ii.long()].reshape(-1, 1))
        unit = model.log_radiance_to_rgb(torch.zeros(1, 3, device=dev), exposure=torch.ones(1, 1, device=dev))
        loss = sum(v.mean() for v in loss_fn(res, {"rgb": buf[2]}).values()) + (0.5 * (unit.float() - u) ** 2).mean()
        opt.zero_grad()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        return res
    for _ in range(5):
        res = one()
    t = []
    for _ in range(MODULE_BLOCKS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _k in range(MODULE_STEPS):
            res = one()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3 / MODULE_STEPS)
    return {"step_ms": _stats(t), "steps_per_block": MODULE_STEPS,
            "samples_per_ray": round(float(res["rm_samples"]) / N, 1)}


def bench_lines(folder, out):
    lines = {}
    for path in sorted(glob.glob(os.path.join(folder, "*.json"))):
        with open(path) as f:
            last = [ln for ln in f.read().splitlines() if ln.startswith("{")][-1]
        lines[os.path.splitext(os.path.basename(path))[0]] = json.loads(last)
    out["bench_py"] = lines
    key = "ms_per_step"
    side = {s: [ln[key] for name, ln in lines.items() if name.startswith(s + "_") and key in ln]
            for s in ("this", "parent")}
    if side["this"] and side["parent"]:
        out["bench_py_summary"] = {
            "field": key,
            "this_median": statistics.median(side["this"]), "parent_median": statistics.median(side["parent"]),
            "this_minus_parent": round(statistics.median(side["this"]) - statistics.median(side["parent"]), 5),
            "this_spread": round(max(side["this"]) - min(side["this"]), 5),
            "parent_spread": round(max(side["parent"]) - min(side["parent"]), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-lines", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hdr_step_bench: no GPU (a timing needs one)")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "blocks": BLOCKS, "settle_steps_per_block": SETTLE,
           "timed_steps_per_block": STEPS,
           "config": "the Lego shape (bench.py's preset): 8192 rays, Hash, T 2^19, rgb 64, calibrated ball occupancy; "
                     "hdr_off on 100 analytic 800x800 views, hdr_on on the same balls at 34 poses x 3 exposures "
                     "(0.25, 1, 4); captured one-graph step, gated prefetched march"}
    ldr, hdr = datasets(dev)
    runs = {"hdr_off": make_step(dev, ldr, False), "hdr_on": make_step(dev, hdr, True)}
    out["training"] = alternate(runs)
    for st in runs.values():
        st.set_lr(0.0)
    out["frozen_field"] = alternate(runs)
    out["module_route_hdr"] = module_route(dev, runs["hdr_on"], hdr)
    out["module_over_fused"] = round(out["module_route_hdr"]["step_ms"]["median_ms"]
                                     / out["frozen_field"]["step_ms"]["hdr_on"]["median_ms"], 1)
    if a.bench_lines:
        bench_lines(a.bench_lines, out)
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
