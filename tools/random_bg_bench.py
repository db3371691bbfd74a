"""Measurements of --random_bg inside the fused step (StepConfig.random_bg), one process, one GPU;
writes one JSON document.

    python tools/random_bg_bench.py --out profiles/r11_random_bg.json [--bench-lines DIR]

* the captured, replayed step with random_bg off and on at BASELINE config 4's shape (4096 rays,
  scale 16 -> 6 cascades and exponential steps, MixedFeature, 8 tables, T 2^20, rgb 128) on bench.py's
  dataset (100 analytic 800x800 views drawn on the device), the two alternated in blocks; ms per step
  by a host clock around synchronised blocks: median, min and max over the blocks, gate_timeouts and
  skipped_steps, and the on - off difference beside the off line's own spread over its blocks.  By
  construction both replay the same number of launches (the colour rides the batch's draw launch; the
  loss-carrying kernel reads three floats instead of three arguments).  Two controls: a second
  random_bg-off instance in the same alternation (what a step's placement alone does to its time), and
  the off / on pair again with the field frozen (learning rate 0: the same samples and weights on both
  sides, where the training steps' workloads drift apart with their losses);
* --bench-lines DIR: bench.py result lines saved as DIR/this_*.json and DIR/parent_*.json by a
  same-session run of this tree and of the parent commit, copied into the document with the
  this - parent difference of their step times beside each side's spread.
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

BLOCKS, SETTLE, STEPS = 7, 20, 200
CONFIG4 = dict(n_rays=4096, scale=16.0, grid="MixedFeature", N_tables=8, log2_T=20, rgb_width=128, lr=2e-2)


def bench_views(dev):
    scene = data.BallScene.matching_grid(seed=0)
    return data.ball_scene_views(scene, 100, synthetic.LEGO_W, synthetic.LEGO_F, seed=100, device=dev)


def make_step(dev, views, grid, on, frozen=False):
    imgs, poses, dirs, K = views
    st = engine.TrainStep(engine.StepConfig(random_bg=on, **CONFIG4), device=dev, seed=0)
    st.set_occupancy(grid)
    if frozen:
        st.set_lr(0.0)
    # the images are shared (already resident: DeviceDataset keeps the tensor it is given)
    st.attach_dataset(data.DeviceDataset(imgs, poses, dirs, K=K, img_wh=(synthetic.LEGO_W, synthetic.LEGO_H),
                                         device=dev, seed=7))
    for _ in range(6):
        st.run()
    torch.cuda.synchronize()
    return st


def _stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "blocks_ms": [round(x, 4) for x in v]}


def compare(dev, views, grid, variants, frozen=False):
    """variants: {name: random_bg}; one captured step each, timed in alternated blocks."""
    runs = {}
    for name, on in variants.items():
        st = make_step(dev, views, grid, on, frozen)
        st.capture()
        st.replay()
        runs[name] = st
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
    off, on = res["step_ms"]["random_bg_off"], res["step_ms"]["random_bg_on"]
    res["on_minus_off_ms"] = round(on["median_ms"] - off["median_ms"], 4)
    res["off_spread_ms"] = round(off["max_ms"] - off["min_ms"], 4)
    res["on_minus_off_exceeds_off_spread"] = abs(res["on_minus_off_ms"]) > res["off_spread_ms"]
    if "random_bg_off_twin" in res["step_ms"]:  # a second instance of the same step: what placement alone does
        res["twin_minus_off_ms"] = round(res["step_ms"]["random_bg_off_twin"]["median_ms"] - off["median_ms"], 4)
    res["gate_timeouts"] = {k: st.gate_timeouts() for k, st in runs.items()}
    res["skipped_steps"] = {k: st.skipped_steps() for k, st in runs.items()}
    res["samples_per_ray"] = {k: round(float(st.live_samples()) / st.cfg.n_rays, 1) for k, st in runs.items()}
    res["last_colour"] = [round(v, 6) for v in runs["random_bg_on"].bg.tolist()]
    return res


def step_timings(dev, views, out):
    """The training step (the model trains while it is timed, so the two steps' workloads drift apart
    with their losses), with a second random_bg-off instance as the placement control; then the same
    pair with the field frozen (learning rate 0): identical samples, weights and launches on both
    sides, so that difference is the option's own cost."""
    grid = synthetic.ball_density_grid(cascades=6, scale=CONFIG4["scale"])
    out.update(compare(dev, views, grid, {"random_bg_off": False, "random_bg_on": True, "random_bg_off_twin": False}))
    out["frozen_field"] = compare(dev, views, grid, {"random_bg_off": False, "random_bg_on": True}, frozen=True)


def bench_lines(folder, out):
    lines = {}
    for path in sorted(glob.glob(os.path.join(folder, "*.json"))):
        with open(path) as f:
            last = [ln for ln in f.read().splitlines() if ln.startswith("{")][-1]
        lines[os.path.splitext(os.path.basename(path))[0]] = json.loads(last)
    out["bench_py"] = lines
    key = "ms_per_step"
    if not lines or not all(key in ln for ln in lines.values()):
        return
    side = {s: [ln[key] for name, ln in lines.items() if name.startswith(s + "_")] for s in ("this", "parent")}
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
        raise SystemExit("random_bg_bench: no GPU (a timing needs one)")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "blocks": BLOCKS, "settle_steps_per_block": SETTLE,
           "timed_steps_per_block": STEPS,
           "config": "BASELINE config 4's shape: 4096 rays, scale 16 (6 cascades, exp steps), MixedFeature, 8 tables, "
                     "T 2^20, rgb 128, ball-union occupancy in every cascade; bench.py's dataset: 100 analytic "
                     "800x800 views drawn on the device; captured one-graph step, gated prefetched march"}
    step_timings(dev, bench_views(dev), out)
    if a.bench_lines:
        bench_lines(a.bench_lines, out)
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
