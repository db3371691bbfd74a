"""Timings of the input-gradient kernels at the Lego step's sample count, on the points a marched
training step produces (not uniform points).  Every comparison alternates its variants round by
round in one process and reports the median and the minimum over the rounds (device events around
REPS back-to-back launches).  Needs a GPU; writes one JSON document.

    python tools/input_grad_bench.py --out profiles/r08_input_grad.json
"""
import argparse
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

from mfnerf import engine, synthetic  # noqa: E402
from mfnerf import field as FLD  # noqa: E402
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
    """{name: fn} -> {name: {median_us, min_us}}, variants alternated within each round."""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            t[k].append(timed(fn))
    return {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2)} for k, v in t.items()}


def make_step(dev, ray_grads, width=64, steps=6):
    st = engine.TrainStep(engine.StepConfig(rgb_width=width, ray_grads=ray_grads), device=dev, seed=0)
    st.set_occupancy(synthetic.ball_density_grid())
    batches = st.make_batches(4, seed=1)
    for k in range(steps):
        st.run(batches[k % 4])
    torch.cuda.synchronize()
    return st, batches


def kernel_timings(dev, out):
    st, _ = make_step(dev, True)
    t, m = st.parts[0], st.state.march.part[0]
    n = int(m.counter[0])
    out["samples"] = n
    out["rays"] = st.cfg.n_rays
    cap = st.cap_p
    table16 = st.p16[st.off_table:st.off_table + st.layout.n_params]
    xs, ts = m.xyzs, m.ts
    dfeat, ddirs = t.dfeat, t.ddirs
    dx = torch.empty(n, 3, device=dev)
    feat_rows = torch.empty(n, 32, dtype=torch.float16, device=dev)
    s = stream()
    out["grid_encode_bw_input_vs_fw"] = compare({
        "grid_encode_bw_input": lambda: FLD.grid_encode_bw_input(xs, n, table16, dfeat, st.desc, st.x_min, st.x_range,
                                                                 out=dx),
        "grid_encode_fw": lambda: FLD.grid_encode_fw(xs, n, table16, st.layout, st.desc, st.x_min, st.x_range,
                                                     out=feat_rows),
        "grid_encode_fw_planar": lambda: call("mfnerf_grid_encode_fw_planar", ptr(xs), n, None, st.x_min, st.x_range,
                                              st.desc, ptr(table16), ptr(t.feat), cap, s),
    })
    o, d = torch.empty(st.Np, 3, device=dev), torch.empty(st.Np, 3, device=dev)
    seg = torch.repeat_interleave(torch.arange(st.Np, device=dev), m.rays_a[:, 2])
    ray_of = m.rays_a[:, 0][seg]

    def unfused():
        FLD.grid_encode_bw_input(xs, n, table16, dfeat, st.desc, st.x_min, st.x_range, out=dx)
        o.zero_()
        o.index_add_(0, ray_of, dx)
        d.zero_()
        d.index_add_(0, ray_of, dx * ts[:n, None] + ddirs[:n])

    out["rays_input_grad_vs_unfused"] = compare({
        "rays_input_grad": lambda: FLD.rays_input_grad(xs[:n], ts[:n], dfeat, ddirs, m.rays_a, table16, st.desc,
                                                       st.x_min, st.x_range, out_o=o, out_d=d),
        "grid_encode_bw_input + 2 index_add_": unfused,
    })
    for width in (64, 128):
        sw = st if width == 64 else make_step(dev, True, width)[0]
        tw, mw = sw.parts[0], sw.state.march.part[0]
        args = (ptr(tw.feat), sw.cap_p, ptr(mw.dirs), sw.cap_p, ptr(mw.counter), ptr(sw.packed), width, ptr(tw.dsig),
                ptr(tw.drgb_s), 65536.0, ptr(tw.dfeat), None, None, ptr(tw.field_ws), None, None)
        res = compare({
            "field_bw": lambda: call("mfnerf_field_bw", *args, s),
            "field_bw_inputs": lambda: call("mfnerf_field_bw_inputs", *args, ptr(tw.ddirs), s),
        })
        res["samples"] = int(mw.counter[0])
        out[f"field_bw_inputs_vs_field_bw_w{width}"] = res


def step_timings(dev, out, steps=200):
    """The captured bench step (replay with the next batch's march prefetched), ray_grads off / on,
    alternated in blocks of `steps` replays; ms per step by a host clock around synchronised blocks."""
    runs = {}
    for name, on in (("ray_grads_off", False), ("ray_grads_on", True)):
        st, batches = make_step(dev, on, steps=3)
        st.capture()
        st.replay(batches[0], next_batch=batches[1])
        runs[name] = (st, batches)
    t = {k: [] for k in runs}
    for _ in range(7):
        for name, (st, batches) in runs.items():
            for k in range(20):
                st.replay(batches[(k + 1) % 4], next_batch=batches[(k + 2) % 4])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(steps):
                st.replay(batches[(k + 1) % 4], next_batch=batches[(k + 2) % 4])
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) * 1e3 / steps)
    out["step_ms"] = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                          "max_ms": round(max(v), 4)} for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("input_grad_bench: no GPU (a timing needs one)")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "reps_per_round": REPS,
           "config": "StepConfig defaults: 8192 rays, Hash L16 F2 T2^19, ball-union occupancy, after 6 steps"}
    kernel_timings(dev, out)
    step_timings(dev, out)
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
