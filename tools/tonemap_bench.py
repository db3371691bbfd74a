"""Timing of the HDR tonemapper kernels (mfnerf_tonemap_fw / _bw) against the torch fp16 composition
of the same maths, one process, one GPU; writes one JSON document.

    python tools/tonemap_bench.py --out profiles/tonemap_bench.json [--n 524288] [--runs 30]

n = 524,288 samples (the Lego step's sample count), C = 3, per-sample exposure.  The composition is
what tcnn's layout implies in torch: per channel a padded (n,16) half row [x, 1, ..., 1], two half
matmuls (16 -> 64 ReLU, 64 -> 16 Sigmoid, column 0 kept), autograd for the backward.  Both sides are
timed with device events around the forward and around the backward, alternated run by run after a
warm-up; the median, min and max over the runs are reported, with the algorithmic bytes per sample
and the two sides' largest output and gradient differences.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mf-nerf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from mfnerf import tonemap  # noqa: E402

# per sample at C = 3: log-radiance 6 B in, rgb 6 B out, exposure 4 B; the backward reads those three
# and the upstream gradient (12 B) and writes the input gradient (12 B)
BYTES_FW = 6 + 6 + 4
BYTES_BW = 6 + 4 + 6 + 12 + 12
# the composition per channel: the (n,16) row and (n,64) hidden written and read in half, the (n,16)
# output written -- forward only, before autograd's saved tensors and the backward's passes
BYTES_TORCH_FW = 3 * (2 * 16 * 2 + 2 * 64 * 2 + 16 * 2)


def composition(lograd, log_e, P):
    ys = []
    n = lograd.shape[0]
    ones = torch.ones(n, 15, dtype=torch.float16, device=lograd.device)
    for c in range(3):
        x = (lograd[:, c:c + 1] + log_e).half()
        W1, W2 = P[c, :1024].view(64, 16).half(), P[c, 1024:].view(16, 64).half()
        h = torch.relu(torch.cat([x, ones], 1) @ W1.t())
        ys.append(torch.sigmoid(h @ W2.t())[:, :1])
    return torch.cat(ys, 1)


def _stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=524288)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tonemap_bench: no GPU (a timing needs one)")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    n = a.n
    lograd16 = torch.empty(n, 3).uniform_(-6, 6, generator=g).half().to(dev)
    e = torch.tensor([0.25, 1.0, 4.0])[torch.randint(3, (n,), generator=g)].to(dev)
    s = (6.0 / 80) ** 0.5
    params = torch.empty(3 * 2048).uniform_(-s, s, generator=g).to(dev)
    dy = torch.empty(n, 3).uniform_(-1, 1, generator=g).to(dev)
    log_e = torch.log(e).reshape(n, 1)

    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    t = {"kernel_fw": [], "kernel_bw": [], "torch_fw": [], "torch_bw": []}
    for it in range(a.warmup + a.runs):
        k0, k1, k2, t0, t1, t2 = ev(), ev(), ev(), ev(), ev(), ev()
        k0.record()
        y = tonemap.tonemap_fw(lograd16, e, 1, params)
        k1.record()
        dx, gp = tonemap.tonemap_bw(lograd16, e, 1, params, y, dy)
        k2.record()
        lg = lograd16.float().requires_grad_(True)
        P = params.reshape(3, 2048).clone().requires_grad_(True)
        t0.record()
        yt = composition(lg, log_e, P)
        t1.record()
        yt.backward(dy.half())
        t2.record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            t["kernel_fw"].append(k0.elapsed_time(k1))
            t["kernel_bw"].append(k1.elapsed_time(k2))
            t["torch_fw"].append(t0.elapsed_time(t1))
            t["torch_bw"].append(t1.elapsed_time(t2))
    out = {"device": torch.cuda.get_device_name(0), "n": n, "C": 3, "exposure": "per sample", "runs": a.runs,
           "warmup": a.warmup, "timing": "device events around each call (host wrappers and their allocations included)",
           "ms": {k: _stats(v) for k, v in t.items()},
           "bytes_per_sample": {"kernel_fw": BYTES_FW, "kernel_bw": BYTES_BW, "torch_fw_at_least": BYTES_TORCH_FW},
           "max_abs_diff": {"rgb": float((y.float() - yt.float()).abs().max()),
                            "dL_dlograd": float((dx - lg.grad).abs().max()),
                            "grad_params_rel": float((gp - P.grad.reshape(-1)).norm() / P.grad.norm())}}
    med = {k: v["median_ms"] for k, v in out["ms"].items()}
    out["GBps"] = {"kernel_fw": round(BYTES_FW * n / med["kernel_fw"] / 1e6, 1),
                   "kernel_bw": round(BYTES_BW * n / med["kernel_bw"] / 1e6, 1)}
    out["kernel_pair_ms"] = round(med["kernel_fw"] + med["kernel_bw"], 4)
    out["torch_pair_ms"] = round(med["torch_fw"] + med["torch_bw"], 4)
    out["kernels_not_slower"] = out["kernel_pair_ms"] <= out["torch_pair_ms"]
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    if not out["kernels_not_slower"]:
        raise SystemExit("tonemap_bench: the kernel pair is slower than the torch composition")


if __name__ == "__main__":
    main()
