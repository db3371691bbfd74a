"""Train the analytic test scene of tools/train_30k.py (or load a checkpoint of it), extract a
triangle mesh of the density field on the device (mfnerf.mesh; the reference's test.ipynb mesh cell)
and write it as PLY.

Prints one JSON line: V, F, the Euler characteristic chi = V - E + F (E = distinct undirected edges of
the faces), and the device time of the three phases -- density lattice, count + scans (with the one
read-back of the totals), emit -- by HIP events: each phase is run `--reps` times after one untimed
pass; the median and the spread are reported, and the count kernel's time without the scans beside
them.  For the count kernel and for emit also the achieved GB/s against
their algorithmic bytes (count: 4 B read + 2 B written per lattice point; emit: the same 4 B + 8 B of
offsets per point read, 36 B per vertex and 12 B per face written -- 24 of the 36 by the emit kernel,
position and normal; the colour pass writes the other 12, so the kernel's own rate is given too).

With --occupancy, --min-faces, --min-fraction or --largest-only the mesh is cleaned (mfnerf.mesh:
occupancy_mask, components, clean_mesh) before it is coloured and written, and each mesh's entry gains
"cleaning": the device time of the phases -- mask, labelling (hook + flatten + count), selection +
scans + read-back, compaction -- measured the same way beside the same run's other phases, and V, F
and the component counts before and after.  Without those flags nothing changes.

    python tools/export_mesh.py [--steps 30000 | --ckpt model.ckpt] [--resolution 256] [--out mesh.ply]
                                [--occupancy] [--min-faces N] [--min-fraction X] [--largest-only]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mf-nerf_amd")]
# graph replays through the per-node launch path, as bench.py (before the HIP runtime initialises)
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
import torch  # noqa: E402

from mfnerf import data, mesh, synthetic  # noqa: E402
from mfnerf.trainer import HParams, Trainer  # noqa: E402


def algorithmic_bytes(n_points, V, F):
    """Bytes each pass must move, from the shapes alone."""
    return {"count": 6 * n_points, "emit": 12 * n_points + 36 * V + 12 * F,
            "emit_kernel": 12 * n_points + 24 * V + 12 * F}


def euler_characteristic(n_vertices, faces):
    """V - E + F on the device."""
    if faces.shape[0] == 0:
        return int(n_vertices)
    f = faces.long()
    a = torch.cat([f[:, 0], f[:, 1], f[:, 2]])
    b = torch.cat([f[:, 1], f[:, 2], f[:, 0]])
    E = torch.unique(torch.minimum(a, b) * int(n_vertices) + torch.maximum(a, b)).numel()
    return int(n_vertices) - E + faces.shape[0]


def timed(fn, reps):
    """(last result, sorted per-call device times in ms) of `reps` calls of fn."""
    times, out = [], None
    for _ in range(reps):
        out = None  # the previous result's memory goes back to the allocator first
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return out, sorted(times)


def summary(times):
    return {"median_ms": round(statistics.median(times), 4), "min_ms": round(times[0], 4),
            "max_ms": round(times[-1], 4)}


def cleaning_bytes(n_points, V, F, Vk, Fk, colors):
    """Bytes each cleaning phase must move, from the shapes alone: every gather counted as its 4 bytes,
    a union-find walk as one step per face vertex."""
    row = 36 if colors else 24
    return {"mask": 8 * n_points,             # sigma read, and written where cleared (the bitfield stays in cache)
            # init 8 V; hook 12 F of faces + 12 F of parents; flatten 8 V; count 12 F + 4 F of labels
            "labelling": 16 * V + 40 * F,
            # best 4 V; vertex flags 9 V; face flags 21 F; the two scans 5 (V + F)
            "selection": 18 * V + 26 * F,
            # flags V + F; kept rows read and written with their offset; kept faces read, remapped, written
            "compaction": V + F + (2 * row + 4) * Vk + 40 * Fk}


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30000, help="training steps (train.py's protocol is 30000)")
    ap.add_argument("--ckpt", default=None, help="load these weights instead of training")
    ap.add_argument("--resolution", type=int, nargs="+", default=[256], help="one or more lattice resolutions")
    ap.add_argument("--threshold", type=float, default=20.0)
    ap.add_argument("--out", default="mesh.ply", help="PLY of the last resolution ('' writes none)")
    ap.add_argument("--tex", type=float, default=40.0)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--W", type=int, default=synthetic.LEGO_W)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-colors", action="store_true")
    ap.add_argument("--occupancy", action="store_true",
                    help="clear the lattice where the occupancy bitfield is clear or the scene box ends")
    ap.add_argument("--min-faces", type=int, default=0, help="drop components with fewer faces")
    ap.add_argument("--min-fraction", type=float, default=0.0,
                    help="drop components with fewer faces than this fraction of the largest one's")
    ap.add_argument("--largest-only", action="store_true", help="keep the largest component alone")
    return ap


def cleaning_requested(args):
    return bool(args.occupancy or args.min_faces > 0 or args.min_fraction > 0.0 or args.largest_only)


def main():
    args = build_parser().parse_args()
    cleaning = cleaning_requested(args)
    select_kw = dict(min_faces=args.min_faces, min_fraction=args.min_fraction, largest_only=args.largest_only)
    dev = torch.device("cuda")
    focal = 0.5 * args.W / math.tan(0.5 * 0.6911112)
    scene = data.BallScene.matching_grid(seed=0)
    scene.texture_freq = args.tex
    imgs, poses, dirs, K = data.ball_scene_views(scene, args.views, args.W, focal, seed=0, device=dev)
    ds = data.DeviceDataset(imgs, poses, dirs, K=K, img_wh=(args.W, args.W), device=dev, seed=5)
    hp = HParams(num_epochs=max(1, math.ceil(args.steps / 1000)))
    tr = Trainer(hp, ds, device=dev)
    if args.ckpt:
        tr.load(args.ckpt)
    else:
        tr.fit(steps=args.steps, log_every=0)
    model = tr.to_ngp()
    lo, hi = -hp.scale, hp.scale
    results = []
    for R in args.resolution:
        n = (R + 1) ** 3

        def run(reps):
            sigma, t_density = timed(lambda: mesh.density_lattice(model, R, lo, hi), reps)
            t_mask = []
            if args.occupancy:
                raw = sigma
                for _ in range(reps):  # in place: each repetition masks a fresh copy, copied outside the events
                    sigma = raw.clone()
                    _, t = timed(lambda: mesh.occupancy_mask(sigma, lo, hi, model.density_bitfield, model.cascades,
                                                             model.scale, model.grid_size), 1)
                    t_mask += t
                del raw
                t_mask.sort()

            _, t_kernel = timed(lambda: mesh.count(sigma, args.threshold), reps)

            def count():
                voff, toff, totals = mesh.count_and_scan(sigma, args.threshold)
                return voff, toff, [int(v) for v in totals.cpu()]
            (voff, toff, (V, F)), t_count = timed(count, reps)
            m, t_emit = timed(lambda: mesh.emit(sigma, args.threshold, lo, hi, voff, toff, V, F), reps)
            clean = None
            if cleaning and V > 0 and F > 0:
                (labels, counts), t_label = timed(lambda: mesh._components(m["faces"], V), reps)
                (flags, sizes), t_select = timed(lambda: mesh.select_and_scan(m, labels, counts, **select_kw), reps)
                cleaned, t_compact = timed(lambda: mesh.compact(m, flags, sizes), reps)
                clean = (cleaned, t_mask, t_label, t_select, t_compact)
            return m, t_density, t_kernel, t_count, t_emit, clean

        run(1)  # untimed: code objects, allocator
        m, t_density, t_kernel, t_count, t_emit, clean = run(args.reps)
        V, F = m["vertices"].shape[0], m["faces"].shape[0]
        nbytes = algorithmic_bytes(n, V, F)
        chi = euler_characteristic(V, m["faces"])
        cleaning_entry = None
        if cleaning:
            cleaning_entry = {"occupancy": args.occupancy, **select_kw, "V_before": V, "F_before": F}
            if clean is None:  # an empty mesh: nothing to label
                m = mesh.clean_mesh(m, **select_kw)
                cleaning_entry.update({"V_after": 0, "F_after": 0, "components_before": m["components"][0],
                                       "components_after": 0})
            else:
                m, t_mask, t_label, t_select, t_compact = clean
                Vk, Fk = m["vertices"].shape[0], m["faces"].shape[0]
                cb = cleaning_bytes(n, V, F, Vk, Fk, colors=False)
                phases = {"labelling": t_label, "selection": t_select, "compaction": t_compact}
                if args.occupancy:
                    phases["mask"] = t_mask
                cleaning_entry.update({"V_after": Vk, "F_after": Fk, "components_before": m["components"][0],
                                       "components_after": m["components"][1],
                                       "chi_after": euler_characteristic(Vk, m["faces"])})
                for name, t in phases.items():
                    cleaning_entry[name] = summary(t)
                    cleaning_entry[name + "_bytes"] = cb[name]
                    cleaning_entry[name + "_GBps"] = round(cb[name] / statistics.median(t) / 1e6, 1)
        if not args.no_colors:
            m["colors"] = mesh.vertex_colors(model, m)
        results.append({
            "resolution": R, "lattice_points": n, "V": V, "F": F, "chi": chi,
            "density_lattice": summary(t_density), "count_and_scans": summary(t_count), "emit": summary(t_emit),
            "count_kernel_alone": summary(t_kernel),
            "count_bytes": nbytes["count"], "emit_bytes": nbytes["emit"],
            "count_kernel_GBps": round(nbytes["count"] / statistics.median(t_kernel) / 1e6, 1),
            "emit_GBps": round(nbytes["emit"] / statistics.median(t_emit) / 1e6, 1),
            "emit_kernel_bytes": nbytes["emit_kernel"],
            "emit_kernel_GBps": round(nbytes["emit_kernel"] / statistics.median(t_emit) / 1e6, 1)})
        if cleaning_entry is not None:
            results[-1]["cleaning"] = cleaning_entry
    if args.out:
        mesh.save_ply(args.out, m)
    print(json.dumps({"scene": f"12-ball scene, texture_freq {args.tex}, {args.views} views at {args.W}x{args.W}",
                      "weights": args.ckpt or f"{tr.global_step} training steps", "threshold": args.threshold,
                      "reps": args.reps, "meshes": results, "out": args.out or None,
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
