"""Stage times of the DTU-protocol Chamfer distance on the device (permuto_sdf_amd/mesh_eval.py).

Workload: a sphere mesh of about 10^6 triangles (marching tetrahedra of an analytic volume), scaled to a scanned scene's
coordinates (radius 100 units around (50, -30, 650)), against a "scan" of 2 x 10^6 points on the same sphere with millimetre-scale
noise; density 0.2, max_dist 20 -- the protocol's defaults.  Per stage: `device_ms_incl_host_reads`, the time between two device
events around the stage -- the stages read the host (the grid's box, the sample total, the undecided counters), so the gaps in
which the device waits for the host are inside it -- and `wall_ms`; median and spread over the repeats after the warm-up; the sweep
count; the share of queries the cooperative nearest-neighbour pass left to the ring search.  Where sklearn is importable, the time
of its KD-tree (the protocol's engine) for the same two queries is printed beside ours, as context: there is no earlier time of
this project to compare with.  One JSON line on stdout; --out writes it to a file as well.

    python tools/mesh_eval_bench.py --out profiles/mesh_eval_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from permuto_sdf_amd import mesh_eval as me                    # noqa: E402
from permuto_sdf_amd.mesh import marching_tetrahedra            # noqa: E402


def timed(fn):
    """-> (result, device ms, wall ms)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def spread(values):
    return {"median": round(statistics.median(values), 3), "min": round(min(values), 3), "max": round(max(values), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=280, help="points per axis of the analytic volume (280: about 10^6 triangles)")
    ap.add_argument("--scan-points", type=int, default=2_000_000)
    ap.add_argument("--radius", type=float, default=100.0)
    ap.add_argument("--noise", type=float, default=0.001, help="scan noise, in units of the scene")
    ap.add_argument("--density", type=float, default=0.2)
    ap.add_argument("--max-dist", type=float, default=20.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    centre = torch.tensor([50.0, -30.0, 650.0], device=dev)

    n, half = args.grid, 1.25 * args.radius
    axis = torch.linspace(-half, half, n, device=dev)
    x, y, z = torch.meshgrid(axis, axis, axis, indexing="ij")
    volume = torch.sqrt(x * x + y * y + z * z) - args.radius
    del x, y, z
    h = 2 * half / (n - 1)
    V, F, _, _ = marching_tetrahedra(volume, 0.0, spacing=(h, h, h), normals=False)
    del volume
    V = V - half + centre
    g = torch.Generator(device=dev).manual_seed(7)
    scan = torch.nn.functional.normalize(torch.randn(args.scan_points, 3, generator=g, device=dev), dim=1) * args.radius
    scan = scan + torch.randn(args.scan_points, 3, generator=g, device=dev) * args.noise + centre

    stages = {k: {"device_ms_incl_host_reads": [], "wall_ms": []} for k in ("sample", "thin", "nearest_data_to_scan", "nearest_scan_to_data")}
    info = {}
    for it in range(args.warmup + args.repeats):
        order_gen = torch.Generator().manual_seed(11)
        cloud, *t_sample = timed(lambda: me.sample_surface(V, F, args.density))
        order = torch.randperm(cloud.shape[0], generator=order_gen).to(dev)
        (mask, sweeps), *t_thin = timed(lambda: me.radius_thin(cloud, args.density, order=order, return_sweeps=True))
        kept = cloud[mask]
        (d2s, _, open_a), *t_a = timed(lambda: me.nearest(kept, scan, args.max_dist, return_stats=True))
        (s2d, _, open_b), *t_b = timed(lambda: me.nearest(scan, kept, args.max_dist, return_stats=True))
        if it >= args.warmup:
            for key, t in zip(stages, (t_sample, t_thin, t_a, t_b)):
                stages[key]["device_ms_incl_host_reads"].append(t[0])
                stages[key]["wall_ms"].append(t[1])
        info = {"triangles": int(F.shape[0]), "vertices": int(V.shape[0]), "sampled_points": int(cloud.shape[0]),
                "kept_points": int(kept.shape[0]), "scan_points": int(scan.shape[0]), "sweeps": int(sweeps),
                "ring_share_data_to_scan": round(int(open_a) / max(kept.shape[0], 1), 6),
                "ring_share_scan_to_data": round(int(open_b) / max(scan.shape[0], 1), 6),
                "mean_d2s": float(d2s[d2s < args.max_dist].double().mean()),
                "mean_s2d": float(s2d[s2d < args.max_dist].double().mean())}
        info["chamfer"] = (info["mean_d2s"] + info["mean_s2d"]) / 2
    result = {"tool": "mesh_eval_bench", "device": torch.cuda.get_device_name(0), "density": args.density,
              "max_dist": args.max_dist, "warmup": args.warmup, "repeats": args.repeats, **info,
              "stages": {k: {m: spread(v) for m, v in s.items()} for k, s in stages.items()}}
    result["total_device_ms_incl_host_reads_median"] = round(sum(s["device_ms_incl_host_reads"]["median"] for s in result["stages"].values()), 3)

    if not args.no_sklearn:
        try:
            import sklearn.neighbors as skln
        except ImportError:
            skln = None
        if skln is not None:
            jobs = min(16, os.cpu_count() or 1)
            kept_h, scan_h = kept.cpu().numpy().astype(np.float64), scan.cpu().numpy().astype(np.float64)
            context = {}
            for key, q, r in (("nearest_data_to_scan", kept_h, scan_h), ("nearest_scan_to_data", scan_h, kept_h)):
                t0 = time.perf_counter()
                engine = skln.NearestNeighbors(n_neighbors=1, algorithm="kd_tree", n_jobs=jobs).fit(r)
                d, _ = engine.kneighbors(q, n_neighbors=1, return_distance=True)
                context[key] = {"wall_ms": round((time.perf_counter() - t0) * 1e3, 1), "n_jobs": jobs,
                                "mean_below_max_dist": float(d[d < args.max_dist].mean())}
            result["sklearn_kd_tree_context"] = context
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
