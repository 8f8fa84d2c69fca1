"""Mesh export timings: MeshExtractor.extract (permuto_sdf_amd/mesh.py) on an SDF net fitted to a sphere, dense and with a
shell occupancy grid, against the host path it replaces -- the reference's loop of 64^3 chunks evaluated on the device, copied
into an n^3 numpy volume and handed to the marching-tetrahedra stand-in (permuto_sdf_py/utils/sdf_utils.py:252-292 through
compat/skimage/measure.py).  Writes one JSON document (default profiles/mesh_extract.json).

    python tools/mesh_extract_bench.py [--sizes 256,512,1024,2048] [--host-sizes 256,512] [--out profiles/mesh_extract.json]

Times are wall clock around a synchronised call, outputs left on the device (the device path) or in host numpy (the host
path); the best of --repeats calls is reported (one call at 2048 and for the host path)."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from permuto_sdf import OccupancyGrid  # noqa: E402
from permuto_sdf_amd import FusedMLP, PermutoEncoding  # noqa: E402
from permuto_sdf_amd.mesh import MeshExtractor  # noqa: E402
from permuto_sdf_amd.optim import FusedAdamW  # noqa: E402


def fit_sphere_sdf(dev, r0=0.3, iters=300):
    torch.manual_seed(0)
    enc = PermutoEncoding(3, 2 ** 16, 8, 2, np.geomspace(1.0, 0.02, 8), concat_points=True, concat_points_scaling=1.0,
                          init_scale=1e-3).to(dev)
    mlp = FusedMLP([enc.output_dims(), 64, 64, 64, 1]).to(dev)
    opt = FusedAdamW(list(enc.parameters())[:1] + list(mlp.parameters()), lr=5e-3)
    win = torch.ones(8, device=dev)
    for _ in range(iters):
        x = torch.rand(16384, 3, device=dev) - 0.5
        loss = ((mlp(enc(x, win)) - (x.norm(dim=1, keepdim=True) - r0)) ** 2).mean()
        for p in opt.param_groups[0]["params"]:
            p.grad = None
        loss.backward()
        opt.step()
    return enc, mlp, win, float(loss)


def shell_grid(dev, n_vox, r0=0.3, width=0.05):
    grid = OccupancyGrid(n_vox, 1.0, [0, 0, 0])
    centres = grid.compute_grid_points(False)
    grid.set_grid_occupancy(((centres.norm(dim=1) - r0).abs() < width).contiguous())
    return grid


def host_path(enc, mlp, win, n, lo, hi, measure):
    """the parent way: 64^3 chunks -> host volume -> stand-in (normals from the volume's finite differences)"""
    N = 64
    X = torch.linspace(lo, hi, n).split(N)
    full = np.zeros([n, n, n], dtype=np.float32)
    dev = win.device
    with torch.no_grad():
        for xi, xs in enumerate(X):
            for yi, ys in enumerate(X):
                for zi, zs in enumerate(X):
                    xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                    pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1).to(dev)
                    cur = mlp(enc(pts, win)).reshape(len(xs), len(ys), len(zs)).cpu().numpy()
                    full[xi * N: xi * N + len(xs), yi * N: yi * N + len(ys), zi * N: zi * N + len(zs)] = cur
    v, f, nrm, _ = measure.marching_cubes(full, 0.0)
    v = v / (n - 1.0) * (hi - lo) + lo
    return v, f, -nrm


def timed(fn, repeats):
    best, out = None, None
    for _ in range(repeats):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        peak = torch.cuda.max_memory_allocated() - base
        best = dt if best is None else min(best, dt)
    return best, peak, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024,2048")
    ap.add_argument("--host-sizes", default="256,512")
    ap.add_argument("--grid", type=int, default=128, help="voxels per dimension of the shell occupancy grid")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_extract.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    spec = importlib.util.spec_from_file_location("_standin_measure", os.path.join(ROOT, "compat", "skimage", "measure.py"))
    measure = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(measure)
    enc, mlp, win, loss = fit_sphere_sdf(dev)
    grid = shell_grid(dev, a.grid)
    ex = MeshExtractor(enc, mlp, win)
    lo, hi = -0.5, 0.5
    doc = {"device": torch.cuda.get_device_name(0), "field": "8-level encoding + 64x3 MLP fitted to |x| - 0.3, loss %.2e" % loss,
           "occupancy_grid": "%d^3 shell, half-width 0.05" % a.grid, "repeats": a.repeats,
           "slab_points": MeshExtractor.DEFAULT_SLAB_POINTS, "point_budget": MeshExtractor.DEFAULT_POINT_BUDGET, "rows": []}
    host_sizes = [int(s) for s in a.host_sizes.split(",") if s]

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    for n in [int(s) for s in a.sizes.split(",") if s]:
        reps = a.repeats if n < 2048 else 1          # 8.6e9 evaluations per dense run
        row = {"n": n, "repeats": reps}
        for name, kw in (("dense", {}), ("sparse", {"occupancy_grid": grid})):
            try:
                t, peak, m = timed(lambda: ex.extract(n, lo, hi, **kw), reps)
                row[name] = {"seconds": round(t, 4), "V": int(m.V.shape[0]), "F": int(m.F.shape[0]),
                             "evaluated_fraction": round(m.nr_evaluated / n ** 3, 4), "peak_device_MiB": round(peak / 2 ** 20, 1)}
                del m
            except torch.cuda.OutOfMemoryError as e:        # an allocation that does not fit: say which (anything else ends the run)
                row[name] = {"error": str(e).splitlines()[0][:300]}
            torch.cuda.empty_cache()
            print(n, name, row[name], flush=True)
        if n in host_sizes:
            t, peak, (v, f, _) = timed(lambda: host_path(enc, mlp, win, n, lo, hi, measure), 1)
            row["host_path"] = {"seconds": round(t, 4), "V": int(len(v)), "F": int(len(f)), "host_volume_MiB": round(n ** 3 * 4 / 2 ** 20, 1)}
            for name in ("dense", "sparse"):
                if "seconds" in row[name]:
                    row["host_path"]["ratio_to_" + name] = round(t / row[name]["seconds"], 1)
            print(n, "host_path", row["host_path"], flush=True)
        doc["rows"].append(row)
        flush()
    flush()


if __name__ == "__main__":
    main()
