"""Time of one isoline slice of a fitted SDF at the two workloads of the reference's viewer
(permuto_sdf_py/experiments/visualization/visualize_sdf_isolines.py:69-72: a layer of 500 x 500 cells, and its "full layer" of
4000 x 4000), two ways in one process:

  (a) `sdf_slice.render_slice`: per chunk of 2^21 cells, points -> masked encode -> masked MLP (1-row head) -> colorize;
  (b) the reference's loop restated over the operators the tree had before (:75-156): the meshgrid in torch, the rotation in
      float64 on the HOST and back, chunks of 6 000 points through the net's forward, the colour map in float64 on the host and
      back, 15 masked assignments in torch, and `check_point_inside_primitive`.

The net is an `SdfFitter` 3-D fit of a few hundred steps to a sphere of radius 0.25: nothing here is a trained scene.  The ways
alternate; one call of each warms it up; a timed window is whole slices, repeated until at least `--min-window` seconds have
passed, between two host clocks with a device synchronise before each.  Reported: the median over the windows and their minimum
and maximum.  Not measured here: a second machine, and kernel times under a profiler.  One JSON line on stdout; --out writes it
to a file as well.

    python tools/sdf_slice_bench.py --out profiles/sdf_slice_bench.json
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from permuto_sdf_amd import sdf_fit                                                          # noqa: E402
from permuto_sdf_amd.box_trace import Box                                                     # noqa: E402
from permuto_sdf_amd.sdf_slice import IsoStyle, SlicePlane, render_slice                      # noqa: E402

CHUNK = 6000                                                                          # visualize_sdf_isolines.py:95


def sphere_cloud(dev, n=200000, seed=0):
    g = torch.Generator().manual_seed(seed)
    nrm = F.normalize(torch.randn(n, 3, generator=g), dim=1)
    return sdf_fit.OrientedCloud((0.25 * nrm).to(dev), nrm.to(dev))


def map_range_tensor(x, in_lo, in_hi, out_lo, out_hi):                                # common_utils.py:150-154
    return out_lo + ((out_hi - out_lo) / (in_hi - in_lo)) * (torch.clamp(x, in_lo, in_hi) - in_lo)


def host_colour_map(x64, table64):
    """ColorMngr.eigen2color(x, "pubu") restated: float64 on the host, piecewise linear over the control points"""
    pos = np.linspace(0.0, 1.0, table64.shape[0])
    return np.stack([np.interp(x64, pos, table64[:, c]) for c in range(3)], 1)


@torch.no_grad()
def operator_chain(net, it, plane, box, S, style):
    """(b) -> (colours [S S, 3], sdf [S S], is_valid [S S, 1])"""
    dev = net.encoding.lattice_values.device
    x_coord = torch.arange(S, device=dev).view(-1, 1, 1).repeat(1, S, 1)
    y_coord = torch.arange(S, device=dev).view(1, -1, 1).repeat(S, 1, 1)
    z_coord = torch.zeros(S, S, device=dev).view(S, S, 1)
    z_coord += plane.z
    x_coord = (x_coord / S - 0.5) * 2.0
    y_coord = (y_coord / S - 0.5) * 2.0
    point_layer = torch.cat([x_coord, y_coord, z_coord], 2).transpose(0, 1).reshape(-1, 3)
    V = point_layer.detach().double().cpu().numpy() @ plane.axes.astype(np.float64).T      # apply_model_matrix_to_cpu
    query = torch.from_numpy(V).float().to(dev)
    nr_points = query.shape[0]
    sdf_full = torch.zeros(nr_points, device=dev)
    chunks = torch.chunk(query, math.ceil(nr_points / CHUNK))
    start = 0
    for pts in chunks:
        sdf, _ = net(pts, it)
        sdf_full[start:start + pts.shape[0]] = sdf.squeeze(1)
        start += pts.shape[0]
    table64 = np.asarray(style.table, np.float64)
    x = map_range_tensor(sdf_full, *style.base_map)
    colours = torch.from_numpy(host_colour_map(x.double().cpu().numpy(), table64)).to(dev).float()
    for i in range(style.nr_lines):
        centre = i * style.distance
        in_range = torch.logical_and(sdf_full > centre - style.width / 2, sdf_full < centre + style.width / 2)
        colours[in_range, :] = 0.0
        a, b, c, d = style.line_map
        val = c + ((d - c) / (b - a)) * (np.clip(np.array([centre]), a, b) - a)
        colours[in_range, :] = torch.from_numpy(host_colour_map(val, table64)).view(1, 3).float().to(dev)
    is_valid = box.check_point_inside_primitive(query)
    return colours, sdf_full, is_valid


def window(fn, min_seconds):
    """-> (seconds per slice, slices) over whole slices until min_seconds have passed; ends in a synchronise"""
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        fn()
        n += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return dt / n, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[500, 4000])
    ap.add_argument("--fit-steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per way and size, alternating")
    ap.add_argument("--min-window", type=float, default=0.5, help="seconds")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sdf_slice_bench measures a device: no GPU is visible, nothing is measured")
    dev = torch.device("cuda:0")
    fitter = sdf_fit.SdfFitter(sphere_cloud(dev))
    for _ in range(args.fit_steps):
        fitter.step()
    torch.cuda.synchronize()
    net, it = fitter.net, fitter.iter
    surface_error = float(fitter.surface_error(sphere_cloud(dev, 20000, seed=1).points))
    box = Box([0.6, 0.65, 0.5], [0.0, 0.0, 0.0])                                      # visualize_sdf_isolines.py:226
    th = math.radians(30.0)                                                           # a layer that is not axis aligned
    plane = SlicePlane([[math.cos(th), 0.0, math.sin(th)], [0.0, 1.0, 0.0], [-math.sin(th), 0.0, math.cos(th)]], -0.057)   # :245
    style = IsoStyle()
    result = {"tool": "sdf_slice_bench", "device": torch.cuda.get_device_name(0), "net": "SdfFitter 3-D fit of a sphere, not a trained scene",
              "fit_steps": args.fit_steps, "fit_surface_error": round(surface_error, 5), "rounds": args.rounds, "min_window_s": args.min_window,
              "not_measured": ["a second machine", "kernel times under a profiler"], "layers": {}}
    for S in args.sizes:
        def way_a():
            return render_slice(net, plane, box, S, style=style, it=it)

        def way_b():
            return operator_chain(net, it, plane, box, S, style)

        a, (colours, sdf, valid) = way_a(), way_b()          # warm-up, and agreement
        torch.cuda.synchronize()
        # (the two ways rotate in another summation order: a cell on a face of the box may fall on either side)
        cells_inside_differ = int(((a.inside.view(-1) == 1.0) != valid.view(-1)).sum())
        inside = valid.view(-1) & (a.inside.view(-1) == 1.0)
        agree = {"cells_whose_inside_flag_differs": cells_inside_differ, "cells_inside": int(inside.sum()),
                 "sdf_max_abs_diff_inside": float((a.sdf.view(-1) - sdf)[inside].abs().max()),
                 "colour_max_abs_diff_over_cells_with_equal_band": None, "cells_with_another_band": None}
        diff = (a.rgb.view(3, -1).t() - colours)[inside].abs().max(1).values
        agree["cells_with_another_band"] = int((diff > 1e-3).sum())
        agree["colour_max_abs_diff_over_cells_with_equal_band"] = float(diff[diff <= 1e-3].max()) if bool((diff <= 1e-3).any()) else None
        del a, colours, sdf, valid, diff
        a_s, b_s = [], []
        for _ in range(args.rounds):
            a_s.append(window(way_a, args.min_window))
            b_s.append(window(way_b, args.min_window))

        def side(w):
            ms = [s * 1e3 for s, _ in w]
            med = statistics.median(ms)
            return {"ms_per_slice_median": round(med, 3), "ms_per_slice_min": round(min(ms), 3), "ms_per_slice_max": round(max(ms), 3),
                    "mcells_per_s": round(S * S / med / 1e3, 3), "windows_ms": [round(m, 3) for m in ms], "slices_per_window": [n for _, n in w]}

        result["layers"][str(S)] = {"cells": S * S, "render_slice": side(a_s), "operator_chain": side(b_s), "agreement": agree}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
