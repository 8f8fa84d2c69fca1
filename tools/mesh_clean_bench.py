"""Stage times of the mesh cleaning on the device (permuto_sdf_amd/mesh_clean.py).

Workload: a sphere mesh of about 10^6 triangles (marching tetrahedra of an analytic volume) plus debris -- a few dozen small
spheres around it, some inside the silhouettes and some outside; 64 views of 1200 x 1600 on a sphere around the scene whose masks
are the large sphere's silhouette; the protocol's 101-row ellipse.  Per stage the time between two device events around the
stage's launches alone (the entries are called as permuto_sdf_amd/mesh_clean.py calls them; the allocations and the host reads sit
outside the events, except in `filter`, whose one host read between its count and emit passes is part of the stage) and the
wall clock; median and spread over the repeats after the warm-up.  Next to the times: the counts the design argues with -- bytes
moved and row tests of the dilation, H W (2 r + 1) per view, projections of the vertex test -- and the rates they give; and the
wall time of the yardstick's host chain (tests/mesh_clean_reference.py, numpy) on the same input, as context: there is no earlier
time of this project to compare with.  The results of the two chains are compared as well.  One JSON line on stdout; --out
writes it to a file.

    python tools/mesh_clean_bench.py --out profiles/mesh_clean_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from permuto_sdf_amd import _lib as L                           # noqa: E402
from permuto_sdf_amd import mesh_clean as mc                    # noqa: E402
from permuto_sdf_amd.mesh import ExtractedMesh, marching_tetrahedra    # noqa: E402


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
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def look_at(c):
    c = np.asarray(c, dtype=np.float64)
    z = -c / np.linalg.norm(c)
    up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z]), c


def scene(args, dev):
    """-> (V, F, world_mats [n, 4, 4] float64 numpy, masks [n, H, W] uint8 on the device)"""
    r = np.random.default_rng(3)
    n = args.grid
    axis = torch.linspace(-args.half, args.half, n, device=dev)
    x, y, z = torch.meshgrid(axis, axis, axis, indexing="ij")
    sdf = torch.sqrt(x * x + y * y + z * z) - args.radius
    for _ in range(args.debris):
        c = r.standard_normal(3)
        c *= r.uniform(args.radius + 0.05, args.half - 0.05) / np.linalg.norm(c)
        sdf = torch.minimum(sdf, torch.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - 0.03)
    del x, y, z
    h = 2.0 * args.half / (n - 1)
    V, F, _, _ = marching_tetrahedra(sdf, 0.0, spacing=(h, h, h), normals=False)
    del sdf
    V = (V - args.half).contiguous()
    H, W, views, distance = args.height, args.width, args.views, 3.0
    focal = 0.8 * min(H, W) / 2 * distance / args.half      # a ball of radius `half` would fill 80 % of the shorter side
    K = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1.0]])
    P = np.zeros((views, 4, 4))
    masks = torch.zeros((views, H, W), dtype=torch.uint8, device=dev)
    vv, uu = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    for i in range(views):
        d = r.standard_normal(3)
        R, c = look_at(d / np.linalg.norm(d) * distance)
        P[i, :3, :3], P[i, :3, 3], P[i, 3, 3] = K @ R, K @ (-R @ c), 1.0
        # the large sphere's silhouette: a disc around the principal point, tan(asin(radius / distance)) focal wide
        disc = focal * np.tan(np.arcsin(args.radius / distance))
        masks[i] = torch.where((uu - W / 2) ** 2 + (vv - H / 2) ** 2 <= disc * disc, 255, 0).to(torch.uint8)
    return V, F, P, masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=350, help="points per axis of the analytic volume (350: about 10^6 triangles)")
    ap.add_argument("--radius", type=float, default=0.8)
    ap.add_argument("--half", type=float, default=1.25, help="half the side of the volume")
    ap.add_argument("--debris", type=int, default=40)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--ksize", type=int, default=101)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-host-chain", action="store_true", help="skip the numpy chain (minutes at the default size)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_clean_bench: no GPU visible; a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    V, F, P, masks = scene(args, dev)
    nV, nF = V.shape[0], F.shape[0]
    views, H, W = masks.shape
    hw = mc.ellipse_half_widths(args.ksize)
    plan = mc.dilate_plan(views, H, W, hw)
    hw_arr = (L.c_i * len(hw))(*hw)
    mats = torch.from_numpy(P[:, :3, :]).to(dev).contiguous()

    names = ("row_distance", "dilation", "vertex_test", "filter", "edge_keys", "sort", "link", "flatten")
    stages = {k: {"device_ms": [], "wall_ms": []} for k in names}
    info = {}
    for it in range(args.warmup + args.repeats):
        hd = torch.empty((views, H, W), dtype=torch.uint8, device=dev)
        words = torch.empty((views, H, plan["words_per_row"]), dtype=torch.int32, device=dev)
        keep8 = torch.empty(nV, dtype=torch.uint8, device=dev)
        t = {}
        _, *t["row_distance"] = timed(lambda: L.call("psdf_mesh_clean_row_distance", L.ptr(masks), L.c_l(views), L.c_i(H), L.c_i(W),
                                                      L.c_i(128), L.ptr(hd), L.stream()))
        _, *t["dilation"] = timed(lambda: L.call("psdf_mesh_clean_dilate", L.ptr(hd), L.c_l(views), L.c_i(H), L.c_i(W), hw_arr,
                                                  L.c_i(len(hw)), L.ptr(words), L.stream()))
        _, *t["vertex_test"] = timed(lambda: L.call("psdf_mesh_clean_inside_masks", L.ptr(V), L.c_l(nV), L.ptr(mats), L.c_i(views),
                                                     L.ptr(words), L.c_i(H), L.c_i(W), L.ptr(keep8), L.stream()))
        keep = keep8.to(torch.bool)
        culled, *t["filter"] = timed(lambda: mc.filter_vertices((V, F), keep))
        F2, nV2, nF2 = culled.F, culled.V.shape[0], culled.F.shape[0]
        keys = torch.empty(3 * nF2, dtype=torch.int64, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        parent = torch.arange(nF2, dtype=torch.int32, device=dev)
        labels = torch.empty(nF2, dtype=torch.int32, device=dev)
        sizes = torch.zeros(nF2, dtype=torch.int32, device=dev)
        _, *t["edge_keys"] = timed(lambda: L.call("psdf_mesh_clean_edge_keys", L.ptr(F2), L.c_l(nF2), L.c_l(nV2), L.ptr(keys), L.ptr(flag),
                                                   L.stream()))
        (skeys, slot), *t["sort"] = timed(lambda: torch.sort(keys, stable=True))
        _, *t["link"] = timed(lambda: L.call("psdf_mesh_clean_link_edges", L.ptr(skeys), L.ptr(slot), L.c_l(nF2), L.ptr(parent), L.ptr(flag),
                                              L.stream()))
        _, *t["flatten"] = timed(lambda: L.call("psdf_mesh_clean_flatten", L.ptr(parent), L.c_l(nF2), L.ptr(labels), L.ptr(sizes),
                                                 L.ptr(flag), L.stream()))
        if int(flag):
            raise SystemExit("mesh_clean_bench: the error flag reads %d" % int(flag))
        if it >= args.warmup:
            for k in names:
                stages[k]["device_ms"].append(t[k][0])
                stages[k]["wall_ms"].append(t[k][1])
        info = {"vertices": nV, "triangles": nF, "vertices_after_masks": nV2, "triangles_after_masks": nF2,
                "components_after_masks": int((sizes > 0).sum()), "largest_component_faces": int(sizes.max()) if nF2 else 0,
                "mask_pixels_set_share": round(float((masks > 128).double().mean()), 4)}
    info["dilated_pixels_set_share"] = round(float(mc.PackedMasks(words, H, W).unpack().double().mean()), 4)
    # the public chain once more, end to end (its own allocations and host reads inside)
    whole = [timed(lambda: mc.clean_mesh_dtu(ExtractedMesh(V, F), P, masks, ksize=args.ksize))[1:] for _ in range(3)]
    out_mesh = mc.clean_mesh_dtu(ExtractedMesh(V, F), P, masks, ksize=args.ksize)

    r = (len(hw) - 1) // 2
    counts = {"row_distance_bytes": 2 * views * H * W,                            # the masks read, the distances written
              "dilation_row_tests": views * H * W * (2 * r + 1),                  # the bound: a lane stops at its first hit
              "dilation_bytes": views * H * W + 4 * views * H * plan["words_per_row"],
              "vertex_test_projections": nV * views,                             # the bound: a culled vertex stops
              "packed_mask_bytes": 4 * views * H * plan["words_per_row"],
              "half_edges": 3 * info["triangles_after_masks"]}
    med = {k: statistics.median(v["device_ms"]) * 1e-3 for k, v in stages.items()}
    rates = {"row_distance_GB_per_s": round(counts["row_distance_bytes"] / med["row_distance"] / 1e9, 2),
             "dilation_row_tests_per_s_bound": round(counts["dilation_row_tests"] / med["dilation"], 0),
             "dilation_GB_per_s": round(counts["dilation_bytes"] / med["dilation"] / 1e9, 2),
             "vertex_test_projections_per_s_bound": round(counts["vertex_test_projections"] / med["vertex_test"], 0),
             "half_edges_linked_per_s": round(counts["half_edges"] / med["link"], 0)}
    result = {"tool": "mesh_clean_bench", "device": torch.cuda.get_device_name(0), "views": views, "height": H, "width": W,
              "ksize": args.ksize, "warmup": args.warmup, "repeats": args.repeats, "plan": plan, **info,
              "stages": {k: {m: spread(v) for m, v in s.items()} for k, s in stages.items()},
              "sum_of_stage_device_ms_median": round(sum(statistics.median(s["device_ms"]) for s in stages.values()), 3),
              "clean_mesh_dtu_device_ms_incl_host_reads": spread([w[0] for w in whole]),
              "clean_mesh_dtu_wall_ms": spread([w[1] for w in whole]),
              "result_vertices": int(out_mesh.V.shape[0]), "result_triangles": int(out_mesh.F.shape[0]), "stats": out_mesh.stats,
              "counts": counts, "rates": rates}

    if not args.no_host_chain:
        from tests import mesh_clean_reference as ref
        Vh, Fh, Mh = V.cpu().numpy(), F.cpu().numpy(), masks.cpu().numpy()
        t0 = time.perf_counter()
        parts = []
        for i in range(views):                                                   # view by view: memory
            parts.append(ref.dilate(ref.threshold(Mh[i:i + 1]), hw))
            if i % 8 == 7:
                print("host chain: %d of %d views dilated, %.0f s" % (i + 1, views, time.perf_counter() - t0), file=sys.stderr, flush=True)
        dilated = np.concatenate(parts)
        t1 = time.perf_counter()
        keep_h = ref.inside_masks(Vh, P, dilated)
        t2 = time.perf_counter()
        V2, F2h = ref.filter_vertices(Vh, Fh, keep_h)[:2]
        t3 = time.perf_counter()
        V3, F3 = ref.largest_component(V2, F2h)
        t4 = time.perf_counter()
        result["yardstick_host_chain_wall_ms"] = {"dilation": round((t1 - t0) * 1e3, 1), "vertex_test": round((t2 - t1) * 1e3, 1),
                                                  "filter": round((t3 - t2) * 1e3, 1), "largest_component": round((t4 - t3) * 1e3, 1),
                                                  "total": round((t4 - t0) * 1e3, 1)}
        result["equals_yardstick"] = bool(np.array_equal(out_mesh.V.cpu().numpy(), V3) and np.array_equal(out_mesh.F.cpu().numpy(), F3))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
