"""Time of one sphere-traced 1920 x 1080 view (permuto_sdf_amd/render.py: render_traced) on a sphere-fitted trainer, two ways in one
process:

  (a) `FrameRenderer.render_traced`: per chunk one select call (predicate + compaction in ray order) and one resolve launch
      straight into the image planes;
  (b) the same image from the operators the tree had before: `SphereTracer.trace`, `check_occupancy`,
      `check_point_inside_primitive`, boolean-mask gathers, the two networks, `F.normalize`, `index_put` into zero planes (the
      yardstick of tests/test_gpu_frame_trace.py).

Both run the same trace and the same networks on the same chunks (one chunk at the default); what differs is the work around
them.  The tracer's own share is printed too: `SphereTracer.trace` alone on the frame's rays.  The ways alternate; one whole frame
of each warms up first; a timed window is whole frames, repeated until at least `--min-window` seconds have passed, between two
host clocks with a device synchronise before each.  The scene is the trainer's sphere fit and a few main-phase iterations on a
SyntheticReel: nothing here is a trained scene.  One JSON line on stdout; --out writes it to a file as well.

    python tools/frame_trace_bench.py --out profiles/frame_trace_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from permuto_sdf_amd import render                                               # noqa: E402
from permuto_sdf_amd.sphere_trace import SphereTracer                            # noqa: E402
from permuto_sdf_amd.train_step import HyperParams, SyntheticReel, Trainer      # noqa: E402

IT = 9999999
TRACE = (15, 0.9, 2e-4)         # render_from_frame.py:335


def tracer_of(tr):
    return SphereTracer(tr.sdf.encoding, tr.sdf.mlp_sdf, tr.grid, tr.sphere, tr.sdf.window(IT).float())


def traced_by_the_operator_chain(tr, rnd, frame, max_rays):
    """(b) -> rgb, normals, weights_sum, depth as [C, H, W]"""
    dev = frame.K.device
    H, W = frame.height, frame.width
    plan = render.FramePlan(H, W, 1, max_rays)
    tracer = tracer_of(tr)
    rows = [torch.zeros(H * W, c, device=dev) for c in (3, 3, 1, 1)]
    with torch.no_grad():
        for first, count in plan.chunks():
            o, d = render.frame_rays(frame, first, count)
            pts = tracer.trace(o, d, *TRACE, return_gradients=False)[0]
            valid = (~tracer.no_hit) & tr.grid.check_occupancy(pts).view(-1) & tr.sphere.check_point_inside_primitive(pts).view(-1)
            if not bool(valid.any()):
                continue
            p, dd, oo = pts[valid], d[valid], o[valid]
            _, grad, feat = rnd._sdf_and_gradient(p, IT)
            rgb = tr.rgb(p, dd, grad, feat)
            q = p - oo
            depth = (q[:, 0] * dd[:, 0] + q[:, 1] * dd[:, 1]) + q[:, 2] * dd[:, 2]
            idx = (torch.nonzero(valid).view(-1) + first,)
            rows[0].index_put_(idx, rgb.float())
            rows[1].index_put_(idx, torch.nn.functional.normalize(grad.float(), dim=1))
            rows[2].index_put_(idx, torch.ones(p.shape[0], 1, device=dev))
            rows[3].index_put_(idx, depth.view(-1, 1))
    return [r.t().reshape(-1, H, W).contiguous() for r in rows]


def window(fn, min_seconds):
    """-> (seconds per frame, frames) over whole frames until min_seconds have passed; ends in a synchronise"""
    torch.cuda.synchronize()
    t0, frames = time.perf_counter(), 0
    while True:
        fn()
        frames += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return dt / frames, frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--sphere-iters", type=int, default=200)
    ap.add_argument("--train-iters", type=int, default=16)
    ap.add_argument("--max-rays-per-chunk", type=int, default=render.OccupancyGrid.POOL)
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per way, alternating")
    ap.add_argument("--min-window", type=float, default=0.5, help="seconds")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frame_trace_bench measures a device: no GPU is visible, nothing is measured")
    dev = torch.device("cuda:0")
    H, W = args.height, args.width
    hp = HyperParams()
    hp.nr_iter_sphere_fit = args.sphere_iters
    reel = SyntheticReel(dev, nr_images=2, height=H, width=W)
    tr = Trainer(dev, hp=hp, reference_schedule=True, nr_images=2)
    for _ in range(args.sphere_iters + args.train_iters):
        tr.step(reel)
    torch.cuda.synchronize()
    frame = render.Frame.from_reel(reel, 0)
    rnd = render.FrameRenderer(tr)
    plan = render.FramePlan(H, W, 1, args.max_rays_per_chunk)
    o_all, d_all = render.frame_rays(frame)
    tracer = tracer_of(tr)

    def way_a():
        return rnd.render_traced(frame, max_rays_per_chunk=args.max_rays_per_chunk)

    def way_b():
        return traced_by_the_operator_chain(tr, rnd, frame, args.max_rays_per_chunk)

    def trace_alone():
        with torch.no_grad():
            return tracer.trace(o_all, d_all, *TRACE, return_gradients=False)

    # warm-up: one whole frame of each (every chunk shape, the allocator's blocks, the pinned landing zone)
    a, b = way_a(), way_b()
    trace_alone()
    torch.cuda.synchronize()
    same = {"rgb": torch.equal(a.rgb, b[0]), "weights_sum": torch.equal(a.weights_sum, b[2]), "depth": torch.equal(a.depth, b[3])}
    normals_diff = float((a.normals - b[1]).abs().max())
    covered = float(a.weights_sum.mean())
    a_s, b_s, t_s = [], [], []
    for _ in range(args.rounds):
        a_s.append(window(way_a, args.min_window))
        b_s.append(window(way_b, args.min_window))
        t_s.append(window(trace_alone, args.min_window))
    a_ms, b_ms, t_ms = (statistics.median(s for s, _ in w) * 1e3 for w in (a_s, b_s, t_s))
    b_windows = [s * 1e3 for s, _ in b_s]
    b_spread = max(b_windows) - min(b_windows)

    def side(ms, w):
        return {"ms_per_frame": round(ms, 3), "mrays_per_s": round(H * W / ms / 1e3, 3), "windows_ms": [round(s * 1e3, 3) for s, _ in w],
                "frames_per_window": [n for _, n in w]}

    result = {"tool": "frame_trace_bench", "device": torch.cuda.get_device_name(0), "height": H, "width": W,
              "sphere_iters": args.sphere_iters, "train_iters": args.train_iters, "rounds": args.rounds,
              "min_window_s": args.min_window, "chunks": plan.nr_chunks, "rays_per_chunk": plan.rays_per_chunk,
              "pixels_hit": round(covered, 4), "render_traced": side(a_ms, a_s), "operator_chain": side(b_ms, b_s),
              "sphere_trace_alone": side(t_ms, t_s), "operator_chain_window_spread_ms": round(b_spread, 3),
              "speedup": round(b_ms / a_ms, 3), "faster_by_more_than_the_spread": bool(b_ms - a_ms > b_spread),
              "bit_identical_to_the_operator_chain": same, "normals_max_abs_difference": normals_diff}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
