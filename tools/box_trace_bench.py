"""Time of one traced view of a fitted 4-D SDF at the workload of the reference's viewer
(permuto_sdf_py/experiments/visualization/vis_4d_sdf.py:91-105: 800 x 510 pixels, 40 iterations, multiplier 0.3, threshold 2e-3,
100 time values), three ways in one process:

  (a) `BoxPlayer.frame_at(t)`: rays, trace and resolve captured once; one fill of the time and one graph replay per frame;
  (b) `render_box_traced(..., time_val=t)`: the same launches issued eagerly;
  (c) the reference's loop restated over the operators the tree had before: the box intersection in torch, boolean-mask
      compaction of the unconverged rays, `torch.cat` of the time column, the net's forward per iteration, `sdf_and_gradient` at
      the end points, filter_unconverged_points, `F.normalize`, the transposes into planes.

The net is an `SdfFitter` 4-D fit of a few hundred steps to a sphere of radius 0.25 whose centre moves along x with time: nothing
here is a trained scene.  The ways alternate; a pass over a few time values warms each up first; a timed window is whole frames
(the time value advances every frame through the 100 values), repeated until at least `--min-window` seconds have passed, between
two host clocks with a device synchronise before each.  One JSON line on stdout; --out writes it to a file as well.

    python tools/box_trace_bench.py --out profiles/box_trace_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from permuto_sdf_amd import render, sdf_fit                                                   # noqa: E402
from permuto_sdf_amd.box_trace import Box, BoxPlayer, render_box_traced                       # noqa: E402

TRACE = dict(nr_sphere_traces=40, sdf_multiplier=0.3, sdf_converged_tresh=2e-3)      # vis_4d_sdf.py:105
NR_TIMES = 100                                                                        # vis_4d_sdf.py:82


def moving_sphere_cloud(dev, n=200000, seed=0):
    g = torch.Generator().manual_seed(seed)
    nrm = F.normalize(torch.randn(n, 3, generator=g), dim=1)
    t = torch.rand(n, 1, generator=g)
    centre = torch.cat([0.2 * (t - 0.5), torch.zeros(n, 2)], 1)
    return sdf_fit.OrientedCloud(torch.cat([centre + 0.25 * nrm, t], 1).to(dev), nrm.to(dev))


def torch_ray_intersection(box, o, d):
    """aabb.py:47-100 as the reference writes it -> (entry points, hit)"""
    bb_min, bb_max = torch.as_tensor(box.bb_min, device=o.device), torch.as_tensor(box.bb_max, device=o.device)
    lo = -torch.ones_like(o[:, 0:1]) * 1e10
    hi = torch.ones_like(o[:, 0:1]) * 1e10
    invalid = torch.zeros_like(o[:, 0:1]).bool()
    for i in range(3):
        dim_lo = ((bb_min[i] - o[:, i]) / d[:, i]).unsqueeze(-1)
        dim_hi = ((bb_max[i] - o[:, i]) / d[:, i]).unsqueeze(-1)
        swap = dim_lo > dim_hi
        dim_lo, dim_hi = torch.where(swap, dim_hi, dim_lo), torch.where(swap, dim_lo, dim_hi)
        invalid = invalid | (dim_hi < lo) | (dim_lo > hi)
        lo = torch.where(dim_lo > lo, dim_lo, lo)
        hi = torch.where(dim_hi < hi, dim_hi, hi)
    lo = torch.clamp(torch.where(invalid, torch.zeros_like(lo), lo), min=0.0)
    return o + lo * d, torch.logical_not(invalid)


def operator_chain(net, box, frame, it, t):
    """(c) -> normals [3, H, W], alpha [1, H, W]: sdf_utils.py:120-231 and vis_4d_sdf.py:101-118"""
    H, W = frame.height, frame.width
    o, d = render.frame_rays(frame)
    n_iter, mult, thr = TRACE["nr_sphere_traces"], TRACE["sdf_multiplier"], TRACE["sdf_converged_tresh"]

    def timed(p):
        time_tensor = torch.empty((p.shape[0], 1), device=p.device)
        time_tensor.fill_(t)
        return torch.cat([p, time_tensor], 1)

    with torch.no_grad():
        pts, _ = torch_ray_intersection(box, o, d)
        pts = pts.clone()
        conv = torch.zeros_like(pts)[:, 0:1].bool()
        for _ in range(n_iter):
            sel = torch.logical_not(conv)
            pu = pts[sel.repeat(1, 3)].view(-1, 3)
            du = d[sel.repeat(1, 3)].view(-1, 3)
            if pu.shape[0] == 0:
                break
            sdf, _ = net(timed(pu), it)
            pu = pu + du * sdf * mult
            conv[sel] = torch.logical_or(conv[sel], (sdf.abs() < thr).view(-1))
            conv = conv.view(-1, 1)
            within = box.check_point_inside_primitive(pu)
            conv[sel] = torch.logical_or(conv[sel], torch.logical_not(within.view(-1)))
            conv = conv.view(-1, 1)
            pts[sel.repeat(1, 3)] = pu.view(-1)
    sdf, grad, _ = net.sdf_and_gradient(timed(pts), it)
    with torch.no_grad():
        grad = grad.detach()[:, 0:3]
        is_converged = (sdf.detach() < 0.01) * 1.0
        normal = F.normalize(grad * is_converged, dim=1)
        return normal.view(H, W, 3).permute(2, 0, 1).contiguous(), is_converged.view(H, W, 1).permute(2, 0, 1).contiguous()


def window(fn, min_seconds, clock):
    """-> (seconds per frame, frames) over whole frames until min_seconds have passed; ends in a synchronise"""
    torch.cuda.synchronize()
    t0, frames = time.perf_counter(), 0
    while True:
        fn(clock[0] % NR_TIMES / NR_TIMES)
        clock[0] += 1
        frames += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return dt / frames, frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=510)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--fit-steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per way, alternating")
    ap.add_argument("--min-window", type=float, default=0.5, help="seconds")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("box_trace_bench measures a device: no GPU is visible, nothing is measured")
    dev = torch.device("cuda:0")
    H, W = args.height, args.width
    fitter = sdf_fit.SdfFitter(moving_sphere_cloud(dev))
    for _ in range(args.fit_steps):
        fitter.step()
    torch.cuda.synchronize()
    net, it, box = fitter.net, fitter.iter, Box([1.0, 1.0, 1.0], [0.0, 0.0, 0.0])     # vis_4d_sdf.py:62
    surface_error = float(fitter.surface_error(moving_sphere_cloud(dev, 20000, seed=1).points))
    K = torch.tensor([[1.1 * W, 0.0, W / 2], [0.0, 1.1 * W, H / 2], [0.0, 0.0, 1.0]])
    tf = torch.eye(4)
    tf[:3, 3] = torch.tensor([0.0, 0.0, -1.8])
    frame = render.Frame(K.to(dev), tf.to(dev), H, W)
    player = BoxPlayer(net, box, frame, it=it, **TRACE)

    def way_a(t):
        return player.frame_at(t)

    def way_b(t):
        return render_box_traced(net, box, frame, it=it, time_val=t, **TRACE)

    def way_c(t):
        return operator_chain(net, box, frame, it, t)

    # warm-up and agreement at a few time values
    same, covered = True, []
    for t in (0.0, 0.37, 0.99):
        a, b, c = way_a(t), way_b(t), way_c(t)
        torch.cuda.synchronize()
        same = same and all(torch.equal(getattr(a, n), getattr(b, n)) for n in ("normals", "weights_sum", "depth"))
        covered.append(float(a.weights_sum.mean()))
        alpha_agrees = float((a.weights_sum == c[1]).float().mean())
    a_s, b_s, c_s = [], [], []
    clock = [0]
    for _ in range(args.rounds):
        a_s.append(window(way_a, args.min_window, clock))
        b_s.append(window(way_b, args.min_window, clock))
        c_s.append(window(way_c, args.min_window, clock))
    a_ms, b_ms, c_ms = (statistics.median(s for s, _ in w) * 1e3 for w in (a_s, b_s, c_s))

    def side(ms, w):
        return {"ms_per_frame": round(ms, 3), "mrays_per_s": round(H * W / ms / 1e3, 3), "windows_ms": [round(s * 1e3, 3) for s, _ in w],
                "frames_per_window": [n for _, n in w]}

    result = {"tool": "box_trace_bench", "device": torch.cuda.get_device_name(0), "height": H, "width": W, "fit_steps": args.fit_steps,
              "fit_surface_error": round(surface_error, 5), "trace": TRACE, "nr_time_values": NR_TIMES, "rounds": args.rounds,
              "min_window_s": args.min_window, "pixels_covered": [round(c, 4) for c in covered],
              "player_frame_at": side(a_ms, a_s), "render_box_traced": side(b_ms, b_s), "operator_chain": side(c_ms, c_s),
              "player_over_eager": round(b_ms / a_ms, 3), "player_over_operator_chain": round(c_ms / a_ms, 3),
              "player_bit_identical_to_eager": bool(same), "alpha_agreement_with_the_operator_chain": round(alpha_agrees, 5)}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
