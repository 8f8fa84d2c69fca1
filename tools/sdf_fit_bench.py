"""SDF fitting from oriented points (permuto_sdf_amd/sdf_fit.py): speed of the step, time of the two kernels, quality of a fit.

Workload: the cloud of an analytic torus (major radius 0.3, minor 0.12, 20 000 points with outward normals) in the box
[-0.5, 0.5]^3, at the reference's batch (3 000 surface + 30 000 off-surface points, 24 lattice levels).

  * steps per second of the hand-written step and of the same step as an autograd graph over the operators the package had before
    (`SdfFitter(hand_written=False)`): after a warm-up of both, windows of --window steps each, the two fitters ALTERNATING, a
    host clock around work that ends in a device synchronise; median and spread over --repeats windows;
  * time per call of psdf_sdf_fit_batch and psdf_sdf_fit_loss (loss = two launches) at that batch: device events around --calls
    back-to-back calls, so launch gaps are inside it;
  * the fit carried through: --fit-steps steps of both fitters from the same seed (lr 1e-3), mean |sdf| on 5 000 held-out surface points,
    MeshExtractor at --grid^3, and mesh_eval's nearest-neighbour distances between the mesh's surface samples and 200 000 points
    of the analytic torus (both directions, mean below max_dist) -- plus the same held-out error at the step count, seed,
    coarse-to-fine length and learning rate of tests/test_gpu_sdf_fit.py, and at the reference's rate, each with its spread over
    the last 20 steps (at 1e-3 the field's offset moves by about the rate per step: one step's value is a sample of that).

    python tools/sdf_fit_bench.py --out profiles/sdf_fit_bench.json --parity-out profiles/sdf_fit_parity.json
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from permuto_sdf_amd import mesh_eval as me                    # noqa: E402
from permuto_sdf_amd import sdf_fit as sf                      # noqa: E402

R_MAJOR, R_MINOR = 0.3, 0.12


def torus(count, seed, dev):
    gen = torch.Generator().manual_seed(seed)
    u, v = (torch.rand(count, generator=gen, dtype=torch.float64) * 2 * math.pi for _ in range(2))
    ring = R_MAJOR + R_MINOR * torch.cos(v)
    p = torch.stack([ring * torch.cos(u), ring * torch.sin(u), R_MINOR * torch.sin(v)], 1)
    n = torch.stack([torch.cos(v) * torch.cos(u), torch.cos(v) * torch.sin(u), torch.sin(v)], 1)
    return p.float().to(dev), n.float().to(dev)


def spread(values):
    return {"median": round(statistics.median(values), 3), "min": round(min(values), 3), "max": round(max(values), 3)}


def window(fitter, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fitter.step()
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def per_call_us(fn, calls):
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def fit_pair(cloud, held_out, steps, c2f, seed, lr=1e-3):
    """-> {name: (fitter, first-five loss mean, last-ten loss mean, held-out mean |sdf| after the last step, its min / median / max
    over the last 20 steps)}"""
    out = {}
    for name, hw in (("hand_written", True), ("autograd", False)):
        f = sf.SdfFitter(cloud, nr_iters_for_c2f=c2f, hand_written=hw, seed=seed, lr=lr)
        losses, errs = [], []
        for i in range(steps):
            losses.append(f.step())
            if i >= steps - 20:
                errs.append(f.surface_error(held_out))
        losses, errs = torch.cat(losses).cpu().double(), torch.stack(errs).cpu().double()
        out[name] = (f, float(losses[:5].mean()), float(losses[-10:].mean()), float(errs[-1]),
                     {"min": float(errs.min()), "median": float(errs.median()), "max": float(errs.max())})
    return out


def short_record(pair):
    return {k: {"loss_first_five": v[1], "loss_last_ten": v[2], "held_out_mean_abs_sdf": v[3], "held_out_over_last_20_steps": v[4]}
            for k, v in pair.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--fit-steps", type=int, default=2000)
    ap.add_argument("--fit-c2f", type=int, default=1000, help="nr_iters_for_c2f of the long fit")
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--max-dist", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parity-out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cloud = sf.OrientedCloud(*torus(20000, 1, dev))
    held_out, _ = torus(5000, 99, dev)

    # ---- steps per second, the two fitters alternating
    fitters = {"hand_written": sf.SdfFitter(cloud, hand_written=True, seed=0), "autograd": sf.SdfFitter(cloud, hand_written=False, seed=0)}
    for f in fitters.values():
        window(f, args.warmup)
    rates = {k: [] for k in fitters}
    for _ in range(args.repeats):
        for k, f in fitters.items():
            rates[k].append(window(f, args.window))
    speed = {k: spread(v) for k, v in rates.items()}

    # ---- the two kernels at the reference's batch
    f = fitters["hand_written"]
    idx, u = f.draw()
    points, normals = sf.sdf_fit_batch_raw(cloud, idx, u, f.box_lo, f.box_hi)
    g = torch.Generator(device=dev).manual_seed(3)
    sdf = (torch.rand(points.shape[0], generator=g, device=dev) - 0.5) * 0.2
    grads = torch.nn.functional.normalize(torch.randn(points.shape[0], 3, generator=g, device=dev), dim=1) * 1.1
    ws = torch.empty(sf.plan(f.n_surf, f.n_off)[1] // 8, dtype=torch.float64, device=dev)
    terms, loss = torch.empty(4, device=dev), torch.zeros(1, device=dev)
    kernels = {
        "psdf_sdf_fit_batch_us_per_call": round(per_call_us(lambda: sf.sdf_fit_batch_raw(cloud, idx, u, f.box_lo, f.box_hi), args.calls), 2),
        "psdf_sdf_fit_loss_us_per_call": round(per_call_us(lambda: sf.sdf_fit_loss_raw(sdf, grads, normals, f.n_surf, loss=loss, workspace=ws,
                                                                                      terms=terms), args.calls), 2)}
    del fitters, f

    # ---- the fit carried through
    quality = {}
    long_fit = fit_pair(cloud, held_out, args.fit_steps, args.fit_c2f, seed=3)
    gt, _ = torus(200000, 7, dev)
    for name, (f, first, last, err, _) in long_fit.items():
        mesh = f.extractor().extract(args.grid, -0.5, 0.5)
        h = 1.0 / (args.grid - 1)
        samples = me.sample_surface(mesh.V, mesh.F, h)
        d2s, _ = me.nearest(samples, gt, args.max_dist)
        s2d, _ = me.nearest(gt, samples, args.max_dist)
        m_d2s, m_s2d = float(d2s[d2s < args.max_dist].double().mean()), float(s2d[s2d < args.max_dist].double().mean())
        quality[name] = {"loss_first_five": first, "loss_last_ten": last, "held_out_mean_abs_sdf": err, "vertices": int(mesh.V.shape[0]),
                         "faces": int(mesh.F.shape[0]), "mean_mesh_to_torus": m_d2s, "mean_torus_to_mesh": m_s2d,
                         "chamfer": (m_d2s + m_s2d) / 2, "share_mesh_samples_within_max_dist": float((d2s < args.max_dist).double().mean())}
    del long_fit
    short = fit_pair(cloud, held_out, 300, 150, seed=3, lr=1e-4)       # tests/test_gpu_sdf_fit.py: STEPS, C2F, seed, FIT_LR
    jitter = fit_pair(cloud, held_out, 300, 150, seed=3, lr=1e-3)      # the same at the reference's rate: what one step's value is worth
    parity = {"tool": "sdf_fit_bench", "device": torch.cuda.get_device_name(0),
              "test_configuration": {"steps": 300, "nr_iters_for_c2f": 150, "seed": 3, "lr": 1e-4, **short_record(short)},
              "test_configuration_at_reference_lr": {"steps": 300, "nr_iters_for_c2f": 150, "seed": 3, "lr": 1e-3, **short_record(jitter)},
              "long_fit": {"steps": args.fit_steps, "nr_iters_for_c2f": args.fit_c2f, "seed": 3, "grid": args.grid, "max_dist": args.max_dist,
                           **quality}}
    result = {"tool": "sdf_fit_bench", "device": torch.cuda.get_device_name(0), "n_surf": 3000, "n_off": 30000, "levels": 24,
              "warmup_steps": args.warmup, "window_steps": args.window, "repeats": args.repeats,
              "steps_per_second": speed,
              "hand_written_over_autograd_median": round(speed["hand_written"]["median"] / speed["autograd"]["median"], 3),
              "kernel_calls_timed": args.calls, **kernels}
    for line, path in ((json.dumps(result), args.out), (json.dumps(parity), args.parity_out)):
        print(line)
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
