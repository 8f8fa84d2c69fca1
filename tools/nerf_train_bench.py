"""NeRF training (permuto_sdf_amd/nerf_train.py): speed of the step in both forms, time of the new kernels against the unfused chain.

Workload: a SyntheticReel of random images (49 cameras of 300 x 400 on a sphere of radius 1.5), the reference's batch
(train_nerf.py:45-55: 512 rays, at most 64 foreground samples per ray in a 64^3 occupancy grid, 32 background samples, two
24-level lattices), with the background net and under --with_mask.

  * steps per second of the hand-written step and of the same step as an autograd graph over the operators the package had before
    (`NerfTrainer(hand_written=False)`): after a warm-up of both, windows of --window steps each, the two trainers ALTERNATING, a
    host clock around work that ends in a device synchronise; median and spread over --repeats windows.  A step includes its
    sampling, its one host synchronisation (the march's sample count) and every 8th its grid refresh;
  * time per call, at the foreground container of a step (512 rays, its sample count is recorded) and at 16 384 rays x 64 samples:
    psdf_nerf_render_forward / _backward against the unfused chain nerf_alpha -> cumprod -> multiply -> integrate ->
    sum_over_each_ray forward and, through autograd, backward; psdf_nerf_loss (two launches) against `nerf_loss_torch` forward and
    forward + backward; psdf_nerf_head_join / _backward against gelu + t() + cat and gelu_backward + cat.  Device events around
    --calls back-to-back calls, so launch gaps are inside it; each pair ALTERNATES --repeats times, median and spread.

    python tools/nerf_train_bench.py --out profiles/nerf_train_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from permuto_sdf_amd import nerf_train as nt                                   # noqa: E402
from permuto_sdf_amd.bridge import PermutoSDF, RaySamplesPacked               # noqa: E402
from permuto_sdf_amd.neus import nerf_alpha                                    # noqa: E402
from permuto_sdf_amd.train_step import SyntheticReel, _Cumprod, _Integrate, _SumRay   # noqa: E402


def spread(values, digits=2):
    return {"median": round(statistics.median(values), digits), "min": round(min(values), digits), "max": round(max(values), digits)}


def window(trainer, reel, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        trainer.step(reel)
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


def alternate(fns, calls, repeats):
    """{name: fn} -> {name: spread of microseconds per call}, the functions alternating"""
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            times[k].append(per_call_us(fn, calls))
    return {k: spread(v) for k, v in times.items()}


def equal_container(R, n, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    rs = RaySamplesPacked(R, R * n, device=dev)
    rs.rays_have_equal_nr_of_samples, rs.fixed_nr_of_samples_per_ray = True, n
    start = torch.arange(R, dtype=torch.int32, device=dev).view(-1, 1) * n
    rs.ray_start_end_idx = torch.cat([start, start + n], 1).contiguous()
    rs.samples_dt = torch.rand(R * n, 1, generator=g, device=dev) * 0.02 + 1e-3
    rs.cur_nr_samples.fill_(R * n)
    return rs


def render_kernels(rs, max_per_ray, dev, calls, repeats, seed=1):
    g = torch.Generator(device=dev).manual_seed(seed)
    R, M = rs.ray_start_end_idx.shape[0], rs.samples_dt.shape[0]
    raw = torch.randn(M, generator=g, device=dev) * 2 - 1
    rgb = torch.rand(M, 3, generator=g, device=dev)
    g_pred, g_ws, g_bg = (torch.randn(R, c, generator=g, device=dev) for c in (3, 1, 1))

    def chain():
        alpha, one_minus = nerf_alpha(raw_g, rs.samples_dt)
        T, bg = _Cumprod.apply(rs, one_minus)
        w = (alpha * T).view(-1, 1)
        ws, _ = _SumRay.apply(rs, w)
        return _Integrate.apply(rs, rgb_g, w), ws, bg

    def chain_both():
        pred, ws, bg = chain()
        torch.autograd.grad([pred, ws, bg], (raw_g, rgb_g), [g_pred, g_ws.view_as(ws), g_bg.view_as(bg)])

    raw_g, rgb_g = raw.view(-1, 1), rgb
    fwd = alternate({"fused": lambda: nt.nerf_render_raw(rs, raw, rgb), "chain": lambda: torch.no_grad()(chain)()}, calls, repeats)
    raw_g, rgb_g = raw.view(-1, 1).clone().requires_grad_(True), rgb.clone().requires_grad_(True)
    both = alternate({"fused": lambda: (nt.nerf_render_raw(rs, raw, rgb), nt.nerf_render_backward_raw(rs, max_per_ray, g_pred, g_ws, g_bg, raw, rgb)),
                      "chain": chain_both}, calls, repeats)
    return {"rays": R, "samples": M, "forward_us": fwd, "forward_and_backward_us": both}


def loss_kernels(R, dev, calls, repeats):
    g = torch.Generator(device=dev).manual_seed(2)
    pred, gt = torch.rand(R, 3, generator=g, device=dev), torch.rand(R, 3, generator=g, device=dev)
    hit = (torch.rand(R, generator=g, device=dev) < 0.8)
    ws, gm = torch.rand(R, generator=g, device=dev), (torch.rand(R, generator=g, device=dev) < 0.5).float()
    work, terms, acc = torch.empty(max(1, nt.plan(R)[1] // 8), dtype=torch.float64, device=dev), torch.empty(2, device=dev), torch.zeros(1, device=dev)
    p_g, w_g = pred.clone().requires_grad_(True), ws.clone().requires_grad_(True)

    def torch_both():
        loss, _ = nt.nerf_loss_torch(p_g, gt, hit, w_g, gm)
        torch.autograd.grad(loss, (p_g, w_g))

    return {"rays": R, "value_and_gradients_us": alternate({
        "fused": lambda: nt.nerf_loss_raw(pred, gt, hit, ws, gm, loss=acc, workspace=work, terms=terms), "torch": torch_both}, calls, repeats)}


def join_kernels(M, dev, calls, repeats):
    g = torch.Generator(device=dev).manual_seed(3)
    fd, dX2, g_raw = torch.randn(65, M, generator=g, device=dev), torch.randn(80, M, generator=g, device=dev), torch.randn(M, generator=g, device=dev)
    sh = PermutoSDF.spherical_harmonics(torch.nn.functional.normalize(torch.randn(M, 3, generator=g, device=dev), dim=1), 4)
    fwd = alternate({"fused": lambda: nt.nerf_head_join_raw(fd, sh),
                     "torch": lambda: torch.cat([torch.nn.functional.gelu(fd[1:65]), sh.t()], 0)}, calls, repeats)
    bwd = alternate({"fused": lambda: nt.nerf_head_join_backward_raw(g_raw, dX2, fd),
                     "torch": lambda: torch.cat([g_raw.view(1, -1), torch.ops.aten.gelu_backward(dX2[:64], fd[1:65])], 0)}, calls, repeats)
    return {"samples": M, "forward_us": fwd, "backward_us": bwd}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--window", type=int, default=120)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    reel = SyntheticReel(dev)
    reel.has_mask = True
    reel.mask_reel[..., reel.mask_reel.shape[-1] // 2:] = 0.0

    # ---- steps per second, the two forms alternating, in both modes
    speed, samples = {}, {}
    for mode, with_mask in (("with_background", False), ("with_mask", True)):
        trainers = {"hand_written": nt.NerfTrainer(dev, with_mask=with_mask, hand_written=True, seed=0),
                    "autograd": nt.NerfTrainer(dev, with_mask=with_mask, hand_written=False, seed=0)}
        for t in trainers.values():
            window(t, reel, args.warmup)
        rates = {k: [] for k in trainers}
        for _ in range(args.repeats):
            for k, t in trainers.items():
                rates[k].append(window(t, reel, args.window))
        speed[mode] = {k: spread(v, 1) for k, v in rates.items()}
        speed[mode]["hand_written_over_autograd_median"] = round(speed[mode]["hand_written"]["median"] / speed[mode]["autograd"]["median"], 3)
        samples[mode] = {k: t.last["nr_fg_samples"] for k, t in trainers.items()}
        step_batch = trainers["hand_written"].draw(reel)
        del trainers

    # ---- the kernels against what the step did before
    kernels = {"render_at_step_container": render_kernels(step_batch.fg, 64, dev, args.calls, args.repeats),
               "render_at_16384_rays_x_64": render_kernels(equal_container(16384, 64, dev, 5), 64, dev, args.calls, args.repeats),
               "loss_at_512_rays": loss_kernels(512, dev, args.calls, args.repeats),
               "loss_at_16384_rays": loss_kernels(16384, dev, args.calls, args.repeats),
               "head_join_at_16384_samples": join_kernels(512 * 32, dev, args.calls, args.repeats),
               "head_join_at_1048576_samples": join_kernels(16384 * 64, dev, args.calls, args.repeats)}
    result = {"tool": "nerf_train_bench", "device": torch.cuda.get_device_name(0), "nr_rays": 512, "max_nr_samples_per_ray": 64,
              "nr_samples_bg": 32, "grid": 64, "warmup_steps": args.warmup, "window_steps": args.window, "repeats": args.repeats,
              "steps_per_second": speed, "foreground_samples_of_the_last_step": samples, "kernel_calls_timed": args.calls, "kernels": kernels}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
