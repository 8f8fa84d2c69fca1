"""NeRF training with the per-image colour calibration (permuto_sdf_amd/nerf_train.py, csrc/colorcal.hip): what the feature costs
and what its kernels save.

Workload and protocol of tools/nerf_train_bench.py: a SyntheticReel of random images (49 cameras of 300 x 400), the reference's
batch (512 rays, at most 64 foreground samples per ray, 32 background samples), with the background net.  All trainers live in
one process and ALTERNATE: after a warm-up of each, --repeats windows of --window steps, a host clock around work that ends in a
device synchronise; min - max over the windows.

  * steps per second of the calibrated hand-written step (`NerfTrainer(nr_images=49)`) against the calibrated autograd step
    (`hand_written=False`: Colorcal.calib_RGB_samples_packed in torch operators inside NerfNet.forward).  THE CONDITION: the
    hand-written step's slowest window beats the autograd step's fastest;
  * the same against the uncalibrated hand-written step: the cost of the feature, reported, not bounded;
  * time per call of the forward and of backward + fold at the step's own containers (foreground and background) against the
    operator chain of train_manual._calib_sigmoid / _calib_sigmoid_backward with ManualTrainer's index_add_ fold on the same
    inputs: device events around --calls back-to-back calls, so host gaps between launches are inside it; each pair alternates.

    python tools/nerf_colorcal_bench.py --out profiles/nerf_colorcal_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from permuto_sdf_amd import nerf_train as nt                                   # noqa: E402
from permuto_sdf_amd.train_manual import _calib_sigmoid, _calib_sigmoid_backward   # noqa: E402
from permuto_sdf_amd.train_step import SyntheticReel                           # noqa: E402


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
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            times[k].append(per_call_us(fn, calls))
    return {k: spread(v) for k, v in times.items()}


def chain_calib(cc, img_idx):
    """ManualTrainer._calib_build: the per-ray gain and bias of the operator chain"""
    cam = img_idx.long()
    fixed = (cam == cc.idx_with_fixed_calib)[:, None]
    cw = torch.where(fixed, torch.ones_like(cc.weight_delta[:1]), 1.0 + cc.weight_delta.index_select(0, cam))
    cb = torch.where(fixed, torch.zeros_like(cc.bias[:1]), cc.bias.index_select(0, cam))
    return SimpleNamespace(cw=cw, cb=cb, fixed=fixed, cam=cam)


@torch.no_grad()
def kernels_at(rs, M, img_idx, cc, dev, calls, repeats, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    raw_fm = torch.rand(3, M, generator=g, device=dev) * 12 - 6
    g_rgb = torch.randn(M, 3, generator=g, device=dev)
    rgb = nt.colorcal_sigmoid_raw(rs, raw_fm, img_idx, cc)

    def fused_bwd():
        g_raw_fm, g_ray = nt.colorcal_sigmoid_backward_raw(rs, g_rgb, rgb, raw_fm, img_idx, cc)
        return nt.colorcal_fold_raw(img_idx, cc, g_ray)

    def chain_fwd():
        return _calib_sigmoid(chain_calib(cc, img_idx), raw_fm, rs.ray_start_end_idx)

    rgb_c, raw_c, ridx = chain_fwd()

    def chain_bwd():
        calib = chain_calib(cc, img_idx)
        g_pre_fm, g_cw, g_cb = _calib_sigmoid_backward(calib, g_rgb, rgb_c, raw_c, ridx)
        fixed3 = calib.fixed.expand(-1, 3)
        gwd = torch.zeros_like(cc.weight_delta).index_add_(0, calib.cam, torch.where(fixed3, torch.zeros_like(g_cw), g_cw))
        gbi = torch.zeros_like(cc.bias).index_add_(0, calib.cam, torch.where(fixed3, torch.zeros_like(g_cb), g_cb))
        return g_pre_fm, gwd, gbi

    return {"rays": int(rs.ray_start_end_idx.shape[0]), "samples": int(M),
            "forward_us": alternate({"fused": lambda: nt.colorcal_sigmoid_raw(rs, raw_fm, img_idx, cc), "chain": chain_fwd}, calls, repeats),
            "backward_and_fold_us": alternate({"fused": fused_bwd, "chain": chain_bwd}, calls, repeats)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--window", type=int, default=120)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    reel = SyntheticReel(dev)
    I = int(reel.rgb_reel.shape[0])

    trainers = {"calibrated_hand_written": nt.NerfTrainer(dev, hand_written=True, seed=0, nr_images=I),
                "calibrated_autograd": nt.NerfTrainer(dev, hand_written=False, seed=0, nr_images=I),
                "uncalibrated_hand_written": nt.NerfTrainer(dev, hand_written=True, seed=0)}
    for t in trainers.values():
        window(t, reel, args.warmup)
    rates = {k: [] for k in trainers}
    for _ in range(args.repeats):
        for k, t in trainers.items():
            rates[k].append(window(t, reel, args.window))
    speed = {k: spread(v, 1) for k, v in rates.items()}
    hw, ag, plain = (speed[k] for k in ("calibrated_hand_written", "calibrated_autograd", "uncalibrated_hand_written"))
    speed["hand_written_over_autograd_median"] = round(hw["median"] / ag["median"], 3)
    speed["calibrated_over_uncalibrated_median"] = round(hw["median"] / plain["median"], 3)
    condition = hw["min"] > ag["max"]

    tr = trainers["calibrated_hand_written"]
    b = tr.draw(reel)
    kernels = {"foreground_container_of_a_step": kernels_at(b.fg, b.fg.samples_pos.shape[0], b.img_idx, tr.colorcal, dev, args.calls, args.repeats, 1),
               "background_container_of_a_step": kernels_at(b.bg, b.bg.samples_pos_4d.shape[0], b.img_idx, tr.colorcal, dev, args.calls, args.repeats, 2)}
    result = {"tool": "nerf_colorcal_bench", "device": torch.cuda.get_device_name(0), "nr_rays": 512, "nr_images": I,
              "warmup_steps": args.warmup, "window_steps": args.window, "repeats": args.repeats, "steps_per_second": speed,
              "condition_slowest_hand_written_window_beats_fastest_autograd_window": bool(condition),
              "foreground_samples_of_the_last_step": {k: t.last["nr_fg_samples"] for k, t in trainers.items()},
              "kernel_calls_timed": args.calls, "kernels": kernels,
              "not_measured": ["a second box", "profiler kernel times (the per-call times are device events around back-to-back calls, host gaps included)"]}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
