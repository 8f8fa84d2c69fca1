"""The `--with_mask` training step (no background model, the per-ray weight sum held to the mask): iterations per second of
  * train_manual.ManualTrainer(with_mask=True): the hand-written step over csrc/neus_render.hip, and
  * train_step.Trainer(with_mask=True): the autograd graph over the per-operator chain, which is what a masked step ran before,
by the protocol of tools/train_bench.py (warm-up, several timed windows; min - max over the windows is reported, the step is host
bound and moves with the state of the box's CPU), and the GPU time per call of the three entries of csrc/neus_render.hip against
the per-operator chain they replace (neus_alpha -> cumprod -> multiply -> sum_over_each_ray -> integrate, through autograd; L1 +
clip + binary cross entropy in torch), on the sample container and the ray batch of the trainer's own last step.
The reel is a SyntheticReel with a mask: a disc in `mask_reel`, `has_mask` set.  One GPU.  Prints one JSON line and writes it to
--out (default profiles/train_mask_bench.json):  python tools/train_mask_bench.py [--steps 60 --warmup 20 --repeats 5]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from permuto_sdf_amd import neus  # noqa: E402
from permuto_sdf_amd import train_manual  # noqa: E402
from permuto_sdf_amd.train_step import SyntheticReel, Trainer, _Cumprod, _Integrate, _SumRay  # noqa: E402


def masked_reel(dev):
    reel = SyntheticReel(dev)
    _, _, H, W = reel.mask_reel.shape
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    reel.mask_reel[:] = (((yy - H / 2) ** 2 + (xx - W / 2) ** 2) <= (H / 3) ** 2).float().view(1, 1, H, W)
    reel.has_mask = True
    return reel


def rate(tr, reel, steps, warmup, repeats):
    for _ in range(warmup):
        tr.step(reel)
    reps, samples = [], 0
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        samples = 0
        for _ in range(steps):
            tr.step(reel)
            samples += tr.last["nr_fg_samples"]
        torch.cuda.synchronize()
        reps.append(steps / (time.perf_counter() - t0))
    assert all(bool(torch.isfinite(p).all()) for p in tr.params), "a parameter is not finite after the run"
    return {"it_per_s_min": round(min(reps), 1), "it_per_s_max": round(max(reps), 1), "it_per_s_windows": [round(r, 1) for r in reps],
            "fg_samples_per_step": samples / steps, "rays_last_step": tr.last["nr_rays"]}


def gpu_us(fn, n=50, warm=10):
    """mean GPU time of one call in microseconds: HIP events around n back-to-back calls (launch gaps included: that is what a
    step pays), after `warm` calls"""
    for _ in range(warm):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return round(s.elapsed_time(e) / n * 1e3, 2)


def per_call(tr, reel):
    """the three new entries against the chain, at the container and batch of one more step of `tr`"""
    seen = {}
    fwd, tail = train_manual.neus_render_forward_raw, train_manual.neus_mask_loss_raw

    def fwd_spy(rs, sdf, grad, rgb, inv_s, cos_r, **k):
        seen["render"] = (rs, sdf, grad, rgb, inv_s, cos_r)
        return fwd(rs, sdf, grad, rgb, inv_s, cos_r, **k)

    def tail_spy(pred, gt, hit, ws, gt_mask, w, **k):
        seen["tail"] = (pred, gt, hit, ws, gt_mask, w)
        return tail(pred, gt, hit, ws, gt_mask, w, **k)
    train_manual.neus_render_forward_raw, train_manual.neus_mask_loss_raw = fwd_spy, tail_spy
    try:
        tr.step(reel)
    finally:
        train_manual.neus_render_forward_raw, train_manual.neus_mask_loss_raw = fwd, tail
    rs, sdf, grad, rgb, inv_s, cos_r = seen["render"]
    pred, gt, hit, ws, gt_mask, w = seen["tail"]
    hp = tr.hp
    per_ray = hp.max_nr_samples_per_ray + 2 * hp.nr_samples_imp_sampling
    _, g_pred, g_ws = neus.neus_mask_loss_raw(pred, gt, hit, ws, gt_mask, w)
    hit_f = hit.reshape(-1, 1).float()

    def chain_forward():
        alpha, one_minus = neus.neus_alpha(sdf, rs.samples_dirs, grad, rs.samples_dt, inv_s, cos_r)
        T, bg = _Cumprod.apply(rs, one_minus)
        wgt = (alpha * T).view(-1, 1)
        w_sum, _ = _SumRay.apply(rs, wgt)
        return _Integrate.apply(rs, rgb, wgt), w_sum

    leaves = [t.detach().clone().requires_grad_(True) for t in (sdf, grad, rgb)]

    def chain_both():
        alpha, one_minus = neus.neus_alpha(leaves[0], rs.samples_dirs, leaves[1], rs.samples_dt, inv_s, cos_r)
        T, bg = _Cumprod.apply(rs, one_minus)
        wgt = (alpha * T).view(-1, 1)
        w_sum, _ = _SumRay.apply(rs, wgt)
        p = _Integrate.apply(rs, leaves[2], wgt)
        torch.autograd.grad([p, w_sum], leaves, [g_pred, g_ws.view_as(w_sum)])

    pl, wl = pred.detach().clone().requires_grad_(True), ws.detach().clone().requires_grad_(True)

    def chain_tail():
        loss = ((pl - gt).abs() * hit_f).mean() + torch.nn.functional.binary_cross_entropy(wl.clip(1e-3, 1.0 - 1e-3), gt_mask.view_as(wl)) * w
        torch.autograd.grad(loss, (pl, wl))

    with torch.no_grad():
        new = {"render_forward": gpu_us(lambda: neus.neus_render_forward_raw(rs, sdf, grad, rgb, inv_s, cos_r)),
               "render_backward": gpu_us(lambda: neus.neus_render_backward_raw(rs, per_ray, g_pred, g_ws, None, sdf, grad, rgb, inv_s, cos_r,
                                                                               need_inv_s=False)),
               "mask_loss": gpu_us(lambda: neus.neus_mask_loss_raw(pred, gt, hit, ws, gt_mask, w))}
        chain_fwd = gpu_us(chain_forward)
    chain_fb = gpu_us(chain_both)
    return {"samples": int(sdf.shape[0]), "rays": int(pred.shape[0]), "max_per_ray": per_ray, "new_entries_us": new,
            "operator_chain_us": {"render_forward": chain_fwd, "render_forward_plus_backward": chain_fb,
                                  "render_backward (difference)": round(chain_fb - chain_fwd, 2), "mask_loss_forward_plus_backward": gpu_us(chain_tail)},
            "note": "GPU time between two events around 50 back-to-back calls, launch gaps included; the chain runs through torch autograd"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--start-iter", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_mask_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    reel = masked_reel(dev)
    res = {"metric": "train iters/sec, --with_mask step (SDF + colour, no background, mask loss; synthetic reel with a disc mask)",
           "unit": "it/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "start_iter": args.start_iter,
           "device": torch.cuda.get_device_name(0)}
    man = train_manual.ManualTrainer(dev, with_mask=True)
    man.iter = args.start_iter
    assert man._hand_written_step_applies()
    res["hand_written"] = rate(man, reel, args.steps, args.warmup, args.repeats)
    res["per_call"] = per_call(man, reel)
    del man
    auto = Trainer(dev, with_mask=True)
    auto.iter = args.start_iter
    res["autograd"] = rate(auto, reel, args.steps, args.warmup, args.repeats)
    res["speedup_min_over_max"] = round(res["hand_written"]["it_per_s_min"] / res["autograd"]["it_per_s_max"], 3)
    res["speedup_max_over_min"] = round(res["hand_written"]["it_per_s_max"] / res["autograd"]["it_per_s_min"], 3)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
