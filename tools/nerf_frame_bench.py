"""Time of one rendered 1600 x 1200 view of a NeRF run (permuto_sdf_amd/nerf_view.py), two ways in one process:

  (a) `NerfFrameRenderer.render`: chunks from psdf_frame_plan (32 768 rays at the default pool), the nets over the raw
      feature-major kernels, one launch per chunk straight into the image planes and one more for the background;
  (b) what the tree could do before the renderer existed, the reference's run_net_in_chunks (train_nerf.py:92-128) on this
      repository's operators: rays of the whole frame, torch.chunk into 200 x 200 rays (train_nerf.py:250), the trainer's
      sampling without jitter, `NerfNet.forward`, `nerf_render_raw` / `nerf_composite_forward_raw` per chunk, results appended
      to lists, torch.cat, transposes.

The two alternate; every shape is warmed up by one whole frame of each first; a timed window is whole frames, repeated until at
least `--min-window` seconds have passed, between two host clocks with a device synchronise before each.  (Host clocks: both ways
wait for the host once per chunk, so the time a user waits for a frame is host time.)  Both render the same rays with the same
networks.  The two images differ by what different batch sizes make of the MLP kernels' dispatch, and by the rays (b) loses:
40 000 rays of up to 64 samples can overflow the march's pool of 2 097 152 samples, and the rays that do not fit are dropped, as
in the reference; (a)'s chunks cannot overflow.  The largest absolute difference of the rgb planes and the foreground samples
of both ways are printed.  The scene is a few hundred `NerfTrainer` steps on a SyntheticReel: the occupancy grid has been
refreshed, so the march reads a grid of a real run, but nothing here is a trained scene.  One JSON line on stdout; --out writes
it to a file as well.

    python tools/nerf_frame_bench.py --out profiles/nerf_frame_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from permuto_sdf_amd import render                                                       # noqa: E402
from permuto_sdf_amd.nerf_train import HyperParams, NerfTrainer, nerf_render_raw        # noqa: E402
from permuto_sdf_amd.neus import nerf_composite_forward_raw                             # noqa: E402
from permuto_sdf_amd.train_step import SyntheticReel                                    # noqa: E402

REFERENCE_CHUNK = 200 * 200         # train_nerf.py:250


def render_in_reference_chunks(tr, frame, stats):
    """(b) -> [3, H, W]"""
    it, dev = tr.iter, tr.dev
    with torch.no_grad():
        o_full, d_full = render.frame_rays(frame)
        nr_chunks = -(-o_full.shape[0] // REFERENCE_CHUNK)
        preds, preds_bg, sums, samples = [], [], [], 0
        for o, d in zip(torch.chunk(o_full, nr_chunks), torch.chunk(d_full, nr_chunks)):
            R = o.shape[0]
            _, fg, bg = tr.sample(o.contiguous(), d.contiguous(), False)
            n = fg.samples_pos.shape[0]
            samples += n
            if n:
                rgb, raw = tr.net(fg.samples_pos, fg.samples_dirs, it)
                pred, ws, bgT = nerf_render_raw(fg, raw.reshape(-1).contiguous(), rgb.contiguous())
            else:
                pred, ws, bgT = torch.zeros(R, 3, device=dev), torch.zeros(R, 1, device=dev), torch.ones(R, 1, device=dev)
            if bg is not None:
                rgb_b, raw_b = tr.net_bg(bg.samples_pos_4d, bg.samples_dirs, it)
                pred_bg, pred = nerf_composite_forward_raw(bg, raw_b.reshape(-1).contiguous(), rgb_b.contiguous(), pred, bgT)
                preds_bg.append(bgT * pred_bg)
            preds.append(pred)
            sums.append(ws)
        img, img_bg, img_ws = (torch.cat(v, 0).t().reshape(-1, frame.height, frame.width).contiguous() if v else None
                               for v in (preds, preds_bg, sums))
    stats["chunks"], stats["fg_samples"] = nr_chunks, samples
    return img


def count_fg_samples(tr, frame, plan, pool):
    """the foreground samples of (a)'s chunks (not timed)"""
    keep, total = tr.grid.max_nr_samples, 0
    tr.grid.max_nr_samples = pool
    for first, count in plan.chunks():
        o, d = render.frame_rays(frame, first, count)
        total += tr.sample(o, d, False)[1].samples_pos.shape[0]
    tr.grid.max_nr_samples = keep
    return total


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
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--train-iters", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per way, alternating")
    ap.add_argument("--min-window", type=float, default=0.5, help="seconds")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nerf_frame_bench measures a device: no GPU is visible, nothing is measured")
    dev = torch.device("cuda:0")
    H, W = args.height, args.width
    hp = HyperParams()
    reel = SyntheticReel(dev, nr_images=2, height=H, width=W)
    tr = NerfTrainer(dev, hp=hp)
    for _ in range(args.train_iters):
        tr.step(reel)
    torch.cuda.synchronize()
    frame = render.Frame.from_reel(reel, 0)
    rnd = tr.renderer()
    pool = render.OccupancyGrid.POOL
    plan = render.FramePlan(H, W, hp.max_nr_samples_per_ray, pool)
    stats = {}
    # warm-up: one whole frame of each (every chunk shape, the allocator's blocks)
    a_out = rnd.render(frame)
    b_img = render_in_reference_chunks(tr, frame, stats)
    torch.cuda.synchronize()
    diff = float((a_out.rgb - b_img).abs().max())
    covered = float((a_out.weights_sum > 0.5).float().mean())
    a_samples = count_fg_samples(tr, frame, plan, pool)
    del a_out, b_img
    a_s, b_s = [], []
    for _ in range(args.rounds):
        a_s.append(window(lambda: rnd.render(frame), args.min_window))
        b_s.append(window(lambda: render_in_reference_chunks(tr, frame, stats), args.min_window))
    a_ms = statistics.median(s for s, _ in a_s) * 1e3
    b_ms = statistics.median(s for s, _ in b_s) * 1e3
    result = {"tool": "nerf_frame_bench", "device": torch.cuda.get_device_name(0), "height": H, "width": W,
              "train_iters": args.train_iters, "rounds": args.rounds, "min_window_s": args.min_window,
              "occupied_share_of_the_grid": round(float(tr.grid.get_grid_occupancy().float().mean()), 4),
              "pixels_with_weight_sum_above_half": round(covered, 4),
              "nerf_frame_renderer": {"ms_per_frame": round(a_ms, 2), "chunks": plan.nr_chunks, "rays_per_chunk": plan.rays_per_chunk,
                                      "fg_samples": a_samples, "mrays_per_s": round(H * W / a_ms / 1e3, 3),
                                      "windows_ms": [round(s * 1e3, 2) for s, _ in a_s], "frames_per_window": [n for _, n in a_s]},
              "run_net_in_40000_ray_chunks": {"ms_per_frame": round(b_ms, 2), "chunks": stats["chunks"], "rays_per_chunk": REFERENCE_CHUNK,
                                              "fg_samples": stats["fg_samples"], "mrays_per_s": round(H * W / b_ms / 1e3, 3),
                                              "windows_ms": [round(s * 1e3, 2) for s, _ in b_s],
                                              "frames_per_window": [n for _, n in b_s]},
              "speedup": round(b_ms / a_ms, 3), "rgb_max_abs_difference": diff}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
