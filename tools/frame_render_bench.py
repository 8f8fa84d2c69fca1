"""Time of one rendered 1600 x 1200 view (permuto_sdf_amd/render.py) on a sphere-fitted trainer, two ways in one process:

  (a) `FrameRenderer.render`: chunks from psdf_frame_plan (32 768 rays at the default pool), one compositing launch per chunk
      straight into the image planes;
  (b) what the tree could do before the renderer existed, the reference's run_net_in_chunks on this repository's operators:
      `Trainer._render` per 3 000-ray chunk (create_my_images.py:80), results appended to lists, torch.cat, transposes.

The two alternate; every shape is warmed up by one whole frame of each first; a timed window is whole frames, repeated until at
least `--min-window` seconds have passed, between two host clocks with a device synchronise before each.  (Host clocks: both ways
wait for the host once per chunk, so the time a user waits for a frame is host time.)  Both render the same rays with the same
networks; the two images differ by what different batch sizes make of the MLP kernels' dispatch, printed as the largest absolute
difference of the rgb planes.  The scene is the trainer's sphere fit and a few main-phase iterations on a SyntheticReel: the
occupancy grid has been refreshed once, so the march skips empty space as it does in a real run, but nothing here is a trained
scene.  One JSON line on stdout; --out writes it to a file as well.

    python tools/frame_render_bench.py --out profiles/frame_render.json
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
from permuto_sdf_amd.train_step import HyperParams, SyntheticReel, Trainer      # noqa: E402

REFERENCE_CHUNK = 3000          # create_my_images.py:80


def render_in_reference_chunks(tr, frame, stats):
    """(b): rays of the whole frame, torch.chunk, Trainer._render per chunk in evaluation mode, lists, cat, transposes -> [3, H, W]"""
    hp = tr.hp
    keep = tr.rgb.last_inv_s
    with torch.no_grad():
        o_full, d_full = render.frame_rays(frame)
        nr_chunks = -(-o_full.shape[0] // REFERENCE_CHUNK)
        preds, samples = [], 0
        for o, d in zip(torch.chunk(o_full, nr_chunks), torch.chunk(d_full, nr_chunks)):
            pred, _, fg, _ = tr._render(o.contiguous(), d.contiguous(), 9999999, 1.0, hp.forced_variance_finish, jitter=False)
            preds.append(pred.detach())
            samples += fg.samples_pos.shape[0]
        img = torch.cat(preds, 0).t().reshape(3, frame.height, frame.width).contiguous()
    tr.rgb.last_inv_s = keep
    stats["chunks"], stats["fg_samples"] = nr_chunks, samples
    return img


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
    ap.add_argument("--sphere-iters", type=int, default=200)
    ap.add_argument("--train-iters", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per way, alternating")
    ap.add_argument("--min-window", type=float, default=0.5, help="seconds")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frame_render_bench measures a device: no GPU is visible, nothing is measured")
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
    plan = render.FramePlan(H, W, hp.max_nr_samples_per_ray, render.OccupancyGrid.POOL)
    stats = {}
    # warm-up: one whole frame of each (every chunk shape, the allocator's blocks, the pinned landing zones)
    a_img = rnd.render(frame).rgb
    b_img = render_in_reference_chunks(tr, frame, stats)
    torch.cuda.synchronize()
    diff = float((a_img - b_img).abs().max())
    covered = float((rnd.render(frame).weights_sum > 0.5).float().mean())
    a_s, b_s = [], []
    for _ in range(args.rounds):
        a_s.append(window(lambda: rnd.render(frame), args.min_window))
        b_s.append(window(lambda: render_in_reference_chunks(tr, frame, stats), args.min_window))
    a_ms = statistics.median(s for s, _ in a_s) * 1e3
    b_ms = statistics.median(s for s, _ in b_s) * 1e3
    result = {"tool": "frame_render_bench", "device": torch.cuda.get_device_name(0), "height": H, "width": W,
              "sphere_iters": args.sphere_iters, "train_iters": args.train_iters, "rounds": args.rounds,
              "min_window_s": args.min_window, "fg_samples": stats["fg_samples"], "pixels_with_weight_sum_above_half": round(covered, 4),
              "frame_renderer": {"ms_per_frame": round(a_ms, 2), "chunks": plan.nr_chunks, "rays_per_chunk": plan.rays_per_chunk,
                                 "mrays_per_s": round(H * W / a_ms / 1e3, 3), "windows_ms": [round(s * 1e3, 2) for s, _ in a_s],
                                 "frames_per_window": [n for _, n in a_s]},
              "render_per_3000_ray_chunk": {"ms_per_frame": round(b_ms, 2), "chunks": stats["chunks"], "rays_per_chunk": REFERENCE_CHUNK,
                                            "mrays_per_s": round(H * W / b_ms / 1e3, 3), "windows_ms": [round(s * 1e3, 2) for s, _ in b_s],
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
