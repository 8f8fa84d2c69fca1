"""Encode forward level by level on the benchmark batch (bench.py's make_batch: 2 097 152 ray-ordered samples, L = 16,
T = 2^18, F = 2).  One-level calls go through offset pointers (every operand of the kernel is contiguous per level), timed with
HIP events.

  python tools/enc_fwd_levels.py                       time every level (and the whole launch), one JSON line
  python tools/enc_fwd_levels.py --level 15 --reps 5   launch that level alone a few times (for a counters-only run)
  python tools/enc_fwd_levels.py --whole --reps 5      launch the whole forward a few times (for a counters-only run)
  python tools/enc_fwd_levels.py --ab 0,4,6,8          time the whole forward with that many coarse-with-fine pairs
                                                       (psdf_encode_set_forward_pairs; 0 = one level per grid row), interleaved
  --levels L, --rays R (x 128 samples) choose another shape; --pairs n sets the form of a --whole run;
  --pos-dim 4 appends |x| as a fourth coordinate (the 4-D lattice of a background model), --feat F features per level
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--level", type=int, default=None)
    ap.add_argument("--whole", action="store_true")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rays", type=int, default=None)
    ap.add_argument("--pos-dim", type=int, default=3)
    ap.add_argument("--feat", type=int, default=2)
    ap.add_argument("--ab", default=None)
    ap.add_argument("--pairs", type=int, default=None)
    ap.add_argument("--inner", type=int, default=10, help="launches between one pair of events (the figure is per launch)")
    args = ap.parse_args()
    import bench
    from permuto_sdf_amd.encoding import _Cfg, encode_forward_raw
    from permuto_sdf_amd.hotpath import SdfHotPath
    dev = torch.device("cuda", 0)
    hp = SdfHotPath(nr_levels=args.levels, hidden=64, out_channels=1, device=dev, seed=0)
    rs, _, _ = bench.make_batch(dev, 7) if args.rays is None else bench.make_batch(dev, 7, nr_rays=args.rays)
    pos = rs.samples_pos
    N = pos.shape[0]
    if (args.pos_dim, args.feat) != (3, 2):      # another lattice over the same ray samples
        import numpy as np
        from permuto_sdf_amd import PermutoEncoding
        torch.manual_seed(0)
        hp.enc = PermutoEncoding(args.pos_dim, 2 ** 18, args.levels, args.feat, np.geomspace(1.0, 1e-4, args.levels),
                                 concat_points=True, concat_points_scaling=1e-3).to(dev)
        pos = torch.cat([pos, pos.norm(dim=1, keepdim=True)], 1)[:, :args.pos_dim].contiguous()
    c = hp.enc.cfg
    F = c.nr_feat
    lat, sf, sh = hp.enc.lattice_values.detach(), hp.enc.scale_factor, hp.enc.random_shift_per_level.detach()
    feat = torch.empty((c.channels, N), dtype=torch.float32, device=dev)
    one = _Cfg(c.pos_dim, c.capacity, 1, F, False, 1.0)

    def level_call(l):
        encode_forward_raw(one, pos, lat[l:l + 1], sf[l:l + 1], sh[l:l + 1], hp.window[l:l + 1], out=feat[F * l:F * (l + 1)])

    def whole_call():
        encode_forward_raw(c, pos, lat, sf, sh, hp.window, out=feat)

    def timed(fn, reps):
        for _ in range(args.warmup):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record()
            for _ in range(args.inner):
                fn()
            b.record()
        torch.cuda.synchronize()
        t = sorted(a.elapsed_time(b) / args.inner for a, b in ev)
        return {"median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1]}

    from permuto_sdf_amd import _lib as L_

    def set_pairs(n):
        L_.call("psdf_encode_set_forward_pairs", L_.c_i(n))

    if args.pairs is not None:
        set_pairs(args.pairs)
    if args.ab is not None:
        forms = [int(x) for x in args.ab.split(",")]
        rounds = {f: [] for f in forms}
        for _ in range(3):          # interleaved: three rounds over the forms
            for f in forms:
                set_pairs(f)
                rounds[f].append(timed(whole_call, args.reps)["median_ms"])
        print(json.dumps({"N": N, "levels": args.levels, "reps": args.reps, "inner": args.inner,
                          "whole_median_ms_by_pairs": {str(f): rounds[f] for f in forms}}))
        return
    if args.level is not None or args.whole:
        fn = whole_call if args.whole else (lambda: level_call(args.level))
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        return
    out = {"N": N, "levels": args.levels, "reps": args.reps, "inner": args.inner, "whole": timed(whole_call, args.reps),
           "per_level": [timed(lambda l=l: level_call(l), args.reps) for l in range(args.levels)]}
    out["sum_levels_median_ms"] = sum(p["median_ms"] for p in out["per_level"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
