"""Time of colouring the vertices of a 256^3 mesh, two ways in one process:

  (a) `MeshColorizer.colors` (permuto_sdf_amd/mesh_color.py): the raw feature-major kernels outside autograd, the colour
      network's input assembled by `psdf_mesh_color_inputs`, float and 8-bit colours by `psdf_mesh_color_finish`; by default the
      colour MLP on fp32 MFMAs, and beside it `fast=True`: the wide fp16 kernel, which is what `RgbNet.forward` runs in (b);
  (b) the old way by hand, in chunks of 2^18 vertices: `FrameRenderer._sdf_and_gradient` (an autograd graph over the encoding and
      the MLP, its input gradient, the graph thrown away), a made-up view direction (-normal), `RgbNet.forward` (an SH launch,
      normalize3, cat_fm with its transposes, the LipshitzMLP module, a sigmoid), `image_eval.to_u8`.

The net is an `SdfNet` whose SDF channel was fitted for a few hundred steps to a sphere of radius 0.3, beside a seeded `RgbNet`
that was never trained: nothing here is a trained scene, and the colours mean nothing.  Both ways spend most of their time in the
same encode and MLP kernels; what (a) removes is the graph, about nine small launches and the [N, C] <-> [C, N] copies per chunk.
The ways alternate; one call of each warms it up; a timed window is whole meshes, repeated until at least `--min-window` seconds
have passed, between two host clocks with a device synchronise before each.  Reported: the median over the windows and their
minimum and maximum, the largest float difference between the two ways and the number of 8-bit channels that differ.  Not
measured here: a second machine, a trained scene, kernel times under a profiler.  One JSON line on stdout; --out writes it to a
file as well.

    python tools/mesh_color_bench.py --out profiles/mesh_color_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from permuto_sdf_amd import image_eval, render                                                # noqa: E402
from permuto_sdf_amd.mesh import MeshExtractor                                                # noqa: E402
from permuto_sdf_amd.mesh_color import _IT_WINDOW_OPEN, MeshColorizer                         # noqa: E402
from permuto_sdf_amd.optim import FusedAdamW                                                  # noqa: E402
from permuto_sdf_amd.train_step import HyperParams, RgbNet, SdfNet                            # noqa: E402

CHUNK = 1 << 18


def sphere_fit(sdf, dev, radius, steps):
    """the SDF channel of the net's head fitted to |x| - radius inside the unit cube -> the last loss"""
    enc, mlp = sdf.encoding, sdf.mlp_sdf
    opt = FusedAdamW(list(enc.parameters())[:1] + list(mlp.parameters()), lr=5e-3)
    win = torch.ones(enc.nr_levels, device=dev)
    loss = None
    for _ in range(steps):
        x = torch.rand(16384, 3, device=dev) - 0.5
        loss = ((mlp(enc(x, win))[:, 0:1] - (x.norm(dim=1, keepdim=True) - radius)) ** 2).mean()
        for p in opt.param_groups[0]["params"]:
            p.grad = None
        loss.backward()
        opt.step()
    return float(loss)


@torch.no_grad()
def old_way(renderer, rgb_net, V):
    """(b) -> (rgb [N, 3] float32, rgb_u8 [N, 3])"""
    out, out_u8 = [], []
    for a in range(0, V.shape[0], CHUNK):
        p = V[a:a + CHUNK]
        _, grad, feat = renderer._sdf_and_gradient(p, _IT_WINDOW_OPEN)
        dirs = -torch.nn.functional.normalize(grad, dim=1)
        rgb = rgb_net(p, dirs, grad, feat).float()
        out.append(rgb)
        out_u8.append(image_eval.to_u8(rgb))
    return torch.cat(out), torch.cat(out_u8)


def window(fn, min_seconds):
    """-> (seconds per mesh, meshes) over whole meshes until min_seconds have passed; ends in a synchronise"""
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        fn()
        n += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return dt / n, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256, help="grid points per axis of the extracted mesh")
    ap.add_argument("--fit-steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per way, alternating")
    ap.add_argument("--min-window", type=float, default=0.5, help="seconds")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_color_bench measures a device: no GPU is visible, nothing is measured")
    dev = torch.device("cuda:0")
    hp = HyperParams()
    torch.manual_seed(0)
    sdf, rgb_net = SdfNet(hp).to(dev), RgbNet(hp).to(dev)
    fit_loss = sphere_fit(sdf, dev, 0.3, args.fit_steps)
    holder = types.SimpleNamespace(sdf=sdf, rgb=rgb_net, bg=None, grid=None, sphere=None, hp=hp, with_mask=True)
    renderer = render.FrameRenderer(holder)
    mesh = MeshExtractor.from_sdf_net(sdf, _IT_WINDOW_OPEN).extract(args.resolution, -0.5, 0.5)
    V = mesh.V.contiguous()
    colorizer = MeshColorizer(sdf, rgb_net)

    def way_a():
        return colorizer.colors(V, chunk=CHUNK)

    def way_a_fast():        # the colour MLP on the wide fp16 kernel, which is what RgbNet.forward of (b) runs too
        return colorizer.colors(V, chunk=CHUNK, fast=True)

    def way_b():
        return old_way(renderer, rgb_net, V)

    a, f, (b_rgb, b_u8) = way_a(), way_a_fast(), way_b()          # warm-up, and agreement
    torch.cuda.synchronize()
    agree = {"max_abs_float_diff": float((a.rgb - b_rgb).abs().max()), "u8_channels_that_differ": int((a.rgb_u8 != b_u8).sum()),
             "fast_max_abs_float_diff": float((f.rgb - b_rgb).abs().max()), "fast_u8_channels_that_differ": int((f.rgb_u8 != b_u8).sum()),
             "fast_took_the_wide_f16_kernel": bool(colorizer.last_used_wide_f16), "u8_channels": int(b_u8.numel())}
    del a, f, b_rgb, b_u8
    a_s, f_s, b_s = [], [], []
    for _ in range(args.rounds):
        a_s.append(window(way_a, args.min_window))
        f_s.append(window(way_a_fast, args.min_window))
        b_s.append(window(way_b, args.min_window))

    def side(w):
        ms = [s * 1e3 for s, _ in w]
        med = statistics.median(ms)
        return {"ms_per_mesh_median": round(med, 3), "ms_per_mesh_min": round(min(ms), 3), "ms_per_mesh_max": round(max(ms), 3),
                "mvertices_per_s": round(V.shape[0] / med / 1e3, 3), "windows_ms": [round(m, 3) for m in ms],
                "meshes_per_window": [n for _, n in w]}

    result = {"tool": "mesh_color_bench", "device": torch.cuda.get_device_name(0),
              "net": "SdfNet sphere-fitted for %d steps beside a seeded, untrained RgbNet: not a trained scene" % args.fit_steps,
              "fit_loss": fit_loss, "resolution": args.resolution, "vertices": int(V.shape[0]), "faces": int(mesh.F.shape[0]),
              "chunk": CHUNK, "rounds": args.rounds, "min_window_s": args.min_window,
              "not_measured": ["a second machine", "a trained scene", "kernel times under a profiler"],
              "mesh_colorizer": side(a_s), "mesh_colorizer_fast": side(f_s), "operator_chain": side(b_s), "agreement": agree}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
