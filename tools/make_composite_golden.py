"""Writes tests/golden/composite_parent_bits.npz: the output bytes of every compositing entry point (csrc/neus.hip,
volume_rendering.hip, composite_fused.hip, frame_composite.hip) on the `bordersK` containers of oracle/composite_cases.py, as the
library in use computes them.  The inputs are seeded there and are not stored.  Run it ONCE on the GPU with the library of the
commit whose results are to be pinned.  PSDF_LIB_PATH must name that library (the tool refuses the in-tree default, which is
whatever was built last) and COMMIT the commit it was built from; both are recorded in the file (`generated_from_commit`, and
`library_sha256` of the shared library), so the claim "these are the parent's bits" can be audited by rebuilding that commit:

    PSDF_LIB_PATH=/path/to/libpsdf_hip.so python tools/make_composite_golden.py OUT.npz COMMIT

tests/test_gpu_composite_parent_bits.py calls outputs() with the library under test and asserts bit equality with the file.

Every output buffer is filled with SENTINEL before the call: an entry that a kernel leaves alone (slots of skipped rays, samples
behind the early-out of volume_render_nerf) is compared as well.  g_inv_s is left out: a sum of per-wave atomics in no fixed
order, held to its float64 bar by tests/test_gpu_composite_float64.py."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import composite_cases as cc  # noqa: E402

SENTINEL = -777.25
RATIO = 0.6
NEUS = (("cross", 1000.0), ("grazing", 300.0))
FH, FW, FIRST = 41, 53, 37                      # the frame kernels write pixels FIRST .. FIRST + R of a 41 x 53 frame


def outputs(dev):
    """-> {name: float32 tensor on the device}, in a fixed order"""
    from permuto_sdf_amd import _lib as L
    out = {}
    i, f, p = L.c_i, L.c_f, L.ptr

    def buf(*shape):
        return torch.full(shape, SENTINEL, dtype=torch.float32, device=dev)

    def d(t):
        return t.to(dev).contiguous()

    def ri(c, se):
        return (i(c["R"]), p(se), i(0), i(0), i(c["N"]))

    c = cc.container("borders321")
    N, R = c["N"], c["R"]
    se = d(c["start_end"])
    rgb, g_pred, g_bg = (d(t) for t in cc.upstream(c, "dense"))
    g = torch.Generator().manual_seed(7000)
    g_alpha, g_om, x3, gy3 = (d(t) for t in (torch.randn(N, generator=g), torch.randn(N, generator=g), torch.randn(N, 3, generator=g),
                                             torch.randn(N, 3, generator=g)))
    x3[::7] *= 1e-13                                                    # below the eps of F.normalize
    fixed_dt = d(torch.rand(R, generator=g) * 0.012)                    # both ends of sdf2alpha's dynamic inv_s range
    rot = d(torch.linalg.qr(torch.randn(3, 3, generator=g))[0])
    # ---- the opacity kernels and the per-ray operators, on the longest container
    for family, inv_s in NEUS:
        sdf, dirs, grad, dt = (d(t) for t in cc.neus_family(c, family))
        inv = torch.tensor([inv_s], device=dev)
        a, om, g_sdf, g_grad, g_inv = buf(N), buf(N), buf(N), buf(N, 3), torch.zeros(1, device=dev)
        L.call("psdf_neus_alpha_forward", L.c_l(N), p(sdf), p(dirs), p(grad), p(dt), p(inv), f(RATIO), p(a), p(om), L.stream())
        L.call("psdf_neus_alpha_backward", L.c_l(N), p(g_alpha), p(sdf), p(dirs), p(grad), p(dt), p(inv), f(RATIO), p(g_sdf), p(g_grad),
               p(g_inv), L.stream())
        out.update({"neus_alpha/%s/alpha" % family: a, "neus_alpha/%s/one_minus" % family: om, "neus_alpha/%s/g_sdf" % family: g_sdf,
                    "neus_alpha/%s/g_gradients" % family: g_grad})
        for dynamic in (0, 1):
            alpha, cdf = buf(N), buf(N)
            args = ri(c, se) + (p(fixed_dt), p(dt), p(sdf), f(inv_s), i(dynamic), f(1.5))
            L.call("psdf_sdf2alpha", *args, p(alpha), L.stream())
            L.call("psdf_sdf_importance_cdf", *args, p(cdf), L.stream())
            out.update({"sdf2alpha/%s/%d" % (family, dynamic): alpha, "sdf_importance_cdf/%s/%d" % (family, dynamic): cdf})
        T, bg = buf(N), buf(R)
        L.call("psdf_cumprod_alpha2transmittance", *ri(c, se), p(om), p(T), p(bg), L.stream())
        out.update({"cumprod/%s/T" % family: T, "cumprod/%s/bg" % family: bg})
        # the fused forward, and the frame's foreground with camera normals
        pred, bg, w = buf(R, 3), buf(R), buf(N)
        L.call("psdf_neus_composite_forward", *ri(c, se), p(sdf), p(dirs), p(grad), p(dt), p(rgb), p(inv), f(RATIO), p(pred), p(bg),
               p(w), L.stream())
        out.update({"neus_composite/%s/pred" % family: pred, "neus_composite/%s/bg" % family: bg, "neus_composite/%s/weights" % family: w})
        img, nimg, cimg, wimg, Tr = buf(3, FH, FW), buf(3, FH, FW), buf(3, FH, FW), buf(1, FH, FW), buf(R + 8)
        L.call("psdf_frame_composite_neus", *ri(c, se), p(sdf), p(dirs), p(grad), p(dt), p(rgb), p(inv), f(RATIO), p(rot), i(FH), i(FW),
               L.c_l(FIRST), p(img), p(nimg), p(cimg), p(wimg), p(Tr), L.stream())
        out.update({"frame_neus/%s/rgb" % family: img.clone(), "frame_neus/%s/normals" % family: nimg, "frame_neus/%s/normals_cam" % family: cimg,
                    "frame_neus/%s/weights_sum" % family: wimg, "frame_neus/%s/transmittance" % family: Tr})
        if family == NEUS[0][0]:
            frame_fg = (img, Tr)
    raw, dtb = cc.nerf_family(c)
    raw, dtb = d(raw), d(dtb.view(-1))
    a, om, g_raw = buf(N), buf(N), buf(N)
    L.call("psdf_nerf_alpha_forward", L.c_l(N), p(raw), p(dtb), p(a), p(om), L.stream())
    L.call("psdf_nerf_alpha_backward", L.c_l(N), p(raw), p(dtb), p(g_alpha), p(g_om), p(g_raw), L.stream())
    out.update({"nerf_alpha/alpha": a, "nerf_alpha/one_minus": om, "nerf_alpha/g_raw": g_raw})
    y, gx = buf(N, 3), buf(N, 3)
    L.call("psdf_normalize3", L.c_l(N), p(x3), None, p(y), L.stream())
    L.call("psdf_normalize3", L.c_l(N), p(x3), p(gy3), p(gx), L.stream())
    out.update({"normalize3/y": y, "normalize3/g_x": gx})
    pred_bg, pred = buf(R, 3), buf(R, 3)
    fg_pred, fg_bg = d(torch.rand(R, 3, generator=g)), d(torch.rand(R, generator=g))
    L.call("psdf_nerf_composite_forward", *ri(c, se), p(raw), p(dtb), p(rgb), p(fg_pred), p(fg_bg), p(pred_bg), p(pred), L.stream())
    out.update({"nerf_composite/pred_bg": pred_bg, "nerf_composite/pred": pred})
    img, bimg = frame_fg[0], buf(3, FH, FW)
    L.call("psdf_frame_composite_nerf", *ri(c, se), p(raw), p(dtb), p(rgb), p(frame_fg[1]), i(FH), i(FW), L.c_l(FIRST), p(img), p(bimg),
           L.stream())
    out.update({"frame_nerf/rgb": img, "frame_nerf/rgb_bg": bimg})
    sigma, z, dts = (d(t.view(-1)) for t in cc.render_nerf_family(c))
    pred, depth, bg, w = buf(R, 3), buf(R), buf(R), buf(N)
    L.call("psdf_volume_render_nerf", *ri(c, se), p(rgb), p(sigma), p(z), p(dts), p(pred), p(depth), p(bg), p(w), L.stream())
    g_rgb, g_sigma = buf(N, 3), buf(N)
    L.call("psdf_volume_render_nerf_backward", *ri(c, se), p(g_pred), p(d(g_bg.view(-1))), p(pred), p(bg), p(rgb), p(sigma), p(dts),
           p(g_rgb), p(g_sigma), L.stream())
    out.update({"render_nerf/pred": pred, "render_nerf/depth": depth, "render_nerf/bg": bg, "render_nerf/weights": w,
                "render_nerf/g_rgb": g_rgb, "render_nerf/g_sigma": g_sigma})
    # ---- the fused backwards: K = 1, 2, 4 register chunks
    for K in (64, 128, 256):
        c = cc.container("borders%d" % K)
        N, R = c["N"], c["R"]
        assert c["max_per_ray"] == K
        se = d(c["start_end"])
        rgb, g_pred, g_bg = (d(t) for t in cc.upstream(c, "dense"))
        g_bg = g_bg.view(-1)
        raw, dtb = cc.nerf_family(c)
        raw, dtb = d(raw), d(dtb.view(-1))
        fg_bg = d(torch.rand(R, generator=torch.Generator().manual_seed(7000 + K)))
        for compat in (0, 1):
            for family, inv_s in NEUS:
                sdf, dirs, grad, dt = (d(t) for t in cc.neus_family(c, family))
                inv = torch.tensor([inv_s], device=dev)
                g_sdf, g_grad, g_rgb, g_inv = buf(N), buf(N, 3), buf(N, 3), torch.zeros(1, device=dev)
                L.call("psdf_neus_composite_backward", *ri(c, se), i(K), p(g_pred), p(g_bg), p(sdf), p(dirs), p(grad), p(dt), p(rgb),
                       p(inv), f(RATIO), i(compat), p(g_sdf), p(g_grad), p(g_rgb), p(g_inv), L.stream())
                tag = "neus_composite_bwd/%d/%s/compat%d/" % (K, family, compat)
                out.update({tag + "g_sdf": g_sdf, tag + "g_gradients": g_grad, tag + "g_rgb": g_rgb})
            g_raw, g_rgb, g_fg = buf(N), buf(N, 3), buf(R)
            L.call("psdf_nerf_composite_backward", *ri(c, se), i(K), p(g_pred), p(fg_bg), p(raw), p(dtb), p(rgb), i(compat), p(g_raw),
                   p(g_rgb), p(g_fg), L.stream())
            tag = "nerf_composite_bwd/%d/compat%d/" % (K, compat)
            out.update({tag + "g_raw": g_raw, tag + "g_rgb": g_rgb, tag + "g_fg_bg": g_fg})
    torch.cuda.synchronize()
    return out


def main(path, commit):
    lib = os.environ.get("PSDF_LIB_PATH")
    in_tree = os.path.join(ROOT, "permuto_sdf_amd", "lib", "libpsdf_hip.so")
    if not lib or not os.path.exists(lib) or os.path.realpath(lib) == os.path.realpath(in_tree):
        raise SystemExit("PSDF_LIB_PATH must name the library of the commit whose results are pinned (not the in-tree build)")
    if len(commit) != 40 or any(ch not in "0123456789abcdef" for ch in commit):
        raise SystemExit("COMMIT must be the full 40-digit id of the commit the library was built from")
    doc = {"generated_from_commit": np.array(commit),
           "library_sha256": np.array(hashlib.sha256(open(lib, "rb").read()).hexdigest())}
    for name, t in outputs(torch.device("cuda")).items():
        doc[name] = t.cpu().numpy()
    np.savez_compressed(path, **doc)
    print(path, os.path.getsize(path), "bytes,", len(doc) - 2, "tensors")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
