"""Writes tests/golden/frame_parent_bits.npz: the output bytes of the entry points that write a fitted field into image planes
(csrc/frame_rays.hip, frame_trace.hip, box_trace.hip, sdf_slice.hip and the NeRF foreground of frame_composite.hip), as the
library in use computes them.  psdf_frame_composite_neus / _nerf are pinned by tools/make_composite_golden.py and not repeated.
The inputs are seeded here and are not stored.  Run it ONCE on the GPU with the library of the commit whose results are to be
pinned.  PSDF_LIB_PATH must name that library (the tool refuses the in-tree default, which is whatever was built last) and COMMIT
the commit it was built from; both are recorded in the file (`generated_from_commit`, and `library_sha256` of the shared
library), so the claim "these are the parent's bits" can be audited by rebuilding that commit:

    PSDF_LIB_PATH=/path/to/libpsdf_hip.so python tools/make_frame_golden.py OUT.npz COMMIT

tests/test_gpu_frame_parent_bits.py calls outputs() with the library under test and asserts bit equality with the file.

Two frames serve every pixel-indexed entry: 7 x 13 whole (91 rays: a partial workgroup) and pixels [77, 410) of 40 x 48 (333
rays: a full and a partial workgroup, an offset, untouched pixels on both sides); the slice layers are S = 7 whole and cells
[77, 410) of S = 40.  The NeRF foreground takes its rays from the `bordersK` containers of oracle/composite_cases.py (9 to 20
rays), written at the same first pixels.  Every output buffer is filled with SENTINEL (float32) or SENTINEL_U8 (the byte
flags) before the call: what a kernel leaves alone is compared as well."""
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
SENTINEL_U8 = 0xA5
# (tag, H, W, first pixel, rays, focal length)
FRAMES = (("7x13", 7, 13, 0, 91, 9.0), ("40x48", 40, 48, 77, 333, 36.0))
LAYERS = (("S7", 7, 0, 49), ("S40", 40, 77, 333))
# dyadic, so that a point can sit EXACTLY on a face: unequal sizes, a translation
BOX_SIZES, BOX_TRANSLATION = (1.0, 1.5, 0.75), (0.125, -0.25, 0.5)
EYE = (1.7, 1.15, -1.4)
COVERAGE, TIME = 0.01, 0.37
SLICE_Z, SLICE_EXTENT = 0.3, 0.8                # the layer passes close to the centre of the box and reaches out of it


def _camera():
    """a tilted camera outside the box that looks at its centre, rolled a little -> tf_world_cam [4, 4] float32"""
    eye, at = torch.tensor(EYE, dtype=torch.float64), torch.tensor(BOX_TRANSLATION, dtype=torch.float64)
    z = torch.nn.functional.normalize(at - eye, dim=0)
    x = torch.nn.functional.normalize(torch.linalg.cross(torch.tensor([0.15, 1.0, 0.05], dtype=torch.float64), z), dim=0)
    y = torch.linalg.cross(z, x)
    tf = torch.eye(4, dtype=torch.float64)
    tf[:3, 0], tf[:3, 1], tf[:3, 2], tf[:3, 3] = x, y, z, eye
    return tf.to(torch.float32)


def _axes():
    """a tilted layer: its normal is no axis of the box -> [3, 3] float32 whose columns are the axes"""
    n = torch.nn.functional.normalize(torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64), dim=0)
    a0 = torch.nn.functional.normalize(torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), n), dim=0)
    return torch.stack([a0, torch.linalg.cross(n, a0), n], 1).to(torch.float32).contiguous()


def outputs(dev):
    """-> {name: float32 or uint8 tensor on the device}, in a fixed order"""
    from permuto_sdf_amd import _lib as L
    from permuto_sdf_amd.sdf_slice import IsoStyle
    out = {}
    i, f, l, p = L.c_i, L.c_f, L.c_l, L.ptr

    def buf(*shape):
        return torch.full(shape, SENTINEL, dtype=torch.float32, device=dev)

    def flags(*shape):
        return torch.full(shape, SENTINEL_U8, dtype=torch.uint8, device=dev)

    def d(t):
        return t.to(dev).contiguous()

    def c3(v):
        return (L.c_f * 3)(*[float(x) for x in v])

    g = torch.Generator().manual_seed(9100)
    tf = _camera()
    rot = d(tf[:3, :3].t())
    s, t, two = np.asarray(BOX_SIZES, np.float32), np.asarray(BOX_TRANSLATION, np.float32), np.float32(2.0)
    bmin, bmax, tr, half = c3(-s / two + t), c3(s - s / two + t), c3(t), c3(s / two)
    time = torch.tensor([TIME], device=dev)
    axes = _axes()
    axes_c = (L.c_f * 9)(*axes.reshape(-1).tolist())
    style = IsoStyle()
    lo, hi, band_rgb = style.band_table()
    n_lines = style.nr_lines
    table = d(torch.from_numpy(style.table32()))
    colours = (p(table), i(table.shape[0]), (L.c_f * 4)(*style.base_map32().tolist()), i(n_lines), (L.c_f * n_lines)(*lo.tolist()),
               (L.c_f * n_lines)(*hi.tolist()), (L.c_f * (3 * n_lines))(*band_rgb.reshape(-1).tolist()))
    edges = torch.from_numpy(np.concatenate([lo, hi]))

    def sdf_on_edges(n):
        """SDF values over the colour map's range: every band edge exactly, its two neighbours, and a NaN"""
        v = torch.rand(n, generator=g) * 0.5 - 0.05
        k = min(len(edges), n // 3)
        v[0:3 * k:3] = edges[:k]
        v[1:3 * k:3] = torch.nextafter(edges[:k], torch.tensor(1.0))
        v[n - 1] = float("nan")
        return d(v)

    for tag, H, W, first, R, focal in FRAMES:
        # the principal point sits in the middle of the chunk's rows: the box is in view of the chunk
        K = d(torch.tensor([[focal, 0.0, W / 2.0], [0.0, focal, (first + R / 2.0) / W], [0.0, 0.0, 1.0]]))
        # ---- the rays (csrc/frame_rays.hip)
        o, dr = buf(R + 2, 3), buf(R + 2, 3)
        L.call("psdf_frame_rays", i(H), i(W), p(K), p(d(tf)), l(first), i(R), p(o), p(dr), L.stream())
        out.update({"frame_rays/%s/origins" % tag: o, "frame_rays/%s/dirs" % tag: dr})
        o, dr = o[:R].contiguous(), dr[:R].clone()
        dr[::11, 0] = 0.0                       # direction components of exactly 0: an infinity, or a NaN, per axis of the box
        dr[5::17, 1] = 0.0
        dr[8::23, 2] = -0.0
        # ---- the sphere-traced frame's last step (csrc/frame_trace.hip)
        # end points on both sides of the layer below, which lies about 2.8 from the eye
        pos = d(o.cpu() + dr.cpu() * (1.5 + 2.5 * torch.rand(R, 1, generator=g)) + 0.01 * torch.randn(R, 3, generator=g))
        grad, rgb = torch.randn(R, 3, generator=g), torch.rand(R, 3, generator=g)
        grad[::7] *= 1e-13                      # below the eps of normalize_eps
        grad, rgb = d(grad), d(rgb)
        valid = torch.rand(R, generator=g) < 0.6
        mixed = torch.where(valid, torch.cumsum(valid.to(torch.int32), 0, dtype=torch.int32) - 1, torch.tensor(-1, dtype=torch.int32))
        slots = (("none", torch.full((R,), -1, dtype=torch.int32), 0), ("all", torch.arange(R, dtype=torch.int32), R),
                 ("mixed", mixed, int(valid.sum())))
        for pattern, slot, M in slots:
            for cam in (1, 0):
                img, nimg, cimg, wimg, dimg = buf(3, H, W), buf(3, H, W), buf(3, H, W), buf(1, H, W), buf(1, H, W)
                dense = (p(pos), p(grad), p(rgb)) if M else (None, None, None)
                L.call("psdf_trace_frame_resolve", i(R), i(M), p(d(slot)), p(o), p(dr), *dense, p(rot) if cam else None, i(H), i(W),
                       l(first), p(img), p(nimg), p(cimg) if cam else None, p(wimg), p(dimg), L.stream())
                name = "trace_resolve/%s/%s/cam%d/" % (tag, pattern, cam)
                out.update({name + "rgb": img, name + "normals": nimg, name + "weights_sum": wimg, name + "depth": dimg})
                if cam:
                    out[name + "normals_cam"] = cimg
        # ---- the box (csrc/box_trace.hip)
        te, tx, pe, px, hit = buf(R + 2), buf(R + 2), buf(R + 2, 3), buf(R + 2, 3), flags(R + 2)
        L.call("psdf_box_ray_intersection", i(R), bmin, bmax, p(o), p(dr), p(te), p(tx), p(pe), p(px), p(hit), L.stream())
        name = "box_intersection/%s/" % tag
        out.update({name + "t_entry": te, name + "t_exit": tx, name + "pts_entry": pe, name + "pts_exit": px, name + "hit": hit})
        for P in (3, 4):
            pts, conv, no_hit = buf(R + 2, P), flags(R + 2), flags(R + 2)
            L.call("psdf_box_trace_begin", i(R), i(P), bmin, bmax, p(o), p(dr), p(time) if P == 4 else None, p(pts), p(conv),
                   p(no_hit), L.stream())
            name = "box_begin/%s/stride%d/" % (tag, P)
            out.update({name + "pts": pts.clone(), name + "converged": conv.clone(), name + "no_hit": no_hit})
            # one step: SDFs on both sides of the threshold, and moved points EXACTLY on a face (strictly inside fails there)
            sdf = torch.rand(R + 2, generator=g) * 0.2 - 0.05
            sdf[3::8] *= 1e-3
            ds = dr.clone()
            ds = torch.cat([ds, ds[:2]])
            conv[4::9] = 0
            conv[5::9] = 0
            # (0, 0, 1) * 0.5 * 0.5 onto the +z face; (-1, 0, 0) * 0.5 * 0.5 onto the -x face; all of it exact in float32
            pts[4::9, :3] = torch.tensor([t[0] + 0.25, t[1] - 0.5, t[2] + 0.375 - 0.25], device=dev)
            ds[4::9] = torch.tensor([0.0, 0.0, 1.0], device=dev)
            pts[5::9, :3] = torch.tensor([t[0] - 0.5 + 0.25, t[1] + 0.125, t[2] - 0.25], device=dev)
            ds[5::9] = torch.tensor([-1.0, 0.0, 0.0], device=dev)
            sdf[4::9] = 0.5
            sdf[5::9] = 0.5
            sdf = d(sdf)
            L.call("psdf_box_trace_step", i(R), i(P), tr, half, p(ds), p(sdf), f(0.5), f(2e-4), p(pts), p(conv), L.stream())
            name = "box_step/%s/stride%d/" % (tag, P)
            out.update({name + "pts": pts, name + "converged": conv})
            # resolve: an sdf_end on either side of the threshold, on it, and a NaN
            end = torch.rand(R, generator=g) * 0.06 - 0.02
            end[2::10] = COVERAGE
            end[3::10] = float(np.nextafter(np.float32(COVERAGE), np.float32(0)))
            end[6::10] = float("nan")
            end = d(end)
            gradP = torch.randn(R, P, generator=g)
            gradP[::7] *= 1e-13
            gradP = d(gradP)
            miss = d((torch.rand(R, generator=g) < 0.2).to(torch.uint8))
            end_pts = d(torch.cat([pos.cpu(), torch.full((R, 1), TIME)], 1)[:, :P])
            for cam in (1, 0):
                nimg, cimg, wimg, dimg = buf(3, H, W), buf(3, H, W), buf(1, H, W), buf(1, H, W)
                L.call("psdf_box_trace_resolve", i(R), i(P), p(o), p(dr), p(end_pts), p(end), p(gradP), p(miss), f(COVERAGE),
                       p(rot) if cam else None, i(H), i(W), l(first), p(nimg), p(cimg) if cam else None, p(wimg), p(dimg), L.stream())
                name = "box_resolve/%s/stride%d/cam%d/" % (tag, P, cam)
                out.update({name + "normals": nimg, name + "weights_sum": wimg, name + "depth": dimg})
                if cam:
                    out[name + "normals_cam"] = cimg
                if P == 3 and cam:
                    view = (wimg, dimg)
        # ---- a layer cut into that view (csrc/sdf_slice.hip); the frame's own rays: the altered ones miss the layer's plane
        o2, d2 = out["frame_rays/%s/origins" % tag][:R].contiguous(), out["frame_rays/%s/dirs" % tag][:R].contiguous()
        for P in (3, 4):
            pts, skip, tt = buf(R + 2, P), flags(R + 2), buf(R + 2)
            L.call("psdf_slice_cut_begin", i(R), i(P), axes_c, f(SLICE_Z), f(SLICE_EXTENT), tr, half, p(o2), p(d2),
                   p(time) if P == 4 else None, i(H), i(W), l(first), p(view[0]), p(view[1]), p(pts), p(skip), p(tt), L.stream())
            name = "slice_cut_begin/%s/stride%d/" % (tag, P)
            out.update({name + "pts": pts, name + "skip": skip, name + "t": tt})
            img, dimg, wimg, mimg = buf(3, H, W), view[1].clone(), view[0].clone(), buf(1, H, W)
            L.call("psdf_slice_cut_resolve", i(R), p(sdf_on_edges(R)), p(skip), p(tt), *colours, i(H), i(W), l(first), p(img), p(dimg),
                   p(wimg), p(mimg), L.stream())
            name = "slice_cut_resolve/%s/stride%d/" % (tag, P)
            out.update({name + "rgb": img, name + "depth": dimg, name + "weights_sum": wimg, name + "slice_mask": mimg})
    # ---- the layer alone
    for tag, S, first, count in LAYERS:
        for P in (3, 4):
            pts, skip = buf(count + 2, P), flags(count + 2)
            L.call("psdf_slice_points", i(S), l(first), i(count), i(P), axes_c, f(SLICE_Z), f(SLICE_EXTENT), tr, half,
                   p(time) if P == 4 else None, p(pts), p(skip), L.stream())
            name = "slice_points/%s/stride%d/" % (tag, P)
            out.update({name + "pts": pts, name + "skip": skip})
        img, simg, iimg = buf(3, S, S), buf(1, S, S), buf(1, S, S)
        L.call("psdf_slice_colorize", i(S), l(first), i(count), p(sdf_on_edges(count)), p(skip), *colours, p(img), p(simg), p(iimg),
               L.stream())
        name = "slice_colorize/%s/" % tag
        out.update({name + "rgb": img, name + "sdf": simg, name + "inside": iimg})
    # ---- the NeRF foreground (csrc/frame_composite.hip: frame_render_nerf_kernel)
    for K_ in (321, 64, 128, 256):
        c = cc.container("borders%d" % K_)
        R = c["R"]
        se = d(c["start_end"])
        rgb = d(cc.upstream(c, "dense")[0])
        raw, dtb = cc.nerf_family(c)
        raw, dtb = d(raw), d(dtb.view(-1))
        z = d(cc.render_nerf_family(c)[1].view(-1))
        for tag, H, W, first, _, _ in FRAMES:
            for depth in (1, 0):
                img, wimg, dimg, Tr = buf(3, H, W), buf(1, H, W), buf(1, H, W), buf(R + 8)
                L.call("psdf_nerf_frame_render", i(R), p(se), i(0), i(0), i(c["N"]), p(raw), p(dtb), p(z) if depth else None, p(rgb),
                       i(H), i(W), l(first), p(img), p(wimg), p(dimg) if depth else None, p(Tr), L.stream())
                name = "nerf_frame/%d/%s/depth%d/" % (K_, tag, depth)
                out.update({name + "rgb": img, name + "weights_sum": wimg, name + "transmittance": Tr})
                if depth:
                    out[name + "depth"] = dimg
    # a container without samples, from null pointers: every ray takes the empty branch
    for tag, H, W, first, _, _ in FRAMES:
        img, wimg, dimg, Tr = buf(3, H, W), buf(1, H, W), buf(1, H, W), buf(R + 8)
        L.call("psdf_nerf_frame_render", i(R), p(se), i(0), i(0), i(0), None, None, None, None, i(H), i(W), l(first), p(img), p(wimg),
               p(dimg), p(Tr), L.stream())
        name = "nerf_frame/empty/%s/" % tag
        out.update({name + "rgb": img, name + "weights_sum": wimg, name + "depth": dimg, name + "transmittance": Tr})
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
