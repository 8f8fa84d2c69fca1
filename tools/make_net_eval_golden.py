"""Writes tests/golden/net_eval_parent_bits.npz: what every entry point that evaluates the SDF (or density) channel of a lattice +
MLP net outside autograd gives, bit for bit, and the sequence of C entry points each of them issues -- as the package of the
commit in the work tree computes them.  Run it on the GPU at the commit whose results are to be pinned:

    python tools/make_net_eval_golden.py OUT.npz $(git rev-parse HEAD)

The file records that commit (`generated_from_commit`).  tests/test_gpu_net_eval_parent_bits.py calls run() with the package
under test and asserts the same bits and the same call sequences.  Only entry points that keep their signature across the move
of the host helpers into permuto_sdf_amd/net_eval.py are used.

Every scenario is run twice from the same seeds.  A tensor both runs agree on bit for bit is pinned; one they do not agree on is
listed under `unpinned` and is not stored.  Results that are sums of float atomics in no fixed order -- the sphere tracer's
normals and MeshExtractor.sdf_gradient (the position gradient's level groups), the gradients a trainer captures (the lattice
scatter, the MLP's parameter sums) -- are listed there without being compared: two runs that agree do not show that such a sum
has an order, and a pinned one would fail some later day.  The existing tolerance tests hold those; here their launches are
held through the call sequences.

The nets are at initialisation scale from fixed seeds.  The traced and meshed ones are NOT fitted: a fit accumulates its lattice
gradient with float atomics, so two processes do not arrive at the same weights and a pinned file could not be reproduced.
Instead the last bias is shifted by the field's mean over fixed points (the product's forward and one torch mean, the same
bits every time), which puts the zero level set through the middle of the volume: rays converge on it, leave the occupied
shell or the box, or keep marching, and the marching tetrahedra find a surface."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = (1, 31, 33, 1000)           # both sides of the 32-sample MLP tile, and a tail
RAYS = 1080                         # not a multiple of 32
TRACE = dict(nr_sphere_traces=5, sdf_multiplier=0.9, sdf_converged_tresh=2e-3)
META = ("generated_from_commit", "calls", "unpinned")
ATOMICS = "#atomics"                # suffix of a result that is a sum of float atomics in no fixed order: never pinned


def _points(N, P, seed, dev):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(N, P, generator=g)
    p[:, :3] -= 0.5
    return p.to(dev)


def _reset(seed):
    from permuto_sdf_amd.bridge import OccupancyGrid, Pcg32, RaySampler, VolumeRendering
    for cls in (OccupancyGrid, RaySampler, VolumeRendering):      # the process-global jitter streams
        cls._rng = Pcg32()
    torch.manual_seed(seed)


def _centred_field(dev, P, width, outputs, seed):
    """a small lattice + MLP net at initialisation scale whose output 0 has mean 0 over fixed points of the unit box"""
    from permuto_sdf_amd import FusedMLP, PermutoEncoding
    torch.manual_seed(seed)
    enc = PermutoEncoding(P, 2 ** 16, 8, 2, np.geomspace(1.0, 0.02, 8), concat_points=True, concat_points_scaling=1.0,
                          init_scale=1e-1).to(dev)
    mlp = FusedMLP([enc.output_dims(), width, width, width, outputs], reference_init=True).to(dev)
    win = torch.ones(8, device=dev)
    with torch.no_grad():
        mean = mlp(enc(_points(4096, P, 900 + seed, dev), win))[:, 0].mean()
        mlp.layers[-1].bias[0] -= mean
    return enc, mlp, win


# ------------------------------------------------------------------------------------------------------------- scenarios
def scalar_only(dev):
    """SdfNet.sdf_only (no key, the same key twice), SdfFitNet.sdf_only (P = 3, 4), time_slice(0.25), NerfNet.get_only_density
    (P = 3, 4); window half open and fully open"""
    from permuto_sdf_amd.nerf_train import NerfNet
    from permuto_sdf_amd.sdf_fit import SdfFitNet
    from permuto_sdf_amd.train_step import HyperParams, SdfNet
    out = {}
    sdf = SdfNet(HyperParams()).to(dev)
    fit3, fit4 = SdfFitNet(3, geom_feat_size=32, nr_iters_for_c2f=5000).to(dev), SdfFitNet(4, nr_iters_for_c2f=3000).to(dev)
    nerf3, nerf4 = NerfNet(3, 100).to(dev), NerfNet(4, 100).to(dev)
    for N in SIZES:
        p3, p4 = _points(N, 3, 10 + N, dev), _points(N, 4, 20 + N, dev)
        for tag, frac in (("half", 2.0 / 7.0), ("open", 1.0)):       # window t = 0.3 + 0.7 frac
            name = "scalar_only/%%s/N%d/%s" % (N, tag)
            it = int(sdf.nr_iters_for_c2f * frac)
            out[name % "SdfNet"] = sdf.sdf_only(p3, it)
            out[name % "SdfNet_key_first"] = sdf.sdf_only(p3, it, key=(N, tag))
            out[name % "SdfNet_key_again"] = sdf.sdf_only(p3, it, key=(N, tag))
            out[name % "SdfFitNet3"] = fit3.sdf_only(p3, int(fit3.nr_iters_for_c2f * frac))
            out[name % "SdfFitNet4"] = fit4.sdf_only(p4, int(fit4.nr_iters_for_c2f * frac))
            out[name % "time_slice"] = fit4.time_slice(0.25, int(fit4.nr_iters_for_c2f * frac))(p3)
            out[name % "NerfNet3"] = nerf3.get_only_density(p3, int(nerf3.nr_iters_for_c2f * frac))
            out[name % "NerfNet4"] = nerf4.get_only_density(p4, int(nerf4.nr_iters_for_c2f * frac))
    return out


def sphere_trace(dev):
    """1080 rays against a 32^3 shell of occupancy (some meet no voxel), 5 iterations, with normals, both forms of the step"""
    from oracle import oracle as O
    from permuto_sdf_amd.bridge import OccupancyGrid, Sphere
    from permuto_sdf_amd.sphere_trace import SphereTracer
    from tests import scene
    enc, mlp, win = _centred_field(dev, 3, 32, 33, 1)
    grid = OccupancyGrid(32, 1.0, [0, 0, 0])
    grid.set_grid_occupancy(torch.from_numpy(scene.shell_occupancy(O.Oracle("port"), 32, r0=0.3, width=0.06)).to(dev))
    on, dn = scene.make_rays(RAYS, seed=8, jitter_target=0.9)
    o, d = torch.from_numpy(on).to(dev), torch.from_numpy(dn).to(dev)
    out = {}
    for compact in (True, False):
        tracer = SphereTracer(enc, mlp, grid, Sphere(0.5, [0, 0, 0]), win)
        tracer.compact_marches = compact
        pts, sdf, grads, conv = tracer.trace(o, d, return_gradients=True, **TRACE)
        tag = "sphere_trace/compact%d/" % compact
        out.update({tag + "pts": pts, tag + "sdf": sdf, tag + "conv": conv, tag + "no_hit": tracer.no_hit,
                    tag + "normals" + ATOMICS: grads})
    return out


def box_trace(dev):
    """3-D, and 4-D at time 0.3: 1080 rays of a fan wider than the box, 5 iterations, with normals"""
    from permuto_sdf_amd.box_trace import Box, BoxTracer
    rng = np.random.default_rng(3)
    o = np.tile(np.asarray((0.2, -0.3, -1.6), np.float32), (RAYS, 1))
    target = np.concatenate([rng.uniform(-0.9, 0.9, (RAYS, 2)), rng.uniform(-0.3, 0.3, (RAYS, 1))], 1).astype(np.float32)
    d = target - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(np.ascontiguousarray(d)).to(dev)
    out = {}
    for P, width, outputs, t in ((3, 32, 33, None), (4, 64, 1, 0.3)):
        enc, mlp, win = _centred_field(dev, P, width, outputs, 2 + P)
        tracer = BoxTracer(enc, mlp, Box([1.0, 1.0, 1.0]), win)
        pts, sdf, grads, conv = tracer.trace(o, d, time_val=t, return_gradients=True, **TRACE)
        tag = "box_trace/%dd/" % P
        out.update({tag + "pts": pts.contiguous(), tag + "sdf": sdf, tag + "conv": conv, tag + "no_hit": tracer.no_hit,
                    tag + "normals": grads.contiguous()})
    return out


def mesh(dev):
    """extract at 24^3 in chunks of 5000 points (two full, one partial); sdf_gradient at 1007 points in chunks of 300"""
    from permuto_sdf_amd.mesh import MeshExtractor
    enc, mlp, win = _centred_field(dev, 3, 32, 33, 7)
    ex = MeshExtractor(enc, mlp, win)
    m = ex.extract(24, -0.5, 0.5, point_budget=5000, normals=False)
    return {"mesh/V": m.V, "mesh/F": m.F, "mesh/sdf_gradient" + ATOMICS: ex.sdf_gradient(_points(1007, 3, 31, dev), 300)}


def _cloud(P, dev):
    from permuto_sdf_amd.sdf_fit import OrientedCloud

    def sphere(radius, seed):
        n = torch.nn.functional.normalize(torch.randn(2000, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64), dim=1)
        return OrientedCloud((radius * n).float().to(dev), n.float().to(dev))
    return sphere(0.3, 1) if P == 3 else OrientedCloud.stack_in_time([sphere(0.2, 2), sphere(0.3, 3)])


def sdf_fit_step0(dev):
    from permuto_sdf_amd.sdf_fit import SdfFitter
    out = {}
    for P in (3, 4):
        f = SdfFitter(_cloud(P, dev), n_surf=63, n_off=65, nr_iters_for_c2f=150, seed=5)
        f.capture_grads = {}
        out["sdf_fit_step0/%dd/loss" % P] = f.step()
        g = f.capture_grads
        for i, t in enumerate(g["dense"]):
            out["sdf_fit_step0/%dd/dense%d" % (P, i) + ATOMICS] = t
        out["sdf_fit_step0/%dd/lattice" % P + ATOMICS] = g["lattice"]
    return out


def nerf_step0(dev):
    from permuto_sdf_amd.nerf_train import HyperParams, NerfTrainer
    from permuto_sdf_amd.train_step import SyntheticReel
    out = {}
    for with_mask in (False, True):
        reel = SyntheticReel(dev, nr_images=4, height=60, width=80)
        if with_mask:
            reel.has_mask = True
            reel.mask_reel[..., reel.mask_reel.shape[-1] // 2:] = 0.0
        hp = HyperParams()
        hp.nr_rays = 64
        tr = NerfTrainer(dev, with_mask=with_mask, hp=hp, seed=5)
        tr.capture_grads = {}
        tag = "nerf_step0/mask%d/" % with_mask
        out[tag + "loss"] = tr.step(reel)
        g = tr.capture_grads
        for i, t in enumerate(g["dense"]):
            out[tag + "dense%d" % i + ATOMICS] = t
        for i, t in enumerate(g["lattices"]):
            out[tag + "lattice%d" % i + ATOMICS] = t
    return out


SCENARIOS = (scalar_only, sphere_trace, box_trace, mesh, sdf_fit_step0, nerf_step0)


def run(dev):
    """-> ({name: tensor on the host, None for a sum of atomics}, {scenario: [C entry names, in the order issued]})"""
    from permuto_sdf_amd import _lib as L
    tensors, calls = {}, {}
    real = L.call
    for k, fn in enumerate(SCENARIOS):
        _reset(100 + k)
        seq = calls[fn.__name__] = []

        def recording(name, *args, _seq=seq):
            _seq.append(name)
            return real(name, *args)
        L.call = recording
        try:
            got = fn(dev)
        finally:
            L.call = real
        torch.cuda.synchronize()
        tensors.update({name: None if name.endswith(ATOMICS) else t.detach().cpu() for name, t in got.items()})
    return tensors, calls


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))      # -0 and NaNs count
    return torch.equal(a, b)


def main(path, commit):
    if len(commit) != 40 or any(ch not in "0123456789abcdef" for ch in commit):
        raise SystemExit("COMMIT must be the full 40-digit id of the commit in the work tree")
    dev = torch.device("cuda")
    first, calls = run(dev)
    second, calls2 = run(dev)
    if calls != calls2:
        raise SystemExit("the two runs issued different call sequences")
    unpinned = sorted(n for n in first if n.endswith(ATOMICS) or not same_bits(first[n], second[n]))
    bad = [n for n in unpinned if not n.endswith(ATOMICS)]
    doc = {"generated_from_commit": np.array(commit), "calls": np.array(json.dumps(calls)),
           "unpinned": np.array(json.dumps(unpinned))}
    doc.update({n: t.numpy() for n, t in first.items() if n not in unpinned})
    np.savez_compressed(path, **doc)
    print(path, os.path.getsize(path), "bytes,", len(first) - len(unpinned), "tensors pinned,", len(unpinned), "unpinned:", unpinned)
    print({k: len(v) for k, v in calls.items()}, "calls")
    for n, t in first.items():      # what the scenarios exercised: rays masked early and late, rays that took no part, the mesh
        if n.endswith(("/conv", "/no_hit")):
            print(n, int(t.sum()), "of", t.numel())
        elif n in ("mesh/V", "mesh/F"):
            print(n, tuple(t.shape))
    if bad:
        raise SystemExit("the commit does not agree with itself on %s" % bad)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
