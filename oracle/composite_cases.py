"""INPUT FAMILIES AND CONTAINERS of the compositing float64 tests (tests/test_oracle_composite_float64.py on the CPU,
tests/test_gpu_composite_float64.py on the GPU: the same inputs, so that the exclusion caps and the "bites" shares verified on
the CPU are those of the GPU cases).  TEST INFRASTRUCTURE ONLY.  Everything is fp32 on the CPU, seeded."""
import torch
import torch.nn.functional as F

EQUAL_COUNTS = (1, 2, 48, 64, 65, 128, 129, 192, 193, 256)
BORDER_COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 321, 0, 40)


def container(name, seed=0):
    """-> dict(counts [R] int64, start_end [R, 2] int32, N pool size (= max_nr_samples), equal, fixed, max_per_ray)
    equalK      : R rays of K samples
    ragged      : 1..256 samples, 30 empty rays
    overflow    : ragged, the pool ends inside the fourth ray from the end (that ray and the three behind it pass max_nr_samples)
    capK        : ragged, at most K samples (K = 64 / 128 / 256), some empty rays
    bordersK    : every 64-sample chunk border -1 / +0 / +1 up to K samples and two empty rays, then rays of 70 and 40 samples that
                  pass max_nr_samples (the pool ends 17 samples into the first of them): the smallest container that reaches every
                  chunk count of the ray kernels (tests/test_gpu_composite_parent_bits.py)"""
    g = torch.Generator().manual_seed(1000 + seed)
    equal, fixed = False, 0
    if name.startswith("equal"):
        fixed = int(name[5:])
        R = 40 if fixed >= 64 else 96
        counts = torch.full((R,), fixed, dtype=torch.int64)
        equal = True
    elif name in ("ragged", "overflow"):
        R = 160
        counts = torch.randint(1, 257, (R,), generator=g)
        counts[torch.randperm(R, generator=g)[:30]] = 0
        counts[:6] = torch.tensor([1, 2, 63, 64, 65, 256])
        counts[-4:] = torch.tensor([70, 1, 130, 40])
    elif name.startswith("cap"):
        cap = int(name[3:])
        R = 120
        counts = torch.randint(1, cap + 1, (R,), generator=g)
        counts[:4] = torch.tensor([cap, 1, min(48, cap), max(1, cap - 63)])
        counts[4 + torch.randperm(R - 4, generator=g)[:10]] = 0
    elif name.startswith("borders"):
        cap = int(name[7:])
        counts = torch.tensor([n for n in BORDER_COUNTS if n <= cap] + [70, 40])
    else:
        raise ValueError(name)
    ends = torch.cumsum(counts, 0)
    starts = ends - counts
    N = int(ends[-1])
    if name == "overflow":
        N = int(starts[-4]) + 17
    elif name.startswith("borders"):
        N = int(starts[-2]) + 17
    # (the longest ray that is rendered: the two overflowed rays of a borders container are skipped)
    max_per_ray = int(counts[:-2].max()) if name.startswith("borders") else int(counts.max())
    return dict(name=name, counts=counts, start_end=torch.stack([starts, ends], 1).to(torch.int32), N=N, total=int(ends[-1]),
                equal=equal, fixed=fixed, max_per_ray=max_per_ray, R=len(counts))


def per_sample_ray(c):
    """ray index of every sample slot of the pool (slots past the last processed ray repeat the last ray)"""
    idx = torch.repeat_interleave(torch.arange(c["R"]), c["counts"])
    if len(idx) < c["N"]:
        idx = torch.cat([idx, idx[-1:].expand(c["N"] - len(idx))])
    return idx[:c["N"]]


def per_sample_pos(c):
    """position of every slot inside its ray, and the ray's length"""
    ray = per_sample_ray(c)
    start = c["start_end"][:, 0].long()[ray]
    return torch.arange(c["N"]) - start, c["counts"][ray]


def neus_family(c, family, seed=0):
    """-> sdf [N,1], dirs [N,3], gradients [N,3], dt [N,1]
    noise    : the inputs of tests/test_gpu_neus.py::_inputs (sdf ~ N(0, 0.01), unrelated directions and normals)
    cross    : every ray crosses a surface at its own depth: the SDF falls linearly through zero (+ 1e-3 noise), normals near -dir
               with |gradient| in 0.8 .. 1.2
    grazing  : the angle between direction and normal sweeps so that true_cos covers -0.3 .. 1.3: both relu kinks (0 and 1)"""
    g = torch.Generator().manual_seed(2000 + seed)
    N, R = c["N"], c["R"]
    ray = per_sample_ray(c)
    pos, length = per_sample_pos(c)
    if family == "noise":
        sdf = torch.randn(N, 1, generator=g) * 0.01
        dirs = F.normalize(torch.randn(N, 3, generator=g), dim=1)
        grad = F.normalize(torch.randn(N, 3, generator=g), dim=1) * (0.5 + torch.rand(N, 1, generator=g))
        dt = torch.rand(N, 1, generator=g) * 0.01 + 1e-4
        return sdf, dirs, grad, dt
    rdir = F.normalize(torch.randn(R, 3, generator=g), dim=1)
    dirs = rdir[ray].contiguous()
    z = (pos.float() / length.clamp_min(2).float()).view(N, 1)
    hit = (0.3 + 0.4 * torch.rand(R, 1, generator=g))[ray]
    sdf = (hit - z) * 0.5 + torch.randn(N, 1, generator=g) * 1e-3
    dt = (1.0 / length.clamp_min(1).float()).view(N, 1).contiguous()
    if family == "cross":
        grad = F.normalize(-dirs + 0.3 * torch.randn(N, 3, generator=g), dim=1) * (0.8 + 0.4 * torch.rand(N, 1, generator=g))
    elif family == "grazing":
        t = torch.rand(N, 1, generator=g) * 1.6 - 0.3
        side = F.normalize(torch.cross(dirs, torch.randn(N, 3, generator=g), dim=1), dim=1)
        grad = dirs * t + side * 0.5 * torch.rand(N, 1, generator=g)
    else:
        raise ValueError(family)
    return sdf.contiguous(), dirs, grad.contiguous(), dt


def upstream(c, kind, seed=0):
    """-> rgb [N,3], g_pred [R,3], g_bg [R,1]
    dense  : uniform colours, normal upstream gradients
    needle : g_pred / g_bg are zero except on every seventh ray (one channel each), rgb is zero except on ONE sample per ray, next
             to a 64-sample border (position 63, 64, 127, 128, 191 or 192, whichever the ray has; else its last sample)"""
    g = torch.Generator().manual_seed(3000 + seed)
    N, R = c["N"], c["R"]
    if kind == "dense":
        return torch.rand(N, 3, generator=g), torch.randn(R, 3, generator=g), torch.randn(R, 1, generator=g)
    rgb = torch.zeros(N, 3)
    borders = torch.tensor([63, 64, 127, 128, 191, 192])
    starts = c["start_end"][:, 0].long()
    for r in range(R):
        n = int(c["counts"][r])
        if n == 0 or int(starts[r]) + n > N:
            continue
        ok = borders[borders < n]
        p = int(ok[int(torch.randint(0, len(ok), (1,), generator=g))]) if len(ok) else n - 1
        rgb[int(starts[r]) + p] = torch.rand(3, generator=g) + 0.1
    g_pred, g_bg = torch.zeros(R, 3), torch.zeros(R, 1)
    pick = torch.arange(0, R, 7)
    g_pred[pick, pick % 3] = torch.randn(len(pick), generator=g)
    g_bg[pick[::2]] = torch.randn(len(pick[::2]), 1, generator=g)
    return rgb, g_pred, g_bg


def nerf_family(c, seed=0):
    """the background container: raw densities from -30 to +25 (softplus' linear branch starts at 20), dt ~ 0.05 with 1e10 on
    every ray's last sample (RaySamplerGPU.cuh:150) -> raw [N], dt [N,1]"""
    g = torch.Generator().manual_seed(4000 + seed)
    N = c["N"]
    raw = torch.rand(N, generator=g) * 55.0 - 30.0
    raw[::5] = torch.randn(len(raw[::5]), generator=g) * 3          # the trained regime in between the extremes
    dt = torch.rand(N, 1, generator=g) * 0.05 + 1e-3
    pos, length = per_sample_pos(c)
    dt[pos == length - 1] = 1e10
    return raw, dt


# seeds of render_nerf_family chosen ON THE CPU, with the float64 evaluator alone, so that the rays whose transmittance comes within
# its own bar of the 1e-4 early-out stay under 1 % of the case (seed 0 leaves 2 of 160 in the overflowing pool)
RENDER_NERF_SEED = {"overflow": 1}


def render_nerf_family(c, seed=None):
    """volume_render_nerf: densities that leave most rays alive to their end, a fifth of the rays with a wall (sigma dt ~ 3 per
    sample from some depth on) that drives T through 1e-4 -> sigma [N,1], z [N,1], dt [N,1] (1e10 on each ray's last sample)"""
    seed = RENDER_NERF_SEED.get(c["name"], 0) if seed is None else seed
    g = torch.Generator().manual_seed(5000 + seed)
    N, R = c["N"], c["R"]
    ray = per_sample_ray(c)
    pos, length = per_sample_pos(c)
    sigma = torch.rand(N, 1, generator=g) * 2.0
    wall = (torch.rand(R, generator=g) < 0.2)[ray]
    depth = (torch.rand(R, generator=g) * 0.8)[ray]
    behind = wall & (pos.float() >= depth * length.float())
    sigma[behind] = 40.0 + 40.0 * torch.rand(int(behind.sum()), 1, generator=g)
    dt = torch.rand(N, 1, generator=g) * 0.05 + 0.02
    z = (pos.float() * 0.05 + 0.5).view(N, 1)
    dt[pos == length - 1] = 1e10
    return sigma, z.contiguous(), dt
