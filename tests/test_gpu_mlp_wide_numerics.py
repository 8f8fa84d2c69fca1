"""GPU: the wide split-fp16 MLP kernels (csrc/mlp_wide.hip) -- the colour network 111-128-128-64-3, the background density net
52-64-64-64-65 and the background colour head 80-64-64-3 -- entry by entry against float64, on inputs built the way the reference
builds them, and their range guard.

Per-entry metric: |ours - f64| / S with S the entry's own absolute sum in float64 (the error scale of a dot product; it does not
blow up where a sum cancels): dW_l: |dZ_l|^T |H_{l-1}|, db_l: sum |dZ_l|, dX: |W_1|^T |dZ_1|, Y: |W_L| |h_{L-1}| + |b_L|.  A per-tensor
bar (max |err| / max |ref|) cannot see a dW1 column of the lattice features (1e-5 at initialisation) next to the columns of the
points and directions; AdamW scales every entry by its own magnitude.

The range guard is process-wide (a sticky switch to the fp32 kernels), so every guard case runs in a fresh child Python process,
one at a time, with a time limit; the parent's own switch is asserted to stay down."""
import json
import os
import subprocess
import sys
import textwrap

import pytest
import torch

from tests.mlp_float64 import _f64_pass, _per_entry

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 2e-5                      # the split-fp16 bar of the project, per entry

COLOUR = [111, 128, 128, 64, 3]
DENSITY = [52, 64, 64, 64, 65]
HEAD = [80, 64, 64, 3]


def _sh_like(dirs, n):
    """n real polynomials of degree <= 4 of unit directions (the magnitudes of the SH encoding: |value| <= 1)"""
    x, y, z = dirs[:, 0:1], dirs[:, 1:2], dirs[:, 2:3]
    cols = [torch.ones_like(x), y, z, x, x * y, y * z, 3 * z * z - 1, x * z, x * x - y * y, y * (3 * x * x - y * y), x * y * z,
            y * (5 * z * z - 1), z * (5 * z * z - 3), x * (5 * z * z - 1), z * (x * x - y * y), x * (x * x - 3 * y * y),
            x * y * (x * x - y * y), y * z * (3 * x * x - y * y), x * y * (7 * z * z - 1), y * z * (7 * z * z - 3),
            35 * z ** 4 - 30 * z * z + 3, x * z * (7 * z * z - 3), (x * x - y * y) * (7 * z * z - 1), x * z * (x * x - 3 * y * y),
            x * x * (x * x - 3 * y * y) - y * y * (3 * x * x - y * y)]
    out = torch.cat(cols[:n], 1)
    return out / out.abs().amax(0, keepdim=True).clamp_min(1.0)


def _inputs(dims, N, lattice, gen):
    """the input of the net as the reference assembles it (models.py): colour net cat(points 3, lattice features 48, SH 25,
    normals 3, geometry features 32); background density net cat(points 4, lattice features 48); background colour head
    cat(density-net features 64, SH 16).  Lattice features ~ `lattice` (1e-5 at initialisation, 1e-2 trained)."""
    dirs = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen, dtype=torch.float64), dim=1)
    if dims == COLOUR:
        pts = torch.rand(N, 3, generator=gen, dtype=torch.float64) * 2 - 1
        lat = torch.randn(N, 48, generator=gen, dtype=torch.float64) * lattice
        nrm = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen, dtype=torch.float64), dim=1)
        geo = torch.randn(N, 32, generator=gen, dtype=torch.float64)
        x = torch.cat([pts, lat, _sh_like(dirs, 25), nrm, geo], 1)
    elif dims == DENSITY:
        pts = torch.rand(N, 4, generator=gen, dtype=torch.float64) * 2 - 1
        lat = torch.randn(N, 48, generator=gen, dtype=torch.float64) * lattice
        x = torch.cat([pts, lat], 1)
    else:
        feat = torch.randn(N, 64, generator=gen, dtype=torch.float64)
        x = torch.cat([feat, _sh_like(dirs, 16)], 1)
    assert x.shape == (N, dims[0])
    return x.float()


def _net(dims, seed):
    torch.manual_seed(seed)
    return [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)]


# (net, N, scale of the lattice features: 1e-5 at initialisation, 1e-2 trained; the colour head has no lattice-feature input)
CASES = [(d, n, s) for d, n in ((COLOUR, 49_152), (COLOUR, 30_001), (DENSITY, 49_152), (DENSITY, 23_001)) for s in (1e-5, 1e-2)] + \
        [(HEAD, 22_753, 1e-5)]


@pytest.mark.parametrize("dy", ["ordinary", "six_decades"])
@pytest.mark.parametrize("dims,N,lattice", CASES)
def test_wide_split_f16_per_entry_against_float64(dev, dims, N, lattice, dy, monkeypatch):
    """every entry of dX, dW_l, db_l (and Y, for the nets with a wide forward) within 2e-5 of its own absolute sum; torch's fp32
    figure on the same metric is printed beside ours"""
    import ctypes
    from permuto_sdf_amd import _lib as L
    from permuto_sdf_amd.mlp import mlp_backward_raw, mlp_forward_wide_f16_raw
    monkeypatch.delenv("PSDF_MLP_WIDE_SPLIT", raising=False)
    gen = torch.Generator().manual_seed(N + int(lattice == 1e-2))
    lin = _net(dims, N)
    x = _inputs(dims, N, lattice, gen)
    gy = torch.randn(N, dims[-1], generator=gen)
    if dy == "six_decades":         # NeuS weights: per-sample magnitudes spread over six decades within a batch
        gy = gy * 10.0 ** (-6.0 * torch.rand(N, 1, generator=gen))
    y64, SY, g64, s64, _ = _f64_pass(lin, x, gy)
    # torch fp32 on the same metric
    net32 = [l.to(dev) for l in lin]
    x32 = x.to(dev).requires_grad_(True)
    h = x32
    for i, l in enumerate(net32):
        h = l(h)
        if i < len(net32) - 1:
            h = torch.nn.functional.gelu(h)
    y32 = h
    y32.backward(gy.to(dev))
    t32 = {"dX": x32.grad.cpu()}
    for i, l in enumerate(net32):
        t32["dW%d" % (i + 1)] = l.weight.grad.cpu()
        t32["db%d" % (i + 1)] = l.bias.grad.cpu()
    # the kernels
    ws = [l.weight.detach() for l in net32]
    bs = [l.bias.detach() for l in net32]
    x_fm, gy_fm = x.t().contiguous().to(dev), gy.t().contiguous().to(dev)
    dx, dWs, dbs = mlp_backward_raw(dims, x_fm, ws, bs, gy_fm, need_dx=True)
    form = L.lib().psdf_mlp_backward_wide_form
    form.restype = ctypes.c_int
    assert form() == 2, "the split-fp16 kernel must be the one under test"
    got = {"dX": dx.t().cpu()}
    for i in range(len(dims) - 1):
        got["dW%d" % (i + 1)] = dWs[i].cpu()
        got["db%d" % (i + 1)] = dbs[i].cpu()
    rows, worst = [], {}
    for k in g64:
        assert bool(torch.isfinite(got[k]).all()), k
        e, bad = _per_entry(got[k], g64[k], s64[k])
        et, _ = _per_entry(t32[k], g64[k], s64[k])
        assert not bad, (k, "an entry without terms is not zero")
        worst[k] = e
        rows.append("%s %.1e/%.1e" % (k, e, et))
    if len(dims) == 5:
        y = mlp_forward_wide_f16_raw(dims, x_fm, ws, bs)
        assert y is not None
        e, bad = _per_entry(y.t().cpu(), y64, SY)
        et, _ = _per_entry(y32.detach().cpu(), y64, SY)
        assert not bad
        worst["Y"] = e
        rows.append("Y %.1e/%.1e" % (e, et))
    print("wide split-f16 %s N=%d lattice=%g dy=%s, per entry (ours/torch fp32): %s" % (dims, N, lattice, dy, " ".join(rows)))
    assert max(worst.values()) <= BAR, worst


# ---------------------------------------------------------------------------------------------------------------------------
# Range guard: one child process per case

_CHILD = textwrap.dedent(r"""
import json, os, sys, ctypes
sys.path.insert(0, sys.argv[1])
import torch
from tests.test_gpu_mlp_wide_numerics import guard_case
print("RESULT " + json.dumps(guard_case(*json.loads(sys.argv[2]))))
""")


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-300)


def guard_case(direction, net, what):
    """(runs in a child process) an in-range batch, then the batch that meets the value, then one more call; returns what the test
    asserts on"""
    import ctypes
    from permuto_sdf_amd import _lib as L
    from permuto_sdf_amd.mlp import mlp_backward_raw, mlp_forward_wide_f16_raw
    dev = torch.device("cuda:0")
    dims = {"colour": COLOUR, "density": DENSITY, "head": HEAD}[net]
    N = 8_195
    gen = torch.Generator().manual_seed(5)
    lin = _net(dims, 7)
    x = _inputs(dims, N, 1e-2, gen)
    gy = torch.randn(N, dims[-1], generator=gen)
    form = L.lib().psdf_mlp_backward_wide_form
    form.restype = ctypes.c_int
    out = {}

    def backward(xin, lin_):
        ws = [l.weight.detach().to(dev) for l in lin_]
        bs = [l.bias.detach().to(dev) for l in lin_]
        dx, dWs, dbs = mlp_backward_raw(dims, xin.t().contiguous().to(dev), ws, bs, gy.t().contiguous().to(dev), need_dx=True)
        torch.cuda.synchronize()
        return [dx.t().cpu()] + [t.cpu() for pair in zip(dWs, dbs) for t in pair]

    def forward(xin, lin_):
        ws = [l.weight.detach().to(dev) for l in lin_]
        bs = [l.bias.detach().to(dev) for l in lin_]
        y = mlp_forward_wide_f16_raw(dims, xin.t().contiguous().to(dev), ws, bs)
        torch.cuda.synchronize()
        return None if y is None else y.t().cpu()

    def reference(xin, lin_):
        """float64 and torch fp32 (the fp32 bar: no worse than 4x torch's fp32, at least 5e-6 of the largest entry)"""
        res = {}
        for dt in (torch.float64, torch.float32):
            xx = xin.to(dt).requires_grad_(True)
            ls = [torch.nn.Linear(l.in_features, l.out_features).to(dt) for l in lin_]
            for a, b in zip(ls, lin_):
                a.weight.data.copy_(b.weight.data)
                a.bias.data.copy_(b.bias.data)
            h = xx
            for i, l in enumerate(ls):
                h = l(h)
                if i < len(ls) - 1:
                    h = torch.nn.functional.gelu(h)
            h.backward(gy.to(dt))
            res[dt] = (h.detach(), [xx.grad] + [t for l in ls for t in (l.weight.grad, l.bias.grad)])
        return res

    # 1. in range: the switch stays down
    if direction == "backward":
        backward(x, lin)
        out["form_in_range"] = form()
    else:
        out["fwd_in_range_declined"] = forward(x, lin) is None
    # 2. the batch that meets the value
    xb = x.clone()
    lb = _net(dims, 7)
    with torch.no_grad():
        if what == "x4e4":
            xb[N // 3, 5] = 4.0e4
        elif what == "x7e4":
            xb[N // 3, 5] = 7.0e4
        elif what == "hidden":
            lb[0].bias[7] = 7.0e4                      # h1[:, 7] ~ 7e4 for every sample: beyond fp16
        elif what == "weight":
            lb[1].weight[3, 9] = 7.0e4
        elif what == "dz":
            lb[-1].weight.mul_(2.0e4)                  # the last layer's weights ~ 2e3: the scaled chain's dZ passes 65504
        elif what == "hidden_small_dy":
            # h1[hot, 7] ~ 8e4, beyond fp16, on ONE sample whose upstream gradient is zero: its T-record factor is ~2^-96, so only
            # the activation itself (it also enters the chain's B records unscaled) can show that it is out of range
            hot = N // 3
            xb[:, 5] = 0.0
            xb[hot, 5] = 20.0
            gy[hot] = 0.0
            lb[0].weight[7, 5] = 4.0e3
    if what == "hidden_small_dy":
        # from float64: the only value beyond its limit is that activation (inputs < 32, the other samples' activations < 128,
        # weights < 32768)
        H = [xb.double()]
        for i, l in enumerate(lb[:-1]):
            H.append(torch.nn.functional.gelu(H[-1] @ l.weight.detach().double().t() + l.bias.detach().double()))
        live = gy.abs().amax(1) > 0
        out["hot_h_max"] = max(float(h[N // 3].abs().max()) for h in H[1:])
        out["live_h_max"] = max(float(h[live].abs().max()) for h in H[1:])
        out["x_max"] = float(xb.abs().max())
        out["w_max"] = max(float(l.weight.detach().abs().max()) for l in lb)
    if what == "dz":
        # from float64: the per-sample scaled dZ of the layer below the linear one passes 65504 while every input, activation and
        # weight stays under its guard (inputs < 32, hidden < 128 with their pre-scales, weights < 32768)
        Ws = [l.weight.detach().double() for l in lb]
        H, Zs = [xb.double()], []
        for i, l in enumerate(lb):
            z = H[-1] @ Ws[i].t() + l.bias.detach().double()
            Zs.append(z)
            if i < len(lb) - 1:
                H.append(torch.nn.functional.gelu(z))
        g = gy.double()
        m = g.abs().amax(1, keepdim=True)
        k = 4 - torch.floor(torch.log2(m))                 # |dY| * 2^k in [2^4, 2^5), the kernel's per-sample scale
        dys = g * torch.exp2(k)
        zz = Zs[-2]
        gp = 0.5 * (1 + torch.erf(zz / 2 ** 0.5)) + zz * torch.exp(-0.5 * zz * zz) / (2 * torch.pi) ** 0.5
        dz = (dys @ Ws[-1]) * gp
        out["dz_max"] = float(dz.abs().max())
        out["x_max"] = float(xb.abs().max())
        out["h_max"] = max(float(h.abs().max()) for h in H[1:])
        out["w_max"] = max(float(w.abs().max()) for w in Ws)
    ref = reference(xb, lb)
    if direction == "backward":
        got = backward(xb, lb)
        out["form_tripping"] = form()
        out["finite"] = all(bool(torch.isfinite(t).all()) for t in got)
        r64, r32 = ref[torch.float64][1], ref[torch.float32][1]
        out["err"] = [_rel(a, b) for a, b in zip(got, r64)]
        out["err_t32"] = [_rel(a, b) for a, b in zip(r32, r64)]
        if what == "weight":
            # fp32 itself drifts from float64 with a 7e4 weight: the batch must equal the fp32 kernel's own answer
            os.environ["PSDF_MLP_WIDE_SPLIT"] = "f32"
            f32 = backward(xb, lb)
            del os.environ["PSDF_MLP_WIDE_SPLIT"]
            out["err_vs_fp32_kernel"] = [_rel(a, b) for a, b in zip(got, f32)]
    else:
        y = forward(xb, lb)
        out["fwd_tripping_declined"] = y is None
        if y is not None:
            out["finite"] = bool(torch.isfinite(y).all())
            out["err"] = [_rel(y, ref[torch.float64][0])]
            out["err_t32"] = [_rel(ref[torch.float32][0], ref[torch.float64][0])]
    # 3. afterwards: the switch is up
    backward(x, lin)
    out["form_after"] = form()
    out["fwd_after_declined"] = forward(x, lin) is None if len(dims) == 5 else True
    return out


GUARD_CASES = [("backward", net, what) for net in ("colour", "head") for what in ("x4e4", "x7e4", "hidden", "weight", "dz")] + \
              [("backward", net, "hidden_small_dy") for net in ("colour", "density", "head")] + [("backward", "density", "x7e4")] + \
              [("forward", "colour", what) for what in ("x4e4", "x7e4", "hidden", "weight")] + [("forward", "density", "x7e4")]


def test_wide_split_f16_range_guard(dev, capsys):
    """A batch that meets a value beyond the split-fp16 range is redone on the device by the fp32 kernel in the SAME call: finite,
    within the fp32 kernel's bar against float64 (with a 7e4 weight, where fp32 itself drifts: equal to the fp32 kernel's answer up
    to the order of its atomics); the sticky switch is up afterwards (backward form 1, wide forward declined); an in-range batch
    before it leaves the switch down.  Cases: one input of 4e4 (inside fp16, above the guard) and of 7e4 (beyond fp16), a hidden
    activation beyond fp16 through a bias, one weight of 7e4, (backward) a dZ of the per-sample scaled chain beyond fp16 and an
    activation beyond fp16 on a single sample without upstream gradient; the background density net's fp32 redo of both directions."""
    import ctypes
    from permuto_sdf_amd import _lib as L
    env = dict(os.environ)
    env.pop("PSDF_MLP_WIDE_SPLIT", None)
    failures = []
    for case in GUARD_CASES:
        p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(case)], cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=300)
        assert p.returncode == 0, (case, p.returncode, p.stdout[-2000:], p.stderr[-4000:])
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        assert line, (case, p.stdout[-2000:])
        r = json.loads(line[-1][7:])
        direction, net, what = case
        with capsys.disabled():
            print("range guard %s: %s" % (case, {k: (["%.1e" % e for e in v] if isinstance(v, list) else v) for k, v in r.items()}))
        msgs = []
        if direction == "backward":
            if r["form_in_range"] != 2:
                msgs.append("in-range batch did not run the split-fp16 kernel (form %d)" % r["form_in_range"])
            if r["form_tripping"] != 2:
                msgs.append("the tripping batch was not a split-fp16 launch")
        else:
            if r["fwd_in_range_declined"]:
                msgs.append("in-range forward declined")
            if r["fwd_tripping_declined"]:
                msgs.append("the tripping forward was declined before it ran")
        if what == "hidden_small_dy":
            if not (r["hot_h_max"] > 65520 and r["live_h_max"] < 128 and r["x_max"] < 32 and r["w_max"] < 32768):
                msgs.append("the hidden_small_dy case does not test what it claims: %s" % r)
        if what == "dz":
            if not (r["dz_max"] > 65504 and r["x_max"] < 32 and r["h_max"] < 128 and r["w_max"] < 32768):
                msgs.append("the dz case does not test what it claims: %s" % r)
        if "finite" in r and not r["finite"]:
            msgs.append("non-finite results")
        if "err" in r:
            if what == "weight" and direction == "backward":
                if max(r["err_vs_fp32_kernel"]) > 1e-5:
                    msgs.append("not the fp32 kernel's answer: %s" % r["err_vs_fp32_kernel"])
            else:
                bars = [max(4 * t, 5e-6) for t in r["err_t32"]]
                if not all(e <= b for e, b in zip(r["err"], bars)):
                    msgs.append("beyond the fp32 bar: %s vs %s" % (r["err"], bars))
        if r["form_after"] != 1 or not r["fwd_after_declined"]:
            msgs.append("the sticky switch is not up afterwards (form %d, forward declined %s)" % (r["form_after"], r["fwd_after_declined"]))
        if msgs:
            failures.append((case, msgs))
    # the parent's own switch is still down: the split-fp16 tests elsewhere assert form() == 2 in any order
    from permuto_sdf_amd.mlp import mlp_backward_raw
    lin = [l.to(dev) for l in _net(COLOUR, 1)]
    mlp_backward_raw(COLOUR, torch.randn(111, 64, device=dev), [l.weight for l in lin], [l.bias for l in lin],
                     torch.randn(3, 64, device=dev), need_dx=True)
    form = L.lib().psdf_mlp_backward_wide_form
    form.restype = ctypes.c_int
    assert form() == 2
    assert not failures, failures
