"""What the per-entry float64 tests share (tests/test_gpu_composite_float64.py, tests/test_gpu_tails_float64.py,
tests/test_gpu_optim_float64.py): every entry of a kernel output against its float64 value and its own bar."""
import torch

from oracle import composite_float64 as c64


def check(out, name, got, ref, bar, keep=None):
    """every entry inside its bar; records worst error / bar and the bites / saturated shares"""
    got = got.detach().cpu().double().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), name
    err = (got - ref).abs()
    rel = err / bar.clamp_min(1e-300)
    if keep is not None:                                            # excluded entries (rows) take no part; indices stay unfiltered
        k = keep if keep.dim() == rel.dim() else keep.view(-1, *([1] * (rel.dim() - 1))).expand_as(rel)
        rel = torch.where(k, rel, torch.zeros_like(rel))
        bad = (err > bar) & k
        b, s = c64.bites(ref[keep], bar[keep])
    else:
        bad = err > bar
        b, s = c64.bites(ref, bar)
    ratio = float(rel.max()) if rel.numel() else 0.0
    out.append("%s %.3f (%.0f%% / %.0f%%)" % (name, ratio, 100 * b, 100 * s))
    if bool(bad.any()):
        at = int(rel.reshape(-1).argmax())
        raise AssertionError("%s: %d entries outside their bar, worst error / bar %.4g at flat index %d of shape %s: kernel %r, float64 %r, bar %r" % (
            name, int(bad.sum()), ratio, at, tuple(ref.shape), float(got.reshape(-1)[at]), float(ref.reshape(-1)[at]),
            float(bar.reshape(-1)[at])))
    return ratio, b


def show(case, out):
    print("%s: worst error / bar (bites / saturated) " % case + ", ".join(out))
