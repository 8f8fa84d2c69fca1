"""The compositing kernels give, bit for bit, what they gave before their shared expressions moved into ONE header
(csrc/composite_device.h: the transmittance step, the ray sweep, the suffix step, the two opacities, F.normalize).

The bit tests between kernels (frame == fused, fused opacity == opacity kernels, fused == operator chain, cdf == chain) now partly
compare a definition with itself, so the bits of the commit before the move are pinned in
tests/golden/composite_parent_bits.npz (tools/make_composite_golden.py wrote it with that commit's library; the file names the
commit and the library's sha256).  Inputs: the `bordersK` containers of oracle/composite_cases.py -- every 64-sample chunk border
-1 / +0 / +1, empty and overflowed rays, one ray longer than four chunks for the any-length kernels, K = 1, 2 and 4 register
chunks of the fused backwards with the reference's channel quirk on and off.  Output buffers start from a sentinel: what a
kernel must leave alone is compared too.  g_inv_s is not in the file (a sum of atomics in no fixed order: its float64 bar is in
tests/test_gpu_composite_float64.py)."""
import os

import numpy as np
import pytest
import torch

from tools.make_composite_golden import outputs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "composite_parent_bits.npz")


def test_every_compositing_entry_point_gives_the_parents_bits(dev):
    gold = np.load(GOLDEN)
    names = [n for n in gold.files if n not in ("generated_from_commit", "library_sha256")]
    got = outputs(dev)
    assert sorted(got) == sorted(names) and len(names) == 105
    assert len(str(gold["generated_from_commit"])) == 40
    differ = []
    for name in names:
        want = torch.from_numpy(gold[name])
        have = got[name].cpu()
        assert have.shape == want.shape and have.dtype == want.dtype == torch.float32, name
        if not torch.equal(have.view(torch.int32), want.view(torch.int32)):       # the bit patterns: -0 and NaNs count
            differ.append("%s: %d of %d entries" % (name, int((have.view(torch.int32) != want.view(torch.int32)).sum()), want.numel()))
    assert not differ, differ
    # the file pins results, not sentinels: every tensor holds written entries, and the skipped slots kept the sentinel
    from tools.make_composite_golden import SENTINEL
    assert all(bool((torch.from_numpy(gold[n]) != SENTINEL).any()) for n in names)
    assert all(bool((torch.from_numpy(gold[n]) == SENTINEL).any()) for n in names if n.endswith(("/g_sdf", "/weights", "/g_raw")) and "alpha/" not in n)
