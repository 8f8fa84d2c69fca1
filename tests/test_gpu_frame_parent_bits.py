"""The writers of image planes give, bit for bit, what they gave before their shared expressions moved into ONE header
(csrc/frame_device.h: the three-channel store, the camera-frame normal, the depth along a ray, the surface pixel, the box test)
and their range checks into ONE function (csrc/frame_plan.h).

The bit tests of whole frames against the operator chains (tests/test_gpu_frame_trace.py, test_gpu_box_trace.py,
test_gpu_sdf_slice.py, test_gpu_nerf_view.py) run a network in between; here the raw entries run alone, on inputs made for the
edges, and the bits of the commit before the move are pinned in tests/golden/frame_parent_bits.npz (tools/make_frame_golden.py
wrote it with that commit's library; the file names the commit and the library's sha256).  Inputs: a 7 x 13 frame whole and pixels
[77, 410) of 40 x 48; slots none / all / mixed; strides 3 and 4; camera normals on and off; gradients below the eps of the
normalisation; direction components of exactly 0; points exactly on a face of the box; an sdf_end on either side of the coverage
threshold, on it, and a NaN; SDF values exactly on the edges of the iso-bands; the `bordersK` containers of
oracle/composite_cases.py for the NeRF foreground, with and without its depth plane, and a container without samples.  Output
buffers start from a sentinel: what a kernel must leave alone is compared too.  psdf_frame_composite_neus / _nerf are pinned in
tests/test_gpu_composite_parent_bits.py."""
import os

import numpy as np
import pytest
import torch

from tools.make_frame_golden import SENTINEL, SENTINEL_U8, outputs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_parent_bits.npz")
BITS = {torch.float32: torch.int32, torch.uint8: torch.uint8}


def test_every_frame_writing_entry_point_gives_the_parents_bits(dev):
    gold = np.load(GOLDEN)
    names = [n for n in gold.files if n not in ("generated_from_commit", "library_sha256")]
    got = outputs(dev)
    assert sorted(got) == sorted(names) and len(names) == 222
    assert len(str(gold["generated_from_commit"])) == 40 and len(str(gold["library_sha256"])) == 64
    differ = []
    for name in names:
        want = torch.from_numpy(gold[name])
        have = got[name].cpu()
        assert have.shape == want.shape and have.dtype == want.dtype and want.dtype in BITS, name
        a, b = have.view(BITS[want.dtype]), want.view(BITS[want.dtype])              # the bit patterns: -0 and NaNs count
        if not torch.equal(a, b):
            differ.append("%s: %d of %d entries" % (name, int((a != b).sum()), want.numel()))
    assert not differ, differ
    # the file pins results, not sentinels: every tensor holds written entries, and what lies outside the chunk (the other pixels
    # of the 40 x 48 frame and of the S = 40 layer, the two rows behind every per-ray array, the pixels the NeRF container's few
    # rays do not reach, the pixels a cut leaves to the view's colour) kept the sentinel

    def sentinel(n):
        return SENTINEL_U8 if gold[n].dtype == np.uint8 else SENTINEL

    assert all(bool((torch.from_numpy(gold[n]) != sentinel(n)).any()) for n in names)
    whole_frame = [n for n in names if ("/7x13/" in n or "/S7/" in n) and gold[n].ndim == 3 and not n.startswith(("nerf_frame/", "slice_cut_resolve/"))]
    assert len(whole_frame) == 44           # 7 x 13 and S = 7 are written whole: no sentinel survives there
    assert not any(bool((torch.from_numpy(gold[n]) == sentinel(n)).any()) for n in whole_frame)
    assert all(bool((torch.from_numpy(gold[n]) == sentinel(n)).any()) for n in names if n not in whole_frame
               and not (n.startswith("slice_cut_resolve/7x13/") and not n.endswith("/rgb")))
