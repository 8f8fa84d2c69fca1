"""The host side of the NeRF frame renderer (permuto_sdf_amd/nerf_view.py, csrc/frame_composite.hip: frame_render_nerf_kernel),
checked without a GPU.

  * the header declares the entry with the reference lines it replaces, and the library exports it;
  * an empty batch returns before any pointer check, and every bad argument returns its code before a launch;
  * the module refuses CPU tensors;
  * the kernel's code object holds no spill, no scratch and no LDS.

The ray kernel uses wave shuffles, which tests/host/hip_on_host does not model: what it computes is covered on the GPU
(tests/test_gpu_nerf_view.py).

The entry is psdf_nerf_frame_render and its section stands BEFORE the NeuS renderer's in the header:
tests/test_frame_host.py pins the `psdf_frame_*` prototypes, and the `replaces:` lines from that section to the end of the
header, to the NeuS renderer's four -- as psdf_trace_frame_* (frame_trace.hip) stands before it for the same reason."""
import ctypes
import os
import re
import types

import pytest
import torch

from tests.test_kernel_resources import _kernels, _one, objdir  # noqa: F401  (the fixture, and the metadata reader)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "psdf_nerf_frame_render"


@pytest.fixture(scope="module")
def lib():
    from permuto_sdf_amd import build
    return ctypes.CDLL(build.build(verbose=False))


def test_header_declares_the_entry_and_the_library_exports_it(lib):
    header = open(os.path.join(ROOT, "include", "psdf.h")).read()
    assert len(re.findall(r"\bint %s\s*\(" % ENTRY, header)) == 1 and hasattr(lib, ENTRY)
    proto = header[header.index("int " + ENTRY + "("):].split(";")[0]
    args = [a.strip().split()[-1].lstrip("*") for a in re.sub(r"\s+", " ", proto[proto.index("(") + 1:proto.rindex(")")]).split(",")]
    assert args == ["nr_rays", "start_end", "equal", "fixed", "max_nr_samples", "raw_density", "dt", "z", "rgb", "H", "W",
                    "pixel_first", "rgb_img", "weights_sum_img", "depth_img", "transmittance", "stream"]
    comment = header[:header.index("int " + ENTRY + "(")].rsplit("/*", 1)[1]
    assert "replaces: train_nerf.py:66-71,92-128" in comment
    # the kernel states its traffic next to the two kernels it joins, and takes every ray helper from the one header
    src = open(os.path.join(ROOT, "permuto_sdf_amd", "csrc", "frame_composite.hip")).read()
    assert "20 B per sample read (raw density 4, dt 4, rgb 12), 24 B with the depth" in src
    body = src[src.index("frame_render_nerf_kernel("):src.index("// the pixel range")]
    for helper in ("RAY_LOOP(", "ri.get(", "ri.valid(", "sweep(", "nerf_alpha(", "wave_sum(", "st_planes("):
        assert helper in body, helper
    assert "__shared__" not in src


def test_empty_batch_returns_before_any_pointer_check_and_bad_arguments_are_refused(lib):
    st = None
    z, p = ctypes.c_int64(0), ctypes.c_void_p(4096)          # (never read: every call below returns before a launch)
    fn = getattr(lib, ENTRY)
    assert fn(0, None, 0, 0, 0, None, None, None, None, 0, 0, z, None, None, None, None, st) == 0
    assert fn(-3, None, 0, 0, 0, None, None, None, None, 0, 0, z, None, None, None, None, st) == 0

    def render(R=10, se=p, equal=0, fixed=0, M=100, raw=p, dt=p, zs=p, rgb=p, H=41, W=53, first=37, img=p, ws=p, depth=p, T=p):
        return fn(R, se, equal, fixed, M, raw, dt, zs, rgb, H, W, ctypes.c_int64(first), img, ws, depth, T, st)

    for k in ("se", "raw", "dt", "rgb", "img", "ws", "T"):      # each required pointer
        assert render(**{k: None}) == -1, k
        assert render(**{k: None}, depth=None, zs=None) == -1, k
    assert render(zs=None) == -1                                 # a depth plane without z
    assert render(M=-1) == -1 and render(equal=1, fixed=-1, se=None) == -1
    assert render(H=0) == -1 and render(W=-1) == -1 and render(first=-1) == -1
    assert render(first=41 * 53 - 9) == -1                       # the last ray lies one pixel past the frame
    assert render(H=65536, W=32768) == -2                        # H W = 2^31
    # a container without samples comes without sample tensors, but never without planes
    for k in ("img", "ws", "T"):
        assert render(M=0, raw=None, dt=None, zs=None, rgb=None, **{k: None}) == -1, k


def test_module_refuses_cpu_tensors_before_it_touches_a_device():
    import permuto_sdf_amd
    from permuto_sdf_amd import nerf_view, render
    from permuto_sdf_amd._lib import PsdfError
    assert permuto_sdf_amd.nerf_view is nerf_view and "nerf_view" in permuto_sdf_amd.__all__
    planes = [torch.zeros(c, 4, 4) for c in (3, 1, 1)]
    rs = types.SimpleNamespace(samples_dt=torch.zeros(8, 1), samples_z=torch.zeros(8, 1))
    with pytest.raises(PsdfError):          # a CPU tensor: there is no CPU path
        nerf_view.frame_render_nerf_raw(rs, torch.zeros(8), torch.zeros(8, 3), 4, 4, 0, planes[0], planes[1], torch.zeros(16), planes[2])
    with pytest.raises(PsdfError):
        nerf_view.frame_render_nerf_raw(rs, None, None, 4, 4, 0, planes[0], planes[1], torch.zeros(16))
    holder = types.SimpleNamespace(net=types.SimpleNamespace(encoding=types.SimpleNamespace(lattice_values=torch.zeros(1))),
                                   net_bg=None, grid=None, sphere=None, hp=None, with_mask=True)
    with pytest.raises(PsdfError):
        nerf_view.NerfFrameRenderer(holder).render(render.Frame(torch.eye(3), torch.eye(4), 4, 4))
    with pytest.raises(PsdfError):
        nerf_view.NerfFrameRenderer.from_checkpoint("nowhere", "cpu")
    with pytest.raises(ValueError):
        nerf_view.NerfFrameRenderer(holder).render_views([])
    fields = [f.name for f in nerf_view.dataclasses.fields(nerf_view.NerfRenderedFrame)]
    assert fields == ["rgb", "rgb_bg", "weights_sum", "depth"]


def test_the_kernel_holds_no_spill_no_scratch_and_no_lds(objdir, tmp_path):  # noqa: F811
    k = _one(_kernels(os.path.join(objdir, "frame_composite.o"), str(tmp_path)), r"frame_render_nerf_kernel")
    print(k)
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] == 0, k
