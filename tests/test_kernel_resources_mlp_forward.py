"""CPU guard on the register budget of the wide workgroup forms of the split forward (csrc/mlp.hip, mlp_fwd_split_wg_kernel):
reads the gfx950 code objects hipcc produced, like tests/test_kernel_resources.py.

The wide forms exist to put FOUR waves on every SIMD (one 16-wave workgroup per CU, or two 8-wave ones, on one weight image
each).  A SIMD lane has 512 registers, so four waves fit only with at most 128 each, and a spill would put scratch traffic
into a kernel that is VALU bound: every instantiation must stay within 128 registers with nothing in scratch."""
import os
import re
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"


def _kernels(obj, tmp):
    """{mangled name: {field: int}} of the gfx950 code object embedded in an object file (as in tests/test_kernel_resources.py)"""
    fat = os.path.join(tmp, "x.fatbin")
    co = os.path.join(tmp, "x.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.devnull])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co])
    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    out = {}
    for block in re.split(r"\n  - \.", notes):
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name:
            continue
        out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.?(\w+):\s+(\d+)\s*$", block, flags=re.M)}
    return out


@pytest.fixture(scope="module")
def objdir():
    from permuto_sdf_amd import build
    build.build(verbose=False)
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip("ROCm LLVM tools not found")
    return build.OBJDIR

# <T1, T2, T3, OUT_T, FINAL_DOT, CH, F16, W>: the 64-wide rows of PSDF_MLP32_ROWS with one output tile
WIDE = re.compile(r"mlp_fwd_split_wg_kernelILi2ELi2ELi([02])ELi1ELb1ELi([1-4])ELb([01])ELi(\d+)E")


def test_wide_forward_forms_fit_four_waves_per_simd(objdir, tmp_path):
    k = _kernels(os.path.join(objdir, "mlp.o"), str(tmp_path))
    wide = {n: v for n, v in k.items() if "mlp_fwd_split_wg_kernel" in n}
    assert wide, "no wide form of the split forward is built"
    seen = set()
    for n, v in wide.items():
        m = WIDE.search(n)
        assert m, "a wide form outside the 64-wide rows: %s" % n
        seen.add((int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4))))
        assert v["vgpr_count"] <= 128, (n, v)
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (n, v)
    widths = {w for _, _, _, w in seen}
    assert widths <= {8, 16}
    for W in widths:
        # every chunk count of layer 0 (1 .. 4 k-steps: up to 64 inputs), both piece forms of the three-hidden-layer net and the
        # bf16 form of the two-hidden-layer one
        want = {(2, ch, f, W) for ch in range(1, 5) for f in (0, 1)} | {(0, ch, 0, W) for ch in range(1, 5)}
        assert {s for s in seen if s[3] == W} == want, sorted(seen)


def test_four_wave_forward_keeps_its_name(objdir, tmp_path):
    """the dispatch and resource tests find the four-wave form by its mangled name: seven template arguments, no W"""
    k = _kernels(os.path.join(objdir, "mlp.o"), str(tmp_path))
    hits = [n for n in k if re.search(r"mlp_fwd_split_kernelILi2ELi2ELi2ELi1ELb1ELi3ELb1EEEv", n)]
    assert len(hits) == 1, hits
