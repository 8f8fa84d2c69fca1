"""CPU guard on the register budget of the paired encode forward (csrc/encode.hip: encode_fwd_pair_kernel), read from the gfx950
code object the way tests/test_kernel_resources.py reads the others.

A thread of that kernel carries two levels: two simplices' worth of loop-invariant scalars is what would cost it a wave (800 scalar
registers per SIMD: 8 waves leave 96 + VCC etc. = 102 allocated per wave), and spilled scalar registers come back as
v_readlane in a loop that is bound by vector issue at its coarse level."""
import os

import pytest

from .test_kernel_resources import LLVM, _kernels, _one


@pytest.fixture(scope="module")
def encode_kernels(tmp_path_factory):
    from permuto_sdf_amd import build
    build.build(verbose=False)
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip("ROCm LLVM tools not found")
    return _kernels(os.path.join(build.OBJDIR, "encode.o"), str(tmp_path_factory.mktemp("encode_co")))


def test_the_bench_instantiation_keeps_eight_waves_per_simd(encode_kernels):
    k = _one(encode_kernels, r"encode_fwd_pair_kernelILi3ELi2ELb1E")        # <P = 3, F = 2, PLAIN>: the hot path's forward
    assert k["vgpr_count"] <= 64 and k["sgpr_count"] <= 102, k
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k


def test_the_general_instantiation_does_not_spill(encode_kernels):
    k = _one(encode_kernels, r"encode_fwd_pair_kernelILi3ELi2ELb0E")        # with a skip mask / a touched-block map
    assert k["vgpr_count"] <= 64, k
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k


def test_no_instantiation_uses_scratch_or_spills_vector_registers(encode_kernels):
    hits = {n: k for n, k in encode_kernels.items() if "encode_fwd_pair_kernel" in n}
    assert len(hits) == 8                                                    # four (P, F) x PLAIN or not
    for n, k in hits.items():
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (n, k)


def test_the_pair_kernel_is_not_counted_as_the_one_level_kernel(encode_kernels):
    # tests/test_kernel_resources.py looks the one-level kernel up by a pattern that must keep matching exactly one name
    assert len([n for n in encode_kernels if "encode_fwd_kernelILi3ELi2ELb1E" in n]) == 1
    assert not [n for n in encode_kernels if "encode_fwd_pair_kernel" in n and "encode_fwd_kernel" in n]
