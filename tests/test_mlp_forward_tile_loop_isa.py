"""CPU guard on the instruction stream of the split forward's tile loop (csrc/mlp.hip, mlp_fwd_split_tiles): reads the gfx950
code object hipcc produced, like tests/test_kernel_resources_mlp_forward.py.

With four waves on every SIMD the forward is bound by vector-ALU issue, so what the tile loop may not grow back is pinned on
the instantiation bench.py runs, mlp_fwd_split_wg_kernel<2, 2, 2, 1, true, 3, true, 8>:
  * no per-lane integer multiply in a tile loop (row bases are scalar; the partial last k-step clamps the scalar row);
  * the loop with 32-bit lane offsets addresses every layer-0 operand as scalar base + 32-bit vector offset;
  * the operand split is v_cvt_pk_f16_f32 + v_fma_mixlo/hi_f16: no conversion back to fp32, no packed fp32 subtraction;
  * max(z, 0) of the GELU tail is one v_med3_f32, not a canonicalising pair of v_max_f32.
The kernel holds two tile loops, one per addressing form (x_offsets_fit32); a tile loop is a backward branch whose body holds
matrix instructions."""
import os
import re
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
BENCH = "mlp_fwd_split_wg_kernelILi2ELi2ELi2ELi1ELb1ELi3ELb1ELi8E"


@pytest.fixture(scope="module")
def tile_loops(tmp_path_factory):
    """[[(opcode, operands)]]: the tile loops of the bench instantiation, in program order"""
    from permuto_sdf_amd import build
    build.build(verbose=False)
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip("ROCm LLVM tools not found")
    tmp = str(tmp_path_factory.mktemp("isa"))
    fat, co = os.path.join(tmp, "x.fatbin"), os.path.join(tmp, "x.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat,
                           os.path.join(build.OBJDIR, "mlp.o"), os.devnull])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co])
    text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", co], text=True)
    ins, cur = [], False
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
        if m:
            cur = BENCH in m.group(1)
            continue
        if not cur:
            continue
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-F]+):", line)
        if m:
            ins.append((m.group(1), m.group(2), int(m.group(3), 16)))
    assert ins, "the bench instantiation is not in mlp.o"
    at = {a: i for i, (_, _, a) in enumerate(ins)}
    spans = []
    for i, (op, args, a) in enumerate(ins):
        if op.startswith(("s_branch", "s_cbranch")):
            off = int(args.split()[0])
            off = off - 65536 if off >= 32768 else off
            tgt = a + 4 + off * 4
            if off < 0 and tgt in at and any(o.startswith("v_mfma") for o, _, _ in ins[at[tgt]:i]):
                spans.append((at[tgt], i))
    # outermost spans only (a loop inside a tile loop is part of it)
    outer = [s for s in spans if not any(t != s and t[0] <= s[0] and s[1] <= t[1] for t in spans)]
    assert outer, "no tile loop found"
    return [[(op, args) for op, args, _ in ins[a:b + 1]] for a, b in sorted(outer)]


def _count(loop, prefix):
    return sum(op.startswith(prefix) for op, _ in loop)


def test_tile_loops_have_no_vector_integer_multiply(tile_loops):
    for loop in tile_loops:
        assert _count(loop, "v_mfma") == 66, "not a whole tile: %d matrix instructions" % _count(loop, "v_mfma")
        for op in ("v_mul_lo_u32", "v_mad_u64_u32", "v_mul_hi_u32", "v_mad_i64_i32"):
            assert _count(loop, op) == 0, (op, _count(loop, op))


def test_one_tile_loop_loads_its_operands_from_scalar_bases(tile_loops):
    scalar_base = re.compile(r"^v\d+, v\d+, s\[\d+:\d+\]")
    hits = 0
    for loop in tile_loops:
        loads = [args for op, args in loop if op == "global_load_dword"]
        assert len(loads) >= 24, len(loads)       # three k-steps of eight values (the partial forms are counted on top)
        if all(scalar_base.match(a) for a in loads):
            hits += 1
    assert hits == 1, "%d of %d tile loops use scalar base + 32-bit lane offset for every operand load" % (hits, len(tile_loops))


def test_operand_split_and_gelu_tail_forms(tile_loops):
    for loop in tile_loops:
        # 11 k-steps of four pairs: one packed conversion and two fma-mix per pair
        assert _count(loop, "v_cvt_pk_f16_f32") == 44 and _count(loop, "v_fma_mix") == 88, \
            (_count(loop, "v_cvt_pk_f16_f32"), _count(loop, "v_fma_mix"))
        assert _count(loop, "v_cvt_f32_f16") == 0 and _count(loop, "v_pk_add_f32") == 0
        # 96 activations per lane (3 layers x 2 tiles x 16 registers): one v_med3_f32 each for max(z, 0)
        assert _count(loop, "v_max_f32") == 0 and _count(loop, "v_med3_f32") == 96, \
            (_count(loop, "v_max_f32"), _count(loop, "v_med3_f32"))
