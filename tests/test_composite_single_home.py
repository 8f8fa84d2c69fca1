"""What the compositing kernels share lives in ONE header, permuto_sdf_amd/csrc/composite_device.h: the transmittance step, the
forward sweep of a ray, the suffix step of the fused backwards, the NeuS and NeRF opacities with their backwards, the mid-point
rule of sdf2alpha, F.normalize.  These tests read the sources with the comments stripped: a constant of one of these expressions
that turns up in a second file, a product scan called outside the header or a helper called without it is a copy coming back.
No GPU, no library."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "permuto_sdf_amd", "csrc")
SOURCES = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))}
CODE = {f: re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S)) for f, src in SOURCES.items()}
HOME = "composite_device.h"
HELPERS = ("section", "section_backward", "clip01", "softplus20", "nerf_alpha", "nerf_alpha_backward", "sdf2alpha_midpoint",
           "normalize_eps", "normalize_bwd", "one_minus", "sweep", "sweep_chunk", "wave_incl_suffix_add", "poison", "poison_ray")
HELPER_TYPES = ("Transmittance", "SuffixStep", "RayIndex")
COMPOSITING = ("neus.hip", "volume_rendering.hip", "composite_fused.hip", "frame_composite.hip")


def _includes(f, seen=None):
    """every csrc file that f includes, directly or through another"""
    seen = set() if seen is None else seen
    for inc in re.findall(r'#include\s+"([^"]+)"', SOURCES[f]):
        if inc in SOURCES and inc not in seen:
            seen.add(inc)
            _includes(inc, seen)
    return seen


def _files_with(text):
    return [f for f, src in CODE.items() if text in src]


def test_the_product_scan_is_called_in_the_header_only():
    callers = [f for f, src in CODE.items() if re.search(r"(?<!float )\bwave_incl_scan_mul\s*\(", src)]
    assert callers == [HOME]
    assert [f for f, src in CODE.items() if re.search(r"float wave_incl_scan_mul\s*\(", src)] == ["psdf_common.h"]


def test_each_constant_of_a_shared_expression_is_written_in_one_file():
    # the factor 1 - alpha + 1e-7, the NaN of an over-long ray, the opacity backward's quotient rule, the eps of F.normalize
    for text in ("1e-7f", "0x7fc00000", "den * den", "1e-12f"):
        assert _files_with(text) == [HOME], text
    # softplus with torch's threshold: here, and mlp_wide.hip's own for the Lipschitz norm (it does not include this header)
    assert _files_with("log1pf(expf(") == [HOME, "mlp_wide.hip"]
    assert HOME not in _includes("mlp_wide.hip")


def test_every_helper_is_defined_once_and_its_callers_include_the_header():
    for name in HELPERS:
        defs = [f for f, src in CODE.items() if re.search(r"__forceinline__\s+[\w:]+\s+%s\s*\(" % name, src)]
        assert defs == [HOME], (name, defs)
    for name in HELPER_TYPES:
        assert [f for f, src in CODE.items() if re.search(r"\bstruct\s+%s\b" % name, src)] == [HOME], name
    use = re.compile(r"\b(%s)\s*\(|\b(%s)\b" % ("|".join(HELPERS), "|".join(HELPER_TYPES)))
    users = [f for f, src in CODE.items() if f != HOME and use.search(src)]
    assert set(COMPOSITING) <= set(users)
    for f in users:
        assert HOME in _includes(f), f
    # the kernels that sweep a ray do so through the helpers: each of these files uses the transmittance step
    for f in ("volume_rendering.hip", "composite_fused.hip", "frame_composite.hip"):
        assert re.search(r"\bTransmittance\b|\bsweep\s*\(", CODE[f]), f
    assert not re.search(r"\bnormalized\s*\(", CODE["frame_composite.hip"])


def test_the_chunk_dispatch_of_the_fused_backwards_is_a_template():
    src = CODE["composite_fused.hip"]
    assert "#define GO(" not in src and not re.search(r"#define\s+GO\b", src)
    assert len(re.findall(r"\bdispatch_chunks\s*\(", src)) == 3          # its definition and the two backwards
