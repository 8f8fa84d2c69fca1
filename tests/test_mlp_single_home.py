"""The GELU evaluators of the MLP kernels live in ONE header, permuto_sdf_amd/csrc/gelu_device.h, and the layout that the two
split backwards of the SDF net share in ONE other, mlp_split_layout.h.  These tests read the sources: a coefficient that turns
up in a second file, an evaluator called without the header, or a second definition of the gradient image is a copy coming
back.  No GPU, no library."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "permuto_sdf_amd", "csrc")
SOURCES = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))}
# first coefficient of the rational fit's P6 and of the two erf polynomials
FIRST_COEFFICIENTS = ("5.384693295e-02", "1.72853470e-5", "5.96761703e-4")
EVALUATORS = ("erf_fast", "erf_fast2", "gelu_exact2", "gelu_rational", "gelu_rational2", "gelu_erf", "gelu_rational_both",
              "gelu_rational4", "gelu_erf2", "gelu_erf2_dd")


def _includes(f, seen=None):
    """every csrc file that f includes, directly or through another"""
    seen = set() if seen is None else seen
    for inc in re.findall(r'#include\s+"([^"]+)"', SOURCES[f]):
        if inc in SOURCES and inc not in seen:
            seen.add(inc)
            _includes(inc, seen)
    return seen


def test_each_fit_is_written_out_in_gelu_device_h_only():
    for coeff in FIRST_COEFFICIENTS:
        assert [f for f, src in SOURCES.items() if coeff in src] == ["gelu_device.h"], coeff


def test_every_caller_of_an_evaluator_includes_gelu_device_h():
    call = re.compile(r"\b(%s)\s*\(" % "|".join(EVALUATORS))
    code = {f: re.sub(r"//[^\n]*", "", src) for f, src in SOURCES.items()}
    callers = [f for f, src in code.items() if f != "gelu_device.h" and call.search(src)]
    assert {"mlp_device.h", "mlp_bwd.hip", "mlp_bwd_split.hip", "mlp_bwd_split_f16.hip", "mlp_wide.hip"} <= set(callers)
    for f in callers:
        assert "gelu_device.h" in _includes(f), f
    # every evaluator is defined once, in the header
    for name in EVALUATORS:
        defs = [f for f, src in code.items() if re.search(r"__forceinline__\s+[\w:]+\s+%s\s*\(" % name, src)]
        assert defs == ["gelu_device.h"], name


def test_the_gradient_image_is_defined_once():
    assert [f for f, src in SOURCES.items() if re.search(r"\bG_TOTAL\s*=", src)] == ["mlp_split_layout.h"]
    for f in ("mlp_bwd_split.hip", "mlp_bwd_split_f16.hip"):
        assert "mlp_split_layout.h" in _includes(f), f
    assert "mlp_split_layout.h" in _includes("mlp_bwd_split_double.hip")     # through mlp_bwd_split.hip
