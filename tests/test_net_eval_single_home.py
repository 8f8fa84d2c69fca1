"""Evaluating a lattice + MLP net outside autograd has ONE home on the host, permuto_sdf_amd/net_eval.py: the 1-row head, the
masked evaluation, the masked analytic gradient, the two-launch scalar-only evaluation and the raw-pass helpers of the
hand-written steps.  These tests read the package's Python with comments and docstrings stripped: a head sliced in a second file,
a masked-gradient launch issued from a second file, a trainer reaching into another trainer's private names, or a second
`map_range_val` is a copy coming back.  No GPU, no library."""
import io
import os
import re
import tokenize

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "permuto_sdf_amd")
HOME = "net_eval.py"


def _code(path):
    """the file's text with comments and docstrings (string literals that are a statement of their own) blanked out"""
    with open(path) as f:
        src = f.read()
    lines = src.splitlines(True)
    prev = tokenize.NEWLINE
    for tok in tokenize.generate_tokens(io.StringIO(src).readline):
        (r0, c0), (r1, _) = tok.start, tok.end
        if tok.type == tokenize.COMMENT:
            lines[r0 - 1] = lines[r0 - 1][:c0] + "\n"
        elif tok.type == tokenize.STRING and prev in (tokenize.NEWLINE, tokenize.INDENT, tokenize.DEDENT):
            for r in range(r0, r1 + 1):
                lines[r - 1] = "\n"
        if tok.type not in (tokenize.NL, tokenize.COMMENT):
            prev = tok.type
    return "".join(lines)


LINES = {f: _code(os.path.join(PKG, f)) for f in sorted(os.listdir(PKG)) if f.endswith(".py")}


def _files_with(needle):
    squeezed = needle.replace(" ", "")
    return [f for f, text in LINES.items() if squeezed in text.replace(" ", "")]


def test_the_stripping_keeps_code_and_drops_docstrings():
    text = LINES[HOME]
    assert "def one_row_head" in text and "channel 0 of the last layer is the SDF" not in text


def test_the_one_row_head_is_sliced_in_one_file():
    assert _files_with("[0:1].contiguous()") == [HOME]


def test_the_masked_gradient_launches_are_issued_from_one_file():
    for name in ("psdf_mlp_backward_data_masked", "psdf_encode_backward_positions_masked",
                 "psdf_encode_backward_positions_workspace_bytes"):
        assert _files_with(name) == [HOME], name


def test_no_trainer_reaches_into_train_manuals_private_names():
    assert _files_with("from .train_manual import _") == []
    local = [f for f, text in LINES.items() if re.search(r"^[ \t]+from \.train_manual import", text, re.M)]
    assert local == []


def test_map_range_val_is_defined_once():
    defs = [(f, m) for f, text in LINES.items() for m in re.findall(r"\bdef _?map_range_val\b", text)]
    assert len(defs) == 1 and defs[0][0] == "encoding.py", defs
    from permuto_sdf_amd import encoding, train_step
    assert train_step.map_range_val is encoding.map_range_val


def test_tracers_and_mesh_do_not_build_the_launch_arguments_themselves():
    for f in ("sphere_trace.py", "box_trace.py", "mesh.py"):
        for name in ("_head", "_tail", "_dims_array"):
            assert not re.search(r"import[^\n]*\b%s\b" % name, LINES[f]), (f, name)
            assert not re.search(r"\b%s\(" % name, LINES[f]), (f, name)


def test_the_home_is_a_leaf():
    imports = re.findall(r"^from \.(\w+) import|^from \. import (\w+)", LINES[HOME], re.M)
    assert {a or b for a, b in imports} == {"_lib", "encoding", "mlp"}
