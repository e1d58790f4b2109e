"""Every compute launcher of the kernel-level ABI (include/visp_hip_kernels.h) is named by some test IN CODE -- a call, an attribute access on
the library, a string of an entry-point table: a launcher no file under tests/ calls is one whose numbers nothing checks, and a comment or a
docstring that mentions its name checks nothing either, so both are stripped before the search. Runtime plumbing is the one allowlist below,
each entry with its reason."""
import io
import re
import tokenize
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "visp_hip_kernels.h"

PLUMBING = {
    "vx_last_error": "error string of the last failed call",
    "vx_device_count": "device query",
    "vx_set_device": "device selection",
    "vx_device_info": "device query",
    "vx_malloc": "allocation",
    "vx_free": "allocation",
    "vx_malloc_host": "pinned host allocation",
    "vx_free_host": "pinned host allocation",
    "vx_memset": "memory fill",
    "vx_memcpy_h2d": "copy",
    "vx_memcpy_d2h": "copy",
    "vx_memcpy_d2d": "copy",
    "vx_memcpy_h2d_async": "copy",
    "vx_memcpy_d2h_async": "copy",
    "vx_event_create": "events",
    "vx_event_destroy": "events",
    "vx_event_record": "events",
    "vx_event_sync": "events",
    "vx_event_elapsed_ms": "events",
    "vx_stream_create": "streams",
    "vx_stream_destroy": "streams",
    "vx_stream_sync": "streams",
    "vx_stream_wait_event": "streams",
    "vx_graph_begin_capture": "graph capture",
    "vx_graph_end_capture": "graph capture",
    "vx_graph_launch": "graph capture",
    "vx_graph_destroy": "graph capture",
    "vx_dconv_prepare": "one-time kernel attribute setup, no arithmetic",
    "vx_conv3x3_supported": "shape query of the lowering; vx_conv3x3_f16 itself is tested",
}


def _launchers():
    text = HEADER.read_text()
    names = set(re.findall(r"VX_API\s+[\w\s\*]+?\b(vx_\w+)\s*\(", text))
    assert len(names) > 100, "the header parse found too few launchers"
    return names


def python_code(text: str) -> str:
    """the tokens of a Python source without its comments and without its docstrings (any string that is a statement of its own)"""
    tokens = [t for t in tokenize.generate_tokens(io.StringIO(text).readline) if t.type not in (tokenize.COMMENT, tokenize.NL)]
    out = []
    for i, tok in enumerate(tokens):
        starts_statement = i == 0 or tokens[i - 1].type in (tokenize.NEWLINE, tokenize.INDENT, tokenize.DEDENT)
        if tok.type == tokenize.STRING and starts_statement and tokens[i + 1].type in (tokenize.NEWLINE, tokenize.ENDMARKER):
            continue
        out.append(tok.string)
    return " ".join(out)


def c_code(text: str) -> str:
    """a C or C++ source without its comments"""
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def _named_in_tests(skip=()):
    corpus = []
    for p in sorted((ROOT / "tests").rglob("*")):
        if p.is_file() and p.suffix in (".py", ".cpp", ".c", ".h") and p.name != Path(__file__).name and p.name not in skip:
            text = p.read_text(errors="replace")
            corpus.append(python_code(text) if p.suffix == ".py" else c_code(text))
    return "\n".join(corpus)


def _missing(corpus):
    names = _launchers()
    return sorted(n for n in names - set(PLUMBING) if not n.endswith("_set_stamps") and not re.search(rf"\b{n}\b", corpus))


def test_every_compute_launcher_is_named_by_a_test():
    names = _launchers()
    assert set(PLUMBING) <= names, sorted(set(PLUMBING) - names)
    missing = _missing(_named_in_tests())
    assert not missing, f"launchers no test names in code: {missing}"


def test_a_comment_or_a_docstring_is_no_coverage():
    src = "\n".join([
        '"""module docstring: vx_in_module_doc"""',
        "import lib  # vx_in_comment",
        'TABLE = {"a": "vx_in_table"}',
        "",
        "",
        "def f(x):",
        '    """vx_in_docstring"""',
        "    'vx_in_second_string_statement'",
        '    y = "vx_in_assigned_string"  # vx_in_trailing_comment',
        '    return lib.vx_called(x) + getattr(lib, f"vx_in_fstring_{x}")(y) + lib.vx_attribute',
        ""])
    code = python_code(src)
    for name in ("vx_in_table", "vx_in_assigned_string", "vx_called", "vx_in_fstring_", "vx_attribute"):
        assert name in code, name
    for name in ("vx_in_module_doc", "vx_in_comment", "vx_in_docstring", "vx_in_second_string_statement", "vx_in_trailing_comment"):
        assert name not in code, name
    c = c_code('int a = vx_called(1); // vx_in_comment\n/* vx_in_block\n vx_in_block2 */ const char* s = "vx_in_string";\n')
    assert "vx_called" in c and "vx_in_string" in c and "vx_in_comment" not in c and "vx_in_block" not in c
