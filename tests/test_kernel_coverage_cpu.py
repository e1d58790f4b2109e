"""Every compute launcher of the kernel-level ABI (include/visp_hip_kernels.h) is named by some test: a launcher no file under tests/ calls is
one whose numbers nothing checks. Runtime plumbing is the one allowlist below, each entry with its reason."""
import re
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


def _named_in_tests():
    corpus = []
    for p in (ROOT / "tests").rglob("*"):
        if p.is_file() and p.suffix in (".py", ".cpp", ".c", ".h") and p.name != Path(__file__).name:
            corpus.append(p.read_text(errors="replace"))
    return "\n".join(corpus)


def test_every_compute_launcher_is_named_by_a_test():
    names = _launchers()
    assert set(PLUMBING) <= names, sorted(set(PLUMBING) - names)
    corpus = _named_in_tests()
    missing = sorted(n for n in names - set(PLUMBING) if not n.endswith("_set_stamps") and not re.search(rf"\b{n}\b", corpus))
    assert not missing, f"launchers no test names: {missing}"
