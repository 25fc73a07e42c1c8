"""CPU suite: the host side of every device entry, rhj_join_dev through rhj_group_join_agg_ids_cols_dev, against a recorded trace.

radixhashjoin_amd/csrc/tsan/entries.cpp drives the entries of rhj_api.hip -- compiled as C++ over the fake runtime and the fake
launchers of tsan/fake_hip.cpp, a plain build with no sanitizer -- through normal, degenerate, count-only, overflowing and invalid
calls and through pairs of calls, and prints after each what a caller can observe (return code, error text, out words, "last.*"
infos, span kinds) and every stream operation and launcher call it made, with the scalar arguments.  tests/golden/
host_entries_trace.txt is that output as recorded before the entries and the keyed-table phases were moved onto shared scaffolding:
host code that changes one line of it has changed the order of checks, an error text, a memset, a copy, a synchronisation, a launch
argument or a piece of observable state.  Fix the code, not the file; a new operator adds its lines at the end of its own blocks."""
import difflib
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radixhashjoin_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_entries_trace.txt")


def test_host_entries_trace_matches_golden():
    b = subprocess.run(["make", "-C", CSRC, "-f", "Makefile.sanitize", "tsan/entries"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, (b.stdout + b.stderr)[-4000:]
    r = subprocess.run([os.path.join(CSRC, "tsan", "entries")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    got = r.stdout.splitlines()
    assert "DIFFERS from a fresh context" not in r.stdout
    if got != want:
        diff = list(difflib.unified_diff(want, got, "golden", "driver", lineterm="", n=8))
        raise AssertionError("%d lines differ:\n%s" % (sum(1 for d in diff if d[:1] in "+-"), "\n".join(diff[:200])))
