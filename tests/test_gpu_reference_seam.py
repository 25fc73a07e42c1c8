"""GPU suite: the REFERENCE's own Query / intermediate / MainScheduler / CLI code driving the GPU join.

oracle/_ref/join_seam  = every reference file compiled unchanged where it lies; Result::multiRadixHashJoin bound at
                         link time to rhj_join (oracle/ref_gpu_seam.cpp)
oracle/_ref/join_optA  = INTEGRATION.md Option A (Result.cpp / JobScheduler.cpp / half of structs.cpp swapped for the mirror)
oracle/_ref/join_optB  = INTEGRATION.md Option B (only the body of the seam replaced)
All three are built in the build container (`make -C oracle bindings`) and travel as binaries.  Each must print
small/small.result byte for byte.  Their run time is the reference's own update_intermediate: one query of the
50 costs three of its four minutes of host CPU, so that query runs through the link-time seam only and everything runs
side by side, each child under its own time limit that reports how far it got."""
import collections
import os
import subprocess

import pytest

from conftest import golden_workdir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BINARIES = ["join_seam", "join_optA", "join_optB"]


HEAVY = 54           # line of small.work whose reference-side update_intermediate alone is 80 % of the workload's CPU time


def small_workload(lines_wanted):
    """(stdin, expected stdout) for the queries of small.work on the given 1-based lines (batch separators kept)"""
    work = open(os.path.join(GOLD, "small", "small.work"), "rb").read().splitlines()
    result = open(os.path.join(GOLD, "small", "small.result"), "rb").read().splitlines()
    stdin, expected, q = [], [], 0
    for ln, text in enumerate(work, 1):
        if text.strip() == b"F":
            stdin.append(text)
            continue
        if lines_wanted(ln):
            stdin.append(text)
            expected.append(result[q])
        q += 1
    assert q == len(result)
    init = open(os.path.join(GOLD, "small", "small.init"), "rb").read()
    return init + b"\n".join(stdin) + b"\n", b"".join(x + b"\n" for x in expected)


def thread_states(pid):
    """[(thread name, kernel wait channel, syscall number)] of a live process, from /proc (diagnostics of a timeout)"""
    out = []
    try:
        for tid in sorted(os.listdir(f"/proc/{pid}/task")):
            def rd(name):
                try:
                    return open(f"/proc/{pid}/task/{tid}/{name}").read().strip()
                except OSError:
                    return "?"
            out.append((rd("comm"), rd("wchan"), rd("syscall").split(" ")[0]))
    except OSError:
        pass
    return out


class ChildTimeout(Exception):
    pass


def run_once(path, stdin, log, limit):
    env = dict(os.environ, RHJ_SEAM_LOG=str(log))
    pr = subprocess.Popen([path], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=golden_workdir(), env=env)
    try:
        out, err = pr.communicate(input=stdin, timeout=limit)            # both pipes drained while the child runs
    except subprocess.TimeoutExpired:
        where = thread_states(pr.pid)                                    # what every thread of the child is blocked in
        pr.kill()
        out, err = pr.communicate()
        done = len(open(log).readlines()) if os.path.exists(log) else -1
        raise ChildTimeout(f"{os.path.basename(path)} still running after {limit} s: {len(out.splitlines())} result lines, "
                           f"{done} joins logged, threads {where}, stderr tail {err[-1500:]!r}")
    return pr.returncode, out, err


def run_binary(path, stdin, log, limit):
    """One run, no second chance: a child that outlives its limit fails the test, and the message names what each of its
    threads was blocked in.  (Round 3 re-ran join_seam / join_optB once, because the reference's JobScheduler::stop --
    JobScheduler.cpp:140-146 -- sets `done` and broadcasts without queueLock and an idle worker can sleep through the only
    wake-up; behind the GPU seam the inner workers are idle from init to stop.  Both binaries now carry the two-line fix
    INTEGRATION.md gives with Option B -- join_optB as the source edit a maintainer makes, tools/bind_reference.sh; join_seam,
    which edits nothing, by binding JobScheduler::stop at link time next to the seam itself, oracle/ref_gpu_seam.cpp -- and
    oracle/_ref/sched_race_fixed loops init / stop / destroy over that stop() 6 x 10^5 times where the reference's own stalls
    within 10^5, tests/test_integration_build.py.  join_optA holds this repo's scheduler.)"""
    try:
        return run_once(path, stdin, log, limit)
    except ChildTimeout as e:
        pytest.fail(str(e))


def test_reference_code_drives_gpu_join(tmp_path, small_joins):
    paths = {b: os.path.join(ROOT, "oracle", "_ref", b) for b in BINARIES}
    missing = [b for b, p in paths.items() if not os.path.exists(p)]
    if missing:
        pytest.skip(f"not built (needs the reference checkout at build time): {missing}")
    # every query but the heavy one through all three binaries, side by side (their time is the reference's own CPU code
    # above the seam); the heavy query through the link-time seam only, so that all 94 joins of the workload are checked
    stdin, expected = small_workload(lambda ln: ln != HEAVY)
    assert len(expected.splitlines()) == 49
    import concurrent.futures
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(paths) + 1) as pool:
        heavy_in, heavy_exp = small_workload(lambda ln: ln == HEAVY)
        heavy = pool.submit(run_binary, paths["join_seam"], heavy_in, tmp_path / "heavy.log", 360)
        jobs = {b: pool.submit(run_binary, p, stdin, tmp_path / f"{b}.log", 240) for b, p in paths.items()}
        for b, job in jobs.items():
            rc, out, err = job.result()
            assert rc == 0, (b, err[-2000:])
            assert out == expected, b                             # 49 lines of SUMs / NULLs, byte-identical
        rc, out, err = heavy.result()
        assert rc == 0, err[-2000:]
        assert out == heavy_exp
    # the seam binary logs every call that went through rhj_join: the same 94 joins the CPU reference makes
    meta, _ = small_joins
    want = collections.Counter((c["nR"], c["nS"], c["count"]) for c in meta)
    got = collections.Counter(tuple(int(x) for x in line.split())
                              for f in ("join_seam.log", "heavy.log") for line in open(tmp_path / f))
    assert sum(got.values()) == 94 and got == want


def test_reference_code_drives_gpu_join_edge_queries():
    """the same three binaries on the edge-case queries of tests/golden/edge (expected lines from the CPU reference)"""
    paths = {b: os.path.join(ROOT, "oracle", "_ref", b) for b in BINARIES}
    if any(not os.path.exists(p) for p in paths.values()):
        pytest.skip("bindings not built (needs the reference checkout at build time)")
    edge = os.path.join(GOLD, "edge")
    stdin = open(os.path.join(edge, "edge.init"), "rb").read() + open(os.path.join(edge, "edge.work"), "rb").read()
    expected = open(os.path.join(edge, "edge.result"), "rb").read()
    for b, p in paths.items():
        rc, out, err = run_binary(p, stdin, os.devnull, 60)
        assert rc == 0, (b, err[-2000:])
        assert out == expected, b
