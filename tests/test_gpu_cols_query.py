"""GPU suite: whole queries with RHJ_QUERY_MODE=cols -- the device-resident executor with its join inputs built as columns
(the stored column itself for an alias without a row list, one 8-byte gather otherwise) and joined by rhj_join_cols_dev.
The reference's golden workloads print the bytes of their .result files, the three-way synthetic query matches an independent
numpy evaluation and the `device` mode, and RHJ_JOIN_LOG shows that the columnar entry point ran (an unknown mode value
silently runs `device`): one line "cols <nR> <nS> <count>" per call."""
import os
import subprocess

import numpy as np
import pytest

from conftest import golden_workdir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
JOIN = os.path.join(ROOT, "radixhashjoin_amd", "host", "join_gpu")


def run(stdin, mode, log=None, cwd=None):
    env = dict(os.environ, RHJ_QUERY_MODE=mode)
    env.pop("RHJ_JOIN_LOG", None)
    if log is not None:
        env["RHJ_JOIN_LOG"] = str(log)
    return subprocess.run([JOIN], input=stdin, cwd=cwd, env=env, capture_output=True, timeout=600, check=True).stdout


def check_log(log):
    lines = open(log).read().splitlines()
    assert lines, "no rhj_join_cols_dev call was logged"
    for line in lines:
        f = line.split()
        assert f[0] == "cols" and len(f) == 4 and all(x.isdigit() for x in f[1:]), line
    return [tuple(int(x) for x in line.split()[1:]) for line in lines]


@pytest.mark.parametrize("name", ["small", "edge"])
def test_golden_workloads_byte_identical(tmp_path, name):
    assert os.path.exists(JOIN), "build with __graft_entry__.build()"
    d = os.path.join(GOLD, name)
    stdin = open(os.path.join(d, f"{name}.init"), "rb").read() + open(os.path.join(d, f"{name}.work"), "rb").read()
    log = tmp_path / "joins.log"
    out = run(stdin, "cols", log, cwd=golden_workdir())
    assert out == open(os.path.join(d, f"{name}.result"), "rb").read()
    calls = check_log(log)
    print(f"{name}: {len(calls)} rhj_join_cols_dev calls")


def write_rel(path, cols):
    with open(path, "wb") as f:
        np.array([len(cols[0]), len(cols)], dtype=np.uint64).tofile(f)
        for c in cols:
            np.ascontiguousarray(c, dtype=np.uint64).tofile(f)


@pytest.mark.parametrize("n,dup", [(300_000, 1), (120_000, 5)])
def test_three_way_join_cols_mode(tmp_path, n, dup):
    """the synthetic query of test_gpu_query_modes.py: SELECT SUM(..) FROM t0,t1,t2 WHERE t0.c1=t1.c0 AND t1.c1=t2.c0 AND t0.c2<X"""
    rng = np.random.default_rng(n)
    T = []
    for t in range(3):
        T.append([np.arange(n, dtype=np.uint64) // dup, rng.integers(0, n // dup, n, dtype=np.uint64),
                  rng.integers(0, 1000, n, dtype=np.uint64)])
        write_rel(tmp_path / f"t{t}", T[t])
    xs = [100, 450, 999, 0]
    work = "".join(f"0 1 2|0.1=1.0&1.1=2.0&0.2<{x}|0.0 1.2 2.2\n" for x in xs) + "F\n"
    stdin = ("".join(str(tmp_path / f"t{t}") + "\n" for t in range(3)) + "Done\n" + work).encode()
    log = tmp_path / "joins.log"
    cols = run(stdin, "cols", log).decode().splitlines()
    device = run(stdin, "device").decode().splitlines()
    assert cols == device
    calls = check_log(log)
    # every query that passes its filter joins a stored column as it stands (n rows, no row list) at least once
    assert sum(1 for c in calls if n in c[:2]) >= 3
    for x, line in zip(xs, cols):
        r0 = np.nonzero(T[0][2] < x)[0]
        if len(r0) == 0:
            assert line == "NULL NULL NULL"
            continue
        r0e = np.repeat(r0, dup)
        r1 = (T[0][1][r0].astype(np.int64)[:, None] * dup + np.arange(dup)[None, :]).ravel()
        r0e2 = np.repeat(r0e, dup)
        r1e = np.repeat(r1, dup)
        r2 = (T[1][1][r1].astype(np.int64)[:, None] * dup + np.arange(dup)[None, :]).ravel()
        exp = [int(T[0][0][r0e2].sum(dtype=np.uint64)), int(T[1][2][r1e].sum(dtype=np.uint64)), int(T[2][2][r2].sum(dtype=np.uint64))]
        assert line == " ".join(str(v) for v in exp)
