"""GPU suite: rhj_join on inputs of hundreds of MiB takes the PIPELINED path (S uploaded, partitioned and joined in chunks
against the partitioned R while finished pairs travel home).  The pair set must be what one join of the whole
relations yields.

At 40-72 M tuples (default knobs): exact count + order-insensitive checksum against the closed form of the PK/FK generators
(numpy restatement of SURVEY §8d / App. A), plus the fall-back to the plain path when a rowID does not fit the narrow format.

At the smallest sizes that reach the path (tests/pipeline_cases.py: RHJ_PIPE_MIN_CHUNK=65536, one side of 4 193 280 tuples,
whose result page is the 64 MiB below which nothing is pipelined): the full sorted pair array against the CPU oracle's, one
fresh child process per case because the knobs are read once per process, and the path that ran ("last.pipelined",
"last.narrow", the plan).  The exits of join_host_pipelined and the cases that reach them:
  success                          fk_S_large_narrow{2,1,0} (duplicates in R, misses), fk_S_small (S chunks are the build side, ragged
                                   last chunk), one_pass, max_chunks (16: the last slot of h_counts / chunk_ev), two_chunks,
                                   matches_only_in_{first,last}_chunk, skewed_chunk, wide_S_rowid_16_byte, page_exactly_full
                                   (count == dcap), context_reuse (K = 4, then 12 on a grown pair buffer, then 4 again)
  abandon, page overflow           page_one_over_{last,first} (count == dcap + 1, seen in the last chunk, earlier ranges already
                                   home), many_to_many (3 x the page, seen in an early chunk), context_reuse (join 4)
  abandon, wide rowID              wide_S_rowid_narrow (in S, chunk 2; then the same context pipelines narrow again); a wide rowID of
                                   R: the large test below
  empty result                     no_match_at_all ("last.pipelined" still reports the chunks that went through)
  not pipelined: |S| < 4 chunks    gate_nS_below / gate_nS_at
  not pipelined: |R| < chunk / 2   gate_nR_below / gate_nR_at
  not pipelined: page < 64 MiB     gate_page_below / gate_page_at, context_reuse (join 2)
tests/test_pipeline_cases.py checks, without a GPU, that every case is the case its name says."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (np_mix / host_inputs: the generators of SURVEY §8d with numpy)
import pipeline_cases as pc  # noqa: E402
from radixhashjoin_amd import Engine, TUPLE  # noqa: E402

pytestmark = pytest.mark.gpu
C = np.uint64(0x100000001B3)


def chunks_of(nS):
    """the S chunks rhj_join uses (rhj_api.hip, join_host_pipelined): >= 8 Mi tuples each, at most 12"""
    k0 = min(12, nS // (8 << 20))
    chunk = (-(-nS // k0) + 4095) // 4096 * 4096
    return -(-nS // chunk)


def checksum(pairs):
    return int(np.sum(bench.np_mix(pairs["keyR"] * C ^ bench.np_mix(pairs["keyS"])), dtype=np.uint64))


def expected(S, n):
    """closed form: S tuple {j, mix(k)} matches exactly R row k - 1, k = 1 + mix(j ^ 42) % n"""
    j = S["key"]
    k1 = bench.np_mix(j ^ np.uint64(42)) % np.uint64(n)
    return len(S), int(np.sum(bench.np_mix(k1 * C ^ bench.np_mix(j)), dtype=np.uint64))


@pytest.mark.parametrize("n", [40_000_000, 72_000_000])
def test_pipelined_host_join_equals_the_closed_form(n):
    R, S = bench.host_inputs(n, TUPLE)
    S = S[: n - 1_234_567].copy()                         # |S| != |R|, last chunk ragged
    e = Engine(0)
    try:
        got = e.join(R, S)
        exp_n, exp_c = expected(S, n)
        assert len(got) == exp_n and checksum(got) == exp_c
        assert e.info("last.narrow") == 2 and e.info("last.pipelined") == chunks_of(len(S))
        # a rowID beyond 2^32 on the build side: the pipelined attempt is abandoned, the plain path repeats the join in the
        # 16-byte format; same pairs but for that one rowID
        R2 = R.copy()
        R2["key"][777] = np.uint64((1 << 40) + 777)
        got2 = e.join(R2, S)
        assert len(got2) == exp_n and e.info("last.narrow") == 0 and e.info("last.pipelined") == 0
        fix = got2["keyR"] == np.uint64((1 << 40) + 777)
        got2["keyR"][fix] = np.uint64(777)
        assert checksum(got2) == exp_c
    finally:
        e.close()


def test_pipelined_with_a_one_pass_plan_and_a_small_build_side():
    """|R| = 6M (one 9-bit pass), |S| = 40M: S still goes through in chunks"""
    n, m = 6_000_000, 40_000_000
    i = np.arange(n, dtype=np.uint64)
    R = np.empty(n, dtype=TUPLE)
    R["key"], R["payload"] = i, bench.np_mix(i + np.uint64(1))
    j = np.arange(m, dtype=np.uint64)
    S = np.empty(m, dtype=TUPLE)
    S["key"] = j
    k1 = bench.np_mix(j ^ np.uint64(42)) % np.uint64(n)
    S["payload"] = bench.np_mix(k1 + np.uint64(1))
    S["payload"][::11] ^= np.uint64(1 << 50)                 # every 11th foreign key matches nothing
    hit = np.ones(m, dtype=bool)
    hit[::11] = False
    exp_c = int(np.sum(bench.np_mix(k1[hit] * C ^ bench.np_mix(j[hit])), dtype=np.uint64))
    e = Engine(0)
    try:
        got = e.join(R, S)
        assert e.info("last.pipelined") == chunks_of(m)
        assert len(got) == int(hit.sum()) and checksum(got) == exp_c
    finally:
        e.close()


# ---- the path at its smallest sizes: one child process per case, full pair arrays against the CPU oracle ------------------
def check_step(step, spec):
    """one join of a child, as its JSON line reports it, against the case's entry in pipeline_cases.CASES"""
    assert step["case"] == spec["name"]
    assert step["equal"] and step["count"] == step["oracle_count"], step
    assert pc.count_class(step["oracle_count"], spec["nR"], spec["nS"]) == spec["count"], step
    assert step["last.pipelined"] == spec["pipelined"], step
    assert step["last.narrow"] == spec["last_narrow"], step
    assert tuple(step["plan"]) == spec["plan"], step
    if "wide" in spec:
        assert step["wide_rowid_pairs"] == 1, step


@pytest.mark.parametrize("run", pc.RUNS)
def test_pipelined_join_equals_the_oracle(run):
    steps = pc.steps_of(run)
    for name in steps:                                       # what the case is about, from the restated host arithmetic
        spec = pc.CASES[name]
        assert spec["pipelined"] in (0, pc.chunks_of(spec["nS"], pc.MIN_CHUNK, spec["max_chunks"], spec["nR"]))
        if "geometry" in spec:
            assert pc.geometry(spec["nS"], pc.MIN_CHUNK, spec["max_chunks"]) == spec["geometry"]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pipeline_cases.py"), run], capture_output=True, text=True,
                         timeout=120, env={**os.environ, **pc.env_of(run)})
    assert out.returncode == 0, f"child exit {out.returncode}\n{out.stderr[-4000:]}"
    line = json.loads(out.stdout.strip().splitlines()[-1])
    got = [line] + line["then"]
    assert line["run"] == run and [s["case"] for s in got] == steps
    for step in got:
        check_step(step, pc.CASES[step["case"]])
    if run == "context_reuse":                               # the first join again, after four others on the same context
        assert got[-1]["same_as_first"] is True
