"""Whole queries through the `join_gpu` CLI in all four executor modes (RHJ_QUERY_MODE = host, device, batch, cols) against
tests/sql_eval.py, the independent numpy evaluator that tests/test_sql_eval.py anchors to the real reference.

One generator with a fixed seed writes six relations -- 0, 1, 65, 3,001, 30,011 and 70,001 rows: the empty and one-row
inputs, one wavefront + 1, and both sides of the two sizes at which a join changes kernels (a build side of 5 x 4224 = 21,120
tuples device-resident, 12 x 4224 = 50,688 from host memory) -- and one workload of hand-written and generated queries:

    c0  dense key: a permutation of 0..n-1
    c1  foreign key into the dense key of another relation (ONE->A, A->B, B->A, C->D, D->C)
    c2  small domain 0..15: filters, and joins with a large fan-out
    c3  full 64-bit width: the row's own dense key (40 %: c0 = c3 is a same-alias predicate that keeps many rows, and c3
        joins across relations) or a draw from a pool shared by every relation, half of it >= 2^63; 0, 2^63 - 1, 2^63 and
        2^64 - 1 occur in every relation of 65 rows or more

The CPU test asserts from the evaluator's records that the workload reaches every path it is meant to reach, so the workload
cannot lose one silently; the GPU test compares every mode's stdout with the evaluator line by line."""
import functools
import os
import subprocess
import time

import numpy as np
import pytest

import sql_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOIN = os.path.join(ROOT, "radixhashjoin_amd", "host", "join_gpu")

Z, ONE, A, B, C, D = range(6)
ROWS = (0, 1, 65, 3_001, 30_011, 70_001)
FK_TARGET = {ONE: A, A: B, B: A, C: D, D: C}
SMALL_DOMAIN = 16
POOL = 20_000
TOP, HALF = (1 << 64) - 1, 1 << 63
SPECIAL = (0, HALF - 1, HALF, TOP)
N_GENERATED = 150
# no join of the workload returns more pairs, whichever way an executor evaluates a predicate between two joined aliases
# (as a mask over the joined rows, or like the reference as a join of their distinct rows: sql_eval.Evaluated.masks)
MAX_JOIN_ROWS = 400_000
DIRECT_DEV, DIRECT_HOST = 5 * 4224, 12 * 4224

# [measured, MI355X] one join_gpu child over this workload with the executors of the commit before this test: host 0.40 s,
# device 0.39 s, batch 0.85 s, cols 0.25 s.  A guard 35 x the slowest of them, not a target.
CHILD_TIMEOUT_S = 30

HAND_WRITTEN = [
    # both kernels of a device-resident join in one query: C x D (build side 30 K: partitioned), then B (3 K: direct) with
    # the alias already joined on the RIGHT: the intermediate is re-gathered through the S side of the pairs
    f"{C} {D} {B}|0.0=1.1&2.0=1.2|0.3 1.3 2.3 2.0",
    f"{C} {D} {B}|0.0=1.1&2.0=1.2|0.3 1.3",
    # the same relation under two aliases, joined on the full-width column: both sides above 51 K, and more pairs than
    # max(nR, nS) + 1024, so the first call overflows and the join runs again with the exact capacity
    f"{D} {D}|0.3=1.3|0.0 1.3 0.3",
    # the overflow retry at a size where the join is direct
    f"{B} {A}|0.2=1.2|0.0 1.1 1.3",
    # same-alias predicate before any join
    f"{B} {A}|0.1=0.2&0.1=1.0|0.0 1.3",
    # ... after a join that does not involve its alias, which then joins one that does
    f"{A} {B} {C}|0.1=1.0&2.0=2.3&1.0=2.0|0.0 1.3 2.3",
    f"{D} {C} {B}|0.1=1.0&2.1=2.2&2.1=0.2|1.0 2.3",
    # ... after a join that involves its alias: a mask over 70 K joined rows
    f"{D} {C}|0.1=1.0&0.0=0.3|0.3 1.3 1.0",
    # a predicate that appears twice; two predicates between one pair of aliases
    f"{C} {D}|0.0=1.1&0.0=1.1|0.0 1.0",
    f"{B} {A}|0.1=1.0&0.2=1.2|0.3 1.3",
    # a cycle of three closed by a predicate between two joined aliases: a mask over 233 K joined rows
    f"{D} {C} {D}|0.1=1.0&2.1=1.0&0.0=2.0|0.0 1.3 2.3",
    # a star of four around A: the joined alias on the right, on the left, on the right
    f"{A} {ONE} {B} {B}|1.1=0.0&0.1=2.0&3.1=0.0|0.3 1.3 2.2 3.0",
    # a cycle of four
    f"{A} {B} {A} {B}|0.1=1.0&1.1=2.0&2.1=3.0&3.2=0.2|0.0 1.0 2.0 3.0",
    # the zero-row relation: unfiltered, filtered, joined late, under a same-alias predicate
    f"{Z} {A}|0.0=1.0|0.1 1.1",
    f"{Z} {A}|0.0=1.0&0.2<5|1.1",
    f"{A} {B} {Z}|0.1=1.0&2.0=1.0|0.0 2.3",
    f"{Z} {B}|0.1=0.2&0.0=1.0|1.0",
    # a join that comes out empty in mid-chain
    f"{B} {A} {C}|0.1=1.0&0.0=2.0&2.1=1.0&0.0<100&2.0>5000|0.0 2.0",
    # filter constants 0, 2^63 and 2^64 - 1 on the full-width column: an unsigned compare, sums that wrap
    f"{C} {D}|0.0=1.1&1.3>{HALF}&0.3<{TOP}&0.0>0|0.3 1.3",
    f"{D} {C}|0.1=1.0&0.3={TOP}|0.3 1.0",
    f"{D} {C}|0.1=1.0&0.3={HALF}&1.3>0|0.3 1.3",
    # a constant below the column's minimum, one above its maximum, an `=` on a value the column does not hold
    f"{B} {A}|0.1=1.0&0.3<0|0.0",
    f"{B} {A}|0.1=1.0&1.3>{TOP}|0.0",
    f"{B} {A}|0.1=1.0&0.2=99|0.0",
    # three filters on one alias chained through the surviving rows: > < =, then = < >
    f"{D} {C}|0.1=1.0&0.0>1000&0.0<60000&0.2=3&1.2>2|0.3 1.3",
    f"{C} {D}|0.1=1.0&0.2=7&0.0<20000&0.3>{HALF - 1}|0.0 1.0",
    # a self-join behind a same-alias predicate on the second alias; its last join returns 18 x its larger input
    f"{B} {B} {A}|0.1=2.0&1.0=1.3&1.1=2.0|0.0 1.0 2.0",
]
assert len(HAND_WRITTEN) >= 25


def make_relations(rng):
    pool = np.concatenate([np.array(SPECIAL, dtype=np.uint64), rng.integers(0, HALF, POOL // 2, dtype=np.uint64),
                           rng.integers(HALF, TOP, POOL // 2 - len(SPECIAL), dtype=np.uint64, endpoint=True)])
    rels = []
    for r, n in enumerate(ROWS):
        c0 = rng.permutation(n).astype(np.uint64)
        c1 = rng.integers(0, ROWS[FK_TARGET[r]], n, dtype=np.uint64) if n else np.empty(0, dtype=np.uint64)
        c2 = rng.integers(0, SMALL_DOMAIN, n, dtype=np.uint64)
        c3 = np.where(rng.random(n) < 0.4, c0, pool[rng.integers(0, len(pool), n)])
        if n >= len(SPECIAL):
            c3[rng.permutation(n)[:len(SPECIAL)]] = SPECIAL
        elif n:
            c3[:] = TOP
        rels.append([c0, c1, c2, c3])
    return rels


def filter_term(rng, rels, tables, a):
    """mostly constants inside the column's range; one in six is taken from the edges: below the minimum, above the
    maximum, absent from the column"""
    n = ROWS[tables[a]]
    c = int(rng.choice([0, 2, 3]))
    op = "<>="[int(rng.choice(3, p=[0.4, 0.4, 0.2]))]
    big = np.array([0, HALF - 1, HALF, TOP, 12345, n], dtype=object)
    if rng.random() < 1 / 6 or n == 0:
        val = int(rng.choice(big)) if c != 2 else int(rng.choice([0, SMALL_DOMAIN - 1, 99]))
    elif c == 0:
        val = int(rng.integers(n // 4, n)) if op == "<" else int(rng.integers(0, 3 * n // 4 + 1))
    elif c == 2:
        val = int(rng.choice([3, 5, 8, 12]))
    else:
        val = int(rng.choice(big[1:4] if op == "<" else big[:3] if op == ">" else np.append(big[:4], int(rels[tables[a]][3][0]))))
    return f"{a}.{c}{op}{val}"


def generate_query(rng, rels):
    k = int(rng.integers(2, 5))
    tables = [int(t) for t in rng.choice(len(ROWS), k, p=[0.02, 0.05, 0.2, 0.25, 0.25, 0.23])]
    shape = rng.choice(["chain", "star", "cycle"])
    edges = [((i - 1) if shape != "star" else 0, i) for i in range(1, k)]
    if shape == "cycle":
        edges.append((k - 1, 0))                                           # k = 2: a second predicate between the pair
    terms = []
    for joined, new in edges:
        c, d = [(0, 1), (1, 0), (0, 0), (3, 3), (0, 3), (3, 0), (1, 1), (2, 2)][int(rng.choice(8, p=[.2, .2, .1, .2, .1, .1, .05, .05]))]
        if (joined, new) == (k - 1, 0) and rng.random() < 0.6:
            c, d = 2, 2                                                    # a closing predicate that keeps one row in 16
        terms.append(f"{joined}.{c}={new}.{d}" if rng.random() < 0.5 else f"{new}.{d}={joined}.{c}")
    if rng.random() < 0.3:                                                 # a same-alias predicate, anywhere in the order
        a = int(rng.integers(0, k))
        c, d = [(0, 3), (3, 0), (1, 2), (1, 0)][int(rng.choice(4, p=[0.4, 0.4, 0.1, 0.1]))]
        terms.insert(int(rng.integers(0, len(terms) + 1)), f"{a}.{c}={a}.{d}")
    if rng.random() < 0.15:                                                # a predicate twice
        terms.insert(int(rng.integers(0, len(terms) + 1)), terms[int(rng.integers(0, len(terms)))])
    for _ in range(int(rng.choice(4, p=[0.3, 0.35, 0.2, 0.15]))):          # 0..3 filters, possibly several on one alias
        terms.insert(int(rng.integers(0, len(terms) + 1)), filter_term(rng, rels, tables, int(rng.integers(0, k))))
    projs = [f"{int(rng.integers(0, k))}.{int(rng.integers(0, 4))}" for _ in range(int(rng.integers(1, 4)))]
    return " ".join(str(t) for t in tables) + "|" + "&".join(terms) + "|" + " ".join(projs)


@functools.lru_cache(maxsize=None)
def workload():
    """(relations, queries, [sql_eval.Evaluated per query]); computed once, treated as read-only"""
    rng = np.random.default_rng(20240917)
    rels = make_relations(rng)
    queries = list(HAND_WRITTEN)
    expected = [sql_eval.evaluate(rels, q) for q in queries]
    while len(queries) < len(HAND_WRITTEN) + N_GENERATED:
        q = generate_query(rng, rels)
        assert sql_eval.in_sql_class(q), q                                 # chains, stars and cycles are connected orders
        try:
            e = sql_eval.evaluate(rels, q, max_rows=MAX_JOIN_ROWS)
        except sql_eval.TooLarge:
            continue
        if any(pairs > MAX_JOIN_ROWS for _, _, pairs in e.masks):
            continue
        queries.append(q)
        expected.append(e)
    return rels, queries, expected


def workload_text(queries):
    # batches of ten, as the reference's workloads come
    return "".join(q + "\n" + ("F\n" if i % 10 == 9 else "") for i, q in enumerate(queries)) + "F\n"


def test_workload_reaches_every_path():
    rels, queries, expected = workload()
    assert [len(r[0]) for r in rels] == list(ROWS)
    assert len(queries) == len(HAND_WRITTEN) + N_GENERATED and all(sql_eval.in_sql_class(q) for q in queries)
    joins = [j for e in expected for j in e.joins]
    first = [e.joins[0] for e in expected if e.joins]                      # both inputs are stored relations: the sizes
    events = {w for e in expected for w in e.events}                       # every mode sees
    for js in (joins, first):
        assert any(min(nR, nS) < DIRECT_DEV and count for nR, nS, count in js)
        assert any(DIRECT_DEV < min(nR, nS) < 43_000 and count for nR, nS, count in js)
        assert any(min(nR, nS) > DIRECT_HOST and count for nR, nS, count in js)
        assert any(count > max(nR, nS) + 1024 for nR, nS, count in js)
    # both sides of the device-resident cut-off inside one query
    assert any(e.joins and min(min(j[:2]) for j in e.joins) < DIRECT_DEV < max(min(j[:2]) for j in e.joins) and
               e.line[0] != "N" for e in expected)
    for word in ("join_empty_mid_chain", "same_alias_before_join", "same_alias_after_other_join", "same_alias_after_own_join",
                 "join_joined_left", "join_joined_right", "mask_between_joined", "filter_empty", "mask_empty"):
        assert word in events, word
    # the three same-alias positions and both orientations also in queries that print sums
    live = {w for e in expected if e.line[0] != "N" for w in e.events}
    assert {"same_alias_before_join", "same_alias_after_other_join", "same_alias_after_own_join", "join_joined_left",
            "join_joined_right", "mask_between_joined"} <= live
    assert max(count for _, _, count in joins) <= MAX_JOIN_ROWS
    assert max(pairs for e in expected for _, _, pairs in e.masks) <= MAX_JOIN_ROWS
    # a mask over many joined rows, and one that keeps none although the distinct rows of its two aliases have pairs
    assert any(e.joins[-1][2] > 200_000 and e.masks and e.line[0] != "N" for e in expected)
    assert any(e.events[-1] == "mask_empty" and e.masks and e.masks[-1][2] for e in expected)
    # the zero-row relation filtered and unfiltered; self-joins; sums at or above 2^63; not too many NULL lines
    parsed = [sql_eval.parse(q) for q in queries]
    assert any(Z in p.tables and any(p.tables[a] == Z for a, _, _, _ in p.filters) for p in parsed)
    assert any(Z in p.tables and not any(p.tables[a] == Z for a, _, _, _ in p.filters) for p in parsed)
    assert sum(1 for p in parsed if len(set(p.tables)) < len(p.tables)) >= 10
    assert any(int(s) >= HALF for e in expected if e.line[0] != "N" for s in e.line.split())
    assert sum(1 for e in expected if e.line[0] != "N") >= len(queries) // 2
    consts = {val for p in parsed for _, _, _, val in p.filters}
    assert {0, HALF, TOP} <= consts
    assert {op for p in parsed for _, _, op, _ in p.filters} == set("<>=")
    assert max(len([f for f in p.filters if f[0] == a]) for p in parsed for a in range(len(p.tables))) >= 2


def write_relation(path, cols):
    with open(path, "wb") as f:
        np.array([len(cols[0]), len(cols)], dtype=np.uint64).tofile(f)
        for c in cols:
            np.ascontiguousarray(c, dtype=np.uint64).tofile(f)


@pytest.mark.gpu
def test_four_modes_match_the_evaluator(tmp_path):
    """one join_gpu child per mode, in the order host, device, batch, cols; [measured, MI355X] 2.7 s for the whole test"""
    assert os.path.exists(JOIN), "build with __graft_entry__.build()"
    rels, queries, expected = workload()
    for r, cols in enumerate(rels):
        write_relation(tmp_path / f"r{r}", cols)
    text = workload_text(queries)
    stdin = ("".join(str(tmp_path / f"r{r}") + "\n" for r in range(len(rels))) + "Done\n" + text).encode()
    for mode in ("host", "device", "batch", "cols"):
        env = dict(os.environ, RHJ_QUERY_MODE=mode)
        env.pop("RHJ_JOIN_LOG", None)
        log = tmp_path / f"joins_{mode}.log"
        if mode == "cols":
            env["RHJ_JOIN_LOG"] = str(log)
        # a child that times out or exits non-zero raises here: no further child is started
        t0 = time.perf_counter()
        r = subprocess.run([JOIN], input=stdin, env=env, capture_output=True, timeout=CHILD_TIMEOUT_S)
        print(f"mode {mode}: join_gpu took {time.perf_counter() - t0:.2f} s")
        assert r.returncode == 0, f"mode {mode}: exit {r.returncode}\n{r.stderr.decode()[-2000:]}\n{text}"
        got = r.stdout.decode().splitlines()
        for i, (q, e) in enumerate(zip(queries, expected)):
            assert i < len(got) and got[i] == e.line, \
                f"mode {mode}, query {i}: {q}\n  join_gpu:  {got[i] if i < len(got) else '(no line)'}\n  evaluator: {e.line}\n{text}"
        assert len(got) == len(queries), f"mode {mode}: {len(got)} lines for {len(queries)} queries"
        if mode == "cols":
            lines = open(log).read().splitlines()
            assert lines, "no rhj_join_cols_dev call was logged"
            for line in lines:
                f = line.split()
                assert f[0] == "cols" and len(f) == 4 and all(x.isdigit() for x in f[1:]), line
            # every join the evaluator ran with a result is a columnar call of the same sizes and count
            logged = {tuple(int(x) for x in line.split()[1:]) for line in lines}
            missing = [j for e in expected for j in e.joins if j[2] and j not in logged]
            assert not missing, missing[:5]
