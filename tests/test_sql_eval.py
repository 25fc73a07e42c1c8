"""CPU suite: tests/sql_eval.py anchored to the real reference.  tests/golden/small/small.result and
tests/golden/edge/edge.result are what the reference printed for small.work and edge.work; every query of the class the
evaluator answers must evaluate to its committed line."""
import os

import pytest

import sql_eval
from conftest import golden_workdir

# small.work queries left out because numpy cannot expand an intermediate of theirs in a few seconds (at most 5 of 50)
SMALL_LEFT_OUT = ()
MAX_ROWS = 40_000_000


def load(name):
    d = os.path.join(golden_workdir(), name)
    init = open(os.path.join(d, f"{name}.init")).read().split()
    assert init[-1] == "Done"
    relations = [sql_eval.read_relation(os.path.join(golden_workdir(), p)) for p in init[:-1]]
    queries = [q for q in open(os.path.join(d, f"{name}.work")).read().splitlines() if q and q != "F"]
    result = open(os.path.join(d, f"{name}.result")).read().splitlines()
    assert len(queries) == len(result)
    return relations, queries, result


@pytest.fixture(scope="module")
def small():
    return load("small")


@pytest.fixture(scope="module")
def edge():
    return load("edge")


def test_small_work_is_in_the_class(small):
    _, queries, _ = small
    assert len(queries) == 50 and len(SMALL_LEFT_OUT) <= 5
    assert all(sql_eval.in_sql_class(q) for q in queries)


def test_small_work_matches_the_reference(small):
    relations, queries, result = small
    bad = []
    for q, line in zip(queries, result):
        if q in SMALL_LEFT_OUT:
            continue
        got = sql_eval.evaluate(relations, q, max_rows=MAX_ROWS).line
        if got != line:
            bad.append((q, got, line))
    assert not bad, bad


def test_edge_work_classified_and_matches_the_reference(edge):
    relations, queries, result = edge
    assert len(queries) == 6
    # a projected alias that is never joined; two disconnected joins: the reference's quirks, not SQL
    assert not sql_eval.in_sql_class(queries[0]) and not sql_eval.in_sql_class(queries[1])
    # a-b, c-d, then b-c: the second join links two new aliases
    assert not sql_eval.in_sql_class(queries[2])
    inside = [i for i, q in enumerate(queries) if sql_eval.in_sql_class(q)]
    assert inside == [3, 4, 5]
    for i in inside:
        assert sql_eval.evaluate(relations, queries[i]).line == result[i], queries[i]
    for i in (0, 1, 2):
        with pytest.raises(sql_eval.Refused):
            sql_eval.evaluate(relations, queries[i])


def test_class_and_refusals():
    assert not sql_eval.in_sql_class("0|0.1=0.2|0.0")                     # no equi-join between distinct aliases
    assert not sql_eval.in_sql_class("0 1|0.1>3|0.0")
    assert sql_eval.in_sql_class("0 1 2|0.1=0.2&1.0=2.0&0.0=1.1|0.0")       # same-alias predicates do not count as joins
    assert sql_eval.in_sql_class("0 1 2|0.0=1.0|0.1")                      # alias 2 is not projected ...
    with pytest.raises(sql_eval.Refused):                                  # ... but SQL would multiply by its row count
        sql_eval.evaluate([[[1, 2]] * 2] * 3, "0 1 2|0.0=1.0|0.1")


def test_tiny_query_by_hand():
    import numpy as np
    u = lambda *v: np.array(v, dtype=np.uint64)
    big = (1 << 64) - 1
    r0 = [u(1, 2, 2, 3), u(5, 6, 7, 2), u(big, big, 1, 0)]
    r1 = [u(2, 2, 3, 9), u(2, 0, 3, 9)]
    # pairs on r0.c0 = r1.c0: rows (1,0) (1,1) (2,0) (2,1) (3,2); r0.c2 sums to 2*big + 2*1 + 0 = 0 mod 2^64
    e = sql_eval.evaluate([r0, r1], "0 1|0.0=1.0|0.2 1.1 0.1")
    assert e.line == "0 7 28" and e.joins == [(4, 4, 5)]
    # r1.c0 = r1.c1 keeps rows 0, 2, 3 of r1: pairs (1,0) (2,0) (3,2)
    for q in ("0 1|1.0=1.1&0.0=1.0|0.1 1.0", "0 1|0.0=1.0&1.0=1.1|0.1 1.0", "0 1|0.0=1.0&1.1=1.0&0.0=1.0|0.1 1.0"):
        assert sql_eval.evaluate([r0, r1], q).line == "15 7"
    assert sql_eval.evaluate([r0, r1], "0 1|0.0=1.0&0.2>%d|0.1" % (1 << 63)).line == "12"       # unsigned compare
    assert sql_eval.evaluate([r0, r1], "0 1|0.0=1.0&0.2>%d|0.1 1.1" % big).line == "NULL NULL"
