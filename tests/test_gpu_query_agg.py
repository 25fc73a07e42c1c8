"""Whole queries through the `join_gpu` CLI with RHJ_QUERY_MODE=agg against tests/sql_eval.py: the workload of
test_gpu_query_sql.py plus two queries with more than RHJ_SUM_MAX_COLS projections on one side of their last join.

In this mode a query whose LAST predicate is an equi-join through the hot path never produces that join's pairs: its projections
are grouped by the side of the join their alias arrives on and summed by rhj_join_sum_cols_dev, which logs "sum <nR> <nS> <count>"
per call (the side the summed columns belong to first: the evaluator's orientation, or the exchanged one).  Every other join logs
its "cols" line as in the cols mode.  Every stdout line must equal the evaluator's, and the log must show that the new path ran
where it applies, in both orientations, and nowhere else."""
import os
import subprocess
import time

import pytest

import sql_eval
from test_gpu_query_sql import A, B, C, CHILD_TIMEOUT_S, D, JOIN, workload, workload_text, write_relation

SUM_MAX_COLS = 4
JOIN_EVENTS = ("join_first", "join_joined_left", "join_joined_right")
# more projections on one side of the last join than one call sums: six on the joined side (and one on the new alias), then five on
# a new alias (and one on the other)
EXTRA = [
    f"{C} {D} {B}|0.0=1.1&2.0=1.2|0.3 1.3 0.0 1.0 0.2 1.2 2.3",
    f"{B} {A}|0.1=1.0|0.0 0.1 0.2 0.3 0.0 1.3",
]


def queries_and_expected():
    rels, queries, expected = workload()
    return rels, list(queries) + EXTRA, list(expected) + [sql_eval.evaluate(rels, q) for q in EXTRA]


def ends_in_a_join(e):
    """the query reached its last predicate, and that predicate ran as a join (its sizes and count: e.joins[-1])"""
    return bool(e.events) and (e.events[-1] in JOIN_EVENTS or e.events[-1] == "join_empty_last")


def sides_of_last_join(q, e):
    """(aliases that arrive on the first input of the last join, ... on the second), in the evaluator's orientation"""
    p = sql_eval.parse(q)
    a, _, b, _ = p.preds[-1]
    earlier = {x for u, _, v, _ in p.preds[:-1] if u != v for x in (u, v)}
    kind = e.events[-2] if e.events[-1] == "join_empty_last" else e.events[-1]
    if kind == "join_first":
        return {a}, {b}
    return (earlier, {b}) if kind == "join_joined_left" else ({a}, earlier)


def test_workload_reaches_the_new_path_and_its_neighbours():
    _, queries, expected = queries_and_expected()
    both = one_side_many = masks_last = 0
    for q, e in zip(queries, expected):
        p = sql_eval.parse(q)
        if e.line[0] == "N":
            continue
        if not ends_in_a_join(e):
            masks_last += 1                                                # ends in a mask: must not take the new path
            continue
        left, right = sides_of_last_join(q, e)
        nl, nr = sum(1 for a, _ in p.projs if a in left), sum(1 for a, _ in p.projs if a in right)
        both += bool(nl and nr)
        one_side_many += max(nl, nr) > SUM_MAX_COLS
    assert both >= 10 and masks_last >= 5 and one_side_many >= 2, (both, masks_last, one_side_many)
    for kind in JOIN_EVENTS:
        assert any(ends_in_a_join(e) and e.events[-1] == kind and e.line[0] != "N" for e in expected), kind
    assert any(e.events and e.events[-1] == "join_empty_last" for e in expected)


@pytest.mark.gpu
def test_agg_mode_matches_the_evaluator_and_sums_without_pairs(tmp_path):
    assert os.path.exists(JOIN), "build with __graft_entry__.build()"
    rels, queries, expected = queries_and_expected()
    for r, cols in enumerate(rels):
        write_relation(tmp_path / f"r{r}", cols)
    text = workload_text(queries)
    stdin = ("".join(str(tmp_path / f"r{r}") + "\n" for r in range(len(rels))) + "Done\n" + text).encode()
    log = tmp_path / "joins_agg.log"
    env = dict(os.environ, RHJ_QUERY_MODE="agg", RHJ_JOIN_LOG=str(log))
    t0 = time.perf_counter()
    r = subprocess.run([JOIN], input=stdin, env=env, capture_output=True, timeout=CHILD_TIMEOUT_S)
    print(f"mode agg: join_gpu took {time.perf_counter() - t0:.2f} s")
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stderr.decode()[-2000:]}\n{text}"
    got = r.stdout.decode().splitlines()
    for i, (q, e) in enumerate(zip(queries, expected)):
        assert i < len(got) and got[i] == e.line, \
            f"query {i}: {q}\n  join_gpu:  {got[i] if i < len(got) else '(no line)'}\n  evaluator: {e.line}\n{text}"
    assert len(got) == len(queries), f"{len(got)} lines for {len(queries)} queries"

    lines = open(log).read().splitlines() if os.path.exists(log) else []
    for line in lines:
        f = line.split()
        assert f[0] in ("cols", "sum") and len(f) == 4 and all(x.isdigit() for x in f[1:]), line
    sums = {tuple(int(x) for x in line.split()[1:]) for line in lines if line.startswith("sum ")}
    cols = {tuple(int(x) for x in line.split()[1:]) for line in lines if line.startswith("cols ")}
    print(f"{len(lines)} log lines: {len(sums)} distinct sum calls, {len(cols)} distinct cols calls")
    assert sums, "no rhj_join_sum_cols_dev call was logged"
    flip = lambda j: (j[1], j[0], j[2])
    last = {e.joins[-1] for e in expected if ends_in_a_join(e)}
    stray = [s for s in sums if s not in last and flip(s) not in last]
    assert not stray, stray[:5]
    # every query that ends in a join summed it, whichever side its joined alias is on
    for kind in JOIN_EVENTS + ("join_empty_last",):
        mine = [e.joins[-1] for e in expected if ends_in_a_join(e) and e.events[-1] == kind]
        assert mine, kind
        missing = [j for j in mine if j not in sums and flip(j) not in sums]
        assert not missing, (kind, missing[:5])
    # ... and every join that is not the last predicate of its query still ran as a columnar pair join
    earlier = [j for e in expected for j in (e.joins[:-1] if ends_in_a_join(e) else e.joins) if j[2]]
    missing = [j for j in earlier if j not in cols]
    assert not missing, missing[:5]
