"""Whole queries through the `join_gpu` CLI with RHJ_QUERY_MODE=tree: a query whose equi-joins form a tree over all its aliases
is summed with no pair set at all.  SUM(a.c) over the result = the sum over the rows of alias a of c[row] * W_a[row], W_a the
product over a's neighbours of a message "how many combinations of the subtree behind this neighbour match this row"; a message
is one rhj_join_mult_cols_dev call, logged as "mult <nR> <nS> <total>".  Every other query runs as in the agg mode.

This file holds its own evaluator of eligible queries: message passing in numpy (uint64, wrapping, for the printed line; Python
integers for the true row count).  It shares no code with the executor, and the CPU test pins it to tests/sql_eval.py on every
eligible query of test_gpu_query_sql.workload().  EXTRA are queries whose joins return 10^11 rows and more: no other mode, and no
evaluator that expands rows, can run them; they are checked against this file's evaluator alone."""
import functools
import os
import subprocess
import time

import numpy as np
import pytest

import sql_eval
from conftest import golden_workdir
from test_gpu_query_sql import B, C, CHILD_TIMEOUT_S, D, JOIN, workload, workload_text, write_relation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MASK = (1 << 64) - 1
EXTRA = [
    # D (70,001 rows) to C (30,011) on the 16-value column, then to D again: about 5.7 * 10^11 joined rows
    f"{D} {C} {D}|0.2=1.2&1.2=2.2|0.3 1.0 2.3",
    # a star of four on c2
    f"{D} {D} {C} {B}|0.2=1.2&0.2=2.2&0.2=3.2|0.3 1.0 2.3 3.1",
    # filters on two aliases, the joined alias on the right
    f"{D} {C} {D}|1.2=0.2&2.2=1.2&0.0<40000&1.2>7|0.0 2.3 1.3",
    # a same-alias predicate before the joins, and one between them on an alias not joined yet
    f"{D} {D} {C}|0.0=0.3&0.2=1.2&2.0=2.3&1.2=2.2|0.3 1.3 2.0",
    # a chain of four, projected from an end alone: three messages in a row
    f"{B} {C} {D} {C}|0.2=1.2&1.2=2.2&2.2=3.2|3.3",
]


def tree_edges(q):
    """the equi-joins of an eligible query (a tree over all aliases), or None.  Walking the predicates in order: a same-alias
    predicate on a joined alias, a predicate between two joined aliases, one between two new aliases while others are joined, and
    an alias that is never joined make a query not eligible"""
    p = sql_eval.parse(q)
    joined, edges = set(), []
    for a, c, b, d in p.preds:
        if a == b:
            if a in joined:
                return None
            continue
        if (a in joined and b in joined) or (joined and a not in joined and b not in joined):
            return None
        joined.update((a, b))
        edges.append((a, c, b, d))
    return edges if joined == set(range(len(p.tables))) else None


def tree_evaluate(rels, q, exact=False):
    """(stdout line, row count of the join) of an eligible query.  exact: Python integers throughout (the true count; the line is
    then reduced mod 2^64 at the end), otherwise wrapping uint64"""
    p, edges = sql_eval.parse(q), tree_edges(q)
    dt, zero, one = (object, 0, 1) if exact else (np.uint64, np.uint64(0), np.uint64(1))
    null = (" ".join(["NULL"] * len(p.projs)), 0)
    col = lambda a, c: rels[p.tables[a]][c]
    rows = [np.arange(len(rels[t][0]), dtype=np.int64) for t in p.tables]
    for a, c, op, val in p.filters:
        v = col(a, c)[rows[a]]
        rows[a] = rows[a][v < np.uint64(val) if op == "<" else v > np.uint64(val) if op == ">" else v == np.uint64(val)]
    for a, c, b, d in p.preds:
        if a == b:
            rows[a] = rows[a][col(a, c)[rows[a]] == col(a, d)[rows[a]]]
    if any(len(r) == 0 for r in rows):
        return null

    @functools.lru_cache(maxsize=None)
    def message(e, to_first):
        """per row of v, the combinations of the subtree behind u that match it; u, v the ends of edge e"""
        a, c, b, d = edges[e]
        (u, cu), (v, cv) = ((b, d), (a, c)) if to_first else ((a, c), (b, d))
        w = weight(u, e)
        keys, inv = np.unique(col(u, cu)[rows[u]], return_inverse=True)
        share = np.zeros(len(keys), dtype=dt)
        np.add.at(share, inv.reshape(-1), one if w is None else w)
        vals = col(v, cv)[rows[v]]
        pos = np.minimum(np.searchsorted(keys, vals), len(keys) - 1)
        out = np.empty(len(vals), dtype=dt)
        out[:] = zero
        hit = keys[pos] == vals
        out[hit] = share[pos[hit]]
        return out

    def weight(a, skip):
        """the product of the messages into alias a over every edge but `skip` (None: there is none)"""
        w = None
        for e, (x, _, y, _) in enumerate(edges):
            if e != skip and a in (x, y):
                m = message(e, x == a)
                w = m if w is None else w * m
        return w

    sums, count = [], None
    for a, c in p.projs:
        W = weight(a, None)
        count = int(W.sum()) if exact else int(W.sum(dtype=np.uint64))
        if count == 0:
            return null
        vals = col(a, c)[rows[a]]
        sums.append(sum(int(x) * y for x, y in zip(vals, W)) & MASK if exact else int((vals * W).sum(dtype=np.uint64)))
    return " ".join(str(s) for s in sums), count


@functools.lru_cache(maxsize=None)
def split_workload():
    """(rels, eligible [(query, expected line)], ineligible [...]) of test_gpu_query_sql.workload()"""
    rels, queries, expected = workload()
    both = [(q, e.line) for q, e in zip(queries, expected)]
    return rels, [x for x in both if tree_edges(x[0]) is not None], [x for x in both if tree_edges(x[0]) is None]


@functools.lru_cache(maxsize=None)
def extra_expected():
    rels = workload()[0]
    return [tree_evaluate(rels, q)[0] for q in EXTRA]


def aliases(q):
    return len(sql_eval.parse(q).tables)


def test_the_evaluator_prints_sql_evals_line_for_every_eligible_query():
    rels, eligible, ineligible = split_workload()
    for q, line in eligible:
        assert tree_evaluate(rels, q)[0] == line, q
    sums = [q for q, line in eligible if line[0] != "N"]
    four = [q for q in sums if aliases(q) == 4]
    several = [q for q in sums if len({a for a, _ in sql_eval.parse(q).projs}) >= 2]
    other_sums = [q for q, line in ineligible if line[0] != "N"]
    print(len(eligible), len(sums), len(four), len(several), len(ineligible), len(other_sums))
    assert len(eligible) >= 80 and len(sums) >= 50 and len(four) >= 10 and len(several) >= 30 and len(other_sums) >= 20


def test_every_extra_query_is_eligible_and_beyond_every_other_mode():
    rels = workload()[0]
    assert any("<" in q or ">" in q for q in EXTRA)
    assert any(a == b for q in EXTRA for a, _, b, _ in sql_eval.parse(q).preds[:1])   # a same-alias predicate before the joins
    assert any(aliases(q) == 4 and len({(a, c) for a, c, _, _ in tree_edges(q)}) == 1 for q in EXTRA)   # a star of four around one column
    for q, line in zip(EXTRA, extra_expected()):
        assert tree_edges(q) is not None and sql_eval.in_sql_class(q), q
        exact_line, count = tree_evaluate(rels, q, exact=True)
        print(q, count, line)
        assert 10**9 < count < 1 << 63, (q, count)
        assert exact_line == line and line[0] != "N", q                     # wrapping uint64 = Python integers mod 2^64


def run_child(tmp_path, rels, queries, name, log=False):
    """one join_gpu child in tree mode over `queries`; a child that times out or exits non-zero raises here, so no further child is
    started.  Returns (stdout lines, log lines)"""
    for r, cols in enumerate(rels):
        if not os.path.exists(tmp_path / f"r{r}"):
            write_relation(tmp_path / f"r{r}", cols)
    text = workload_text(queries)
    stdin = ("".join(str(tmp_path / f"r{r}") + "\n" for r in range(len(rels))) + "Done\n" + text).encode()
    env = dict(os.environ, RHJ_QUERY_MODE="tree")
    env.pop("RHJ_JOIN_LOG", None)
    path = tmp_path / f"joins_{name}.log"
    if log:
        env["RHJ_JOIN_LOG"] = str(path)
    t0 = time.perf_counter()
    r = subprocess.run([JOIN], input=stdin, env=env, capture_output=True, timeout=CHILD_TIMEOUT_S)
    print(f"{name}: join_gpu took {time.perf_counter() - t0:.2f} s over {len(queries)} queries")
    assert r.returncode == 0, f"{name}: exit {r.returncode}\n{r.stderr.decode()[-2000:]}\n{text}"
    return r.stdout.decode().splitlines(), (open(path).read().splitlines() if log and os.path.exists(path) else [])


def same_lines(got, queries, lines, name):
    for i, (q, line) in enumerate(zip(queries, lines)):
        assert i < len(got) and got[i] == line, \
            f"{name}, query {i}: {q}\n  join_gpu:  {got[i] if i < len(got) else '(no line)'}\n  evaluator: {line}"
    assert len(got) == len(queries), f"{name}: {len(got)} lines for {len(queries)} queries"


@pytest.mark.gpu
def test_tree_mode_matches_the_evaluators_and_joins_without_pairs(tmp_path):
    """three join_gpu children, each started only if the one before exited 0; [measured, MI355X] 0.45 - 0.47 s per child, 215
    multiplicity joins for the 102 eligible queries (bounds 119 and 388), 1.4 s for the whole test"""
    assert os.path.exists(JOIN), "build with __graft_entry__.build()"
    rels, eligible, ineligible = split_workload()
    _, queries, expected = workload()
    # 1. the whole workload and EXTRA
    got, _ = run_child(tmp_path, rels, list(queries) + EXTRA, "all")
    same_lines(got, list(queries) + EXTRA, [e.line for e in expected] + extra_expected(), "all")
    # 2. the eligible queries alone: nothing but multiplicity joins, no more of them than two per edge
    qs = [q for q, _ in eligible] + EXTRA
    lines = [line for _, line in eligible] + extra_expected()
    got, log = run_child(tmp_path, rels, qs, "eligible", log=True)
    same_lines(got, qs, lines, "eligible")
    for entry in log:
        f = entry.split()
        assert f[0] == "mult" and len(f) == 4 and all(x.isdigit() for x in f[1:]), entry
    at_least = sum(aliases(q) - 1 for q, line in zip(qs, lines) if line[0] != "N")
    at_most = sum(2 * (aliases(q) - 1) for q in qs)
    print(f"{len(log)} multiplicity joins for {len(qs)} eligible queries: at least {at_least}, at most {at_most}")
    assert at_least <= len(log) <= at_most
    # 3. the others alone: as in the agg mode, no multiplicity join
    qs = [q for q, _ in ineligible]
    got, log = run_child(tmp_path, rels, qs, "ineligible", log=True)
    same_lines(got, qs, [line for _, line in ineligible], "ineligible")
    assert not [entry for entry in log if entry.startswith("mult")]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "edge"])
def test_golden_workloads_byte_identical_in_tree_mode(name):
    """the reference's own workload and the corner queries (a projected alias that is never joined, two disconnected joins, a
    predicate between joined aliases: not eligible, they take the agg mode's path) print what the reference printed"""
    assert os.path.exists(JOIN), "build with __graft_entry__.build()"
    d = os.path.join(GOLD, name)
    stdin = open(os.path.join(d, name + ".init"), "rb").read() + open(os.path.join(d, name + ".work"), "rb").read()
    env = dict(os.environ, RHJ_QUERY_MODE="tree")
    env.pop("RHJ_JOIN_LOG", None)
    out = subprocess.run([JOIN], input=stdin, cwd=golden_workdir(), env=env, capture_output=True, timeout=120, check=True).stdout
    assert out == open(os.path.join(d, name + ".result"), "rb").read()
