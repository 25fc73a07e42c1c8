"""A plain numpy evaluator of the query language `aliases|predicates|projections` (the reference's join.cpp protocol):
SELECT SUM(p0), SUM(p1), .. FROM the aliases WHERE every predicate holds.  It is the independent side of
tests/test_sql_eval.py and tests/test_gpu_query_sql.py and shares nothing with the executors under test: no intermediate
columns, no rowID de-duplication, no per-alias "already joined" data structure beyond one row-index array per alias.

    relations   list (one entry per relation file) of lists of uint64 columns
    query       "t0 t1 ..|a.c=b.d&a.c>N&a.c=a.d&..|a.c b.d .."   (a, b: positions in the alias list)

A conjunction does not depend on the order of its terms, and `NULL` is printed exactly when some step -- hence every
order of the steps -- leaves no row, so the answer below is the one SQL gives, whatever order an executor takes.

Outside `in_sql_class` the reference prints quirks instead of SQL (an alias that is never joined sums to 0; older columns
are dropped when a later join links two new aliases; tests/golden/edge pins them): `evaluate` refuses such a query."""
import collections

import numpy as np

U64 = np.uint64
MASK = (1 << 64) - 1

Parsed = collections.namedtuple("Parsed", "tables preds filters projs")
# what `evaluate` returns: the stdout line; (nR, nS, count) per equi-join between two different aliases that ran as a join
# (sizes of its two inputs in the query's orientation: surviving rows of an alias not joined yet, joined rows otherwise);
# masks: per predicate between two aliases already joined, (dA, dB, pairs): their distinct joined rows and the number of
# pairs of those that satisfy it -- the join an executor runs that keeps the reference's way of evaluating such a predicate
# (join the distinct rows, keep the joined rows whose pair is in the result), so a workload can bound that too;
# events: words about the path a query took, for coverage assertions
Evaluated = collections.namedtuple("Evaluated", "line joins events masks")


class Refused(ValueError):
    """the query is outside the class this evaluator answers"""


class TooLarge(RuntimeError):
    """a join result above `max_rows`: not expanded"""


def parse(query):
    tables_s, preds_s, projs_s = query.strip().split("|")
    tables = [int(t) for t in tables_s.split()]
    preds, filters = [], []                            # preds: (a1, c1, a2, c2) in text order, a1 == a2 for a same-alias one
    for term in (t for t in preds_s.split("&") if t):
        op = next(ch for ch in term if ch in "<>=")
        lhs, rhs = term.split(op)
        a, c = (int(x) for x in lhs.split("."))
        if "." in rhs:
            assert op == "=", term
            b, d = (int(x) for x in rhs.split("."))
            preds.append((a, c, b, d))
        else:
            filters.append((a, c, op, int(rhs) & MASK))
    projs = [tuple(int(x) for x in p.split(".")) for p in projs_s.split()]
    return Parsed(tables, preds, filters, projs)


def in_sql_class(query):
    """at least one equi-join between distinct aliases, every later one touches an alias already joined (a connected
    order), and every projected alias is joined"""
    q = parse(query)
    joined = set()
    for a, _, b, _ in q.preds:
        if a == b:
            continue
        if joined and a not in joined and b not in joined:
            return False
        joined.update((a, b))
    return bool(joined) and all(a in joined for a, _ in q.projs)


def read_relation(path):
    """[num_tuples, num_columns] then column-major uint64"""
    raw = np.fromfile(path, dtype=U64)
    n, nc = int(raw[0]), int(raw[1])
    assert len(raw) == 2 + n * nc, path
    return [raw[2 + c * n: 2 + (c + 1) * n] for c in range(nc)]


def match_pairs(lv, rv, max_rows):
    """positions (li, ri) of every pair with lv[li] == rv[ri]: sort one side, searchsorted the other, expand with repeat"""
    order = np.argsort(rv, kind="stable")
    rs = rv[order]
    lo, hi = np.searchsorted(rs, lv, "left"), np.searchsorted(rs, lv, "right")
    cnt = hi - lo
    total = int(cnt.sum())
    if total > max_rows:
        raise TooLarge(total)
    li = np.repeat(np.arange(len(lv), dtype=np.int64), cnt)
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    ri = order[np.repeat(lo, cnt) + within]
    return li, ri


def count_pairs(lv, rv):
    rs = np.sort(rv)
    return len(lv), len(rv), int((np.searchsorted(rs, lv, "right") - np.searchsorted(rs, lv, "left")).sum())


def evaluate(relations, query, max_rows=1 << 26):
    if not in_sql_class(query):
        raise Refused(query)
    q = parse(query)
    if {x for a, _, b, _ in q.preds if a != b for x in (a, b)} != set(range(len(q.tables))):
        raise Refused("an alias that is never joined (SQL: a cross product; the executors ignore it): " + query)
    col = lambda a, c: relations[q.tables[a]][c]
    null = Evaluated(" ".join(["NULL"] * len(q.projs)), [], [], [])
    joins, events, masks = null.joins, null.events, null.masks

    # one row-index array per alias; a filter is a boolean mask over it
    rows = [np.arange(len(relations[t][0]), dtype=np.int64) for t in q.tables]
    for a, c, op, val in q.filters:
        v = col(a, c)[rows[a]]
        keep = v < U64(val) if op == "<" else v > U64(val) if op == ">" else v == U64(val)
        rows[a] = rows[a][keep]
        if len(rows[a]) == 0:
            events.append("filter_empty")
            return null

    idx = {}                                           # alias -> its row per joined row (every array of one length)
    for k, (a, c, b, d) in enumerate(q.preds):
        last = k == len(q.preds) - 1
        if a == b or (a in idx and b in idx):          # a mask: over the alias' rows, or over the joined rows
            if a == b and a not in idx:
                events.append("same_alias_after_other_join" if idx else "same_alias_before_join")
                rows[a] = rows[a][col(a, c)[rows[a]] == col(a, d)[rows[a]]]
                n = len(rows[a])
            else:
                events.append("same_alias_after_own_join" if a == b else "mask_between_joined")
                keep = col(a, c)[idx[a]] == col(b, d)[idx[b]]
                if a != b:
                    masks.append(count_pairs(col(a, c)[np.unique(idx[a])], col(b, d)[np.unique(idx[b])]))
                idx = {x: r[keep] for x, r in idx.items()}
                n = int(keep.sum())
            if n == 0:
                events.append("mask_empty")
                return null
            continue
        if a not in idx and b not in idx:
            if idx:
                raise Refused(query)                   # not reached: in_sql_class
            li, ri = match_pairs(col(a, c)[rows[a]], col(b, d)[rows[b]], max_rows)
            joins.append((len(rows[a]), len(rows[b]), len(li)))
            events.append("join_first")
            idx = {a: rows[a][li], b: rows[b][ri]}
        elif a in idx:
            events.append("join_joined_left")
            li, ri = match_pairs(col(a, c)[idx[a]], col(b, d)[rows[b]], max_rows)
            joins.append((len(idx[a]), len(rows[b]), len(li)))
            idx = {x: r[li] for x, r in idx.items()}
            idx[b] = rows[b][ri]
        else:
            events.append("join_joined_right")
            li, ri = match_pairs(col(a, c)[rows[a]], col(b, d)[idx[b]], max_rows)
            joins.append((len(rows[a]), len(idx[b]), len(li)))
            idx = {x: r[ri] for x, r in idx.items()}
            idx[a] = rows[a][li]
        if joins[-1][2] == 0:
            events.append("join_empty_last" if last else "join_empty_first" if len(joins) == 1 else "join_empty_mid_chain")
            return null
    sums = [int(col(a, c)[idx[a]].sum(dtype=U64)) for a, c in q.projs]       # wraps mod 2^64
    return Evaluated(" ".join(str(s) for s in sums), joins, events, masks)
