#!/usr/bin/env python3
"""tools/sum_ab.py -- COUNT(*) and two SUMs over a join, two ways, on the same value columns and the same context, alternating:
  (a) sum    rhj_join_sum_cols_dev with 2 weight columns: no pair is written
  (b) pairs  the route the query executor takes without it: rhj_join_cols_dev into a pair buffer, rhj_pairs_split, then one
             rhj_sum_gather per weight column through R's side of the pairs
NULL ids, automatic plan below 10^9 rows per side and 8+8 bits from there on (--plan auto / 8+8 overrides).

R (kind 0, unique join values) and S (kind 1 uniform, then kind 2 Zipf 0.9) are generated in HBM at --rows per side; the columns
are derived with rhj_pairs_split; the weight columns are R's generated rowID column and its value column (any 64-bit words do: the
sums wrap).  After --warmup runs of each route they are timed alternately for --steps steps.  One JSON line per step and route:
  wall_ms     host clock around the route's (synchronising) calls; (b) also per stage: join_wall_ms, split_wall_ms, gather_wall_ms
  total_ms    first launch start -> last launch end of the join call, from the HIP events of rhj_get_timings
  join_ms     the bucket-join kernel of that call (k_agg_bkt, or the pair kernel "last.join_kernel" names) on the same partitions
  semi_tables "last.semi_tables"; max_part_S: the largest partition of S
Checked: (a)'s count and sums against (b)'s, and the count against rhj_expected_pkfk_dev.  A summary line per distribution closes."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import radixhashjoin_amd as rhj  # noqa: E402
from radixhashjoin_amd.binding import GEN_R, GEN_S_UNIFORM, GEN_S_ZIPF  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=64_000_000)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--dists", default="uniform,zipf0.9")
ap.add_argument("--plan", default=None, choices=("auto", "8+8"))
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
a = ap.parse_args()
n = a.rows
plan = a.plan or ("8+8" if n >= 1_000_000_000 else "auto")
OPTS = rhj.Opts(2, 8, 8) if plan == "8+8" else None
ROUTES = ("sum", "pairs")
sink = open(a.out, "a") if a.out else None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


def med_spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


eng = rhj.Engine(0)
vR, vS, ids, t = eng.alloc(8 * n), eng.alloc(8 * n), eng.alloc(8 * n), eng.alloc(16 * n)
eng.generate(GEN_R, t, n, 0, n)
eng.pairs_split(t, n, ids, vR)
W = (ids, vR)                                          # the weight columns, indexed by R's rowID (= position)
for dist in a.dists.split(","):
    if dist == "uniform":
        eng.generate(GEN_S_UNIFORM, t, n, 0, n, seed=42)
    else:
        eng.generate(GEN_S_ZIPF, t, n, 0, n, seed=42, theta_milli=int(round(float(dist[4:]) * 1000)))
    kr = eng.alloc(8 * n)
    eng.pairs_split(t, n, kr, vS)
    exp_pairs = eng.expected_pkfk(t, n)[0]
    pairs, ks = eng.alloc(16 * exp_pairs), eng.alloc(8 * exp_pairs)
    if exp_pairs > n:
        kr.free()
        kr = eng.alloc(8 * exp_pairs)
    answers = {}

    def run(route, step, timed):
        eng.set_profiling(True)
        stages = {}
        t0 = time.perf_counter()
        if route == "sum":
            cnt, sums = eng.join_sum_cols_dev(vR, None, n, vS, n, W, n, opts=OPTS)
        else:
            cnt = eng.join_cols_dev(vR, None, n, vS, None, n, pairs, exp_pairs, opts=OPTS)
        t1 = time.perf_counter()
        tm = eng.timings()
        info = {k: eng.info("last." + k) for k in ("narrow", "countfree_R", "countfree_S", "join_kernel", "semi_tables", "max_part_R", "max_part_S")}
        wall = (t1 - t0) * 1e3
        if route == "pairs":
            t2 = time.perf_counter()
            eng.pairs_split(pairs, cnt, kr, ks)
            eng.sync()
            t3 = time.perf_counter()
            sums = [eng.sum_gather(w, kr, cnt) for w in W]
            t4 = time.perf_counter()
            stages = {"join_wall_ms": round(wall, 4), "split_wall_ms": round((t3 - t2) * 1e3, 4), "gather_wall_ms": round((t4 - t3) * 1e3, 4)}
            wall += (t4 - t2) * 1e3
        eng.set_profiling(False)
        assert answers.setdefault(route, (cnt, sums)) == (cnt, sums), "a route's answer changed between runs"
        rec = {"dist": dist, "rows": n, "plan": [tm["passes"], tm["bits1"], tm["bits2"]], "route": route, "step": step if timed else -1,
               "count": cnt, "sums": sums, "wall_ms": round(wall, 4), **stages, "total_ms": round(tm["total_ms"], 4),
               "join_ms": round(tm["join"]["ms"], 4), "tasks_ms": round(tm["tasks"]["ms"], 4), "ntasks": tm["ntasks"],
               "kinds": {k: [round(tm[k]["ms"], 4), tm[k]["launches"]] for k in rhj.binding.KERNEL_KINDS}, **info}
        emit(rec)
        return rec

    for w in range(a.warmup):
        for route in ROUTES:
            run(route, w, False)
    recs = {r: [] for r in ROUTES}
    for step in range(a.steps):
        for route in ROUTES:
            recs[route].append(run(route, step, True))
    assert answers["sum"] == answers["pairs"], answers
    assert answers["sum"][0] == exp_pairs, (answers, exp_pairs)
    summary = {"dist": dist, "rows": n, "steps": a.steps, "summary": True, "count": answers["sum"][0], "sums": answers["sum"][1]}
    for route in ROUTES:
        r = recs[route]
        summary[route] = {"wall_ms": med_spread([x["wall_ms"] for x in r]), "total_ms": med_spread([x["total_ms"] for x in r]),
                          "join_ms": med_spread([x["join_ms"] for x in r]), "join_kernel": r[-1]["join_kernel"],
                          "semi_tables": r[-1]["semi_tables"], "max_part_S": r[-1]["max_part_S"], "plan": r[-1]["plan"]}
        if route == "pairs":
            for k in ("join_wall_ms", "split_wall_ms", "gather_wall_ms"):
                summary[route][k] = med_spread([x[k] for x in r])
    emit(summary)
    for b in (kr, ks, pairs):
        b.free()
for b in (vR, vS, ids, t):
    b.free()
eng.close()
