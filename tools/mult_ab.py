#!/usr/bin/env python3
"""tools/mult_ab.py -- the per-row multiplicity join next to the aggregating join, on the same value columns and the same context,
alternating:
  (a) mult   rhj_join_mult_cols_dev, unweighted: out[i] = the number of partners of R's row i (8 B per row of R written by atomics)
  (b) multw  rhj_join_mult_cols_dev with a weight column on S: the 64-bit slot, a weight load per tuple of S
  (c) sum    rhj_join_sum_cols_dev with one weight column on R: the same table, folded into one accumulator
NULL ids, automatic plan below 10^9 rows per side and 8+8 bits from there on (--plan auto / 8+8 overrides).

R (kind 0, unique join values) and S (kind 1 uniform, then kind 2 Zipf 0.9) are generated in HBM at --rows per side; the columns
are derived with rhj_pairs_split; the weight column is R's generated rowID column (any 64-bit words do: the sums wrap).  After
--warmup runs of each route they are timed alternately for --steps steps.  One JSON line per step and route:
  wall_ms     host clock around the route's (synchronising) call
  total_ms    first launch start -> last launch end of the call, from the HIP events of rhj_get_timings
  join_ms     the bucket-join kernel of that call (k_mult_bkt / k_agg_bkt) on the same partitions
  semi_tables "last.semi_tables"; max_part_S: the largest partition of S
Checked: (a)'s total against (c)'s count and rhj_expected_pkfk_dev; up to 256 M rows also (a)'s out, summed, against its total and,
weighted by R's column in numpy, against (c)'s sum.  A summary line per distribution closes."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

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
ROUTES = ("mult", "multw", "sum")
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
vR, vS, ids, t, out = eng.alloc(8 * n), eng.alloc(8 * n), eng.alloc(8 * n), eng.alloc(16 * n), eng.alloc(8 * n)
eng.generate(GEN_R, t, n, 0, n)
eng.pairs_split(t, n, ids, vR)                         # ids: R's generated rowID column, the weight column of either side (any words do)
for dist in a.dists.split(","):
    if dist == "uniform":
        eng.generate(GEN_S_UNIFORM, t, n, 0, n, seed=42)
    else:
        eng.generate(GEN_S_ZIPF, t, n, 0, n, seed=42, theta_milli=int(round(float(dist[4:]) * 1000)))
    scratch = eng.alloc(8 * n)
    eng.pairs_split(t, n, scratch, vS)
    scratch.free()
    exp_pairs = eng.expected_pkfk(t, n)[0]
    answers = {}

    def run(route, step, timed):
        eng.set_profiling(True)
        t0 = time.perf_counter()
        if route == "mult":
            ans = eng.join_mult_cols_dev(vR, None, n, vS, None, n, out, n, opts=OPTS)
        elif route == "multw":
            ans = eng.join_mult_cols_dev(vR, None, n, vS, None, n, out, n, ids, n, opts=OPTS)
        else:
            ans = eng.join_sum_cols_dev(vR, None, n, vS, n, (ids,), n, opts=OPTS)
        t1 = time.perf_counter()
        tm = eng.timings()
        info = {k: eng.info("last." + k) for k in ("narrow", "countfree_R", "countfree_S", "join_kernel", "semi_tables", "max_part_R", "max_part_S")}
        eng.set_profiling(False)
        assert answers.setdefault(route, ans) == ans, "a route's answer changed between runs"
        rec = {"dist": dist, "rows": n, "plan": [tm["passes"], tm["bits1"], tm["bits2"]], "route": route, "step": step if timed else -1,
               "answer": ans, "wall_ms": round((t1 - t0) * 1e3, 4), "total_ms": round(tm["total_ms"], 4),
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
    # (a) against (c) and the generator's own count; out summed, and weighted by R's column, against (a)'s total and (c)'s sum
    count, sums = answers["sum"]
    assert answers["mult"] == count == exp_pairs, (answers, exp_pairs)
    run("mult", -1, False)
    if n <= 256_000_000:
        m = out.to_numpy(np.uint64, n)
        assert int(m.sum(dtype=np.uint64)) == count
        assert int((m * ids.to_numpy(np.uint64, n)).sum(dtype=np.uint64)) == sums[0]
    summary = {"dist": dist, "rows": n, "steps": a.steps, "summary": True, "answers": answers}
    for route in ROUTES:
        r = recs[route]
        summary[route] = {"wall_ms": med_spread([x["wall_ms"] for x in r]), "total_ms": med_spread([x["total_ms"] for x in r]),
                          "join_ms": med_spread([x["join_ms"] for x in r]), "join_kernel": r[-1]["join_kernel"],
                          "semi_tables": r[-1]["semi_tables"], "max_part_S": r[-1]["max_part_S"], "plan": r[-1]["plan"]}
    emit(summary)
for b in (vR, vS, ids, t, out):
    b.free()
eng.close()
