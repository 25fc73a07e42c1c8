#!/usr/bin/env python3
"""tools/semi_ab.py -- the semi / anti join entry next to the inner join, on the same value columns and the same context:
rhj_semi_join_cols_dev (RHJ_SEMI, then RHJ_ANTI) alternating with rhj_join_cols_dev, all three in count-only mode, NULL ids,
automatic plan below 10^9 rows per side and 8+8 bits from there on (--plan auto / 8+8 overrides).

R (kind 0, unique join values) and S (kind 1 uniform, then kind 2 Zipf 0.9) are generated in HBM at --rows per side; the columns
are derived with rhj_pairs_split.  After --warmup runs of each entry they are timed alternately for --steps steps.  One JSON line
per step and entry:
  wall_ms     host clock around the (synchronising) call
  total_ms    first launch start -> last launch end, from the HIP events of rhj_get_timings
  kinds       summed device ms and launches per kernel kind (join_ms: the bucket-join kernel -- k_semi_bkt, or the pair kernel
              "last.join_kernel" names -- on the same partitions)
  semi_tables "last.semi_tables"; max_part_S: the largest partition of S
Checked: semi + anti == rows, and the inner join's count against rhj_expected_pkfk_dev.  A summary line per distribution closes."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import radixhashjoin_amd as rhj  # noqa: E402
from radixhashjoin_amd.binding import ANTI, GEN_R, GEN_S_UNIFORM, GEN_S_ZIPF, SEMI  # noqa: E402

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
ENTRIES = ("semi", "anti", "inner")
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
for dist in a.dists.split(","):
    if dist == "uniform":
        eng.generate(GEN_S_UNIFORM, t, n, 0, n, seed=42)
    else:
        eng.generate(GEN_S_ZIPF, t, n, 0, n, seed=42, theta_milli=int(round(float(dist[4:]) * 1000)))
    eng.pairs_split(t, n, ids, vS)
    exp_pairs = eng.expected_pkfk(t, n)[0]
    counts = {}

    def run(entry, step, timed):
        eng.set_profiling(True)
        t0 = time.perf_counter()
        if entry == "inner":
            cnt = eng.join_cols_dev(vR, None, n, vS, None, n, opts=OPTS)
        else:
            cnt = eng.semi_join_cols_dev(vR, None, n, vS, n, SEMI if entry == "semi" else ANTI, opts=OPTS)
        wall = (time.perf_counter() - t0) * 1e3
        tm = eng.timings()
        info = {k: eng.info("last." + k) for k in ("narrow", "countfree_R", "countfree_S", "join_kernel", "semi_tables", "max_part_R", "max_part_S")}
        eng.set_profiling(False)
        assert counts.setdefault(entry, cnt) == cnt
        rec = {"dist": dist, "rows": n, "plan": [tm["passes"], tm["bits1"], tm["bits2"]], "entry": entry, "step": step if timed else -1,
               "count": cnt, "wall_ms": round(wall, 4), "total_ms": round(tm["total_ms"], 4), "join_ms": round(tm["join"]["ms"], 4),
               "tasks_ms": round(tm["tasks"]["ms"], 4), "ntasks": tm["ntasks"],
               "kinds": {k: [round(tm[k]["ms"], 4), tm[k]["launches"]] for k in rhj.binding.KERNEL_KINDS}, **info}
        emit(rec)
        return rec

    for w in range(a.warmup):
        for entry in ENTRIES:
            run(entry, w, False)
    recs = {e: [] for e in ENTRIES}
    for step in range(a.steps):
        for entry in ENTRIES:
            recs[entry].append(run(entry, step, True))
    assert counts["semi"] + counts["anti"] == n, counts
    assert counts["inner"] == exp_pairs, (counts, exp_pairs)
    summary = {"dist": dist, "rows": n, "steps": a.steps, "summary": True, "counts": counts}
    for entry in ENTRIES:
        r = recs[entry]
        summary[entry] = {"wall_ms": med_spread([x["wall_ms"] for x in r]), "total_ms": med_spread([x["total_ms"] for x in r]),
                          "join_ms": med_spread([x["join_ms"] for x in r]), "join_kernel": r[-1]["join_kernel"],
                          "semi_tables": r[-1]["semi_tables"], "max_part_S": r[-1]["max_part_S"], "plan": r[-1]["plan"]}
    emit(summary)
for b in (vR, vS, ids, t):
    b.free()
eng.close()
