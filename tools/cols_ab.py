#!/usr/bin/env python3
"""tools/cols_ab.py -- A/B of the two device-resident entry points on the same data and the same context:
rhj_join_dev on 16-byte tuples against rhj_join_cols_dev on the value columns with NULL ids (rowID = index), plan 8+8.

R (kind 0) and S (kind 1 uniform, then kind 2 Zipf 0.9) are generated in HBM at --rows per side; the columns are derived with
rhj_pairs_split (a tuple array has the layout of a pair array: d_r gets the rowIDs, d_s the join values).  After --warmup
runs of each entry the two are timed alternately for --steps steps.  One JSON line per step and entry:
  wall_ms     host clock around the (synchronising) call
  total_ms    first launch start -> last launch end, from the HIP events of rhj_get_launch_timings
  launches    [[kind, ms], ...] in launch order; pass1_ms = the pass-1 scatter launches of R and S (the first and third
              scatter span of a fused two-pass join, see rhj.h rhj_get_launch_timings)
Count and checksum of both entries are verified against rhj_expected_pkfk_dev.  A summary line per distribution closes."""
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
ap.add_argument("--rows", type=int, default=1_000_000_000)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--dists", default="uniform,zipf0.9")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
a = ap.parse_args()
if a.steps < 10:
    ap.error("at least 10 timed steps")
n = a.rows
PLAN = rhj.Opts(2, 8, 8)
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
dR, dS, out = eng.alloc(16 * n), eng.alloc(16 * n), eng.alloc(16 * n)
vR, vS, ids = eng.alloc(8 * n), eng.alloc(8 * n), eng.alloc(8 * n)
eng.generate(GEN_R, dR, n, 0, n)
eng.pairs_split(dR, n, ids, vR)
for dist in a.dists.split(","):
    if dist == "uniform":
        eng.generate(GEN_S_UNIFORM, dS, n, 0, n, seed=42)
    else:
        eng.generate(GEN_S_ZIPF, dS, n, 0, n, seed=42, theta_milli=int(round(float(dist[4:]) * 1000)))
    eng.pairs_split(dS, n, ids, vS)
    exp = eng.expected_pkfk(dS, n)

    def run(entry, step, timed):
        eng.set_profiling(True)
        t0 = time.perf_counter()
        if entry == "aos":
            cnt = eng.join_dev(dR, n, dS, n, out, n, opts=PLAN)
        else:
            cnt = eng.join_cols_dev(vR, None, n, vS, None, n, out, n, opts=PLAN)
        wall = (time.perf_counter() - t0) * 1e3
        launches = eng.launch_timings()
        t = eng.timings()
        info = {k: eng.info("last." + k) for k in ("narrow", "countfree_R", "countfree_S", "cols_R", "cols_S")}
        eng.set_profiling(False)
        if not timed or step == a.steps - 1:                      # every warm-up run and the last timed step are verified
            got = (cnt, eng.pairs_checksum(out, cnt))
            assert got == exp, (dist, entry, got, exp)
        assert cnt == exp[0]
        scat = [ms for kind, ms in launches if kind == "scatter"]
        rec = {"dist": dist, "rows": n, "entry": entry, "step": step if timed else -1, "wall_ms": round(wall, 4),
               "total_ms": round(t["total_ms"], 4), "pass1_ms": [round(scat[0], 4), round(scat[2], 4)] if len(scat) == 4 else None,
               "narrow": info["narrow"], "countfree": [info["countfree_R"], info["countfree_S"]], "cols": [info["cols_R"], info["cols_S"]],
               "launches": [[kind, round(ms, 4)] for kind, ms in launches]}
        emit(rec)
        return rec

    for w in range(a.warmup):
        for entry in ("aos", "cols"):
            run(entry, w, False)
    recs = {"aos": [], "cols": []}
    for step in range(a.steps):
        for entry in ("aos", "cols"):
            recs[entry].append(run(entry, step, True))
    summary = {"dist": dist, "rows": n, "steps": a.steps, "summary": True}
    for entry in ("aos", "cols"):
        r = recs[entry]
        summary[entry] = {"wall_ms": med_spread([x["wall_ms"] for x in r]), "total_ms": med_spread([x["total_ms"] for x in r])}
        if all(x["pass1_ms"] for x in r):
            summary[entry]["pass1_R_ms"] = med_spread([x["pass1_ms"][0] for x in r])
            summary[entry]["pass1_S_ms"] = med_spread([x["pass1_ms"][1] for x in r])
    emit(summary)
for b in (dR, dS, out, vR, vS, ids):
    b.free()
eng.close()
