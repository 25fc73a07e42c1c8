#!/usr/bin/env python3
"""tools/outer_ab.py -- the outer join entry next to the calls it replaces, on the same value columns and the same context, all in
count-only mode, NULL ids, automatic plan below 10^9 rows per side and 8+8 bits from there on (--plan auto / 8+8 overrides):
  left        rhj_outer_join_cols_dev(RHJ_OUTER_LEFT)
  left2       rhj_join_cols_dev, then rhj_semi_join_cols_dev(R, S, RHJ_ANTI): the two-call form
  full        rhj_outer_join_cols_dev(RHJ_OUTER_FULL)
  full3       rhj_join_cols_dev, then the anti join of R against S, then of S against R: the three-call form

R (kind 0, unique join values) and S (kind 1 uniform, then kind 2 Zipf 0.9) are generated in HBM at --rows per side; the columns
are derived with rhj_pairs_split.  After --warmup runs of each variant they are timed alternately for --steps steps.  One JSON line
per step and variant (a variant of several calls: the sums over its calls):
  wall_ms     host clock around the (synchronising) call(s)
  total_ms    first launch start -> last launch end of every call, from the HIP events of rhj_get_timings
  join_ms     the RHJ_K_JOIN spans: the pair kernel and the k_semi_bkt sweeps; part_ms: histograms + scans + scatters
  sections    {matched, R-only, S-only}
Checked: the sections of both outer calls against the counts of the separate calls, and the inner join's count against
rhj_expected_pkfk_dev.  A summary line per distribution closes."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import radixhashjoin_amd as rhj  # noqa: E402
from radixhashjoin_amd.binding import ANTI, GEN_R, GEN_S_UNIFORM, GEN_S_ZIPF, OUTER_FULL, OUTER_LEFT  # noqa: E402

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
VARIANTS = ("left", "left2", "full", "full3")
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


def timed_call(fn):
    """one entry call under profiling: (result, wall ms, timings, last.*)"""
    eng.set_profiling(True)
    t0 = time.perf_counter()
    res = fn()
    wall = (time.perf_counter() - t0) * 1e3
    tm = eng.timings()
    info = {k: eng.info("last." + k) for k in ("narrow", "countfree_R", "countfree_S", "join_kernel", "semi_tables", "outer_sweeps")}
    eng.set_profiling(False)
    return res, wall, tm, info


CALLS = {
    "outer_left": lambda: eng.outer_join_cols_dev(vR, None, n, vS, None, n, OUTER_LEFT, opts=OPTS)[1],
    "outer_full": lambda: eng.outer_join_cols_dev(vR, None, n, vS, None, n, OUTER_FULL, opts=OPTS)[1],
    "inner": lambda: eng.join_cols_dev(vR, None, n, vS, None, n, opts=OPTS),
    "anti_RS": lambda: eng.semi_join_cols_dev(vR, None, n, vS, n, ANTI, opts=OPTS),
    "anti_SR": lambda: eng.semi_join_cols_dev(vS, None, n, vR, n, ANTI, opts=OPTS),
}
PARTS = {"left": ("outer_left",), "left2": ("inner", "anti_RS"), "full": ("outer_full",), "full3": ("inner", "anti_RS", "anti_SR")}

for dist in a.dists.split(","):
    if dist == "uniform":
        eng.generate(GEN_S_UNIFORM, t, n, 0, n, seed=42)
    else:
        eng.generate(GEN_S_ZIPF, t, n, 0, n, seed=42, theta_milli=int(round(float(dist[4:]) * 1000)))
    eng.pairs_split(t, n, ids, vS)
    exp_pairs = eng.expected_pkfk(t, n)[0]
    seen = {}

    def run(variant, step, timed):
        wall = total = join = tasks = part = 0.0
        results, infos, plans = [], [], None
        for call in PARTS[variant]:
            res, w, tm, info = timed_call(CALLS[call])
            wall, total, join, tasks = wall + w, total + tm["total_ms"], join + tm["join"]["ms"], tasks + tm["tasks"]["ms"]
            part += tm["hist"]["ms"] + tm["scan"]["ms"] + tm["scatter"]["ms"]
            plans = [tm["passes"], tm["bits1"], tm["bits2"]]
            results.append(res)
            infos.append(info)
        if len(results) == 1:
            sections = list(results[0])
        else:
            sections = [results[0], results[1], results[2] if len(results) > 2 else 0]
        assert seen.setdefault(variant, sections) == sections
        rec = {"dist": dist, "rows": n, "plan": plans, "variant": variant, "calls": list(PARTS[variant]), "step": step if timed else -1,
               "sections": sections, "wall_ms": round(wall, 4), "total_ms": round(total, 4), "join_ms": round(join, 4),
               "tasks_ms": round(tasks, 4), "part_ms": round(part, 4), "last": infos}
        emit(rec)
        return rec

    for w in range(a.warmup):
        for variant in VARIANTS:
            run(variant, w, False)
    recs = {v: [] for v in VARIANTS}
    for step in range(a.steps):
        for variant in VARIANTS:
            recs[variant].append(run(variant, step, True))
    assert seen["left"] == seen["left2"] and seen["full"] == seen["full3"], seen
    assert seen["left"][0] == exp_pairs and seen["left"][:2] == seen["full"][:2] and seen["left"][2] == 0, (seen, exp_pairs)
    summary = {"dist": dist, "rows": n, "steps": a.steps, "summary": True, "sections": {v: seen[v] for v in VARIANTS}}
    for variant in VARIANTS:
        r = recs[variant]
        summary[variant] = {"wall_ms": med_spread([x["wall_ms"] for x in r]), "total_ms": med_spread([x["total_ms"] for x in r]),
                            "join_ms": med_spread([x["join_ms"] for x in r]), "part_ms": med_spread([x["part_ms"] for x in r]),
                            "plan": r[-1]["plan"], "last": r[-1]["last"]}
    emit(summary)
for b in (vR, vS, ids, t):
    b.free()
eng.close()
