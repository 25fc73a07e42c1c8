#!/usr/bin/env python3
"""tools/lookup_ab.py -- the lookup join next to the routes it replaces, on the same key tensors and the same context, alternating:
  (a) lookup    rhj_lookup_cols_dev (first): idx[i] = the row of S with R's key i, -1 where there is none; 8 B per row of R
  (b) mult      rhj_join_mult_cols_dev, unweighted, on the same inputs: the same kernel shape with an add whose return is unused where
                (a) has a returning minimum -- (a) / (b) is the price of the returned atomic (and of the 64-bit slot word)
  (c) pairs     today's route: rhj_join_cols_dev into a pair buffer of nR rows (the count pass of join_columns is left out: S is
                unique, nR pairs at most), rhj_pairs_split, then torch: out.fill_(-1); out[idx_R] = idx_S
  (d) lookup+gather   (a) plus rhj_gather_cols_fill of two columns of S
      pairs+gather    (c) plus, per column, torch.where(out >= 0, col[out.clamp(min=0)], fill)
S: --rows unique keys (the generator's kind 0); R: --rows foreign keys into it, uniform or Zipf 0.9 (kinds 1 and 2); "uniform-miss10":
every 10th key of R has one high bit flipped and so meets no key of S.  NULL ids, automatic plan.

Everything runs on ONE torch side stream the engine is bound to, so a route's torch parts and engine parts are ordered and a pair of
torch (HIP) events around the route times all of it, the host's read-backs inside the engine calls included.  After --warmup runs of
each route they are timed alternately for --steps steps.  One JSON line per step and route:
  route_ms    the event pair around the whole route
  total_ms    first launch start -> last launch end of the route's join call, from the HIP events of rhj_get_timings
  join_ms     the bucket-join kernel of that call
Checked every step: (a)'s index column equals (c)'s, (a)'s matched equals (b)'s total and (c)'s pair count; the gathered columns of
(d) are equal.  A summary line per case closes: medians, and the ratios (a) / (c), (a) / (b) and (d) lookup / pairs."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import radixhashjoin_amd as rhj  # noqa: E402
from radixhashjoin_amd.binding import GEN_R, GEN_S_UNIFORM, GEN_S_ZIPF  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--steps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--cases", default="uniform,zipf0.9,uniform-miss10")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
a = ap.parse_args()
n = a.rows
ROUTES = ("lookup", "mult", "pairs", "lookup+gather", "pairs+gather")
FILLS = (-1, 0)
sink = open(a.out, "a") if a.out else None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


def med_spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


dev = torch.device("cuda", 0)
eng = rhj.Engine(0)
stream = torch.cuda.Stream(dev)
with torch.cuda.stream(stream):
    eng.set_stream(stream.cuda_stream)
    new = lambda rows, cols=None: torch.empty(rows if cols is None else (rows, cols), dtype=torch.int64, device=dev)  # noqa: E731
    t, kS, kR, scratch = new(n, 2), new(n), new(n), new(n)
    eng.generate(GEN_R, t, n, 0, n)
    eng.pairs_split(t, n, scratch, kS)                  # S: the unique keys
    eng.sync()
    cols = [kS * 3 + 1, kS ^ 0x5555]                    # two payload columns of S (any words do)
    idx, mult, pairs, pr, ps, out = new(n), new(n), new(n, 2), new(n), new(n), new(n)
    got_a, got_c = [new(n), new(n)], None
    for case in a.cases.split(","):
        dist = case.split("-")[0]
        if dist == "uniform":
            eng.generate(GEN_S_UNIFORM, t, n, 0, n, seed=42)
        else:
            eng.generate(GEN_S_ZIPF, t, n, 0, n, seed=42, theta_milli=int(round(float(dist[4:]) * 1000)))
        eng.pairs_split(t, n, scratch, kR)              # R: foreign keys into S
        eng.sync()
        if case.endswith("-miss10"):
            kR[::10] ^= 1 << 62                         # absent from S (the generated values are 64-bit mixes: a flipped one is no key)
        stream.synchronize()
        answers = {}

        def run(route, step, timed):
            global got_c
            eng.set_profiling(True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            if route.startswith("lookup"):
                ans = eng.lookup_cols_dev(kR, None, n, kS, None, n, idx, n, rhj.LOOKUP_FIRST)
                tm = eng.timings()
                if route.endswith("gather"):
                    eng.gather_cols_fill(cols, n, idx, n, FILLS, got_a)
            elif route == "mult":
                ans = eng.join_mult_cols_dev(kR, None, n, kS, None, n, mult, n)
                tm = eng.timings()
            else:
                ans = eng.join_cols_dev(kR, None, n, kS, None, n, pairs, n)
                tm = eng.timings()
                eng.pairs_split(pairs, ans, pr, ps)
                out.fill_(-1)
                out[pr[:ans]] = ps[:ans]
                if route.endswith("gather"):
                    got_c = [torch.where(out >= 0, c[out.clamp(min=0)], f) for c, f in zip(cols, FILLS)]
            e1.record(stream)
            stream.synchronize()
            info = {k: eng.info("last." + k) for k in ("narrow", "join_kernel", "semi_tables", "max_part_S")}
            eng.set_profiling(False)
            assert answers.setdefault(route, ans) == ans, "a route's answer changed between runs"
            rec = {"case": case, "rows": n, "plan": [tm["passes"], tm["bits1"], tm["bits2"]], "route": route, "step": step if timed else -1,
                   "answer": ans, "route_ms": round(e0.elapsed_time(e1), 4), "total_ms": round(tm["total_ms"], 4),
                   "join_ms": round(tm["join"]["ms"], 4), "ntasks": tm["ntasks"], **info}
            emit(rec)
            return rec

        def check():
            assert answers["lookup"] == answers["mult"] == answers["pairs"] == int((idx >= 0).sum()), answers
            assert torch.equal(idx, out) and torch.equal((mult != 0), (idx >= 0))
            assert all(torch.equal(x, y) for x, y in zip(got_a, got_c))

        for w in range(a.warmup):
            for route in ROUTES:
                run(route, w, False)
        check()
        recs = {r: [] for r in ROUTES}
        for step in range(a.steps):
            for route in ROUTES:
                recs[route].append(run(route, step, True))
            check()
        summary = {"case": case, "rows": n, "steps": a.steps, "summary": True, "matched": answers["lookup"]}
        for route in ROUTES:
            r = recs[route]
            summary[route] = {"route_ms": med_spread([x["route_ms"] for x in r]), "total_ms": med_spread([x["total_ms"] for x in r]),
                              "join_ms": med_spread([x["join_ms"] for x in r]), "join_kernel": r[-1]["join_kernel"],
                              "semi_tables": r[-1]["semi_tables"], "plan": r[-1]["plan"]}
        med = lambda route, key="route_ms": summary[route][key]["median"]  # noqa: E731
        summary["ratio_a_over_c"] = round(med("lookup") / med("pairs"), 4)
        summary["ratio_a_over_b"] = round(med("lookup") / med("mult"), 4)
        summary["ratio_a_over_b_join_kernel"] = round(med("lookup", "join_ms") / med("mult", "join_ms"), 4)
        summary["ratio_d_lookup_over_pairs"] = round(med("lookup+gather") / med("pairs+gather"), 4)
        emit(summary)
    eng.set_stream(None)
eng.close()
