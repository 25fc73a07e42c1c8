#!/usr/bin/env python3
"""tools/window_ab.py -- the window entry next to the route a caller had before it, on the same int64 tensors, alternating:
  (a) window        Engine.window_columns(part, order, [None, x], ["row_number", "cumsum"]): ROW_NUMBER() and a running SUM(x) OVER
                    (PARTITION BY part ORDER BY order), aligned with the rows
  (b) chain         the same two tensors from the entries that were there before (that code is unchanged):
                    group_by_columns_with_inverse(part) for dense ids, sort_columns([ids, order], values=[x]) for the order,
                    torch.cumsum with per-group offset corrections, a running maximum of head positions for the row number, and a
                    scatter back through the permutation
and rhj_window_cols_dev on preallocated outputs, timed by the HIP events of rhj_get_launch_timings:
  (c) dev           "sort_ms": the launches of the two inner sorts and the gather between them; "sweep_ms": the eight launches behind
                    them -- heads, the partition start's reduce / carry / apply, the row-number launch, the sum's reduce / carry /
                    apply --; "model_gbs": the bytes of the cost model for those eight (25 + 10 + 24 + 42 = 101 per
                    row) over sweep_ms
at 10^6, 10^7 and 10^8 rows (--rows) for ~n / 100 uniform partitions, Zipf(0.9) over as many, and one partition (--shapes); the order
column is full-range, the summed column small enough that torch's int64 cumsum and the entry's sum mod 2^64 agree without a wrap.

After --warmup runs of each route they are timed alternately for --steps steps.  One JSON line per step and route on stdout
(total_ms: a torch.cuda.Event pair around the whole route, allocations inside; (c): the sum of its launches; wall_ms: host clock,
synchronised at both ends).  Checked at every case: (a) equals (b), (c) equals (a).  A summary line (medians, min, max, and the ratio
chain / window) closes each case; the summary lines, and only they, also go to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import radixhashjoin_amd as rhj  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--rows", default="1000000,10000000,100000000")
ap.add_argument("--shapes", default="uniform,zipf,one")
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_window_ab.jsonl"))
a = ap.parse_args()
sink = open(a.out, "w")
ROUTES = ("window", "chain", "dev")
SWEEP_LAUNCHES, SWEEP_BYTES = 8, 25 + 10 + 24 + 42


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if rec.get("summary"):
        sink.write(line + "\n")
        sink.flush()


def med_spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def make_part(shape, n, gen):
    groups = max(n // 100, 1)
    if shape == "uniform":
        ids = torch.randint(0, groups, (n,), device="cuda", dtype=torch.int64, generator=gen)
    elif shape == "zipf":                                                  # inverse CDF of p(i) ~ (i + 1)^-0.9 over the groups
        p = torch.arange(1, groups + 1, device="cuda", dtype=torch.float64) ** -0.9
        cdf = torch.cumsum(p / p.sum(), 0)
        ids = torch.searchsorted(cdf, torch.rand(n, device="cuda", dtype=torch.float64, generator=gen)).clamp_(max=groups - 1)
    elif shape == "one":
        return torch.full((n,), 42, device="cuda", dtype=torch.int64)
    else:
        raise ValueError(shape)
    return ids * -7046029254386353131 - (1 << 62)                        # (0x9E3779B97F4A7C15 as int64, odd: a bijection) keys over the 64-bit range, not dense ids


def chain(eng, part, order, x):
    n = part.numel()
    inverse = eng.group_by_columns_with_inverse(part)[3]
    sorted_keys, perm, (xs,) = eng.sort_columns([inverse, order], values=[x])
    ids = sorted_keys[0]
    pos = torch.arange(n, device=part.device, dtype=torch.int64)
    head = torch.ones(n, device=part.device, dtype=torch.bool)
    head[1:] = ids[1:] != ids[:-1]
    start = torch.cummax(torch.where(head, pos, torch.zeros_like(pos)), 0).values
    c = torch.cumsum(xs, 0)
    running = c - (c[start] - xs[start])
    number, total = torch.empty_like(pos), torch.empty_like(pos)
    number[perm] = pos - start + 1
    total[perm] = running
    return number, total


eng = rhj.Engine(0)
gen = torch.Generator(device="cuda")
gen.manual_seed(22)
for n, shape in [(int(r), s) for r in a.rows.split(",") if r for s in a.shapes.split(",") if s]:
    part = make_part(shape, n, gen).contiguous()
    order = torch.randint(-(1 << 63), (1 << 63) - 1, (n,), device="cuda", dtype=torch.int64, generator=gen)
    x = torch.randint(-1000, 1000, (n,), device="cuda", dtype=torch.int64, generator=gen)
    out_number, out_total = (torch.empty(n, device="cuda", dtype=torch.int64) for _ in range(2))
    last = {}

    def run(route, step, timed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if route == "dev":
            eng.set_profiling(True)
            partitions = eng.window_cols_dev(part, order, n, rhj.SORT_I64, [rhj.WIN_ROW_NUMBER, rhj.WIN_CUMSUM], None, [None, x],
                                             [out_number, out_total])
            spans, units = eng.launch_timings(), eng.info("last.window_units")
            eng.set_profiling(False)                                        # (resets "last.*")
            sort_ms, sweep_ms = sum(ms for _, ms in spans[:-SWEEP_LAUNCHES]), sum(ms for _, ms in spans[-SWEEP_LAUNCHES:])
            extra = {"total_ms": round(sort_ms + sweep_ms, 4), "launches": len(spans), "sort_ms": round(sort_ms, 4), "sweep_ms": round(sweep_ms, 4),
                     "partitions": partitions, "units": units,
                     "model_gbs": round(SWEEP_BYTES * n / (sweep_ms * 1e6), 1) if sweep_ms > 0 else None}
            res = (out_number.clone(), out_total.clone()) if not timed else None
        else:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            if route == "window":
                res = tuple(eng.window_columns(part, order, [None, x], ["row_number", "cumsum"]))
            else:
                res = chain(eng, part, order, x)
            ev[1].record()
            torch.cuda.synchronize()
            extra = {"total_ms": round(ev[0].elapsed_time(ev[1]), 4)}
        last[route] = res if not timed else None
        del res
        t1 = time.perf_counter()
        rec = {"rows": n, "shape": shape, "route": route, "step": step if timed else -1, "wall_ms": round((t1 - t0) * 1e3, 4), **extra}
        emit(rec)
        return rec

    for s in range(max(a.warmup, 1)):                                       # (the last warm-up's results are the ones checked)
        for route in ROUTES:
            run(route, s, False)
    for j in range(2):
        assert torch.equal(last["window"][j], last["chain"][j]) and torch.equal(last["dev"][j], last["window"][j])
    last.clear()
    torch.cuda.empty_cache()
    recs = {r: [] for r in ROUTES}
    for s in range(a.steps):
        for route in ROUTES:
            recs[route].append(run(route, s, True))
    summary = {"rows": n, "shape": shape, "steps": a.steps, "summary": True}
    for route in ROUTES:
        y = recs[route]
        summary[route] = {"total_ms": med_spread([z["total_ms"] for z in y]), "wall_ms": med_spread([z["wall_ms"] for z in y])}
    summary["dev"].update({k: recs["dev"][-1][k] for k in ("launches", "partitions", "units")})
    for k in ("sort_ms", "sweep_ms"):
        summary["dev"][k] = med_spread([z[k] for z in recs["dev"]])
    summary["dev"]["model_bytes_per_row"] = SWEEP_BYTES
    summary["dev"]["model_gbs"] = med_spread([z["model_gbs"] for z in recs["dev"] if z["model_gbs"] is not None] or [0])
    summary["chain_over_window"] = round(summary["chain"]["total_ms"]["median"] / summary["window"]["total_ms"]["median"], 3)
    emit(summary)
    del part, order, x, out_number, out_total
    torch.cuda.empty_cache()
eng.close()
sink.close()
