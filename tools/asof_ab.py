#!/usr/bin/env python3
"""tools/asof_ab.py -- the as-of join entry next to the routes a caller had before it, on the same int64 tensors, alternating:
  (a) asof          Engine.asof_join_columns(on_R, on_S, by_R, by_S): for every row of R the index of the last row of S of its
                    partition at or before it, -1 where there is none, aligned with R
  (b) torch         the same tensor without the entry:
                    without `by`: torch.sort(on_S, stable=True), torch.searchsorted(.., right=True) - 1 and a gather of the
                    permutation;
                    with `by` (searchsorted has no lexicographic form): the engine's sort_columns chain over the concatenation
                    [S ; R] of both tables, torch.cummax over the flagged positions of S, cut at the partition offsets, and a scatter
                    through the permutation
and rhj_asof_cols_dev on a preallocated output, timed by the HIP events of rhj_get_launch_timings:
  (c) dev           "order_ms": the concatenation, the inner sorts, the gather between them and the heads launch; "scan_ms": the
                    three launches behind them -- reduce, carry, apply --; "model_gbs": the bytes of the cost model for those three
                    (1 + 9 per row of nR + nS, and a gathered 8-byte load and a scattered 8-byte store per row of R) over
                    scan_ms
at 10^6, 10^7 and 10^8 rows per side (--rows), distinct timestamps and heavy duplicates (--times: distinct,dup), for one partition
(no `by`), 10^3 uniform partitions and Zipf(0.9) over 10^3 (--shapes: one,uniform,zipf).

After --warmup runs of each route they are timed alternately for --steps steps.  One JSON line per step and route on stdout
(total_ms: a torch.cuda.Event pair around the whole route, allocations inside; (c): the sum of its launches; wall_ms: host clock,
synchronised at both ends).  Checked at every case: (a) equals (b), (c) equals (a).  A summary line (medians, min, max, and the ratio
torch / asof, "slower" where it is below 1) closes each case; the summary lines, and only they, are also APPENDED to --out, so that
a run over some of the sizes adds to the table instead of replacing it (start a new table by removing the file)."""
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
ap.add_argument("--times", default="distinct,dup")
ap.add_argument("--shapes", default="one,uniform,zipf")
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_asof_ab.jsonl"))
a = ap.parse_args()
sink = open(a.out, "a")
ROUTES = ("asof", "torch", "dev")
SCAN_LAUNCHES = 3
GROUPS = 1000


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if rec.get("summary"):
        sink.write(line + "\n")
        sink.flush()


def med_spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def make_by(shape, n, gen):
    if shape == "one":
        return None
    if shape == "uniform":
        ids = torch.randint(0, GROUPS, (n,), device="cuda", dtype=torch.int64, generator=gen)
    elif shape == "zipf":                                                  # inverse CDF of p(i) ~ (i + 1)^-0.9 over the groups
        p = torch.arange(1, GROUPS + 1, device="cuda", dtype=torch.float64) ** -0.9
        cdf = torch.cumsum(p / p.sum(), 0)
        ids = torch.searchsorted(cdf, torch.rand(n, device="cuda", dtype=torch.float64, generator=gen)).clamp_(max=GROUPS - 1)
    else:
        raise ValueError(shape)
    return (ids * -7046029254386353131 - (1 << 62)).contiguous()          # (0x9E3779B97F4A7C15 as int64, odd: a bijection) words over the 64-bit range


def make_on(kind, n, gen):
    """both tables' timestamps at once: a permutation of 0 .. 2n - 1 (no two rows share one), or 2n draws of n / 100 values"""
    if kind == "distinct":
        t = torch.randperm(2 * n, device="cuda", dtype=torch.int64, generator=gen)
    elif kind == "dup":
        t = torch.randint(0, max(n // 100, 1), (2 * n,), device="cuda", dtype=torch.int64, generator=gen)
    else:
        raise ValueError(kind)
    t = t * 1000 - (1 << 40)                                                # negative and positive values
    return t[:n].contiguous(), t[n:].contiguous()


def torch_route(eng, on_R, on_S, by_R, by_S):
    nR, nS = on_R.numel(), on_S.numel()
    if by_R is None:
        s, perm = torch.sort(on_S, stable=True)
        k = torch.searchsorted(s, on_R, right=True) - 1
        return torch.where(k >= 0, perm[k.clamp(min=0)], torch.full_like(k, -1))
    n = nR + nS
    by, on = torch.cat([by_S, by_R]), torch.cat([on_S, on_R])
    keys, perm, _ = eng.sort_columns([by, on])                              # equal (by, on): S in front of R, in input order
    sb = keys[0]
    pos = torch.arange(n, device=on.device, dtype=torch.int64)
    head = torch.ones(n, device=on.device, dtype=torch.bool)
    head[1:] = sb[1:] != sb[:-1]
    start = torch.cummax(torch.where(head, pos, torch.zeros_like(pos)), 0).values
    is_s = perm < nS
    seen = torch.cummax(torch.where(is_s, pos + 1, torch.zeros_like(pos)), 0).values
    partner = torch.where(seen - 1 >= start, perm[(seen - 1).clamp(min=0)], torch.full_like(pos, -1))
    out = torch.empty(nR, device=on.device, dtype=torch.int64)
    r = ~is_s
    out[perm[r] - nS] = partner[r]
    return out


eng = rhj.Engine(0)
gen = torch.Generator(device="cuda")
gen.manual_seed(23)
cases = [(int(r), t, s) for r in a.rows.split(",") if r for t in a.times.split(",") if t for s in a.shapes.split(",") if s]
for n, kind, shape in cases:
    on_R, on_S = make_on(kind, n, gen)
    by = make_by(shape, 2 * n, gen)
    by_R, by_S = (None, None) if by is None else (by[:n].contiguous(), by[n:].contiguous())
    del by
    out_rows = torch.empty(n, device="cuda", dtype=torch.int64)
    model_bytes = (1 + 9) * 2 * n + (8 + 8) * n
    last = {}

    def run(route, step, timed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if route == "dev":
            eng.set_profiling(True)
            matched = eng.asof_cols_dev(by_R, on_R, n, by_S, on_S, n, rhj.ASOF_I64, 0, out_rows)
            spans, units = eng.launch_timings(), eng.info("last.asof_units")
            eng.set_profiling(False)                                        # (resets "last.*")
            order_ms, scan_ms = sum(ms for _, ms in spans[:-SCAN_LAUNCHES]), sum(ms for _, ms in spans[-SCAN_LAUNCHES:])
            extra = {"total_ms": round(order_ms + scan_ms, 4), "launches": len(spans), "order_ms": round(order_ms, 4), "scan_ms": round(scan_ms, 4),
                     "matched": matched, "units": units, "model_gbs": round(model_bytes / (scan_ms * 1e6), 1) if scan_ms > 0 else None}
            res = out_rows.clone() if not timed else None
        else:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            if route == "asof":
                res = eng.asof_join_columns(on_R, on_S, by_R, by_S)[0]
            else:
                res = torch_route(eng, on_R, on_S, by_R, by_S)
            ev[1].record()
            torch.cuda.synchronize()
            extra = {"total_ms": round(ev[0].elapsed_time(ev[1]), 4)}
        last[route] = res if not timed else None
        del res
        t1 = time.perf_counter()
        rec = {"rows_per_side": n, "times": kind, "shape": shape, "route": route, "step": step if timed else -1,
               "wall_ms": round((t1 - t0) * 1e3, 4), **extra}
        emit(rec)
        return rec

    for s in range(max(a.warmup, 1)):                                       # (the last warm-up's results are the ones checked)
        for route in ROUTES:
            run(route, s, False)
    assert torch.equal(last["asof"], last["torch"]) and torch.equal(last["dev"], last["asof"])
    last.clear()
    torch.cuda.empty_cache()
    recs = {r: [] for r in ROUTES}
    for s in range(a.steps):
        for route in ROUTES:
            recs[route].append(run(route, s, True))
    summary = {"rows_per_side": n, "times": kind, "shape": shape, "steps": a.steps, "summary": True}
    for route in ROUTES:
        y = recs[route]
        summary[route] = {"total_ms": med_spread([z["total_ms"] for z in y]), "wall_ms": med_spread([z["wall_ms"] for z in y])}
    summary["dev"].update({k: recs["dev"][-1][k] for k in ("launches", "matched", "units")})
    for k in ("order_ms", "scan_ms"):
        summary["dev"][k] = med_spread([z[k] for z in recs["dev"]])
    summary["dev"]["model_bytes"] = model_bytes
    summary["dev"]["model_gbs"] = med_spread([z["model_gbs"] for z in recs["dev"] if z["model_gbs"] is not None] or [0])
    summary["torch_over_asof"] = round(summary["torch"]["total_ms"]["median"] / summary["asof"]["total_ms"]["median"], 3)
    summary["verdict"] = "faster" if summary["torch_over_asof"] >= 1 else "**slower**"
    emit(summary)
    del on_R, on_S, by_R, by_S, out_rows
    torch.cuda.empty_cache()
eng.close()
sink.close()
