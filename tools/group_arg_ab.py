#!/usr/bin/env python3
"""tools/group_arg_ab.py -- which row holds each group's maximum (the latest record per key), next to what a torch user writes today
with the ids entry and next to the aggregate the row sweep adds to, on the same tensors, alternating:
  (a) arg    rhj_group_arg_cols_dev: keys, counts, MAX_I64 of one column and the row that holds it (ties: first), NULL ids, automatic plan
  (b) ids    Engine.group_by_columns_with_inverse(keys, [t], ops=["max"]), then vals[inverse] == t and a scatter_reduce_(amin) of the
             row numbers that tie -- keys, counts, maxima and the same rows through the inverse index
  (c) agg    rhj_group_agg_cols_dev with the same one MAX_I64 column: what (a) costs without its rows
at 10^6, 10^7 and 10^8 rows (--rows), for all-distinct keys, n/4 distinct keys and Zipf 0.9 over n/4 keys (--dists), and for the worst
case of (a): --worst rows (10^7) of ONE key with a constant column, where every tuple ties and takes a global atomic on one word.
Keys and the column are int64 tensors made by torch on the device.

After --warmup runs of each route they are timed alternately for --steps steps.  One JSON line per step and route:
  total_ms   (a), (c) first launch start -> last launch end of the call, from the HIP events of rhj_get_timings ("kinds": per kernel
             kind); (b) a torch.cuda.Event pair around the whole route on torch's stream (the engine's call inside it is waited for
             on the host, so the pair spans it; torch's allocations are inside)
  wall_ms    host clock around the route, synchronised at both ends
  groups     the number of groups; (a), (c) also "group_rounds", "max_part_R", the plan and the format
Checked at every size: the three routes find the same number of groups, (a)'s counts add up to the rows, every row (a) names holds its
group's maximum and its group's key, and up to 10^7 rows the sorted groups and rows of (a) equal (b)'s.  A summary line (medians, min,
max) per size and distribution closes."""
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
ap.add_argument("--dists", default="distinct,quarter,zipf0.9")
ap.add_argument("--worst", type=int, default=10_000_000, help="rows of the one-key, constant-column case (0: skip it)")
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_group_arg_ab.jsonl"))
a = ap.parse_args()
sink = open(a.out, "w")
ROUTES = ("arg", "ids", "agg")


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    sink.write(line + "\n")
    sink.flush()


def med_spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def make_keys(dist, n, gen):
    if dist == "one-key":
        return torch.full((n,), 0x0FEDCBA987654321, device="cuda", dtype=torch.int64)
    if dist == "distinct":
        return torch.randperm(n, device="cuda", generator=gen) * 0x2545F4914F6CDD1D + 12345        # (odd multiplier: a bijection)
    D = max(n // 4, 1)
    base = torch.randint(-(1 << 62), 1 << 62, (D,), device="cuda", dtype=torch.int64, generator=gen)
    if dist == "quarter":
        return base[torch.randint(0, D, (n,), device="cuda", generator=gen)]
    theta = float(dist[4:])                                                                      # Zipf: inverse CDF of the continuous approximation
    e = 1.0 - theta
    u = torch.rand(n, device="cuda", dtype=torch.float64, generator=gen)
    r = torch.floor((1.0 + u * ((D + 1.0) ** e - 1.0)) ** (1.0 / e)).to(torch.int64).clamp_(1, D)
    return base[r - 1]


eng = rhj.Engine(0)
gen = torch.Generator(device="cuda")
gen.manual_seed(19)
cases = [(int(x), d) for x in a.rows.split(",") if x for d in a.dists.split(",") if d] + ([(a.worst, "one-key")] if a.worst else [])
for n, dist in cases:
    if dist == "one-key":
        t = torch.full((n,), 42, device="cuda", dtype=torch.int64)
    else:
        t = torch.randint(-(1 << 62), 1 << 62, (n,), device="cuda", dtype=torch.int64, generator=gen)
    out_keys, out_counts, out_vals, out_rows = (torch.empty(n, device="cuda", dtype=torch.int64) for _ in range(4))
    keys = make_keys(dist, n, gen).contiguous()
    arange = torch.arange(n, device="cuda", dtype=torch.int64)
    last = {}

    def run(route, step, timed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if route != "ids":
            eng.set_profiling(True)
            if route == "arg":
                groups = eng.group_arg_cols_dev(keys, None, n, [t], [rhj.ARG_MAX_I64], [rhj.ARG_TIE_FIRST], n, out_keys, out_counts,
                                                [out_vals], [out_rows], n)
            else:
                groups = eng.group_agg_cols_dev(keys, None, n, [t], [rhj.AGG_MAX_I64], n, out_keys, out_counts, [out_vals], n)
            tm = eng.timings()
            extra = {"total_ms": round(tm["total_ms"], 4), "plan": [tm["passes"], tm["bits1"], tm["bits2"]], "ntasks": tm["ntasks"],
                     "kinds": {k: [round(tm[k]["ms"], 4), tm[k]["launches"]] for k in rhj.binding.KERNEL_KINDS},
                     **{k: eng.info("last." + k) for k in ("narrow", "countfree_R", "cols_R", "join_kernel", "group_rounds", "max_part_R")}}
            eng.set_profiling(False)
            last[route] = groups
        else:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            uk, cnt, (vals,), inv = eng.group_by_columns_with_inverse(keys, [t], ops=["max"])
            tie = vals[inv] == t
            rows = torch.full_like(uk, n).scatter_reduce_(0, inv[tie], arange[tie], "amin")
            ev[1].record()
            torch.cuda.synchronize()
            groups = uk.numel()
            extra = {"total_ms": round(ev[0].elapsed_time(ev[1]), 4)}
            last[route] = (uk, cnt, vals, rows)
            del inv, tie
        t1 = time.perf_counter()
        rec = {"rows": n, "dist": dist, "cols": 1, "route": route, "step": step if timed else -1, "groups": groups,
               "wall_ms": round((t1 - t0) * 1e3, 4), **extra}
        emit(rec)
        return rec

    for s in range(a.warmup):
        for route in ("agg", "ids", "arg"):                                 # (the outputs are left holding (a)'s)
            run(route, s, False)
    recs = {r: [] for r in ROUTES}
    for s in range(a.steps):
        for route in ("agg", "ids", "arg"):
            recs[route].append(run(route, s, True))
    groups = last["arg"]
    uk, cnt, vals, rows = last["ids"]
    assert groups == uk.numel() == last["agg"], (groups, uk.numel(), last["agg"])
    assert int(out_counts[:groups].sum()) == n
    r = out_rows[:groups]
    assert bool((r >= 0).all()) and bool((r < n).all())
    assert torch.equal(t[r], out_vals[:groups]) and torch.equal(keys[r], out_keys[:groups])
    if n <= 10_000_000:
        oa, ob = torch.argsort(out_keys[:groups]), torch.argsort(uk)
        assert torch.equal(out_keys[:groups][oa], uk[ob]) and torch.equal(out_counts[:groups][oa], cnt[ob])
        assert torch.equal(out_vals[:groups][oa], vals[ob]) and torch.equal(r[oa], rows[ob])
    last.clear()
    del uk, cnt, vals, rows, r
    summary = {"rows": n, "dist": dist, "cols": 1, "steps": a.steps, "summary": True, "groups": groups}
    for route in ROUTES:
        x = recs[route]
        summary[route] = {"total_ms": med_spread([y["total_ms"] for y in x]), "wall_ms": med_spread([y["wall_ms"] for y in x])}
    summary["arg"].update({k: recs["arg"][-1][k] for k in ("plan", "narrow", "group_rounds", "max_part_R", "ntasks")})
    summary["ids_over_arg"] = round(summary["ids"]["total_ms"]["median"] / summary["arg"]["total_ms"]["median"], 3)
    summary["arg_over_agg"] = round(summary["arg"]["total_ms"]["median"] / summary["agg"]["total_ms"]["median"], 3)
    emit(summary)
    del keys, t, arange, out_keys, out_counts, out_vals, out_rows
    torch.cuda.empty_cache()
eng.close()
sink.close()
