#!/usr/bin/env python3
"""tools/group_ids_ab.py -- GROUP BY with the group of every row (torch.unique's return_inverse), next to what a torch user writes
today and next to the same call without ids, on the same tensors, alternating:
  (a) ids    rhj_group_agg_ids_cols_dev: keys, counts and one id per row, no weight column, NULL ids, automatic plan
  (b) plain  rhj_group_agg_cols_dev: keys and counts of the same rows (what the id sweep and its stores are added to)
  (c) torch  torch.unique(keys, return_inverse=True, return_counts=True)
at 10^6, 10^7 and 10^8 rows (--rows), for all-distinct keys, n/4 distinct keys and Zipf 0.9 over n/4 keys (--dists).  Keys are int64
tensors made by torch on the device.

After --warmup runs of each route they are timed alternately for --steps steps.  One JSON line per step and route:
  total_ms   (a), (b) first launch start -> last launch end of the call, from the HIP events of rhj_get_timings ("kinds": per kernel
             kind); (c) a torch.cuda.Event pair around the route on torch's stream
  wall_ms    host clock around the route, synchronised at both ends
  groups     the number of groups; (a), (b) also "group_rounds", "max_part_R", the plan and the format
Checked at every size: the three routes find the same number of groups, (a)'s keys[ids] are the input keys and the bincount of its
ids is its count column, and up to 10^7 rows the sorted groups of (a) equal (c)'s.  A summary line (medians, min, max) per size and
distribution closes."""
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
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_group_ids_ab.jsonl"))
a = ap.parse_args()
sink = open(a.out, "w")
ROUTES = ("ids", "plain", "torch")


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    sink.write(line + "\n")
    sink.flush()


def med_spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def make_keys(dist, n, gen):
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
gen.manual_seed(14)
for n in (int(x) for x in a.rows.split(",")):
    out_keys, out_counts, out_ids = (torch.empty(n, device="cuda", dtype=torch.int64) for _ in range(3))
    for dist in a.dists.split(","):
        keys = make_keys(dist, n, gen).contiguous()
        last = {}

        def run(route, step, timed):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if route != "torch":
                eng.set_profiling(True)
                if route == "ids":
                    groups = eng.group_agg_ids_cols_dev(keys, None, n, (), None, 0, out_keys, out_counts, (), n, out_ids, n)
                else:
                    groups = eng.group_agg_cols_dev(keys, None, n, (), None, 0, out_keys, out_counts, (), n)
                tm = eng.timings()
                extra = {"total_ms": round(tm["total_ms"], 4), "plan": [tm["passes"], tm["bits1"], tm["bits2"]], "ntasks": tm["ntasks"],
                         "kinds": {k: [round(tm[k]["ms"], 4), tm[k]["launches"]] for k in rhj.binding.KERNEL_KINDS},
                         **{k: eng.info("last." + k) for k in ("narrow", "countfree_R", "cols_R", "join_kernel", "group_rounds", "max_part_R")}}
                eng.set_profiling(False)
                last[route] = groups
            else:
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                uk, inv, cnt = torch.unique(keys, return_inverse=True, return_counts=True)
                ev[1].record()
                torch.cuda.synchronize()
                groups = uk.numel()
                extra = {"total_ms": round(ev[0].elapsed_time(ev[1]), 4)}
                last[route] = (uk, cnt)
                del inv
            t1 = time.perf_counter()
            rec = {"rows": n, "dist": dist, "route": route, "step": step if timed else -1, "groups": groups,
                   "wall_ms": round((t1 - t0) * 1e3, 4), **extra}
            emit(rec)
            return rec

        for s in range(a.warmup):
            for route in ("plain", "ids", "torch"):                         # (the outputs are left holding (a)'s)
                run(route, s, False)
        recs = {r: [] for r in ROUTES}
        for s in range(a.steps):
            for route in ("plain", "ids", "torch"):
                recs[route].append(run(route, s, True))
        groups = last["ids"]
        uk, cnt = last["torch"]
        assert groups == uk.numel() == last["plain"], (groups, uk.numel(), last["plain"])
        assert torch.equal(out_keys[:groups][out_ids], keys)
        assert torch.equal(torch.bincount(out_ids, minlength=groups), out_counts[:groups])
        if n <= 10_000_000:
            order = torch.argsort(out_keys[:groups])
            assert torch.equal(out_keys[:groups][order], uk) and torch.equal(out_counts[:groups][order], cnt)
        last.clear()
        del uk, cnt
        summary = {"rows": n, "dist": dist, "steps": a.steps, "summary": True, "groups": groups}
        for route in ROUTES:
            r = recs[route]
            summary[route] = {"total_ms": med_spread([x["total_ms"] for x in r]), "wall_ms": med_spread([x["wall_ms"] for x in r])}
        summary["ids"].update({k: recs["ids"][-1][k] for k in ("plan", "narrow", "group_rounds", "max_part_R", "ntasks")})
        summary["torch_over_ids"] = round(summary["torch"]["total_ms"]["median"] / summary["ids"]["total_ms"]["median"], 3)
        summary["ids_over_plain"] = round(summary["ids"]["total_ms"]["median"] / summary["plain"]["total_ms"]["median"], 3)
        emit(summary)
        del keys
    del out_keys, out_counts, out_ids
    torch.cuda.empty_cache()
eng.close()
sink.close()
