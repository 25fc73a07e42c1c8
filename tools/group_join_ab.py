#!/usr/bin/env python3
"""tools/group_join_ab.py -- the join with GROUP BY on the key, next to the best composition of the calls the library had before it,
on the same tensors, alternating:
  (a) gjoin    rhj_group_join_cols_dev: keys, cntR, cntS and the sums of --cols weight columns PER SIDE, NULL ids, automatic plan
  (b) compose  rhj_group_sum_cols_dev on R, the same on S, then a torch key intersection: sort both key sets, searchsorted, and
               gather the counts and sums of the keys both sides hold (--how left: every key of R, zeros where S has none)
at 10^6, 10^7 and 10^8 rows per side (--rows), for n/4 distinct keys drawn uniformly and by Zipf 0.9 (--dists), with 0 and 4 weight
columns per side (--cols).  S draws three quarters of its rows from R's key pool without its first quarter and a quarter of its rows
from foreign keys, so both sides hold keys the other lacks.  Keys and weights are int64 tensors made by torch on the device.

After --warmup runs of each route they are timed alternately for --steps steps.  One JSON line per step and route:
  total_ms   HIP events: (a) first launch start -> last launch end of the call, from rhj_get_timings ("kinds": per kernel kind);
             (b) the same for each of the two group-by calls plus a torch.cuda.Event pair around the intersection on torch's stream
             ("parts": the three figures)
  span_ms    a torch.cuda.Event pair around the whole route (the host's share between the launches included)
  wall_ms    host clock around the route, synchronised at both ends
  groups     the number of groups; (a) also "group_rounds", "max_part_R", "max_part_S", the plan and the format
Checked at every size: both routes find the same number of groups; up to 10^7 rows the sorted groups of (a) equal (b)'s, field by
field.  A summary line (medians, min, max) per size, distribution and column count closes."""
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
ap.add_argument("--dists", default="quarter,zipf0.9")
ap.add_argument("--cols", default="0,4")
ap.add_argument("--how", default="inner", choices=("inner", "left"))
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_group_join_ab.jsonl"))
a = ap.parse_args()
sink = open(a.out, "w")
ROUTES = ("gjoin", "compose")
MODE = rhj.GJ_LEFT if a.how == "left" else rhj.GJ_INNER


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    sink.write(line + "\n")
    sink.flush()


def med_spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def draw(dist, src, n, gen):
    D = src.numel()
    if dist == "quarter":
        return src[torch.randint(0, D, (n,), device="cuda", generator=gen)]
    theta = float(dist[4:])                                                                      # Zipf: inverse CDF of the continuous approximation
    e = 1.0 - theta
    u = torch.rand(n, device="cuda", dtype=torch.float64, generator=gen)
    r = torch.floor((1.0 + u * ((D + 1.0) ** e - 1.0)) ** (1.0 / e)).to(torch.int64).clamp_(1, D)
    return src[r - 1]


def make_sides(dist, n, gen):
    P = max(n // 4, 4)
    F = max(P // 4, 1)
    u = torch.unique(torch.randint(-(1 << 62), 1 << 62, (P + F + 1024,), device="cuda", dtype=torch.int64, generator=gen))
    assert u.numel() >= P + F
    u = u[torch.randperm(u.numel(), device="cuda", generator=gen)]
    pool, foreign = u[:P], u[P:P + F]
    nf = n // 4
    kS = torch.cat([draw(dist, pool[P // 4:], n - nf, gen), draw(dist, foreign, nf, gen)])
    return draw(dist, pool, n, gen).contiguous(), kS[torch.randperm(n, device="cuda", generator=gen)].contiguous()


def timings(eng):
    tm = eng.timings()
    return tm, {k: [round(tm[k]["ms"], 4), tm[k]["launches"]] for k in rhj.binding.KERNEL_KINDS}


eng = rhj.Engine(0)
gen = torch.Generator(device="cuda")
gen.manual_seed(12)
new = lambda m: torch.empty(m, device="cuda", dtype=torch.int64)
for n in (int(x) for x in a.rows.split(",")):
    wR = [torch.randint(-(1 << 62), 1 << 62, (n,), device="cuda", dtype=torch.int64, generator=gen) for _ in range(4)]
    wS = [torch.randint(-(1 << 62), 1 << 62, (n,), device="cuda", dtype=torch.int64, generator=gen) for _ in range(4)]
    cap = n // 3 + 1024                                                    # (n/4 keys per pool and their foreign quarter)
    out = {"keys": new(cap), "cntR": new(cap), "cntS": new(cap), "sumsR": [new(cap) for _ in range(4)], "sumsS": [new(cap) for _ in range(4)]}
    gR = {"keys": new(cap), "cnt": new(cap), "sums": [new(cap) for _ in range(4)]}
    gS = {"keys": new(cap), "cnt": new(cap), "sums": [new(cap) for _ in range(4)]}
    for dist in a.dists.split(","):
        kR, kS = make_sides(dist, n, gen)
        for ncols in (int(x) for x in a.cols.split(",")):
            last = {}

            def run(route, step, timed):
                torch.cuda.synchronize()
                span = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                t0 = time.perf_counter()
                span[0].record()
                eng.set_profiling(True)
                if route == "gjoin":
                    groups = eng.group_join_cols_dev(kR, None, n, kS, None, n, wR[:ncols], n, wS[:ncols], n, MODE, out["keys"], out["cntR"],
                                                     out["cntS"], out["sumsR"][:ncols], out["sumsS"][:ncols], cap)
                    tm, kinds = timings(eng)
                    extra = {"total_ms": round(tm["total_ms"], 4), "plan": [tm["passes"], tm["bits1"], tm["bits2"]], "ntasks": tm["ntasks"],
                             "kinds": kinds, **{k: eng.info("last." + k) for k in ("narrow", "countfree_R", "countfree_S", "join_kernel",
                                                                                     "group_rounds", "max_part_R", "max_part_S")}}
                    last[route] = groups
                else:
                    nR_ = eng.group_sum_cols_dev(kR, None, n, wR[:ncols], n, gR["keys"], gR["cnt"], gR["sums"][:ncols], cap)
                    t_R = eng.timings()["total_ms"]
                    nS_ = eng.group_sum_cols_dev(kS, None, n, wS[:ncols], n, gS["keys"], gS["cnt"], gS["sums"][:ncols], cap)
                    t_S = eng.timings()["total_ms"]
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    ev[0].record()
                    sR, pR = torch.sort(gR["keys"][:nR_])
                    sS, pS = torch.sort(gS["keys"][:nS_])
                    pos = torch.searchsorted(sS, sR).clamp_(max=nS_ - 1)
                    hit = sS[pos] == sR
                    if a.how == "inner":
                        iR, iS = pR[hit], pS[pos[hit]]
                        res = (sR[hit], gR["cnt"][iR], gS["cnt"][iS], [s[iR] for s in gR["sums"][:ncols]], [s[iS] for s in gS["sums"][:ncols]])
                    else:
                        iS = pS[pos]
                        zero = torch.zeros((), device="cuda", dtype=torch.int64)
                        res = (sR, gR["cnt"][pR], torch.where(hit, gS["cnt"][iS], zero), [s[pR] for s in gR["sums"][:ncols]],
                               [torch.where(hit, s[iS], zero) for s in gS["sums"][:ncols]])
                    ev[1].record()
                    torch.cuda.synchronize()
                    t_X = ev[0].elapsed_time(ev[1])
                    groups = res[0].numel()
                    extra = {"total_ms": round(t_R + t_S + t_X, 4), "parts": [round(t_R, 4), round(t_S, 4), round(t_X, 4)],
                             "groups_R": nR_, "groups_S": nS_}
                    last[route] = res
                eng.set_profiling(False)
                span[1].record()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                rec = {"rows": n, "dist": dist, "cols": ncols, "how": a.how, "route": route, "step": step if timed else -1, "groups": groups,
                       "span_ms": round(span[0].elapsed_time(span[1]), 4), "wall_ms": round((t1 - t0) * 1e3, 4), **extra}
                emit(rec)
                return rec

            for s in range(a.warmup):
                for route in ROUTES:
                    run(route, s, False)
            recs = {r: [] for r in ROUTES}
            for s in range(a.steps):
                for route in ROUTES:
                    recs[route].append(run(route, s, True))
            groups = last["gjoin"]
            res = last["compose"]
            assert groups == res[0].numel(), (groups, res[0].numel())
            if n <= 10_000_000:
                order = torch.argsort(out["keys"][:groups])
                assert torch.equal(out["keys"][:groups][order], res[0])
                assert torch.equal(out["cntR"][:groups][order], res[1]) and torch.equal(out["cntS"][:groups][order], res[2])
                for j in range(ncols):
                    assert torch.equal(out["sumsR"][j][:groups][order], res[3][j]) and torch.equal(out["sumsS"][j][:groups][order], res[4][j])
            last.clear()
            del res
            summary = {"rows": n, "dist": dist, "cols": ncols, "how": a.how, "steps": a.steps, "summary": True, "groups": groups}
            for route in ROUTES:
                r = recs[route]
                summary[route] = {k: med_spread([x[k] for x in r]) for k in ("total_ms", "span_ms", "wall_ms")}
            summary["gjoin"].update({k: recs["gjoin"][-1][k] for k in ("plan", "narrow", "group_rounds", "max_part_R", "max_part_S", "ntasks")})
            summary["compose"]["parts"] = [round(statistics.median(x["parts"][i] for x in recs["compose"]), 4) for i in range(3)]
            summary["compose_over_gjoin"] = round(summary["compose"]["total_ms"]["median"] / summary["gjoin"]["total_ms"]["median"], 3)
            emit(summary)
        del kR, kS
    del wR, wS, out, gR, gS
    torch.cuda.empty_cache()
eng.close()
sink.close()
