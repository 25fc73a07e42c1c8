#!/usr/bin/env python3
"""tools/sort_ab.py -- the sort entry next to what a torch user writes today, on the same int64 tensors, alternating:
  (a) sort          Engine.sort_columns(keys): sorted keys and the stable permutation
  (b) torch_sort    torch.sort(keys, stable=True)
  (c) argsort       Engine.argsort_columns(keys): the permutation alone (the last pass stores no key)
  (d) torch_argsort torch.argsort(keys, stable=True)
and the three payload forms of rhj_sort_cols_dev on preallocated outputs, timed by the HIP events of rhj_get_timings:
  (e) keys_only     no row output                       24 B per tuple and pass
  (f) narrow        implicit rowIDs, both outputs       32 B
  (g) wide          explicit rowIDs, both outputs       40 B
at 10^6, 10^7 and 10^8 rows (--rows) for full-range 64-bit keys, 32-bit-range keys, 20-bit dense ids and a 16-value column (--dists).

After --warmup runs of each route they are timed alternately for --steps steps.  One JSON line per step and route:
  total_ms   (a) - (d) a torch.cuda.Event pair around the whole route on torch's stream (the engine's call inside it is waited for on
             the host, so the pair spans it; allocations are inside); (e) - (g) first launch start -> last launch end of the call
             ("kinds": per kernel kind), with "sort_bits", "sort_passes" and "pass_gbs": bytes per pass of the form x passes x rows
             over the summed histogram + scan + scatter time, to be read against the 4.9 - 5.3 TB/s of a copy
  wall_ms    host clock around the route, synchronised at both ends
Checked at every size: (a)'s keys and permutation and (c)'s permutation equal torch's, (e) - (g) give the same order.  A summary line
(medians, min, max) per size and distribution closes."""
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
ap.add_argument("--dists", default="full64,range32,dense20,sixteen")
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_sort_ab.jsonl"))
a = ap.parse_args()
sink = open(a.out, "w")
TORCH_ROUTES = ("sort", "torch_sort", "argsort", "torch_argsort")
FORMS = {"keys_only": 24, "narrow": 32, "wide": 40}                         # bytes per tuple and pass (include/rhj.h)
ROUTES = TORCH_ROUTES + tuple(FORMS)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    sink.write(line + "\n")
    sink.flush()


def med_spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def make_keys(dist, n, gen):
    if dist == "full64":
        return torch.randint(-(1 << 63), (1 << 63) - 1, (n,), device="cuda", dtype=torch.int64, generator=gen)
    if dist == "range32":
        return torch.randint(0, 1 << 32, (n,), device="cuda", dtype=torch.int64, generator=gen) - (1 << 31)
    if dist == "dense20":
        return torch.randint(0, 1 << 20, (n,), device="cuda", dtype=torch.int64, generator=gen)
    if dist == "sixteen":
        vals = torch.randint(-(1 << 62), 1 << 62, (16,), device="cuda", dtype=torch.int64, generator=gen)
        return vals[torch.randint(0, 16, (n,), device="cuda", generator=gen)]
    raise ValueError(dist)


eng = rhj.Engine(0)
gen = torch.Generator(device="cuda")
gen.manual_seed(20)
for n, dist in [(int(x), d) for x in a.rows.split(",") if x for d in a.dists.split(",") if d]:
    keys = make_keys(dist, n, gen).contiguous()
    rows = torch.randint(-(1 << 62), 1 << 62, (n,), device="cuda", dtype=torch.int64, generator=gen)
    out_keys, out_rows = (torch.empty(n, device="cuda", dtype=torch.int64) for _ in range(2))
    last = {}

    def run(route, step, timed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if route in FORMS:
            eng.set_profiling(True)
            eng.sort_cols_dev(keys, rows if route == "wide" else None, n, rhj.SORT_I64, out_keys, None if route == "keys_only" else out_rows)
            tm = eng.timings()
            bits, passes = eng.info("last.sort_bits"), eng.info("last.sort_passes")
            pass_ms = tm["hist"]["ms"] + tm["scan"]["ms"] + tm["scatter"]["ms"]
            extra = {"total_ms": round(tm["total_ms"], 4), "sort_bits": bits, "sort_passes": passes,
                     "kinds": {k: [round(tm[k]["ms"], 4), tm[k]["launches"]] for k in rhj.binding.KERNEL_KINDS},
                     "pass_gbs": round(FORMS[route] * passes * n / (pass_ms * 1e6), 1) if pass_ms > 0 else None}
            eng.set_profiling(False)
            last[route] = (out_keys.clone(), None if route == "keys_only" else out_rows.clone()) if not timed else None
        else:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            if route == "sort":
                res = eng.sort_columns(keys)[:2]
            elif route == "torch_sort":
                res = tuple(torch.sort(keys, stable=True))
            elif route == "argsort":
                res = (None, eng.argsort_columns(keys))
            else:
                res = (None, torch.argsort(keys, stable=True))
            ev[1].record()
            torch.cuda.synchronize()
            extra = {"total_ms": round(ev[0].elapsed_time(ev[1]), 4)}
            last[route] = res if not timed else None
            del res
        t1 = time.perf_counter()
        rec = {"rows": n, "dist": dist, "route": route, "step": step if timed else -1, "wall_ms": round((t1 - t0) * 1e3, 4), **extra}
        emit(rec)
        return rec

    for s in range(max(a.warmup, 1)):                                       # (the last warm-up's results are the ones checked)
        for route in ROUTES:
            run(route, s, False)
    exp_keys, exp_perm = last["torch_sort"]
    assert torch.equal(last["sort"][0], exp_keys) and torch.equal(last["sort"][1], exp_perm)
    assert torch.equal(last["argsort"][1], exp_perm) and torch.equal(last["torch_argsort"][1], exp_perm)
    assert torch.equal(last["keys_only"][0], exp_keys)
    assert torch.equal(last["narrow"][0], exp_keys) and torch.equal(last["narrow"][1], exp_perm)
    assert torch.equal(last["wide"][0], exp_keys) and torch.equal(last["wide"][1], rows[exp_perm])
    last.clear()
    del exp_keys, exp_perm
    torch.cuda.empty_cache()
    recs = {r: [] for r in ROUTES}
    for s in range(a.steps):
        for route in ROUTES:
            recs[route].append(run(route, s, True))
    summary = {"rows": n, "dist": dist, "steps": a.steps, "summary": True}
    for route in ROUTES:
        x = recs[route]
        summary[route] = {"total_ms": med_spread([y["total_ms"] for y in x]), "wall_ms": med_spread([y["wall_ms"] for y in x])}
    for route in FORMS:
        summary[route].update({k: recs[route][-1][k] for k in ("sort_bits", "sort_passes")})
        summary[route]["pass_gbs"] = med_spread([y["pass_gbs"] for y in recs[route]])
    summary["torch_sort_over_sort"] = round(summary["torch_sort"]["total_ms"]["median"] / summary["sort"]["total_ms"]["median"], 3)
    summary["torch_argsort_over_argsort"] = round(summary["torch_argsort"]["total_ms"]["median"] / summary["argsort"]["total_ms"]["median"], 3)
    emit(summary)
    del keys, rows, out_keys, out_rows
    torch.cuda.empty_cache()
eng.close()
sink.close()
