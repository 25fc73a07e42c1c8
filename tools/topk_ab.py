#!/usr/bin/env python3
"""tools/topk_ab.py -- the top-k entry next to the routes it replaces, on the same int64 tensors, alternating:
  (a) topk          Engine.topk_columns(keys, k): the k smallest keys, sorted, and their rows
  (b) sort_slice    Engine.sort_columns(keys) and a slice [:k]: what the engine offered before (that code is unchanged)
  (c) torch_topk    torch.topk(keys, k, largest=False, sorted=True)
  (d) kth           Engine.kth_value_columns(keys, k): the pure selection
  (e) torch_kth     torch.kthvalue(keys, k)
and rhj_topk_cols_dev on preallocated outputs, timed by the HIP events of rhj_get_timings:
  (f) dev           both outputs; "kinds" per kernel kind, "passes" / "candidates" / "sorted_rows" from rhj_get_info, and "model_gbs":
                    the bytes of the cost model -- 8 per row for the probe, each select pass, the count and the compaction read -- over
                    the summed kernel time of the call
at 10^6, 10^7 and 10^8 rows (--rows) for full-range 64-bit keys, 32-bit-range keys, 20-bit dense ids, a 16-value column and
"outliers" (all but 10 keys below 2^8, 10 near 2^40) (--dists), with k in 10, 10^3, 10^5 and n / 2 (--ks; "half" is n / 2).

After --warmup runs of each route they are timed alternately for --steps steps.  One JSON line per step and route (total_ms: a
torch.cuda.Event pair around the whole route, allocations inside; (f): first launch start -> last launch end; wall_ms: host clock,
synchronised at both ends).  Checked at every case: (a)'s keys and rows equal (b)'s, (a)'s keys equal (c)'s, (d)'s value equals (e)'s,
(f) equals (a).  A summary line (medians, min, max, and the ratios sort_slice / topk, torch_topk / topk, torch_kth / kth) closes each
case."""
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
ap.add_argument("--dists", default="full64,range32,dense20,sixteen,outliers")
ap.add_argument("--ks", default="10,1000,100000,half")
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--max-candidates", type=int, default=-1, help='"topk.max_candidates" for every engine route (-1: automatic)')
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_topk_ab.jsonl"))
a = ap.parse_args()
sink = open(a.out, "w")
ROUTES = ("topk", "sort_slice", "torch_topk", "kth", "torch_kth", "dev")


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
    if dist == "outliers":
        k = torch.randint(0, 1 << 8, (n,), device="cuda", dtype=torch.int64, generator=gen)
        where = torch.randperm(n, device="cuda", generator=gen)[:10]
        k[where] = (1 << 40) - torch.randint(1, 1 << 8, (len(where),), device="cuda", dtype=torch.int64, generator=gen)
        return k
    raise ValueError(dist)


eng = rhj.Engine(0)
eng.set_option("topk.max_candidates", a.max_candidates)
gen = torch.Generator(device="cuda")
gen.manual_seed(21)
for n, dist in [(int(x), d) for x in a.rows.split(",") if x for d in a.dists.split(",") if d]:
    keys = make_keys(dist, n, gen).contiguous()
    for k in [n // 2 if x == "half" else int(x) for x in a.ks.split(",") if x]:
        if k < 1 or k > n:
            continue
        out_keys, out_rows = (torch.empty(k, device="cuda", dtype=torch.int64) for _ in range(2))
        last = {}

        def run(route, step, timed):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            extra = {}
            if route == "dev":
                eng.set_profiling(True)
                eng.topk_cols_dev(keys, None, n, k, rhj.SORT_I64, out_keys, out_rows)
                tm = eng.timings()
                info = {x: eng.info("last.topk_" + x) for x in ("bits", "passes", "candidates", "sorted_rows")}
                kernel_ms = sum(tm[x]["ms"] for x in rhj.binding.KERNEL_KINDS)
                model = 8 * n * (3 + info["passes"]) if info["passes"] else 8 * n
                extra = {"total_ms": round(tm["total_ms"], 4), **info, "kernel_ms": round(kernel_ms, 4),
                         "kinds": {x: [round(tm[x]["ms"], 4), tm[x]["launches"]] for x in rhj.binding.KERNEL_KINDS},
                         "model_bytes_per_row": model // n, "model_gbs": round(model / (kernel_ms * 1e6), 1) if kernel_ms > 0 else None}
                eng.set_profiling(False)
                res = (out_keys.clone(), out_rows.clone()) if not timed else None
            else:
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                if route == "topk":
                    res = eng.topk_columns(keys, k)[:2]
                elif route == "sort_slice":
                    s = eng.sort_columns(keys)
                    res = (s[0][:k], s[1][:k])
                    del s
                elif route == "torch_topk":
                    res = tuple(torch.topk(keys, k, largest=False, sorted=True))
                elif route == "kth":
                    res = eng.kth_value_columns(keys, k)
                else:
                    t = torch.kthvalue(keys, k)
                    res = (int(t.values), int(t.indices))
                ev[1].record()
                torch.cuda.synchronize()
                extra = {"total_ms": round(ev[0].elapsed_time(ev[1]), 4)}
            last[route] = res if not timed else None
            del res
            t1 = time.perf_counter()
            rec = {"rows": n, "dist": dist, "k": k, "route": route, "step": step if timed else -1, "wall_ms": round((t1 - t0) * 1e3, 4), **extra}
            emit(rec)
            return rec

        for s in range(max(a.warmup, 1)):                                   # (the last warm-up's results are the ones checked)
            for route in ROUTES:
                run(route, s, False)
        assert torch.equal(last["topk"][0], last["sort_slice"][0]) and torch.equal(last["topk"][1], last["sort_slice"][1])
        assert torch.equal(last["topk"][0], last["torch_topk"][0])          # (torch.topk's choice among equal keys is its own)
        assert torch.equal(last["dev"][0], last["topk"][0]) and torch.equal(last["dev"][1], last["topk"][1])
        assert last["kth"][0] == last["torch_kth"][0] == int(last["topk"][0][-1]) and last["kth"][1] == int(last["topk"][1][-1])
        last.clear()
        torch.cuda.empty_cache()
        recs = {r: [] for r in ROUTES}
        for s in range(a.steps):
            for route in ROUTES:
                recs[route].append(run(route, s, True))
        summary = {"rows": n, "dist": dist, "k": k, "steps": a.steps, "summary": True, "max_candidates": a.max_candidates}
        for route in ROUTES:
            x = recs[route]
            summary[route] = {"total_ms": med_spread([y["total_ms"] for y in x]), "wall_ms": med_spread([y["wall_ms"] for y in x])}
        summary["dev"].update({x: recs["dev"][-1][x] for x in ("bits", "passes", "candidates", "sorted_rows", "model_bytes_per_row")})
        summary["dev"]["kernel_ms"] = med_spread([y["kernel_ms"] for y in recs["dev"]])
        summary["dev"]["model_gbs"] = med_spread([y["model_gbs"] for y in recs["dev"] if y["model_gbs"] is not None] or [0])
        med = {r: summary[r]["total_ms"]["median"] for r in ROUTES}
        summary["sort_slice_over_topk"] = round(med["sort_slice"] / med["topk"], 3)
        summary["torch_topk_over_topk"] = round(med["torch_topk"] / med["topk"], 3)
        summary["torch_kth_over_kth"] = round(med["torch_kth"] / med["kth"], 3)
        emit(summary)
        del out_keys, out_rows
        torch.cuda.empty_cache()
    del keys
    torch.cuda.empty_cache()
eng.close()
sink.close()
