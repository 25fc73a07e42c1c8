#!/usr/bin/env python3
"""tools/keys_ab.py -- composite keys (rhj_keys_pack_dev) next to what a torch user writes today, on the same tensors,
alternating:
  (a) pack        Engine.pack_keys(keys_R, keys_S): the surrogate key columns of both sides, dictionaries kept
  (b) join        Engine.join_columns(keys_R, keys_S) on lists: pack without dictionaries, then count, allocate, join
  (c) group       Engine.group_by_columns(keys_R) on a list: pack, group-by with counts, unpack of the key output
  (d) torch_enc   torch.unique(torch.stack(cols, 1), dim=0, return_inverse=True) over the concatenation of both sides
  (e) torch_join  (d), then Engine.join_columns on the two halves of the inverse
for two and three key columns (--cols) in three data shapes (--layouts) at 10^6, 10^7 and 10^8 rows per side (--rows):
  range  every column 20 bits wide around a negative base: RANGE only, one streaming pass
  dict   every column full-range int64 with rows / 4 distinct values: every column a dictionary
  fold   as dict; with three columns and more than 2^21 rows in all the three ids no longer fit and the layout folds (the layout a run
         found is in every record: below that size, and with two columns, "fold" is a second "dict" run)
After --warmup runs of each route they are timed alternately for --steps steps, each on a torch stream of its own between two HIP
events (torch.cuda.Event), so the figure holds what the engine launched and waited for.  The torch routes run up to --torch-max-rows.
One JSON line per step and route on stdout: total_ms (the events), wall_ms (host clock, synchronised at both ends); (a) also the layout and
gbs = (K + 1) * 8 * rows of both sides / total_ms, the pack's own traffic (a RANGE-only pack reads every column once more for the
probe, which gbs does not count).  Checked at every size: (a) unpacks to its inputs, (b) and (e) find the same number of pairs, (c)
and torch.unique(dim=0) over R the same number of groups.  A summary line (medians, min, max) per configuration closes it, and only those go to --out."""
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
ap.add_argument("--cols", default="2,3")
ap.add_argument("--layouts", default="range,dict,fold")
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--torch-max-rows", type=int, default=10_000_000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_keys_ab.jsonl"))
a = ap.parse_args()
sink = open(a.out, "w")
ROUTES = ("pack", "join", "group", "torch_enc", "torch_join")


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if rec.get("summary"):                      # the steps go to stdout only: the file keeps one line per configuration
        sink.write(line + "\n")
        sink.flush()


def med_spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def make_cols(layout, k, n, gen):
    """k key columns of n rows per side: (cols_R, cols_S); a row of S meets rows of R (both sides draw rows of one pool)"""
    D = max(n // 4, 1)
    if layout == "range":
        pool = [torch.randint(-(1 << 19), 1 << 19, (D,), device="cuda", dtype=torch.int64, generator=gen) for _ in range(k)]
    else:
        pool = [torch.randint(-(1 << 62), 1 << 62, (D,), device="cuda", dtype=torch.int64, generator=gen) * 2 + 1 for _ in range(k)]
    out = []
    for _ in range(2):
        pick = torch.randint(0, D, (n,), device="cuda", generator=gen)
        out.append([p[pick].contiguous() for p in pool])
    return out


eng = rhj.Engine(0)
gen = torch.Generator(device="cuda")
gen.manual_seed(17)
stream = torch.cuda.Stream()
for n in (int(x) for x in a.rows.split(",")):
    for k in (int(x) for x in a.cols.split(",")):
        for layout in a.layouts.split(","):
            cols_R, cols_S = make_cols(layout, k, n, gen)
            routes = [r for r in ROUTES if not r.startswith("torch") or n <= a.torch_max_rows]
            last = {}

            def run(route, step, timed):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                extra = {}
                with torch.cuda.stream(stream):
                    ev[0].record()
                    if route == "pack":
                        pR, pS, plan = eng.pack_keys(cols_R, cols_S)
                        extra["layout"] = plan.layout.as_dict()
                        if not timed:
                            assert all(torch.equal(x, y) for x, y in zip(plan.unpack(pR), cols_R))
                            assert all(torch.equal(x, y) for x, y in zip(plan.unpack(pS), cols_S))
                        plan.close()
                        del pR, pS
                    elif route == "join":
                        iR, _ = eng.join_columns(cols_R, cols_S)
                        last[route] = extra["pairs"] = iR.numel()
                    elif route == "group":
                        keys, counts, _ = eng.group_by_columns(cols_R)
                        last[route] = extra["groups"] = counts.numel()
                        del keys, counts
                    else:
                        rows = torch.stack([torch.cat([r, s]) for r, s in zip(cols_R, cols_S)], 1)
                        uniq, inv = torch.unique(rows, dim=0, return_inverse=True)
                        extra["distinct"] = uniq.shape[0]
                        if route == "torch_join":
                            iR, _ = eng.join_columns(inv[:n].contiguous(), inv[n:].contiguous())
                            last[route] = extra["pairs"] = iR.numel()
                        del rows, uniq, inv
                    ev[1].record()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                rec = {"rows": n, "cols": k, "shape": layout, "route": route, "step": step if timed else -1,
                       "total_ms": round(ev[0].elapsed_time(ev[1]), 4), "wall_ms": round((t1 - t0) * 1e3, 4), **extra}
                if route == "pack":
                    rec["gbs"] = round((k + 1) * 8 * 2 * n / (rec["total_ms"] * 1e-3) / 1e9, 2)
                emit(rec)
                return rec

            for s in range(a.warmup):
                for route in routes:
                    run(route, s, False)
            recs = {r: [] for r in routes}
            for s in range(a.steps):
                for route in routes:
                    recs[route].append(run(route, s, True))
            if "torch_join" in routes:
                assert last["join"] == last["torch_join"], last
                groups = torch.unique(torch.stack(cols_R, 1), dim=0).shape[0]
                assert groups == last["group"], (groups, last)
            lay = recs["pack"][-1]["layout"]
            summary = {"rows": n, "cols": k, "shape": layout, "steps": a.steps, "summary": True, "kind": lay["kind"],
                       "folds": len(lay["folds"]), "total_bits": lay["total_bits"], "pairs": last.get("join"), "groups": last.get("group")}
            for route in routes:
                r = recs[route]
                summary[route] = {"total_ms": med_spread([x["total_ms"] for x in r]), "wall_ms": med_spread([x["wall_ms"] for x in r])}
            summary["pack"]["gbs"] = med_spread([x["gbs"] for x in recs["pack"]])
            if "torch_enc" in routes:
                summary["torch_enc_over_pack"] = round(summary["torch_enc"]["total_ms"]["median"] / summary["pack"]["total_ms"]["median"], 3)
                summary["torch_join_over_join"] = round(summary["torch_join"]["total_ms"]["median"] / summary["join"]["total_ms"]["median"], 3)
            emit(summary)
            del cols_R, cols_S
            torch.cuda.empty_cache()
eng.close()
sink.close()
