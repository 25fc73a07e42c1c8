#!/usr/bin/env python3
"""tools/frame_range_ab.py -- the RANGE frame entry next to the routes a caller had before it, on the same int64 tensors, alternating:
  (a) range_sum     Engine.frame_range_columns(part, order, [x, None], ["sum", "count"], d, 0): the sum and the count of the rows of
                    the same partition whose order value lies in [t - d, t]
      torch_sum     the best route of the parent: ONE composite key per row -- the group id from factorize_columns in the high bits,
                    the order value in the low 40 --, torch.sort, two torch.searchsorted (the lower bound clamped to the group's first
                    key), a cumsum and gathers, scattered back through the permutation.  It needs order values of at most 40 bits
                    beside the group id: full-range order words, which the entry takes in all four views, do not fit it at all
  (b) rows_sum      Engine.frame_columns on the same data with the ROWS frame of the mean width of (a)'s frames: the same sorts, scans
                    and emit without the searches; "search_ms" is the difference of the medians
  (c) max_w<w>      Engine.frame_range_columns(.., ["max"], d_w, 0) at distances whose frames hold about w = 4, 64, 4096 and 10^5
                    rows (--widths; clipped by the partition): "max_spread" is (slowest - fastest) / fastest of the medians across w.
                    Width-independence is NOT claimed: the searches and the walk depend on the width
  (d) dev           rhj_frame_range_cols_dev for MAX at w = 64 on a preallocated output under rhj_set_profiling: "emit_ms" the search
                    / emit launch (the last), "table_ms" the table levels (the RHJ_K_TASKS spans), "scan_ms" the six launches of its
                    two value scans (the six before them), "model_gbs" the bytes of the cost model for the scans (2 x 2 x
                    (1 + 8) read, 2 x 8 written per row) over scan_ms -- to be read against the copy rate of DESIGN 6
at 10^6, 10^7 and 10^8 rows (--rows) for one partition, ~n / 100 uniform partitions and Zipf(0.9) over as many (--shapes); the order
column holds 40-bit values, the value column is small enough that torch's int64 cumsum and the entry's sum mod 2^64 agree.

Checked at every case, on the last warm-up's results: range_sum equals torch_sum (sum and count); every max_w equals the maximum of
the slice between torch's two searchsorted positions at 256 sampled rows; (d) equals max_w64.

After --warmup runs of each route they are timed alternately for --steps steps (total_ms: a torch.cuda.Event pair around the whole
route, allocations inside; (d): the sum of its launches).  One JSON line per step and route on stdout; a summary line (medians, min,
max, the ratios) closes each case; the summary lines, and only they, also go to --out."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import radixhashjoin_amd as rhj  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--rows", default="1000000,10000000,100000000")
ap.add_argument("--shapes", default="one,uniform,zipf")
ap.add_argument("--widths", default="4,64,4096,100000")
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_frame_range_ab.jsonl"))
a = ap.parse_args()
sink = open(a.out, "w")
WIDTHS = [int(w) for w in a.widths.split(",") if w]
ROUTES = ["range_sum", "torch_sum", "rows_sum"] + [f"max_w{w}" for w in WIDTHS] + ["dev"]
ORDER_BITS, SUM_ROWS, DEV_W = 40, 10, 64
SCAN_LAUNCHES, SCAN_BYTES = 6, 2 * (2 * 9 + 8)


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
        return None
    else:
        raise ValueError(shape)
    return ids * -7046029254386353131 - (1 << 62)                        # (0x9E3779B97F4A7C15 as int64, odd: a bijection) keys over the 64-bit range, not dense ids


def torch_positions(eng, part, order, d):
    """(perm, lo, hi): the rows in (group, order) order and every position's frame [lo, hi] for the distance d before it"""
    key = order if part is None else (eng.factorize_columns(part)[0] << ORDER_BITS) | order
    skey, perm = torch.sort(key)
    floor = (skey >> ORDER_BITS) << ORDER_BITS                               # the group's smallest possible key
    lo = torch.searchsorted(skey, torch.maximum(skey - d, floor), right=False)
    hi = torch.searchsorted(skey, skey, right=True) - 1
    return perm, lo, hi


def torch_sum(eng, part, order, x, d):
    perm, lo, hi = torch_positions(eng, part, order, d)
    xs = x[perm]
    c = torch.cumsum(xs, 0)
    total, count = torch.empty_like(x), torch.empty_like(x)
    total[perm] = c[hi] - c[lo] + xs[lo]
    count[perm] = hi - lo + 1
    return total, count


eng = rhj.Engine(0)
gen = torch.Generator(device="cuda")
gen.manual_seed(25)
for n, shape in [(int(r), s) for r in a.rows.split(",") if r for s in a.shapes.split(",") if s]:
    part = make_part(shape, n, gen)
    order = torch.randint(0, 1 << ORDER_BITS, (n,), device="cuda", dtype=torch.int64, generator=gen)
    x = torch.randint(-1000, 1000, (n,), device="cuda", dtype=torch.int64, generator=gen)
    out_dev = torch.empty(n, device="cuda", dtype=torch.int64)
    per_part = n if part is None else 100                                   # the mean rows of a partition: what a distance is sized by
    dist = lambda w: min(max(w * (1 << ORDER_BITS) // per_part, 1), (1 << ORDER_BITS))
    state = {"rows_w": SUM_ROWS}
    last = {}

    def run(route, step, timed):
        torch.cuda.synchronize()
        if route == "dev":
            eng.set_profiling(True)
            partitions = eng.frame_range_cols_dev(part, order, n, rhj.SORT_I64, [rhj.FRAME_MAX_I64], [dist(DEV_W)], [0], [x], [out_dev])
            spans, units = eng.launch_timings(), eng.info("last.frame_range_units")
            scans, levels = eng.info("last.frame_range_scans"), eng.info("last.frame_range_levels")
            eng.set_profiling(False)                                        # (resets "last.*")
            assert scans * 3 == SCAN_LAUNCHES and [k for k, _ in spans[-1 - levels:-1]] == ["tasks"] * levels
            scan_ms = sum(ms for _, ms in spans[-1 - levels - SCAN_LAUNCHES:-1 - levels])
            extra = {"total_ms": round(sum(ms for _, ms in spans), 4), "launches": len(spans), "scan_ms": round(scan_ms, 4),
                     "table_ms": round(sum(ms for _, ms in spans[-1 - levels:-1]), 4), "emit_ms": round(spans[-1][1], 4),
                     "partitions": partitions, "units": units, "levels": levels,
                     "model_gbs": round(SCAN_BYTES * n / (scan_ms * 1e6), 1) if scan_ms > 0 else None}
            res = out_dev.clone() if not timed else None
        else:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            if route == "range_sum":
                res = eng.frame_range_columns(part, order, [x, None], ["sum", "count"], dist(SUM_ROWS), 0)
            elif route == "torch_sum":
                res = torch_sum(eng, part, order, x, dist(SUM_ROWS))
            elif route == "rows_sum":
                res = eng.frame_columns(part, order, [x, None], ["sum", "count"], state["rows_w"] - 1, 0)
            else:
                res = eng.frame_range_columns(part, order, [x], ["max"], dist(int(route[5:])), 0)[0]
            ev[1].record()
            torch.cuda.synchronize()
            extra = {"total_ms": round(ev[0].elapsed_time(ev[1]), 4)}
        last[route] = res if not timed else None
        del res
        rec = {"rows": n, "shape": shape, "route": route, "step": step if timed else -1, **extra}
        emit(rec)
        return rec

    for s in range(max(a.warmup, 1)):                                       # (the last warm-up's results are the ones checked)
        for route in ROUTES:
            run(route, s, False)
            if route == "range_sum":
                state["rows_w"] = max(int(round(float(last["range_sum"][1].double().mean()))), 1)
    for got, want in zip(last["range_sum"], last["torch_sum"]):
        assert torch.equal(got, want)
    sample = torch.randint(0, n, (256,), device="cuda", generator=gen).tolist()
    for w in WIDTHS:
        perm, lo, hi = torch_positions(eng, part, order, dist(w))
        xs = x[perm]
        for p in sample:
            assert int(last[f"max_w{w}"][perm[p]]) == int(xs[int(lo[p]):int(hi[p]) + 1].max()), (w, p)
        del perm, lo, hi, xs
    if DEV_W in WIDTHS:
        assert torch.equal(last["dev"], last[f"max_w{DEV_W}"])
    last.clear()
    torch.cuda.empty_cache()
    recs = {r: [] for r in ROUTES}
    for s in range(a.steps):
        for route in ROUTES:
            recs[route].append(run(route, s, True))
    summary = {"rows": n, "shape": shape, "steps": a.steps, "summary": True, "sum_distance": dist(SUM_ROWS), "rows_frame_width": state["rows_w"]}
    for route in ROUTES:
        summary[route] = {"total_ms": med_spread([z["total_ms"] for z in recs[route]])}
    summary["dev"].update({k: recs["dev"][-1][k] for k in ("launches", "partitions", "units", "levels")})
    for k in ("scan_ms", "table_ms", "emit_ms"):
        summary["dev"][k] = med_spread([z[k] for z in recs["dev"]])
    summary["dev"]["model_bytes_per_row"] = SCAN_BYTES
    summary["dev"]["model_gbs"] = med_spread([z["model_gbs"] for z in recs["dev"] if z["model_gbs"] is not None] or [0])
    med = {r: summary[r]["total_ms"]["median"] for r in ROUTES}
    summary["torch_over_range"] = round(med["torch_sum"] / med["range_sum"], 3)
    summary["search_ms"] = round(med["range_sum"] - med["rows_sum"], 4)
    across = [med[f"max_w{w}"] for w in WIDTHS]
    summary["max_spread"] = round((max(across) - min(across)) / min(across), 3) if across else None
    emit(summary)
    del part, order, x, out_dev
    torch.cuda.empty_cache()
eng.close()
sink.close()
