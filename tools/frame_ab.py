#!/usr/bin/env python3
"""tools/frame_ab.py -- the frame entry next to the routes a caller had before it, on the same int64 tensors, alternating:
  (a) sum_frame     Engine.frame_columns(part, order, [x], ["sum"], 10, 0): SUM(x) over the current row and the 10 before it
      sum_chain     the route of the parent: window_columns(part, order, [x, None], ["cumsum", "lag"], offsets=[1, 11]) -- the running
                    sum and the row 11 positions back --, a gather of the running sum through that row and a subtraction
  (b) max_w<w>      Engine.frame_columns(part, order, [x], ["max"], w - 1, 0) at w = 4, 64, 4096 and 10^5 (--widths): the claim to
                    confirm or refute is that the time does not depend on w; "max_spread" is (slowest - fastest) / fastest of the
                    medians across w
  (c) count_frame   Engine.frame_columns(part, None, (), ["count"], None, None): COUNT(*) OVER (PARTITION BY part)
      count_chain   group_by_columns_with_inverse(part) and counts[inverse]
  (d) dev           rhj_frame_cols_dev for MAX at w = 64 on a preallocated output under rhj_set_profiling: "scan_ms" the six launches
                    of its two value scans (the last six before the emit launch), "model_gbs" the bytes of the cost model for them
                    (2 x 42 per row) over scan_ms -- to be read against the copy rate of DESIGN 6
at 10^6, 10^7 and 10^8 rows (--rows) for ~n / 100 uniform partitions, Zipf(0.9) over as many, and one partition (--shapes); the order
column is full-range, the value column small enough that torch's int64 cumsum and the entry's sum mod 2^64 agree without a wrap.

Checked at every case, on the last warm-up's results: sum_frame equals sum_chain; count_frame equals count_chain; every max_w equals a
torch route of its own -- the rows ordered by sort_columns([ids, order]), then doubling steps max(M[p], M[p - d]) that never reach
across a partition start, and two overlapping power-of-two windows for a w that is no power of two; (d) equals max_w64.

After --warmup runs of each route they are timed alternately for --steps steps (total_ms: a torch.cuda.Event pair around the whole
route, allocations inside; (d): the sum of its launches).  One JSON line per step and route on stdout; a summary line (medians, min,
max, the ratios chain / frame) closes each case; the summary lines, and only they, also go to --out."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_frame_ab.jsonl"))
a = ap.parse_args()
sink = open(a.out, "w")
WIDTHS = [int(w) for w in a.widths.split(",") if w]
ROUTES = ["sum_frame", "sum_chain"] + [f"max_w{w}" for w in WIDTHS] + ["count_frame", "count_chain", "dev"]
SCAN_LAUNCHES, SCAN_BYTES, DEV_W = 6, 2 * 42, 64


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


def sum_chain(eng, part, order, x):
    running, back = eng.window_columns(part, order, [x, None], ["cumsum", "lag"], offsets=[1, 11])
    return running - torch.where(back >= 0, running[back.clamp(min=0)], torch.zeros_like(running))


def count_chain(eng, part):
    _, counts, _, inverse = eng.group_by_columns_with_inverse(part)
    return counts[inverse]


def sorted_view(eng, part, order, x):
    """(perm, xs, dist): the rows in (partition, order, input position) order, x in that order, and each position's distance from its
    partition's start -- from entries that were there before"""
    n = part.numel()
    inverse = eng.group_by_columns_with_inverse(part)[3]
    sorted_keys, perm, (xs,) = eng.sort_columns([inverse, order], values=[x])
    ids = sorted_keys[0]
    pos = torch.arange(n, device=part.device, dtype=torch.int64)
    head = torch.ones(n, device=part.device, dtype=torch.bool)
    head[1:] = ids[1:] != ids[:-1]
    start = torch.cummax(torch.where(head, pos, torch.zeros_like(pos)), 0).values
    return perm, xs, pos - start


def max_check(perm, xs, dist, w):
    """MAX(x) over the w positions ending at each, cut at the partition's start, back in row order"""
    n = xs.numel()
    k = 1
    m = xs.clone()
    while 2 * k <= w:                                                      # m: the maximum over the k positions ending here
        shifted = torch.cat([m[:k], m[:n - k]]) if k < n else m
        m = torch.where(dist >= k, torch.maximum(m, shifted), m)
        k *= 2
    if k < w:                                                              # w - k <= k: two windows of k cover one of w
        d = w - k
        shifted = torch.cat([m[:d], m[:n - d]]) if d < n else m
        m = torch.where(dist >= d, torch.maximum(m, shifted), m)
    out = torch.empty_like(m)
    out[perm] = m
    return out


eng = rhj.Engine(0)
gen = torch.Generator(device="cuda")
gen.manual_seed(24)
for n, shape in [(int(r), s) for r in a.rows.split(",") if r for s in a.shapes.split(",") if s]:
    part = make_part(shape, n, gen).contiguous()
    order = torch.randint(-(1 << 63), (1 << 63) - 1, (n,), device="cuda", dtype=torch.int64, generator=gen)
    x = torch.randint(-1000, 1000, (n,), device="cuda", dtype=torch.int64, generator=gen)
    out_dev = torch.empty(n, device="cuda", dtype=torch.int64)
    last = {}

    def run(route, step, timed):
        torch.cuda.synchronize()
        if route == "dev":
            eng.set_profiling(True)
            partitions = eng.frame_cols_dev(part, order, n, rhj.SORT_I64, [rhj.FRAME_MAX_I64], [DEV_W - 1], [0], [x], [out_dev])
            spans, units, scans = eng.launch_timings(), eng.info("last.frame_units"), eng.info("last.frame_scans")
            eng.set_profiling(False)                                        # (resets "last.*")
            assert scans * 3 == SCAN_LAUNCHES
            scan_ms = sum(ms for _, ms in spans[-1 - SCAN_LAUNCHES:-1])
            extra = {"total_ms": round(sum(ms for _, ms in spans), 4), "launches": len(spans), "scan_ms": round(scan_ms, 4),
                     "emit_ms": round(spans[-1][1], 4), "partitions": partitions, "units": units,
                     "model_gbs": round(SCAN_BYTES * n / (scan_ms * 1e6), 1) if scan_ms > 0 else None}
            res = out_dev.clone() if not timed else None
        else:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            if route == "sum_frame":
                res = eng.frame_columns(part, order, [x], ["sum"], 10, 0)[0]
            elif route == "sum_chain":
                res = sum_chain(eng, part, order, x)
            elif route == "count_frame":
                res = eng.frame_columns(part, None, (), ["count"], None, None)[0]
            elif route == "count_chain":
                res = count_chain(eng, part)
            else:
                res = eng.frame_columns(part, order, [x], ["max"], int(route[5:]) - 1, 0)[0]
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
    assert torch.equal(last["sum_frame"], last["sum_chain"]) and torch.equal(last["count_frame"], last["count_chain"])
    perm, xs, dist = sorted_view(eng, part, order, x)
    for w in WIDTHS:
        assert torch.equal(last[f"max_w{w}"], max_check(perm, xs, dist, w)), w
    if DEV_W in WIDTHS:
        assert torch.equal(last["dev"], last[f"max_w{DEV_W}"])
    del perm, xs, dist
    last.clear()
    torch.cuda.empty_cache()
    recs = {r: [] for r in ROUTES}
    for s in range(a.steps):
        for route in ROUTES:
            recs[route].append(run(route, s, True))
    summary = {"rows": n, "shape": shape, "steps": a.steps, "summary": True}
    for route in ROUTES:
        summary[route] = {"total_ms": med_spread([z["total_ms"] for z in recs[route]])}
    summary["dev"].update({k: recs["dev"][-1][k] for k in ("launches", "partitions", "units")})
    for k in ("scan_ms", "emit_ms"):
        summary["dev"][k] = med_spread([z[k] for z in recs["dev"]])
    summary["dev"]["model_bytes_per_row"] = SCAN_BYTES
    summary["dev"]["model_gbs"] = med_spread([z["model_gbs"] for z in recs["dev"] if z["model_gbs"] is not None] or [0])
    med = {r: summary[r]["total_ms"]["median"] for r in ROUTES}
    summary["sum_chain_over_frame"] = round(med["sum_chain"] / med["sum_frame"], 3)
    summary["count_chain_over_frame"] = round(med["count_chain"] / med["count_frame"], 3)
    across = [med[f"max_w{w}"] for w in WIDTHS]
    summary["max_spread"] = round((max(across) - min(across)) / min(across), 3)
    emit(summary)
    del part, order, x, out_dev
    torch.cuda.empty_cache()
eng.close()
sink.close()
