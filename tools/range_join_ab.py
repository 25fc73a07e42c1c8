#!/usr/bin/env python3
"""tools/range_join_ab.py -- the range join entry next to the route a torch caller had before it, on the same int64 tensors, alternating:
  (a) pairs         Engine.range_join_columns(lo_R, hi_R, on_S, by_R, by_S): the ordered index pairs -- one csr call, one
                    rhj_range_expand_dev, one rhj_pairs_split
  (b) csr           Engine.range_join_csr_columns(..) alone: offsets, first and rows_S, no pair is written -- next to (a) it shows the
                    share of the expansion
  (c) torch         the same pairs without the entry: torch.sort(stable) of S's order values, two torch.searchsorted, a cumsum and a
                    torch.repeat_interleave expansion; with `by` the group ids of Engine.factorize_columns and the order value go
                    into one composite key first (id << 40 | value: the order values here have at most 40 bits -- the route's limit)
at 10^6, 10^7 and 10^8 rows per side (--rows), for one partition (no `by`), about n / 100 uniform partitions and Zipf(0.9) over as
many (--shapes: one,uniform,zipf).  The intervals hold about 4 rows of S on average.

After --warmup runs of each route they are timed alternately for --steps steps.  One JSON line per step and route on stdout
(total_ms: a torch.cuda.Event pair around the whole route, allocations inside; wall_ms: host clock, synchronised at both ends).
Checked at every case: (a) equals (c) pair for pair and in order, (b)'s total is theirs.  A summary line (medians, min, max, the ratio
torch / pairs, "slower" where it is below 1, and the share of the csr call in the pair route) closes each case; the summary lines,
and only they, are also APPENDED to --out, so that a run over some of the sizes adds to the table instead of replacing it."""
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
ap.add_argument("--shapes", default="one,uniform,zipf")
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_range_join_ab.jsonl"))
a = ap.parse_args()
sink = open(a.out, "a")
ROUTES = ("pairs", "csr", "torch")
SPAN = 1 << 38                                                             # the order values: 38 bits, so value + width fits 40
PARTNERS = 4


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if rec.get("summary"):
        sink.write(line + "\n")
        sink.flush()


def med_spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def make_by(shape, n, groups, gen):
    """(the `by` words of 2n rows, the sum of the squared group probabilities) or (None, 1)"""
    if shape == "one":
        return None, 1.0
    if shape == "uniform":
        ids, p2 = torch.randint(0, groups, (2 * n,), device="cuda", dtype=torch.int64, generator=gen), 1.0 / groups
    elif shape == "zipf":                                                  # inverse CDF of p(i) ~ (i + 1)^-0.9 over the groups
        p = torch.arange(1, groups + 1, device="cuda", dtype=torch.float64) ** -0.9
        p = p / p.sum()
        ids = torch.searchsorted(torch.cumsum(p, 0), torch.rand(2 * n, device="cuda", dtype=torch.float64, generator=gen)).clamp_(max=groups - 1)
        p2 = float((p * p).sum())
    else:
        raise ValueError(shape)
    return (ids * -7046029254386353131 - (1 << 62)).contiguous(), p2      # (0x9E3779B97F4A7C15 as int64, odd: a bijection)


def torch_route(eng, lo_R, hi_R, on_S, by_R, by_S):
    nR, nS = lo_R.numel(), on_S.numel()
    if by_R is not None:
        codes, _ = eng.factorize_columns(torch.cat([by_S, by_R]))
        on_S, lo_R, hi_R = (codes[:nS] << 40) | on_S, (codes[nS:] << 40) | lo_R, (codes[nS:] << 40) | hi_R
    s, perm = torch.sort(on_S, stable=True)
    first = torch.searchsorted(s, lo_R, right=False)
    cnt = (torch.searchsorted(s, hi_R, right=True) - first).clamp_(min=0)
    ends = torch.cumsum(cnt, 0)
    idx_R = torch.repeat_interleave(torch.arange(nR, device=s.device, dtype=torch.int64), cnt)
    at = torch.arange(idx_R.numel(), device=s.device, dtype=torch.int64) - (ends - cnt)[idx_R] + first[idx_R]
    return idx_R, perm[at]


eng = rhj.Engine(0)
gen = torch.Generator(device="cuda")
gen.manual_seed(26)
cases = [(int(r), s) for r in a.rows.split(",") if r for s in a.shapes.split(",") if s]
for n, shape in cases:
    groups = max(n // 100, 1)
    by, p2 = make_by(shape, n, groups, gen)
    by_R, by_S = (None, None) if by is None else (by[:n].contiguous(), by[n:].contiguous())
    del by
    width = max(min(int(PARTNERS * SPAN / (n * p2)), SPAN), 1)            # E[partners] = nS * sum p^2 * width / SPAN
    on_S = torch.randint(0, SPAN, (n,), device="cuda", dtype=torch.int64, generator=gen)
    lo_R = torch.randint(0, SPAN, (n,), device="cuda", dtype=torch.int64, generator=gen)
    hi_R = lo_R + width
    last = {}

    def run(route, step, timed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        if route == "pairs":
            res = eng.range_join_columns(lo_R, hi_R, on_S, by_R, by_S)
            total = res[0].numel()
        elif route == "csr":
            res = eng.range_join_csr_columns(lo_R, hi_R, on_S, by_R, by_S)
            total = res[3]
        else:
            res = torch_route(eng, lo_R, hi_R, on_S, by_R, by_S)
            total = res[0].numel()
        ev[1].record()
        torch.cuda.synchronize()
        last[route] = res if not timed else None
        del res
        t1 = time.perf_counter()
        rec = {"rows_per_side": n, "shape": shape, "route": route, "step": step if timed else -1, "pairs": total,
               "total_ms": round(ev[0].elapsed_time(ev[1]), 4), "wall_ms": round((t1 - t0) * 1e3, 4)}
        emit(rec)
        return rec

    for s in range(max(a.warmup, 1)):                                       # (the last warm-up's results are the ones checked)
        for route in ROUTES:
            run(route, s, False)
    assert torch.equal(last["pairs"][0], last["torch"][0]) and torch.equal(last["pairs"][1], last["torch"][1])
    assert last["csr"][3] == last["pairs"][0].numel()
    last.clear()
    torch.cuda.empty_cache()
    recs = {r: [] for r in ROUTES}
    for s in range(a.steps):
        for route in ROUTES:
            recs[route].append(run(route, s, True))
    summary = {"rows_per_side": n, "shape": shape, "groups": groups if shape != "one" else 1, "width": width, "steps": a.steps,
               "total_pairs": recs["pairs"][-1]["pairs"], "summary": True}
    for route in ROUTES:
        y = recs[route]
        summary[route] = {"total_ms": med_spread([z["total_ms"] for z in y]), "wall_ms": med_spread([z["wall_ms"] for z in y])}
    summary["torch_over_pairs"] = round(summary["torch"]["total_ms"]["median"] / summary["pairs"]["total_ms"]["median"], 3)
    summary["csr_share"] = round(summary["csr"]["total_ms"]["median"] / summary["pairs"]["total_ms"]["median"], 3)
    summary["verdict"] = "faster" if summary["torch_over_pairs"] >= 1 else "**slower**"
    emit(summary)
    del on_S, lo_R, hi_R, by_R, by_S
    torch.cuda.empty_cache()
eng.close()
sink.close()
