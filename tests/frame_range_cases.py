"""The RANGE frame entry's oracles and case helpers (numpy only; they share nothing with the product, and neither oracle uses blocks
or a sparse table).  The order and the generators are tests/frame_cases.py's.

With v the order word in the transformed view (frame_cases.transform: unsigned, non-decreasing along a partition in all four views)
the frame of a row is the rows r of its partition with max(0, v - preceding) <= v_r <= min(2^64 - 1, v + following) -- in both
directions, PRECEDING being "earlier in the order".
Oracle one, `brute`, is deliberately naive: per partition and per row the two saturated bounds are computed in Python integers, the
rows between them are selected by comparing every word of the partition with them, and the slice is reduced with numpy.
Oracle two, `fast`, finds the two positions with np.searchsorted (left / right) per partition on the transformed words, the bounds
saturated in uint64 arithmetic; COUNT, FIRST_ROW and LAST_ROW come from the positions, SUM from cumulative sums, MIN / MAX from
np.minimum.reduceat / np.maximum.reduceat over the (lo, hi + 1) pairs."""
import numpy as np

import frame_cases as FC

SORT_I64, SORT_DESC, FLAGS = FC.SORT_I64, FC.SORT_DESC, FC.FLAGS
COUNT, SUM, MIN_U64, MAX_U64, MIN_I64, MAX_I64, FIRST_ROW, LAST_ROW = range(8)
EXTREMES = FC.EXTREMES
UNBOUNDED = FC.UNBOUNDED
TOP = (1 << 64) - 1
BLOCK = 64                                    # only `paths` and `levels` below know it: they describe what a case exercises


def _bound(side, j, default):
    return default if side is None else int(side[j])


def brute(part, order, flags, ops, preceding=None, following=None, cols=None):
    """oracle one -- (outs, partitions): outs[j] the uint64 array the entry must write for ops[j], aligned with the rows"""
    n = len(order)
    perm, starts = FC.sorted_order(part, order, flags, n)
    v = FC.transform(order, flags)[perm]
    outs, frames = [], {}
    for j, op in enumerate(ops):
        pre, fol = _bound(preceding, j, UNBOUNDED), _bound(following, j, 0)
        if (pre, fol) not in frames:                                        # the selection once per distinct frame of the call
            ends = []
            for a, b in zip(starts[:-1].tolist(), starts[1:].tolist()):
                vv = v[a:b]
                for q in range(b - a):
                    t = int(vv[q])
                    low, high = max(0, t - pre), min(TOP, t + fol)          # Python integers: nothing wraps
                    inside = np.nonzero((vv >= np.uint64(low)) & (vv <= np.uint64(high)))[0]
                    assert int(inside[-1]) - int(inside[0]) + 1 == len(inside)   # a contiguous run of sorted positions
                    ends.append((a + int(inside[0]), a + int(inside[-1])))
            frames[(pre, fol)] = ends
        col = np.asarray(cols[j], dtype=np.uint64)[perm] if op in (SUM,) + EXTREMES else None
        res = np.empty(n, dtype=np.uint64)
        for p, (lo, hi) in enumerate(frames[(pre, fol)]):
            if op == COUNT:
                res[p] = hi - lo + 1
            elif op == FIRST_ROW:
                res[p] = perm[lo]
            elif op == LAST_ROW:
                res[p] = perm[hi]
            else:
                res[p] = FC._reduce(op, col[lo:hi + 1])
        out = np.empty(n, dtype=np.uint64)
        out[perm] = res
        outs.append(out)
    return outs, len(starts) - 1 if n else 0


def positions(part, order, flags, pre, fol, sorted_=None):
    """(perm, ps, pe, lo, hi) by sorted position, int64, all inclusive: the partition's and the frame's first and last position
    (sorted_: the (perm, starts) of frame_cases.sorted_order, where the caller has them)"""
    n = len(order)
    perm, starts = sorted_ if sorted_ is not None else FC.sorted_order(part, order, flags, n)
    v = FC.transform(order, flags)[perm]
    pre, fol = np.uint64(pre), np.uint64(fol)
    with np.errstate(over="ignore"):
        low = np.where(v >= pre, v - pre, np.uint64(0))
        high = np.where(v > np.uint64(TOP) - fol, np.uint64(TOP), v + fol)
    lo, hi = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    for a, b in zip(starts[:-1].tolist(), starts[1:].tolist()):
        lo[a:b] = a + np.searchsorted(v[a:b], low[a:b], side="left")
        hi[a:b] = a + np.searchsorted(v[a:b], high[a:b], side="right") - 1
    sizes = np.diff(starts)
    ps = np.repeat(starts[:-1], sizes).astype(np.int64)
    pe = np.repeat(starts[1:] - 1, sizes).astype(np.int64)
    return perm, ps, pe, lo, hi


def fast(part, order, flags, ops, preceding=None, following=None, cols=None):
    """oracle two -- (outs, partitions)"""
    n = len(order)
    sorted_ = FC.sorted_order(part, order, flags, n)
    outs, frames = [], {}
    for j, op in enumerate(ops):
        pre, fol = _bound(preceding, j, UNBOUNDED), _bound(following, j, 0)
        if (pre, fol) not in frames:
            frames[(pre, fol)] = positions(part, order, flags, pre, fol, sorted_)
        perm, ps, pe, lo, hi = frames[(pre, fol)]
        if op == COUNT:
            res = (hi - lo + 1).astype(np.uint64)
        elif op == FIRST_ROW:
            res = perm[lo].astype(np.uint64)
        elif op == LAST_ROW:
            res = perm[hi].astype(np.uint64)
        else:
            col = np.asarray(cols[j], dtype=np.uint64)[perm]
            if op == SUM:
                c = np.cumsum(col, dtype=np.uint64)                         # wraps mod 2^64
                res = c[hi] - c[lo] + col[lo]
            else:
                x = col.view(np.int64) if op in (MIN_I64, MAX_I64) else col
                pairs = np.empty(2 * n, dtype=np.int64)
                pairs[0::2], pairs[1::2] = lo, hi + 1
                take = np.minimum if op in (MIN_U64, MIN_I64) else np.maximum
                res = take.reduceat(np.append(x, x[-1:]), pairs)[0::2].view(np.uint64)   # (one more word: hi + 1 may be n)
        out = np.empty(n, dtype=np.uint64)
        out[perm] = res
        outs.append(out)
    return outs, len(sorted_[1]) - 1 if n else 0


def value_scans(ops, preceding, following):
    """"last.frame_range_scans": 1 per SUM; per minimum / maximum 1 when a side is all ones, else 2; 0 for the other ops"""
    total = 0
    for j, op in enumerate(ops):
        pre, fol = _bound(preceding, j, UNBOUNDED), _bound(following, j, 0)
        if op == SUM:
            total += 1
        elif op in EXTREMES:
            total += 1 if UNBOUNDED in (pre, fol) else 2
    return total


def levels(n, ops, preceding, following):
    """"last.frame_range_levels": with a two-sided minimum / maximum in the call T_0 .. T_floor(log2 c), c = (n - 1) // 64 - 1 the most
    whole blocks that can lie strictly between a frame's two ends; 0 without such an op or with c < 1"""
    two_sided = any(op in EXTREMES and UNBOUNDED not in (_bound(preceding, j, UNBOUNDED), _bound(following, j, 0)) for j, op in enumerate(ops))
    c = (n - 1) // BLOCK - 1 if n else 0
    return c.bit_length() if two_sided and c >= 1 else 0


def paths(ps, pe, lo, hi):
    """which of the five answers of a two-sided minimum / maximum each position takes, from an oracle's positions: a dict of counts
    -- "start" (one block, from the block's or partition's start), "end" (one block, to its end, not from its start), "walk" (one block,
    neither), "neighbours" (two blocks side by side), and ("table", c) for c >= 1 whole blocks strictly between the two ends"""
    bl, bh = lo // BLOCK, hi // BLOCK
    same = bl == bh
    at_start = lo == np.maximum(bl * BLOCK, ps)
    at_end = hi == np.minimum(bl * BLOCK + BLOCK - 1, pe)
    out = {"start": int((same & at_start).sum()), "end": int((same & ~at_start & at_end).sum()),
           "walk": int((same & ~at_start & ~at_end).sum()), "neighbours": int((bh - bl == 1).sum())}
    inner = (bh - bl - 1)[bh - bl >= 2]
    for c, k in zip(*np.unique(inner, return_counts=True)):
        out[("table", int(c))] = int(k)
    return out


def rank_order(part, n, rng=None):
    """each row's 0-based rank inside its partition in input order (shuffled inside the partition when rng is given): distinct inside
    a partition, so RANGE (a, b) over it is ROWS (a, b)"""
    pk = np.asarray(part, dtype=np.uint64) if part is not None else np.zeros(n, dtype=np.uint64)
    idx = np.arange(n) if rng is None else rng.permutation(n)
    by = idx[np.argsort(pk[idx], kind="stable")]
    sp = pk[by]
    head = np.ones(n, dtype=bool)
    head[1:] = sp[1:] != sp[:-1]
    first = np.maximum.accumulate(np.where(head, np.arange(n), 0))
    out = np.empty(n, dtype=np.uint64)
    out[by] = (np.arange(n) - first).astype(np.uint64)
    return out


def make_order(kind, n, seed=0):
    if kind == "equal":
        return np.full(n, 1 << 63, dtype=np.uint64)
    if kind == "near":                        # small distances reach a few rows: values 0 .. about 3 n, some ties
        return np.random.default_rng(19000 + n % 991 + seed).integers(0, 3 * n + 1, n).astype(np.uint64)
    return FC.make_order(kind, n, seed)
