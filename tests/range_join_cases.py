"""The range join entries' oracles and case generators (numpy only; shares nothing with the product).

oracle: the rows of S in a stable lexsort by (by word, on in the view, index) -- that IS rowsS --, and per distinct `by` word of R two
np.searchsorted of the rows' bounds in that partition's slice of it: side "left" for a closed lower end ("right" for an open one),
side "right" for a closed upper end ("left" for an open one).  The band form's bounds are computed in the view with saturation first.
brute: O(nR * nS) in plain Python ints, for tables of at most ~200 rows: every pair is tested against the contract's sentences, the
saturating band arithmetic and the open ends included; the pairs are ordered by (row of R, on in the view, row of S)."""
import numpy as np

import window_cases as WC

RANGE_I64, RANGE_LO_OPEN, RANGE_HI_OPEN, RANGE_BAND = 1, 2, 4, 8          # include/rhj.h RHJ_RANGE_*
FLAGS16 = tuple(range(16))
BIAS = np.uint64(1 << 63)
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
GUARD, NGUARD = WC.GUARD, WC.NGUARD
SHAPES = WC.SHAPES
ONS = ("distinct", "sixteen", "constant", "extremes")
DISTANCES = (0, 1, 1 << 63, (1 << 64) - 1)


def view(on, flags):
    """the uint64 word whose ascending unsigned order is the view's order"""
    t = np.asarray(on, dtype=np.uint64)
    return t ^ BIAS if flags & RANGE_I64 else t


def bounds(loR, hiR, flags, below=0, above=0):
    """(lo, hi) of every row of R as view words; under RANGE_BAND loR holds x and the ends saturate at 0 and all ones of the view"""
    x = view(loR, flags)
    if not flags & RANGE_BAND:
        return x, view(hiR, flags)
    below, above = np.uint64(below), np.uint64(above)
    lo = np.where(x >= below, x - below, np.uint64(0))
    hi = np.where(above > ~x, ONES, x + above)
    return lo.astype(np.uint64), hi.astype(np.uint64)


def oracle(byR, loR, hiR, byS, onS, flags, below=0, above=0):
    """(offsets, first, defined, rowsS, pairs): offsets uint64[nR + 1], first uint64[nR] with defined the mask of the rows where it
    says something (cnt > 0), rowsS uint64[nS], pairs uint64[total, 2] in the contract's order; byR and byS both None: one partition"""
    nR, nS = len(loR), len(onS)
    bR = np.asarray(byR, dtype=np.uint64) if byR is not None else np.zeros(nR, dtype=np.uint64)
    bS = np.asarray(byS, dtype=np.uint64) if byS is not None else np.zeros(nS, dtype=np.uint64)
    tS = view(onS, flags)
    rowsS = np.lexsort((np.arange(nS), tS, bS)).astype(np.uint64)
    first, cnt = np.zeros(nR, dtype=np.uint64), np.zeros(nR, dtype=np.int64)
    if nR and nS:
        lo, hi = bounds(loR, hiR, flags, below, above)
        sb, st = bS[rowsS.astype(np.int64)], tS[rowsS.astype(np.int64)]
        words, starts, counts = np.unique(sb, return_index=True, return_counts=True)
        orderR = np.argsort(bR, kind="stable")
        wR, startR, countR = np.unique(bR[orderR], return_index=True, return_counts=True)
        at = np.searchsorted(words, wR)
        for g in range(len(wR)):
            k = at[g]
            if k >= len(words) or words[k] != wR[g]:
                continue                                                   # a partition without S
            r = orderR[startR[g]:startR[g] + countR[g]]
            ts = st[starts[k]:starts[k] + counts[k]]
            a = np.searchsorted(ts, lo[r], side="right" if flags & RANGE_LO_OPEN else "left")
            b = np.searchsorted(ts, hi[r], side="left" if flags & RANGE_HI_OPEN else "right")
            first[r] = (starts[k] + a).astype(np.uint64)
            cnt[r] = np.maximum(b - a, 0)
    offsets = np.zeros(nR + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(cnt).astype(np.uint64)
    total = int(offsets[-1])
    rows = np.repeat(np.arange(nR, dtype=np.int64), cnt)
    at = np.arange(total, dtype=np.int64) - offsets[:-1].astype(np.int64)[rows] + first.astype(np.int64)[rows]
    pairs = np.stack([rows.astype(np.uint64), rowsS[at]], axis=1) if total else np.zeros((0, 2), dtype=np.uint64)
    return offsets, first, cnt > 0, rowsS, pairs


def brute(byR, loR, hiR, byS, onS, flags, below=0, above=0):
    """the ordered pairs from the contract's sentences, in Python ints: uint64[total, 2]"""
    signed = bool(flags & RANGE_I64)
    vmin, vmax = (-(1 << 63), (1 << 63) - 1) if signed else (0, (1 << 64) - 1)

    def val(w):
        w = int(w)
        return w - (1 << 64) if signed and w >= 1 << 63 else w
    out = []
    for i in range(len(loR)):
        if flags & RANGE_BAND:
            x = val(loR[i])
            lo, hi = max(x - below, vmin), min(x + above, vmax)
        else:
            lo, hi = val(loR[i]), val(hiR[i])
        mine = []
        for j in range(len(onS)):
            if byR is not None and int(byR[i]) != int(byS[j]):
                continue
            y = val(onS[j])
            if (y > lo if flags & RANGE_LO_OPEN else y >= lo) and (y < hi if flags & RANGE_HI_OPEN else y <= hi):
                mine.append((y, j))
        out += [(i, j) for _, j in sorted(mine)]
    return np.array(out, dtype=np.uint64).reshape(-1, 2)


# ---- generators ----------------------------------------------------------------------------------------------------------------------
def make_tables(shape, kind, nR, nS, T, seed=0, groups=None, by=True, flags=0, reach=8):
    """(byR, loR, hiR, byS, onS): window_cases' partition shape and order kind over the nR + nS rows of both tables, the first nR of
    them R's (the generators shuffle, so either table holds rows of every partition, anywhere).  A row's lower bound is its order
    word; its upper bound is the word 0 .. reach places further in the view's order of ALL words -- so an interval holds a handful
    of rows of S whatever the words are, and often ends on a word that S holds --, and for every eighth row the word before its lower
    bound: an empty interval.  by=False: no `by` columns"""
    n = nR + nS
    on = WC.make_order(kind, n, seed)
    rng = np.random.default_rng(13000 + 31 * n + seed)
    allv = np.sort(view(on, flags))
    lo = on[:nR].copy()
    lv = view(lo, flags)
    at = np.searchsorted(allv, lv, side="right") - 1 + rng.integers(0, reach + 1, nR)
    hv = allv[np.minimum(at, n - 1)] if n else lv
    empty = (rng.integers(0, 8, nR) == 0) & (lv > 0)
    hv = np.where(empty, lv - np.uint64(1), hv).astype(np.uint64)
    hi = view(hv, flags)                                                   # (the transform is its own inverse)
    if not by:
        return None, lo, hi, None, on[nR:].copy()
    part = WC.make_part(shape, n, T, seed, groups)
    return part[:nR].copy(), lo, hi, part[nR:].copy(), on[nR:].copy()


def splits(n):
    """(nR, nS) for a total of n rows: roughly half, one row of S, one row of R, no S, no R"""
    out = [(n - n // 2, n // 2), (n - 1, 1), (1, n - 1), (n, 0), (0, n)]
    return [s for i, s in enumerate(out) if s[0] >= 0 and s[1] >= 0 and s not in out[:i]]
