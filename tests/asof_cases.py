"""The as-of join entry's oracles and case generators (numpy only; shares nothing with the product).

oracle: per distinct `by` word the rows of S in a stable lexsort by (on in the view, index), np.searchsorted of the R rows' `on` words
in it -- side "right" for backward (strict: "left") and the entry before the insertion point, side "left" for forward (strict:
"right") and the entry at it.  Because the index is the second sort key, the entry before an insertion point is the LAST index of its
duplicate run and the entry at one the FIRST: the step to the end of the run is the lexsort's.  The tolerance is compared as a
difference of the view-transformed words, larger minus smaller, which is exact in uint64.
brute: O(nR * nS) in plain Python ints, for tables of at most ~200 rows: every candidate is tested against the contract's sentences."""
import numpy as np

import window_cases as WC

ASOF_I64, ASOF_FORWARD, ASOF_STRICT, ASOF_TOLERANCE = 1, 2, 4, 8          # include/rhj.h RHJ_ASOF_*
FLAGS8 = tuple(range(8))                                                  # every combination of view, direction and strictness
BIAS = np.uint64(1 << 63)
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
NO_ROW = ONES
GUARD, NGUARD = WC.GUARD, WC.NGUARD
SHAPES = WC.SHAPES
ONS = ("distinct", "sixteen", "constant", "extremes")


def view(on, flags):
    """the uint64 word whose ascending unsigned order is the view's order"""
    t = np.asarray(on, dtype=np.uint64)
    return t ^ BIAS if flags & ASOF_I64 else t


def oracle(byR, onR, byS, onS, flags, tolerance=0):
    """(rows, matched): rows the uint64 array the entry must write, aligned with R; byR and byS both None: one partition"""
    nR, nS = len(onR), len(onS)
    rows = np.full(nR, NO_ROW, dtype=np.uint64)
    if nR == 0 or nS == 0:
        return rows, 0
    bR = np.asarray(byR, dtype=np.uint64) if byR is not None else np.zeros(nR, dtype=np.uint64)
    bS = np.asarray(byS, dtype=np.uint64) if byS is not None else np.zeros(nS, dtype=np.uint64)
    tR, tS = view(onR, flags), view(onS, flags)
    forward, strict = bool(flags & ASOF_FORWARD), bool(flags & ASOF_STRICT)
    orderS = np.lexsort((np.arange(nS), tS, bS))                           # by partition, then (on, index)
    wS, startS, countS = np.unique(bS[orderS], return_index=True, return_counts=True)
    orderR = np.argsort(bR, kind="stable")
    wR, startR, countR = np.unique(bR[orderR], return_index=True, return_counts=True)
    at = np.searchsorted(wS, wR)
    for g in range(len(wR)):
        if at[g] >= len(wS) or wS[at[g]] != wR[g]:
            continue                                                       # a partition without S
        r = orderR[startR[g]:startR[g] + countR[g]]
        s = orderS[startS[at[g]]:startS[at[g]] + countS[at[g]]]
        ts = tS[s]
        if forward:
            k = np.searchsorted(ts, tR[r], side="right" if strict else "left")
            ok = k < len(s)
        else:
            k = np.searchsorted(ts, tR[r], side="left" if strict else "right") - 1
            ok = k >= 0
        k = np.where(ok, k, 0)
        if flags & ASOF_TOLERANCE:
            a, b = tR[r], ts[k]
            ok &= np.where(a > b, a - b, b - a) <= np.uint64(tolerance)
        rows[r[ok]] = s[k[ok]].astype(np.uint64)
    return rows, int((rows != NO_ROW).sum())


def brute(byR, onR, byS, onS, flags, tolerance=0):
    """the same from the contract's sentences, in Python ints"""
    def val(w):
        w = int(w)
        return w - (1 << 64) if flags & ASOF_I64 and w >= 1 << 63 else w
    forward, strict = bool(flags & ASOF_FORWARD), bool(flags & ASOF_STRICT)
    rows = []
    for i in range(len(onR)):
        x, best = val(onR[i]), None
        for j in range(len(onS)):
            if byR is not None and int(byR[i]) != int(byS[j]):
                continue
            y = val(onS[j])
            if forward:
                cand = y > x if strict else y >= x
            else:
                cand = y < x if strict else y <= x
            if not cand or (flags & ASOF_TOLERANCE and abs(x - y) > tolerance):
                continue
            if best is None:
                best = (y, j)
            elif forward:
                best = min(best, (y, j))                                   # the smallest on, then the smallest index
            else:
                best = max(best, (y, j))                                   # the largest on, then the largest index
        rows.append(int(NO_ROW) if best is None else best[1])
    rows = np.array(rows, dtype=np.uint64)
    return rows, int((rows != NO_ROW).sum())


# ---- generators ----------------------------------------------------------------------------------------------------------------------
def make_on(kind, n, seed=0):
    """the `on` words of the n rows of both tables together: `distinct` has no exact match, the others many"""
    return WC.make_order(kind, n, seed)


def make_tables(shape, kind, nR, nS, T, seed=0, groups=None, by=True):
    """(byR, onR, byS, onS): window_cases' partition shape and `on` kind over the nR + nS rows of both tables, the first nR of them R's
    (the generators shuffle, so either table holds rows of every partition, anywhere); by=False: no `by` columns"""
    n = nR + nS
    on = make_on(kind, n, seed)
    if not by:
        return None, on[:nR].copy(), None, on[nR:].copy()
    part = WC.make_part(shape, n, T, seed, groups)
    return part[:nR].copy(), on[:nR].copy(), part[nR:].copy(), on[nR:].copy()


def splits(n):
    """(nR, nS) for a total of n rows: roughly half, one row of S, one row of R, no S, no R"""
    out = [(n - n // 2, n // 2), (n - 1, 1), (1, n - 1), (n, 0), (0, n)]
    return [s for i, s in enumerate(out) if s[0] >= 0 and s[1] >= 0 and s not in out[:i]]
