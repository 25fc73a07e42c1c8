"""The window entry's oracle and case generators (numpy only; shares nothing with the product).

Oracle: a stable np.lexsort((arange, t(order), part)) -- t the sort oracle's view transform: the sign bit flipped for the int64
order, the complement for descending, so ties keep their input order in both directions -- then segment arithmetic on the sorted
positions: heads where the sorted partition word changes, peer heads where the order word changes too; the two starts as running
maxima of head positions; CUMSUM as a wrapped uint64 cumsum minus the segment base; minimum and maximum per segment by doubling
steps that never reach across a segment start.  Results go back to the rows through the permutation."""
import numpy as np

SORT_I64, SORT_DESC = 1, 2                    # include/rhj.h RHJ_SORT_*
FLAGS = (0, SORT_I64, SORT_DESC, SORT_I64 | SORT_DESC)
ROW_NUMBER, RANK, DENSE_RANK, LAG_ROW, LEAD_ROW, CUMSUM, CUMMIN_U64, CUMMAX_U64, CUMMIN_I64, CUMMAX_I64 = range(10)   # RHJ_WIN_*
MAX_OPS = 4
BIAS = np.uint64(1 << 63)
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
NO_ROW = ONES
GUARD = np.uint64(0xDEADBEEFCAFEF00D)
NGUARD = 16
SPECIAL = np.array([0, (1 << 64) - 1, 1 << 63], dtype=np.uint64)      # words every partition column holds


def transform(order, flags):
    """the uint64 word whose ascending unsigned order is the order asked for"""
    t = np.asarray(order, dtype=np.uint64)
    if flags & SORT_I64:
        t = t ^ BIAS
    if flags & SORT_DESC:
        t = ~t
    return t


def _seg_extreme(v, pos, pstart, take):
    """running minimum / maximum (take: np.minimum / np.maximum) of v inside segments: after the step of distance d every position
    holds the extreme over the 2d positions ending at it, cut at its segment's start"""
    v = v.copy()
    longest = int((pos - pstart).max()) + 1 if len(v) else 0
    d = 1
    while d < longest:
        reach = np.nonzero(pos - pstart >= d)[0]
        v[reach] = take(v[reach], v[reach - d])
        d *= 2
    return v


def oracle(part, order, flags, ops, args=None, cols=None, n=None):
    """(outs, partitions): outs[j] the uint64 array the entry must write for ops[j], aligned with the rows (n: the number of rows,
    needed only where no column says it)"""
    if n is None:
        n = len(next(c for c in [part, order] + list(cols or ()) if c is not None))
    idx = np.arange(n, dtype=np.int64)
    pk = np.asarray(part, dtype=np.uint64) if part is not None else np.zeros(n, dtype=np.uint64)
    ok = transform(order, flags) if order is not None else np.zeros(n, dtype=np.uint64)
    perm = np.lexsort((idx, ok, pk))
    sp, so = pk[perm], ok[perm]
    head = np.ones(n, dtype=bool)
    head[1:] = sp[1:] != sp[:-1]
    peer = np.ones(n, dtype=bool)
    if order is not None:
        peer[1:] = head[1:] | (so[1:] != so[:-1])
    pos = np.arange(n, dtype=np.int64)
    pstart = np.maximum.accumulate(np.where(head, pos, 0)) if n else pos
    qstart = np.maximum.accumulate(np.where(peer, pos, 0)) if n else pos
    heads = np.nonzero(head)[0]
    pend = np.append(heads[1:], n)[np.cumsum(head) - 1] if n else pos     # one past the last position of the partition
    outs = []
    for j, op in enumerate(ops):
        off = 1 if args is None else min(int(args[j]), n + 1)              # (an offset beyond n finds no row, whatever it is)
        if op == ROW_NUMBER:
            res = (pos - pstart + 1).astype(np.uint64)
        elif op == RANK:
            res = (qstart - pstart + 1).astype(np.uint64)
        elif op == DENSE_RANK:
            c = np.cumsum(peer)
            res = (c - c[pstart] + 1).astype(np.uint64) if n else c.astype(np.uint64)
        elif op == LAG_ROW:
            there = pos - pstart >= off
            res = np.full(n, NO_ROW, dtype=np.uint64)
            res[there] = perm[pos[there] - off]
        elif op == LEAD_ROW:
            there = pend - pos > off
            res = np.full(n, NO_ROW, dtype=np.uint64)
            res[there] = perm[pos[there] + off]
        else:
            v = np.asarray(cols[j], dtype=np.uint64)[perm]
            if op == CUMSUM:
                c = np.cumsum(v, dtype=np.uint64)                          # wraps mod 2^64
                res = c - (c[pstart] - v[pstart]) if n else c
            else:
                bias = BIAS if op in (CUMMIN_I64, CUMMAX_I64) else np.uint64(0)
                take = np.minimum if op in (CUMMIN_U64, CUMMIN_I64) else np.maximum
                res = _seg_extreme(v ^ bias, pos, pstart, take) ^ bias
        out = np.empty(n, dtype=np.uint64)
        out[perm] = res
        outs.append(out)
    return outs, int(head.sum()) if n else 0


# ---- generators ----------------------------------------------------------------------------------------------------------------------
SHAPES = ("one", "each", "runs64", "runsT", "runsT-1", "runsT+1", "edges", "geometric", "zipf")
ORDERS = ("none", "constant", "sixteen", "distinct", "extremes")
VALUES = ("full64", "extremes", "constant")


def _words(m, rng):
    """m distinct uint64 words in ascending order that include 0, all ones and 1 << 63 (as many of them as m allows)"""
    w = SPECIAL[:min(m, 3)]
    while len(w) < m:
        w = np.unique(np.concatenate([w, rng.integers(0, 1 << 64, m - len(w), dtype=np.uint64)]))
    return np.sort(w)


def part_sizes(shape, n, T):
    """the partition sizes in SORTED order of their words (zipf: None, its sizes are drawn)"""
    if n == 0:
        return []
    if shape == "one":
        return [n]
    if shape == "each":
        return [1] * n
    if shape in ("runs64", "runsT", "runsT-1", "runsT+1"):
        run = {"runs64": 64, "runsT": T, "runsT-1": T - 1, "runsT+1": T + 1}[shape]
        return [run] * (n // run) + ([n % run] if n % run else [])
    if shape == "edges":                      # a one-row partition at the first and at the last sorted position
        if n < 3:
            return [1] * n
        mid = n - 2
        return [1] + [s for s in (mid // 2, mid - mid // 2) if s] + [1]
    if shape == "geometric":
        sizes, s = [], 1
        while sum(sizes) + s <= n:
            sizes.append(s)
            s *= 2
        if sum(sizes) < n:
            sizes.append(n - sum(sizes))
        return sizes
    raise ValueError(shape)


def make_part(shape, n, T, seed=0, groups=None):
    """the partition column: n uint64 words, shuffled -- the rows of a partition lie anywhere in the input"""
    rng = np.random.default_rng(7000 * (SHAPES.index(shape) + 1) + n % 991 + seed)
    if shape == "zipf":
        m = max(1, min(n, groups if groups else max(n // 100, 3)))
        w = _words(m, rng)
        p = 1.0 / np.arange(1, m + 1) ** 0.9
        return rng.permutation(w)[rng.choice(m, n, p=p / p.sum())] if n else np.zeros(0, dtype=np.uint64)
    sizes = part_sizes(shape, n, T)
    col = np.repeat(_words(len(sizes), rng), sizes) if n else np.zeros(0, dtype=np.uint64)
    return col[rng.permutation(n)]


def make_order(kind, n, seed=0):
    """the order column, or None"""
    rng = np.random.default_rng(9000 * (ORDERS.index(kind) + 1) + n % 983 + seed)
    if kind == "none":
        return None
    if kind == "constant":                    # one run of peers per partition: rank and dense rank are all 1
        return np.full(n, 0xFEDCBA9876543210, dtype=np.uint64)
    if kind == "sixteen":                     # long peer runs
        return rng.integers(0, 1 << 64, 16, dtype=np.uint64)[rng.integers(0, 16, n)]
    if kind == "distinct":
        return (rng.permutation(n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) if n else np.zeros(0, dtype=np.uint64)   # an odd multiplier: a bijection mod 2^64
    if kind == "extremes":                    # the extremes of both views and their neighbours, with ties
        special = np.array([0, 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 2, (1 << 64) - 1], dtype=np.uint64)
        return special[rng.integers(0, len(special), n)]
    raise ValueError(kind)


def make_values(kind, n, seed=0):
    rng = np.random.default_rng(11000 * (VALUES.index(kind) + 1) + n % 977 + seed)
    if kind == "full64":                      # the running sum wraps
        return rng.integers(0, 1 << 64, n, dtype=np.uint64)
    if kind == "extremes":
        special = np.array([0, 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 2, (1 << 64) - 1], dtype=np.uint64)
        v = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        where = rng.random(n) < 0.3
        v[where] = special[rng.integers(0, len(special), int(where.sum()))]
        return v
    if kind == "constant":
        return np.full(n, 0x8000000000000001, dtype=np.uint64)
    raise ValueError(kind)
