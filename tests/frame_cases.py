"""The frame entry's oracles and case generators (numpy only; they share nothing with the product, and neither uses the block
decomposition the product's sliding minimum and maximum rest on).

Order: a stable np.lexsort((arange, t(order), part)), t the sort oracle's view transform, so ties keep their input order in both
directions; partitions are runs of equal sorted partition words.
Oracle one, `brute`, is deliberately naive: per partition, per row, the frame [max(0, q - preceding), min(m - 1, q + following)] in
Python integers, sliced out of the partition's values and reduced with numpy.
Oracle two, `windows`, covers the minimum and maximum only: a bounded frame is gathered whole as one row of a (rows x width) matrix,
positions outside the partition replaced by the op's identity, and reduced along the row; an unbounded side is a running extreme
inside the partition (np.minimum.accumulate per partition), read at the frame's other end.
`sums` is SUM from cumulative sums: c[hi] - c[lo] + v[lo] mod 2^64."""
import numpy as np

SORT_I64, SORT_DESC = 1, 2                    # include/rhj.h RHJ_SORT_*
FLAGS = (0, SORT_I64, SORT_DESC, SORT_I64 | SORT_DESC)
COUNT, SUM, MIN_U64, MAX_U64, MIN_I64, MAX_I64, FIRST_ROW, LAST_ROW = range(8)   # RHJ_FRAME_*
MAX_OPS = 4
UNBOUNDED = (1 << 64) - 1                     # RHJ_FRAME_UNBOUNDED
BIAS = np.uint64(1 << 63)
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
GUARD = np.uint64(0xDEADBEEFCAFEF00D)
NGUARD = 16
EXTREME_WORDS = np.array([0, (1 << 64) - 1, 1 << 63, (1 << 63) - 1], dtype=np.uint64)   # the identities and extremes of both views
EXTREMES = (MIN_U64, MAX_U64, MIN_I64, MAX_I64)


def transform(order, flags):
    """the uint64 word whose ascending unsigned order is the order asked for"""
    t = np.asarray(order, dtype=np.uint64)
    if flags & SORT_I64:
        t = t ^ BIAS
    if flags & SORT_DESC:
        t = ~t
    return t


def sorted_order(part, order, flags, n):
    """(perm, starts): perm[p] the row at sorted position p; starts the first position of every partition, and n behind them"""
    idx = np.arange(n, dtype=np.int64)
    pk = np.asarray(part, dtype=np.uint64) if part is not None else np.zeros(n, dtype=np.uint64)
    ok = transform(order, flags) if order is not None else np.zeros(n, dtype=np.uint64)
    perm = np.lexsort((idx, ok, pk))
    sp = pk[perm]
    head = np.ones(n, dtype=bool)
    head[1:] = sp[1:] != sp[:-1]
    return perm, np.append(np.nonzero(head)[0], n)


def _rows(n, part, order, cols):
    if n is not None:
        return n
    return len(next(c for c in [part, order] + list(cols or ()) if c is not None))


def _bound(side, j, default):
    return default if side is None else int(side[j])


def _reduce(op, seg):
    if op == SUM:
        return np.add.reduce(seg, dtype=np.uint64)
    if op == MIN_U64:
        return seg.min()
    if op == MAX_U64:
        return seg.max()
    s = seg.view(np.int64)
    return np.int64(s.min() if op == MIN_I64 else s.max()).astype(np.uint64)


def brute(part, order, flags, ops, preceding=None, following=None, cols=None, n=None):
    """oracle one -- (outs, partitions): outs[j] the uint64 array the entry must write for ops[j], aligned with the rows"""
    n = _rows(n, part, order, cols)
    perm, starts = sorted_order(part, order, flags, n)
    outs = []
    for j, op in enumerate(ops):
        pre, fol = _bound(preceding, j, UNBOUNDED), _bound(following, j, 0)
        v = np.asarray(cols[j], dtype=np.uint64)[perm] if op in (SUM,) + EXTREMES else None
        res = np.empty(n, dtype=np.uint64)
        for a, b in zip(starts[:-1].tolist(), starts[1:].tolist()):
            m = b - a
            rows = perm[a:b]
            seg = v[a:b] if v is not None else None
            for q in range(m):
                lo, hi = max(0, q - pre), min(m - 1, q + fol)
                if op == COUNT:
                    res[a + q] = hi - lo + 1
                elif op == FIRST_ROW:
                    res[a + q] = rows[lo]
                elif op == LAST_ROW:
                    res[a + q] = rows[hi]
                else:
                    res[a + q] = _reduce(op, seg[lo:hi + 1])
        out = np.empty(n, dtype=np.uint64)
        out[perm] = res
        outs.append(out)
    return outs, len(starts) - 1 if n else 0


def _bounds(starts, n, pre, fol):
    """(pos, ps, pe, lo, hi) by sorted position, int64; pe inclusive"""
    pos = np.arange(n, dtype=np.int64)
    sizes = np.diff(starts)
    ps = np.repeat(starts[:-1], sizes).astype(np.int64)
    pe = np.repeat(starts[1:] - 1, sizes).astype(np.int64)
    lo = np.maximum(ps, pos - min(pre, n))
    hi = np.minimum(pe, pos + min(fol, n))
    return pos, ps, pe, lo, hi


def windows(part, order, flags, ops, preceding=None, following=None, cols=None, n=None, chunk_words=1 << 22):
    """oracle two -- the outputs of the minimum / maximum ops (None in the place of any other op)"""
    n = _rows(n, part, order, cols)
    perm, starts = sorted_order(part, order, flags, n)
    outs = []
    for j, op in enumerate(ops):
        if op not in EXTREMES:
            outs.append(None)
            continue
        pre, fol = _bound(preceding, j, UNBOUNDED), _bound(following, j, 0)
        signed, small = op in (MIN_I64, MAX_I64), op in (MIN_U64, MIN_I64)
        v = np.asarray(cols[j], dtype=np.uint64)[perm]
        v = v.view(np.int64) if signed else v
        info = np.iinfo(v.dtype)
        ident = v.dtype.type(info.max if small else info.min)
        take = np.minimum if small else np.maximum
        pos, ps, pe, lo, hi = _bounds(starts, n, pre, fol)
        res = np.empty(n, dtype=v.dtype)
        if pre >= n or fol >= n:
            run = np.empty(n, dtype=v.dtype)
            for a, b in zip(starts[:-1].tolist(), starts[1:].tolist()):
                run[a:b] = take.accumulate(v[a:b]) if pre >= n else take.accumulate(v[a:b][::-1])[::-1]
            res = run[hi] if pre >= n else run[lo]           # from the partition's start up to hi / from lo up to its end
        else:
            offs = np.arange(-pre, fol + 1, dtype=np.int64)
            step = max(1, chunk_words // len(offs))
            for c in range(0, n, step):
                at = pos[c:c + step, None] + offs[None, :]
                inside = (at >= ps[c:c + step, None]) & (at <= pe[c:c + step, None])
                vals = np.where(inside, v[np.clip(at, 0, n - 1)], ident)
                res[c:c + step] = vals.min(axis=1) if small else vals.max(axis=1)
        out = np.empty(n, dtype=np.uint64)
        out[perm] = res.view(np.uint64)
        outs.append(out)
    return outs


def sums(part, order, flags, col, pre, fol, n=None):
    """SUM of one column under one frame from cumulative sums, aligned with the rows"""
    n = _rows(n, part, order, [col])
    perm, starts = sorted_order(part, order, flags, n)
    v = np.asarray(col, dtype=np.uint64)[perm]
    c = np.cumsum(v, dtype=np.uint64)                        # wraps mod 2^64
    _, _, _, lo, hi = _bounds(starts, n, pre, fol)
    out = np.empty(n, dtype=np.uint64)
    out[perm] = c[hi] - c[lo] + v[lo]
    return out


def ntile(part, order, flags, buckets, n=None):
    """SQL's NTILE per row, from the definition: the first m % buckets buckets hold m // buckets + 1 rows, the others m // buckets"""
    n = _rows(n, part, order, None)
    perm, starts = sorted_order(part, order, flags, n)
    res = np.empty(n, dtype=np.int64)
    for a, b in zip(starts[:-1].tolist(), starts[1:].tolist()):
        m = b - a
        sizes = [m // buckets + (1 if t < m % buckets else 0) for t in range(buckets)]
        res[a:b] = np.repeat(np.arange(1, buckets + 1), sizes)
    out = np.empty(n, dtype=np.int64)
    out[perm] = res
    return out


# ---- generators ----------------------------------------------------------------------------------------------------------------------
def dense_part(sizes, rng=None):
    """a partition column of dense ids 0, 1, .. with the given sizes IN SORTED ORDER: partition i starts at sorted position
    sum(sizes[:i]), so the heads land where the sizes put them.  Shuffled over the rows when rng is given."""
    col = np.repeat(np.arange(len(sizes), dtype=np.uint64), np.asarray(sizes, dtype=np.int64))
    return col[rng.permutation(len(col))] if rng is not None else col


def sizes_with_heads_at(n, heads):
    """partition sizes that put a head at every position of `heads` inside (0, n)"""
    cuts = sorted({h for h in heads if 0 < h < n})
    edges = [0] + cuts + [n]
    return [b - a for a, b in zip(edges[:-1], edges[1:])]


def heads_around(n, marks):
    """one before, on and one after every multiple of every mark below n"""
    out = set()
    for mark in marks:
        for k in range(mark, n, mark):
            out.update((k - 1, k, k + 1))
    return out


def sizes_1_to(top, n):
    """1, 2, .. top, again and again, up to n rows"""
    sizes, s = [], 1
    while sum(sizes) + s <= n:
        sizes.append(s)
        s = s % top + 1
    if sum(sizes) < n:
        sizes.append(n - sum(sizes))
    return sizes


def make_values(kind, n, seed=0):
    rng = np.random.default_rng(13000 + n % 977 + seed)
    if kind == "full64":                      # sums wrap
        return rng.integers(0, 1 << 64, n, dtype=np.uint64)
    if kind == "extremes":                    # only 0, all ones, 1 << 63, (1 << 63) - 1: the four extremes differ between the views
        return EXTREME_WORDS[rng.integers(0, 4, n)]
    if kind == "mixed":
        v = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        where = rng.random(n) < 0.2
        v[where] = EXTREME_WORDS[rng.integers(0, 4, int(where.sum()))]
        return v
    raise ValueError(kind)


def make_order(kind, n, seed=0):
    rng = np.random.default_rng(17000 + n % 983 + seed)
    if kind == "none":
        return None
    if kind == "sixteen":                     # long runs of ties
        return rng.integers(0, 1 << 64, 16, dtype=np.uint64)[rng.integers(0, 16, n)]
    if kind == "distinct":
        return rng.permutation(n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) if n else np.zeros(0, dtype=np.uint64)
    if kind == "extremes":
        special = np.array([0, 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 2, (1 << 64) - 1], dtype=np.uint64)
        return special[rng.integers(0, len(special), n)]
    raise ValueError(kind)


def frame_widths(T, n):
    """the (preceding, following) pairs of the issue"""
    U = UNBOUNDED
    return [(0, 0), (1, 0), (0, 1), (2, 3), (63, 0), (32, 31), (64, 0), (T - 1, 0), (T, 0), (T // 2, T // 2), (n, n), (1 << 63, 1 << 63),
            (U, 0), (0, U), (U, U), (U, 5), (5, U)]


def value_scans(n, ops, preceding, following):
    """"last.frame_scans": 1 per SUM; per minimum / maximum 1 when a side is unbounded or reaches n - 1 positions (every partition's
    edge from every row), else 2; 0 for the other ops"""
    total = 0
    for j, op in enumerate(ops):
        pre, fol = _bound(preceding, j, UNBOUNDED), _bound(following, j, 0)
        if op == SUM:
            total += 1
        elif op in EXTREMES:
            total += 1 if pre >= n - 1 or fol >= n - 1 else 2
    return total
