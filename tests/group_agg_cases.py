"""What the two per-column-aggregate GPU suites share (test_gpu_group_agg.py, test_gpu_group_join_agg.py): the numpy oracle of one
side and the columns that tell a minimum from a sum.  Nothing of the product is used: a stable sort by value, then np.add /
np.minimum / np.maximum .reduceat over every group's run -- on the uint64 view for RHJ_AGG_SUM and the U64 ops, on the int64 view for
the I64 ops."""
import numpy as np

from radixhashjoin_amd import AGG_MAX_I64, AGG_MAX_U64, AGG_MIN_I64, AGG_MIN_U64, AGG_SUM

MASK64 = (1 << 64) - 1
I64_MIN, I64_MAX = 1 << 63, (1 << 63) - 1                                  # as 64-bit words
ALL_OPS = [AGG_SUM, AGG_MIN_U64, AGG_MAX_U64, AGG_MIN_I64, AGG_MAX_I64]
# include/rhj.h: what a column of S holds at a group of RHJ_GJ_LEFT that no tuple of S carries
IDENTITY = {AGG_SUM: 0, AGG_MIN_U64: MASK64, AGG_MAX_U64: 0, AGG_MIN_I64: I64_MAX, AGG_MAX_I64: I64_MIN}
_REDUCE = {AGG_SUM: (np.add, np.uint64), AGG_MIN_U64: (np.minimum, np.uint64), AGG_MAX_U64: (np.maximum, np.uint64),
           AGG_MIN_I64: (np.minimum, np.int64), AGG_MAX_I64: (np.maximum, np.int64)}


def side_oracle(values, rows, cols, ops):
    """(keys ascending, counts, [aggregates as uint64 words]).  rows: the rowID of every tuple (int64); cols: uint64 columns indexed
    by rowID, column j aggregated with ops[j]"""
    keys, counts = np.unique(values, return_counts=True)
    if len(keys) == 0:
        return keys, counts.astype(np.uint64), [np.zeros(0, dtype=np.uint64) for _ in cols]
    order = np.argsort(values, kind="stable")
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    aggs = []
    for c, op in zip(cols, ops):
        fn, view = _REDUCE[op]
        aggs.append(fn.reduceat(c[rows][order].view(view), starts).view(np.uint64))
    return keys, counts.astype(np.uint64), aggs


def full_range_cols(rows, k=4, seed=1):
    """k columns drawn from all 64 bits: signed and unsigned answers differ, sums wrap"""
    rng = np.random.default_rng(rows * 3 + seed)
    return [rng.integers(0, 1 << 64, rows, dtype=np.uint64) for _ in range(k)]


def adversarial_col(kind, values, rows, seed=5):
    """a column of len(values) rows (rowID = rows[i] is a permutation of the indices) that sum code gets wrong under some op"""
    n = len(values)
    rng = np.random.default_rng(n + seed)
    if kind == "zeros":                                                    # MIN must be 0: a sweep that skips zeros leaves the start word
        return np.zeros(n, dtype=np.uint64)
    if kind == "all-ones":                                                 # the start word of MIN, -1 as int64
        return np.full(n, MASK64, dtype=np.uint64)
    if kind == "int64-min":                                                # the bias itself: 0 in the biased domain
        return np.full(n, I64_MIN, dtype=np.uint64)
    if kind == "int64-max":                                                # all ones in the biased domain
        return np.full(n, I64_MAX, dtype=np.uint64)
    if kind == "negative":                                                 # MAX_I64 < 0: a start word of 0 would win as a signed value
        return rng.integers(-(1 << 63), 0, n, dtype=np.int64).view(np.uint64)
    if kind == "one-zero-per-group":                                       # exactly one row of each group is 0, the rest are large
        col = rng.integers(1 << 62, 1 << 63, n, dtype=np.uint64)
        _, first = np.unique(values, return_index=True)
        col[rows[first]] = 0
        return col
    raise ValueError(kind)


ADVERSARIAL = ["zeros", "all-ones", "int64-min", "int64-max", "negative", "one-zero-per-group"]
