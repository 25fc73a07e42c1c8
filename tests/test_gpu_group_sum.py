"""GPU suite: GROUP BY on a key column, rhj_group_sum_cols_dev / rhj_group_sum_dev (include/rhj.h) and Engine.group_by_columns:
one output row per distinct join value of R -- the value, how many tuples carry it, up to four sums over those tuples.

The oracle is numpy and uses nothing of the product: np.unique(values, return_counts=True); the sums by a stable sort on the values
and np.add.reduceat in wrapping uint64.  Weights are drawn from the full 64-bit range, so the sums wrap.  The returned groups are
sorted by key and every comparison is exact; besides, the counts add up to nR and the sums of a column to the column's total over
R's rows.
  * paths by size: 3,000 rows unpartitioned, 70,000 one pass, 3,000,000 under Opts(2, 8, 8) in the narrow format; all-distinct,
    n/4 distinct and Zipf 0.9 values; NULL and permuted ids; 0, 1 and 4 columns; the AoS entry once per size;
  * heavy groups: one value 70,000 times, 16 values over 1,000,000 rows, the all-ones key alone and among 5,000 others;
  * more distinct keys than one LDS table in a partition: the class walk (last.group_rounds >= 9), then one table again;
  * capacity: count-only, one slot too few (RHJ_E_OVERFLOW, exact count, complete groups, guard words untouched), exactly enough;
  * the repeats inside a call: a count-free region that overflows, one rowID of 2^32 in the narrow format;
  * the row guard, n = 0 and n = 1, every invalid argument, the workspace (no second relation-sized partition buffer);
  * group_by_columns on int64 tensors: negative keys and weights, refused tensors, queued torch work on a side stream."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.pyoracle import TUPLE
from radixhashjoin_amd import GROUP_MAX_COLS, Engine, Opts, RhjError, unmix64
from radixhashjoin_amd.binding import RHJ_E_INVALID, RHJ_E_OVERFLOW, plan as resolve_plan

pytestmark = pytest.mark.gpu
PLAN = Opts(2, 8, 8)
JK_GROUP = 15
AGG_FILL = 4608                                                            # rhj_internal.h: distinct keys one LDS table takes
MASK64 = (1 << 64) - 1
GUARD, NGUARD = np.uint64(0xFEEDFACECAFEBEEF), 64                          # words behind every output array


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


# ---- inputs and the oracle ---------------------------------------------------------------------------------------------------
def zipf_ranks(rng, n, D, theta=0.9):
    e = 1.0 - theta
    span = (D + 1.0) ** e - 1.0
    r = np.floor((1.0 + rng.random(n) * span) ** (1.0 / e)).astype(np.int64)
    return np.clip(r, 1, D)


def make_values(dist, n, seed=0):
    rng = np.random.default_rng(n * 31 + seed)
    if dist == "distinct":
        return rng.permutation(n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(12345)   # (odd multiplier: a bijection)
    base = rng.integers(1, 1 << 63, max(n // 4, 1), dtype=np.uint64)
    if dist == "quarter":
        return base[rng.integers(0, len(base), n)]
    if dist == "zipf":
        return base[zipf_ranks(rng, n, len(base)) - 1]
    raise ValueError(dist)


def weight_cols(rows, k=GROUP_MAX_COLS, seed=1):
    rng = np.random.default_rng(rows + seed)
    return [rng.integers(0, 1 << 64, rows, dtype=np.uint64) for _ in range(k)]


def oracle(values, rows, cols):
    """(keys ascending, counts, [sums]).  rows: the rowID of every tuple (int64); cols: uint64 columns indexed by rowID"""
    keys, counts = np.unique(values, return_counts=True)
    if len(keys) == 0:
        return keys, counts.astype(np.uint64), [np.zeros(0, dtype=np.uint64) for _ in cols]
    order = np.argsort(values, kind="stable")
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return keys, counts.astype(np.uint64), [np.add.reduceat(c[rows][order], starts) for c in cols]


@pytest.fixture(scope="module")
def inputs():
    """(dist, n, permuted ids) -> (values, ids or None, cols, oracle): built once, shared, never written"""
    cache = {}

    def get(dist, n, ids=False, seed=0):
        key = (dist, n, ids, seed)
        if key not in cache:
            v = make_values(dist, n, seed)
            rid = np.random.default_rng(n + 7).permutation(n).astype(np.uint64) if ids else None
            cols = weight_cols(n)
            cache[key] = (v, rid, cols, oracle(v, rid.astype(np.int64) if ids else np.arange(n), cols))
        return cache[key]
    return get


class Outputs:
    """capacity + NGUARD words per output array, the tail filled with GUARD"""
    def __init__(self, eng, capacity, ncols, counts=True):
        self.eng, self.cap = eng, capacity
        fill = np.full(capacity + NGUARD, GUARD, dtype=np.uint64)
        self.keys = eng.to_device(fill)
        self.counts = eng.to_device(fill) if counts else None
        self.sums = [eng.to_device(fill) for _ in range(ncols)]

    def all(self):
        return [self.keys] + ([self.counts] if self.counts is not None else []) + self.sums

    def read(self, groups):
        """the first min(groups, capacity) groups sorted by key; asserts the guard words"""
        k = min(groups, self.cap)
        arrs = [b.to_numpy(np.uint64, self.cap + NGUARD) for b in self.all()]
        for a in arrs:
            assert (a[self.cap:] == GUARD).all(), "a word at or past capacity was written"
        order = np.argsort(arrs[0][:k], kind="stable")
        keys = arrs[0][:k][order]
        counts = arrs[1][:k][order] if self.counts is not None else None
        sums = [a[:k][order] for a in arrs[(2 if self.counts is not None else 1):]]
        return keys, counts, sums

    def free(self):
        for b in self.all():
            b.free()


def check_exact(got, exp, ncols, values=None, cols=None, rows=None):
    keys, counts, sums = got
    ek, ec, es = exp
    wrong = int((keys != ek).sum()) if len(keys) == len(ek) else -1
    print(f"groups {len(keys)} expected {len(ek)} wrong keys {wrong}")
    assert len(keys) == len(ek) and np.array_equal(keys, ek)
    if counts is not None:
        assert np.array_equal(counts, ec)
        if values is not None:
            assert int(counts.sum(dtype=np.uint64)) == len(values)
    for j in range(ncols):
        assert np.array_equal(sums[j], es[j]), f"column {j}"
        if cols is not None:
            assert int(sums[j].sum(dtype=np.uint64)) == int(cols[j][rows].sum(dtype=np.uint64))


def run_cols(eng, values, ids, cols, exp, ncols, opts=None, col_rows=None):
    """the columnar entry against the oracle with capacity = the number of groups; returns the group count"""
    n = len(values)
    dv = eng.to_device(np.ascontiguousarray(values))
    di = eng.to_device(np.ascontiguousarray(ids)) if ids is not None else None
    dc = [eng.to_device(c) for c in cols[:ncols]]
    out = Outputs(eng, len(exp[0]), ncols)
    try:
        groups = eng.group_sum_cols_dev(dv, di, n, dc, len(cols[0]) if col_rows is None else col_rows, out.keys, out.counts, out.sums,
                                        out.cap, opts=opts)
        print(f"n {n} groups {groups} kernel {eng.info('last.join_kernel')} rounds {eng.info('last.group_rounds')} "
              f"narrow {eng.info('last.narrow')} tasks {eng.timings()['ntasks']} passes {eng.timings()['passes']}")
        assert groups == len(exp[0])
        rows = ids.astype(np.int64) if ids is not None else np.arange(n)
        check_exact(out.read(groups), exp, ncols, values, cols, rows)
        assert eng.info("last.join_kernel") == JK_GROUP and eng.info("last.cols_S") == 0 and eng.info("last.countfree_S") == 0
        assert eng.info("last.semi_tables") == 0
    finally:
        for b in [dv] + ([di] if di is not None else []) + dc:
            b.free()
        out.free()
    return groups


# ---- paths by size -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncols", [0, 1, 4])
@pytest.mark.parametrize("ids", [False, True], ids=["null", "ids"])
@pytest.mark.parametrize("dist", ["distinct", "quarter", "zipf"])
def test_three_thousand_unpartitioned(eng, inputs, dist, ids, ncols):
    v, rid, cols, exp = inputs(dist, 3_000, ids)
    eng.set_option("partition.narrow", -1)
    run_cols(eng, v, rid, cols, exp, ncols)
    assert eng.timings()["passes"] == 0 and eng.info("last.group_rounds") == 1 and eng.info("last.cols_R") == 2
    assert eng.timings()["ntasks"] == 1


@pytest.mark.parametrize("ncols", [0, 1, 4])
@pytest.mark.parametrize("ids", [False, True], ids=["null", "ids"])
@pytest.mark.parametrize("dist", ["distinct", "quarter", "zipf"])
def test_seventy_thousand_one_pass(eng, inputs, dist, ids, ncols):
    n = 70_000
    assert resolve_plan(n, n).passes == 1
    v, rid, cols, exp = inputs(dist, n, ids)
    eng.set_option("partition.narrow", -1)
    run_cols(eng, v, rid, cols, exp, ncols)
    assert eng.timings()["passes"] == 1 and eng.info("last.group_rounds") == 1 and eng.info("last.narrow") == 0


@pytest.mark.parametrize("ncols", [0, 1, 4])
@pytest.mark.parametrize("ids", [False, True], ids=["null", "ids"])
@pytest.mark.parametrize("dist", ["distinct", "quarter", "zipf"])
def test_three_million_narrow_two_pass(eng, inputs, dist, ids, ncols):
    v, rid, cols, exp = inputs(dist, 3_000_000, ids)
    eng.set_option("partition.narrow", 2)
    eng.set_option("partition.countfree", 0)
    try:
        run_cols(eng, v, rid, cols, exp, ncols, opts=PLAN)
        assert eng.info("last.narrow") == 2 and eng.info("last.cols_R") == 1 and eng.info("last.countfree_R") == 0
        assert eng.timings()["passes"] == 2
    finally:
        eng.set_option("partition.narrow", -1)
        eng.set_option("partition.countfree", -1)


@pytest.mark.parametrize("n,opts,narrow", [(3_000, None, -1), (70_000, None, -1), (3_000_000, PLAN, 2)])
def test_aos_entry(eng, inputs, n, opts, narrow):
    v, rid, cols, exp = inputs("quarter", n, True)
    R = np.empty(n, dtype=TUPLE)
    R["key"], R["payload"] = rid, v
    dR, dc, out = eng.to_device(R), [eng.to_device(c) for c in cols], Outputs(eng, len(exp[0]), 4)
    eng.set_option("partition.narrow", narrow)
    try:
        groups = eng.group_sum_dev(dR, n, dc, n, out.keys, out.counts, out.sums, out.cap, opts=opts)
        assert groups == len(exp[0])
        check_exact(out.read(groups), exp, 4, v, cols, rid.astype(np.int64))
        assert eng.info("last.join_kernel") == JK_GROUP and eng.info("last.cols_R") == 0 and eng.info("last.cols_S") == 0
        assert eng.info("last.narrow") == max(narrow, 0)
        assert np.array_equal(dR.to_numpy(TUPLE, n), R)                     # the input stands as it was
    finally:
        eng.set_option("partition.narrow", -1)
        for b in [dR] + dc:
            b.free()
        out.free()


# ---- heavy groups ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [0x0FEDCBA987654321, MASK64, unmix64(MASK64)], ids=["one-value", "all-ones", "all-ones-mixed"])
def test_one_value_seventy_thousand_times(eng, value):
    n = 70_000
    v, cols = np.full(n, value, dtype=np.uint64), weight_cols(n)
    exp = oracle(v, np.arange(n), cols)
    assert run_cols(eng, v, None, cols, exp, 4) == 1 and int(exp[1][0]) == n


def test_sixteen_values_over_a_million_rows(eng):
    n = 1_000_000
    rng = np.random.default_rng(16)
    v = rng.integers(0, 1 << 64, 16, dtype=np.uint64)[rng.integers(0, 16, n)]
    cols = weight_cols(n, 2)
    assert run_cols(eng, v, None, cols, oracle(v, np.arange(n), cols), 2) == 16


@pytest.mark.parametrize("opts", [None, Opts(1, 4, 0), Opts(0, 0, 0)], ids=["auto", "one-pass", "unpartitioned"])
def test_the_all_ones_key_among_five_thousand_others(eng, opts):
    n = 5_001
    rng = np.random.default_rng(5)
    v = rng.integers(1, 1 << 62, n, dtype=np.uint64)
    v[::9] = np.uint64(MASK64)
    v[4::9] = np.uint64(unmix64(MASK64))                                   # (a partition holds mix64(value): this one becomes all ones)
    cols = weight_cols(n, 1)
    run_cols(eng, v, None, cols, oracle(v, np.arange(n), cols), 1, opts=opts)


# ---- more distinct keys than a table: the class walk -------------------------------------------------------------------------
def beyond_a_table(case):
    rng = np.random.default_rng(40)
    if case == "unpartitioned":                                            # 40,000 distinct values, each twice at shuffled positions
        keys = rng.permutation(np.arange(1, 160_000, 4, dtype=np.uint64))
        return np.concatenate([keys, keys])[rng.permutation(80_000)], Opts(0, 0, 0)
    if case == "two-bits":                                                 # 100,000 distinct values over four partitions
        return rng.permutation(100_000).astype(np.uint64) * np.uint64(0x2545F4914F6CDD1D) + np.uint64(99), Opts(1, 2, 0)
    # the mix defeated: 20,000 values whose mix64 ends in sixteen zero bits -- one partition out of 65,536 gets them all
    return np.array([unmix64(k << 16) for k in range(1, 20_001)], dtype=np.uint64)[rng.permutation(20_000)], Opts(2, 8, 8)


@pytest.mark.parametrize("ncols", [4, 0])
@pytest.mark.parametrize("case", ["unpartitioned", "two-bits", "one-partition-of-65536"])
def test_more_distinct_keys_than_a_table(eng, inputs, case, ncols):
    v, opts = beyond_a_table(case)
    n = len(v)
    cols = weight_cols(n)
    eng.set_option("partition.narrow", -1)
    assert eng.info("partition.mix") == 1
    run_cols(eng, v, None, cols, oracle(v, np.arange(n), cols), ncols, opts=opts)
    # 20,000 keys or more in one partition over tables of 4608: at least 5 leaves, hence 9 builds of the binary walk
    assert eng.info("last.group_rounds") >= 9
    if case == "one-partition-of-65536":
        assert eng.timings()["ntasks"] == 1
    v, rid, cols, exp = inputs("quarter", 3_000)                           # ... and one table again
    run_cols(eng, v, rid, cols, exp, ncols)
    assert eng.info("last.group_rounds") == 1


# ---- capacity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,opts", [(3_000, None), (70_000, None), (80_000, Opts(0, 0, 0))], ids=["3000", "70000", "classes"])
def test_capacity(eng, inputs, n, opts):
    if opts is None:
        v, _, cols, exp = inputs("quarter", n)
    else:
        v, _ = beyond_a_table("unpartitioned")
        cols = weight_cols(n)
        exp = oracle(v, np.arange(n), cols)
    G = len(exp[0])
    eng.set_option("partition.narrow", -1)
    dv, dc = eng.to_device(v), [eng.to_device(c) for c in cols]
    try:
        assert eng.group_sum_cols_dev(dv, None, n, opts=opts) == G         # count only, NULL outputs
        assert eng.group_sum_cols_dev(dv, None, n, dc, n, opts=opts) == G  # ... the columns given and not read
        out = Outputs(eng, G - 1, 4)
        with pytest.raises(RhjError) as err:
            eng.group_sum_cols_dev(dv, None, n, dc, n, out.keys, out.counts, out.sums, out.cap, opts=opts)
        assert err.value.code == RHJ_E_OVERFLOW
        groups = eng.group_sum_cols_dev(dv, None, n, dc, n, out.keys, out.counts, out.sums, out.cap, opts=opts, allow_overflow=True)
        assert groups == G                                                 # the exact count
        keys, counts, sums = out.read(groups)                              # (asserts the guard words behind every array)
        out.free()
        assert len(keys) == G - 1 and len(np.unique(keys)) == G - 1        # complete, distinct groups of the result
        pos = np.searchsorted(exp[0], keys)
        assert np.array_equal(exp[0][pos], keys) and np.array_equal(exp[1][pos], counts)
        for j in range(4):
            assert np.array_equal(exp[2][j][pos], sums[j])
        out = Outputs(eng, G, 4, counts=False)                             # exactly enough; no counts array
        assert eng.group_sum_cols_dev(dv, None, n, dc, n, out.keys, None, out.sums, out.cap, opts=opts) == G
        keys, counts, sums = out.read(G)
        out.free()
        assert counts is None and np.array_equal(keys, exp[0]) and all(np.array_equal(sums[j], exp[2][j]) for j in range(4))
    finally:
        for b in [dv] + dc:
            b.free()


# ---- the repeats inside a call -----------------------------------------------------------------------------------------------
def test_count_free_overflow_repeats_with_exact_cursors():
    n = 3_000_000
    v = make_values("quarter", n, seed=3)
    v[np.random.default_rng(3).permutation(n)[: n // 4]] = v[0]            # one value on a quarter of the rows: no count-free region holds it
    cols = weight_cols(n, 1)
    e = Engine(0)
    try:
        e.set_option("partition.narrow", 2)
        e.set_option("partition.countfree", 1)
        run_cols(e, v, None, cols, oracle(v, np.arange(n), cols), 1, opts=PLAN)
        assert e.info("last.narrow") == 2 and e.info("last.countfree_R") == 2 and e.info("last.cols_R") == 1
    finally:
        e.close()


def test_one_wide_id_repeats_at_sixteen_bytes_for_that_call_only(inputs):
    n = 90_000
    v, _, cols, exp = inputs("quarter", n)
    ids = np.arange(n, dtype=np.uint64)
    wide = ids.copy()
    wide[n // 3] = np.uint64(1 << 32)
    e = Engine(0)
    try:
        e.set_option("partition.narrow", 2)                                # set once, never re-armed below
        for rid, narrow in ((ids, 2), (wide, 0), (ids, 2)):
            dv, di, out = e.to_device(v), e.to_device(rid), Outputs(e, len(exp[0]), 0)
            groups = e.group_sum_cols_dev(dv, di, n, (), 0, out.keys, out.counts, (), out.cap, opts=PLAN)   # ncols = 0: the ids travel all the same
            check_exact(out.read(groups), exp, 0, v)
            assert e.info("last.narrow") == narrow and e.info("last.join_kernel") == JK_GROUP
            assert e.info("last.cols_R") == (1 if narrow else 2)
            for b in (dv, di):
                b.free()
            out.free()
    finally:
        e.close()


# ---- the row guard -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3_000, 70_000])
def test_a_row_at_col_rows_is_refused_and_the_context_goes_on(eng, inputs, n):
    v, rid, cols, exp = inputs("quarter", n, True)
    bad = rid.copy()
    bad[n // 2] = np.uint64(n)                                             # == col_rows
    eng.set_option("partition.narrow", -1)
    dv, di, dc, out = eng.to_device(v), eng.to_device(bad), eng.to_device(cols[0]), Outputs(eng, n, 1)
    try:
        with pytest.raises(RhjError) as err:
            eng.group_sum_cols_dev(dv, di, n, [dc], n, out.keys, out.counts, out.sums, out.cap)
        assert err.value.code == RHJ_E_INVALID
        assert eng.group_sum_cols_dev(dv, di, n, (), 0, out.keys, out.counts, (), out.cap) == len(exp[0])   # no column, no guard
        assert eng.group_sum_cols_dev(dv, di, n, [dc], n) == len(exp[0])                                      # count only: no column read
    finally:
        for b in (dv, di, dc):
            b.free()
        out.free()
    run_cols(eng, v, rid, cols, exp, 1)                                    # a valid call on the same context is exact


# ---- edges -------------------------------------------------------------------------------------------------------------------
def test_empty_and_single_row(eng):
    cols = weight_cols(1, 2)
    out = Outputs(eng, 4, 2)
    dc = [eng.to_device(c) for c in cols]
    try:
        assert eng.group_sum_cols_dev(None, None, 0, dc, 1, out.keys, out.counts, out.sums, out.cap) == 0
        assert eng.info("last.join_kernel") == -1 and eng.info("last.group_rounds") == 0 and eng.timings()["ntasks"] == 0
        assert eng.group_sum_cols_dev(None, None, 0) == 0 and eng.group_sum_dev(None, 0) == 0
        assert len(out.read(0)[0]) == 0
    finally:
        for b in dc:
            b.free()
        out.free()
    for value in (0, 7, MASK64):
        v = np.array([value], dtype=np.uint64)
        assert run_cols(eng, v, None, cols, oracle(v, np.arange(1), cols), 2) == 1
        assert eng.info("last.group_rounds") == 1
    dk = eng.to_device(np.arange(10, dtype=np.uint64))
    assert eng.join_sum_cols_dev(dk, None, 10, dk, 10)[0] == 10
    assert eng.info("last.group_rounds") == 0                              # ... and 0 after every other call
    dk.free()


def test_invalid_arguments(eng):
    n = 100
    v = np.arange(n, dtype=np.uint64)
    R = np.empty(n, dtype=TUPLE)
    R["key"], R["payload"] = v, v
    dv, dR, dc, dk, ds = eng.to_device(v), eng.to_device(R), eng.to_device(v), eng.alloc(8 * n), eng.alloc(8 * n)
    cols = (C.c_void_p * 5)(*[dc.ptr] * 5)
    sums = (C.c_void_p * 5)(*[ds.ptr] * 5)
    holes = (C.c_void_p * 5)(dc.ptr, None, dc.ptr, dc.ptr, dc.ptr)
    g = C.c_uint64()
    lib, ctx = eng.lib, eng.ctx

    def cols_call(val, nR, c, ncols, keys, s, cap, og=g):
        return lib.rhj_group_sum_cols_dev(ctx, val, None, nR, c, ncols, n, None, keys, None, s, cap, C.byref(og) if og is not None else None)

    def aos_call(rel, nR, c, ncols, keys, s, cap, og=g):
        return lib.rhj_group_sum_dev(ctx, rel, nR, c, ncols, n, None, keys, None, s, cap, C.byref(og) if og is not None else None)
    for call, rel in ((cols_call, dv.ptr), (aos_call, dR.ptr)):
        assert call(rel, n, cols, GROUP_MAX_COLS + 1, dk.ptr, sums, n) == RHJ_E_INVALID        # too many columns
        assert call(rel, n, cols, GROUP_MAX_COLS + 1, None, sums, 0) == RHJ_E_INVALID          # ... also when only counting
        assert call(rel, n, None, 1, dk.ptr, sums, n) == RHJ_E_INVALID                          # NULL d_cols
        assert call(rel, n, cols, 1, dk.ptr, None, n) == RHJ_E_INVALID                          # NULL d_out_sums
        assert call(rel, n, holes, 2, dk.ptr, sums, n) == RHJ_E_INVALID                         # a NULL column
        assert call(rel, n, cols, 2, dk.ptr, holes, n) == RHJ_E_INVALID                         # a NULL sum column
        assert call(None, n, cols, 1, dk.ptr, sums, n) == RHJ_E_INVALID                         # NULL values with nR > 0
        assert call(rel, n, cols, 1, dk.ptr, sums, n, og=None) == RHJ_E_INVALID                 # NULL out_groups
        assert call(rel, n, cols, 1, None, sums, n) == RHJ_E_INVALID                            # NULL d_out_keys with capacity
        assert call(rel, n, None, 1, None, None, 0) == 0 and g.value == n                       # count only: d_cols is never read
        assert call(rel, n, cols, 4, dk.ptr, sums, n) == 0 and g.value == n
    bad = Opts(3, 0, 0)
    with pytest.raises(RhjError) as err:
        eng.group_sum_cols_dev(dv, None, n, opts=bad)
    assert err.value.code == RHJ_E_INVALID
    with pytest.raises(RhjError) as err:
        eng.group_sum_cols_dev(dv, None, n, [dc], n, dk, None, (), n)     # one column, no sum column
    assert err.value.code == RHJ_E_INVALID
    for b in (dv, dR, dc, dk, ds):
        b.free()


# ---- workspace ---------------------------------------------------------------------------------------------------------------
def test_no_second_relation_sized_partition_buffer(inputs):
    """What a fresh context allocates for 3,000,000 tuples: part_R (16 B per tuple) and the pass-1 intermediate of the same size, and
    no part_S beside them.  Every workspace table is rounded up to 2 MiB, a few dozen MiB in all whatever the size, so the same call
    on 90,000 tuples measures that part: what GROWS with the relation is between one and two and a half times part_R (a part_S would
    make it three), and the same relation joined with itself holds at least another part_R."""
    n, small = 3_000_000, 90_000
    part_R = 16 * n
    used = {}
    for what, rows in (("small", small), ("group", n), ("join", n)):
        v, _, _, exp = inputs("quarter", rows)
        e = Engine(0)
        try:
            e.set_option("partition.narrow", 2)
            e.set_option("partition.countfree", 0)
            dv, out = e.to_device(v), Outputs(e, len(exp[0]), 0)
            before = e.mem_info()[0]
            if what == "join":
                e.join_sum_cols_dev(dv, None, rows, dv, rows, opts=PLAN)
            else:
                assert e.group_sum_cols_dev(dv, None, rows, (), 0, out.keys, out.counts, (), out.cap, opts=PLAN) == len(exp[0])
                assert e.info("last.narrow") == 2
            used[what] = before - e.mem_info()[0]
        finally:
            e.close()
    print(f"workspace: group-by {used['group']} B ({used['small']} B at {small} rows), self-join {used['join']} B, part_R {part_R} B")
    assert part_R <= used["group"] - used["small"] < 2 * part_R + part_R // 2
    assert used["join"] - used["group"] >= part_R - part_R // 8


# ---- Engine.group_by_columns -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1_000, 300_000])
def test_group_by_columns_against_torch(n):
    rng = np.random.default_rng(n)
    k = rng.integers(-(1 << 62), 1 << 62, max(n // 5, 1), dtype=np.int64)[rng.integers(0, max(n // 5, 1), n)]
    k[0], k[1], k[2] = -1, np.iinfo(np.int64).min, 0                       # (-1: the all-ones word)
    w = [rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64) for _ in range(3)]
    e = Engine(0)
    try:
        tk, tw = torch.from_numpy(k).cuda(), [torch.from_numpy(x).cuda() for x in w]
        uk, inv, cnt = torch.unique(tk, return_inverse=True, return_counts=True)
        exp_sums = [torch.zeros_like(uk).index_add_(0, inv, x) for x in tw]
        for nw in (0, 3):
            keys, counts, sums = e.group_by_columns(tk, tw[:nw])
            assert keys.dtype == counts.dtype == torch.int64 and keys.device == tk.device and len(sums) == nw
            assert keys.shape == counts.shape == uk.shape
            order = torch.argsort(keys)
            assert torch.equal(keys[order], uk) and torch.equal(counts[order], cnt)
            for j in range(nw):
                assert sums[j].dtype == torch.int64 and torch.equal(sums[j][order], exp_sums[j])
        keys, counts, sums = e.group_by_columns(tk[:0].contiguous(), [tw[0][:0].contiguous()])
        assert keys.shape == counts.shape == sums[0].shape == (0,)
    finally:
        e.close()


def test_group_by_columns_refuses_what_it_cannot_read():
    e = Engine(0)
    try:
        good = torch.arange(100, device="cuda", dtype=torch.int64)
        for bad in (good.to(torch.int32), good.to(torch.float64), torch.arange(200, device="cuda")[::2], good.cpu(),
                    good.reshape(10, 10), list(range(5))):
            with pytest.raises(ValueError):
                e.group_by_columns(bad)
            with pytest.raises(ValueError):
                e.group_by_columns(good, [bad])
        with pytest.raises(ValueError):
            e.group_by_columns(good, [good[:50].contiguous()])             # a weight of another length
        with pytest.raises(ValueError):
            e.group_by_columns(good, [good] * (GROUP_MAX_COLS + 1))
        keys, counts, sums = e.group_by_columns(good, [good])
        order = torch.argsort(keys)
        assert torch.equal(keys[order], good) and bool((counts == 1).all()) and torch.equal(sums[0][order], good)
    finally:
        e.close()


def test_group_by_columns_is_ordered_behind_queued_torch_work():
    """the keys and the weights are the last products of a queue of torch kernels issued right before the call, on a stream of its own"""
    F, n, rounds = 50_000_000, 300_000, 20
    e = Engine(0)
    try:
        stream = torch.cuda.Stream()
        filler = torch.arange(F, device="cuda", dtype=torch.int64)
        torch.cuda.synchronize()
        stream.wait_stream(torch.cuda.default_stream())
        with torch.cuda.stream(stream):
            assert torch.cuda.current_stream().cuda_stream != 0
            for _ in range(rounds):
                filler.mul_(3).add_(1)
            k = filler[:n].clone() >> 3                                    # (a few rows per key)
            wt = filler[F - n:].clone()
            keys, counts, sums = e.group_by_columns(k, [wt])
        torch.cuda.synchronize()
        x, y = np.arange(n, dtype=np.uint64), np.arange(F - n, F, dtype=np.uint64)
        with np.errstate(over="ignore"):
            for _ in range(rounds):
                x, y = x * np.uint64(3) + np.uint64(1), y * np.uint64(3) + np.uint64(1)
        ek, ec, es = oracle((x.view(np.int64) >> 3).view(np.uint64), np.arange(n), [y])
        order = np.argsort(keys.cpu().numpy().view(np.uint64), kind="stable")
        assert np.array_equal(keys.cpu().numpy().view(np.uint64)[order], ek)
        assert np.array_equal(counts.cpu().numpy().view(np.uint64)[order], ec)
        assert np.array_equal(sums[0].cpu().numpy().view(np.uint64)[order], es[0])
        assert e.bound_stream is None
    finally:
        e.close()
