"""GPU suite: MIN and MAX beside SUM in the group-by, rhj_group_agg_cols_dev / rhj_group_agg_dev (include/rhj.h) and
Engine.group_by_columns(ops=...): one output row per distinct join value of R -- the value, how many tuples carry it, and per column
the aggregate its op names.

The oracle is numpy only (group_agg_cases.side_oracle): a stable sort by value, then np.add / np.minimum / np.maximum .reduceat on the
uint64 view for the U64 ops and the int64 view for the I64 ops.  Every comparison is exact, on groups sorted by key, with guard words
behind every output array.  Three places where sum code is wrong for a minimum or maximum are what the cases are built around: the
word the accumulators start from, the zero a sum sweep skips, and the word of the all-ones key.
  * paths by size: 3,000 rows unpartitioned, 70,000 one pass, 3,000,000 under Opts(2, 8, 8) narrow; all-distinct, n/4 distinct and
    Zipf 0.9 values; NULL and permuted ids; [SUM, MIN_I64, MAX_U64, SUM] -- the start word changes in both directions between
    columns -- and [MIN_U64, MAX_I64] on the SAME column pointer; the AoS entry once per size;
  * full-range weights everywhere (signed and unsigned answers differ) and adversarial columns under every op: all zero, all ones,
    only INT64_MIN, only INT64_MAX, all negative, exactly one zero per group;
  * one value 70,000 times; the all-ones key and unmix64(all ones) among 5,000 others under three plans;
  * the class walk (last.group_rounds >= 9) with mixed ops, then one table again;
  * ops == NULL and [SUM] * 4 against rhj_group_sum_cols_dev: identical arrays;
  * capacity: count-only with ops given, one slot too few, exactly enough with NULL counts;
  * the row guard under a MIN column, an op of 5, ncols above the maximum, nR 0 and 1;
  * group_by_columns(ops=["min", "max", "sum"]) against torch.unique + scatter_reduce_ / index_add_."""
import ctypes as C

import numpy as np
import pytest
import torch

from group_agg_cases import ADVERSARIAL, ALL_OPS, MASK64, adversarial_col, full_range_cols, side_oracle
from oracle.pyoracle import TUPLE
from radixhashjoin_amd import (AGG_MAX_I64, AGG_MAX_U64, AGG_MIN_I64, AGG_MIN_U64, AGG_SUM, GROUP_MAX_COLS, Engine, Opts, RhjError,
                               unmix64)
from radixhashjoin_amd.binding import RHJ_E_INVALID, RHJ_E_OVERFLOW, plan as resolve_plan
from test_gpu_group_sum import Outputs, beyond_a_table, make_values

pytestmark = pytest.mark.gpu
PLAN = Opts(2, 8, 8)
JK_GROUP = 15
MIXED = [AGG_SUM, AGG_MIN_I64, AGG_MAX_U64, AGG_SUM]                       # the start word: 0 -> all ones -> 0 -> 0 (biased, then not)
TWICE = [AGG_MIN_U64, AGG_MAX_I64]                                         # ... on one column pointer
SIZES = [(3_000, None, -1), (70_000, None, -1), (3_000_000, PLAN, 2)]
SIZE_IDS = ["3000-unpartitioned", "70000-one-pass", "3000000-narrow"]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def inputs():
    """(dist, n, permuted ids) -> (values, ids or None, rows, four full-range columns, oracle(cols, ops)): built once, shared, never
    written; an oracle is computed once per list of (column index, op)"""
    cache = {}

    def get(dist, n, ids=False):
        key = (dist, n, ids)
        if key not in cache:
            v = make_values(dist, n)
            rid = np.random.default_rng(n + 7).permutation(n).astype(np.uint64) if ids else None
            rows = rid.astype(np.int64) if ids else np.arange(n)
            cols, memo = full_range_cols(n), {}

            def exp(which, ops, v=v, rows=rows, cols=cols, memo=memo):
                k = (tuple(which), tuple(ops))
                if k not in memo:
                    memo[k] = side_oracle(v, rows, [cols[j] for j in which], ops)
                return memo[k]
            cache[key] = (v, rid, rows, cols, exp)
        return cache[key]
    return get


def check_exact(got, exp):
    keys, counts, aggs = got
    ek, ec, ea = exp
    wrong = int((keys != ek).sum()) if len(keys) == len(ek) else -1
    print(f"groups {len(keys)} expected {len(ek)} wrong keys {wrong}")
    assert len(keys) == len(ek) and np.array_equal(keys, ek)
    if counts is not None:
        assert np.array_equal(counts, ec)
    assert len(aggs) == len(ea)
    for j in range(len(ea)):
        bad = np.flatnonzero(aggs[j] != ea[j])
        if len(bad):
            print(f"column {j}: {len(bad)} wrong, first at key {keys[bad[0]]:#x}: got {aggs[j][bad[0]]:#x} expected {ea[j][bad[0]]:#x}")
        assert len(bad) == 0, f"column {j}"


class Uploaded:
    """a relation's value column, ids and weight columns on the device; a numpy column given twice is uploaded once, so that its two
    entries are the same pointer"""
    def __init__(self, eng, values, ids, cols):
        self.n = len(values)
        self.v = eng.to_device(np.ascontiguousarray(values))
        self.i = eng.to_device(np.ascontiguousarray(ids)) if ids is not None else None
        self.bufs = {}
        for c in cols:
            if id(c) not in self.bufs:
                self.bufs[id(c)] = eng.to_device(c)
        self.c = [self.bufs[id(c)] for c in cols]

    def free(self):
        for b in [self.v] + ([self.i] if self.i is not None else []) + list(self.bufs.values()):
            b.free()


def run_ops(eng, values, ids, cols, ops, exp, opts=None, dev=None):
    """the columnar entry against the oracle with capacity = the number of groups, twice (bit-identical); returns the group count"""
    own = dev is None
    dev = Uploaded(eng, values, ids, cols) if own else dev
    out, again = Outputs(eng, len(exp[0]), len(cols)), Outputs(eng, len(exp[0]), len(cols))
    try:
        groups = eng.group_agg_cols_dev(dev.v, dev.i, dev.n, dev.c, ops, len(cols[0]) if cols else 0, out.keys, out.counts, out.sums,
                                        out.cap, opts=opts)
        print(f"n {dev.n} ops {ops} groups {groups} kernel {eng.info('last.join_kernel')} rounds {eng.info('last.group_rounds')} "
              f"narrow {eng.info('last.narrow')} tasks {eng.timings()['ntasks']} passes {eng.timings()['passes']}")
        assert groups == len(exp[0])
        got = out.read(groups)
        check_exact(got, exp)
        assert eng.info("last.join_kernel") == JK_GROUP and eng.info("last.cols_S") == 0 and eng.info("last.semi_tables") == 0
        assert eng.group_agg_cols_dev(dev.v, dev.i, dev.n, dev.c, ops, len(cols[0]) if cols else 0, again.keys, again.counts, again.sums,
                                      again.cap, opts=opts) == groups
        check_exact(again.read(groups), got)
    finally:
        out.free()
        again.free()
        if own:
            dev.free()
    return groups


# ---- paths by size -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", [False, True], ids=["null", "ids"])
@pytest.mark.parametrize("dist", ["distinct", "quarter", "zipf"])
@pytest.mark.parametrize("n,opts,narrow", SIZES, ids=SIZE_IDS)
def test_paths_by_size(eng, inputs, n, opts, narrow, dist, ids):
    v, rid, rows, cols, exp = inputs(dist, n, ids)
    if opts is None:
        assert resolve_plan(n, n).passes == (0 if n == 3_000 else 1)
    eng.set_option("partition.narrow", narrow)
    if opts is not None:
        eng.set_option("partition.countfree", 0)
    dev = Uploaded(eng, v, rid, cols)
    try:
        run_ops(eng, v, rid, cols, MIXED, exp([0, 1, 2, 3], MIXED), opts=opts, dev=dev)
        assert eng.timings()["passes"] == (0 if n == 3_000 else 1 if opts is None else 2)
        assert eng.info("last.narrow") == max(narrow, 0) and eng.info("last.group_rounds") == 1
        dev.c = [dev.c[1], dev.c[1]]                                       # MIN and MAX of one column in one call
        run_ops(eng, v, rid, [cols[1], cols[1]], TWICE, exp([1, 1], TWICE), opts=opts, dev=dev)
    finally:
        eng.set_option("partition.narrow", -1)
        eng.set_option("partition.countfree", -1)
        dev.free()


@pytest.mark.parametrize("n,opts,narrow", SIZES, ids=SIZE_IDS)
def test_aos_entry(eng, inputs, n, opts, narrow):
    v, rid, rows, cols, exp = inputs("quarter", n, True)
    e = exp([0, 1, 2, 3], MIXED)
    R = np.empty(n, dtype=TUPLE)
    R["key"], R["payload"] = rid, v
    dR, dc, out = eng.to_device(R), [eng.to_device(c) for c in cols], Outputs(eng, len(e[0]), 4)
    eng.set_option("partition.narrow", narrow)
    try:
        groups = eng.group_agg_dev(dR, n, dc, MIXED, n, out.keys, out.counts, out.sums, out.cap, opts=opts)
        assert groups == len(e[0])
        check_exact(out.read(groups), e)
        assert eng.info("last.join_kernel") == JK_GROUP and eng.info("last.cols_R") == 0 and eng.info("last.narrow") == max(narrow, 0)
        assert np.array_equal(dR.to_numpy(TUPLE, n), R)                     # the input stands as it was
    finally:
        eng.set_option("partition.narrow", -1)
        for b in [dR] + dc:
            b.free()
        out.free()


# ---- adversarial columns: every op over each ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", [False, True], ids=["null", "ids"])
@pytest.mark.parametrize("n", [3_000, 70_000])
@pytest.mark.parametrize("kind", ADVERSARIAL)
def test_adversarial_column_under_every_op(eng, inputs, kind, n, ids):
    v, rid, rows, _, _ = inputs("quarter", n, ids)
    col = adversarial_col(kind, v, rows)
    eng.set_option("partition.narrow", -1)
    dev = Uploaded(eng, v, rid, [col])
    try:
        for ops in (ALL_OPS[:4], ALL_OPS[4:] + [AGG_SUM]):                 # five ops over one pointer, four columns per call
            dev.c = [dev.bufs[id(col)]] * len(ops)
            exp = side_oracle(v, rows, [col] * len(ops), ops)
            run_ops(eng, v, rid, [col] * len(ops), ops, exp, dev=dev)
        if kind == "zeros" or kind == "one-zero-per-group":                # (the oracle says so too: the case means what it should)
            exp = side_oracle(v, rows, [col, col], [AGG_MIN_U64, AGG_MIN_I64])
            assert not exp[2][0].any() and not exp[2][1].any()
        if kind == "negative":
            assert (side_oracle(v, rows, [col], [AGG_MAX_I64])[2][0].view(np.int64) < 0).all()
    finally:
        dev.free()


# ---- heavy and special keys --------------------------------------------------------------------------------------------------
def test_one_value_seventy_thousand_times(eng):
    n = 70_000
    v, cols = np.full(n, 0x0FEDCBA987654321, dtype=np.uint64), full_range_cols(n)
    rows = np.arange(n)
    assert run_ops(eng, v, None, cols, MIXED, side_oracle(v, rows, cols, MIXED)) == 1
    assert run_ops(eng, v, None, [cols[1], cols[1]], TWICE, side_oracle(v, rows, [cols[1], cols[1]], TWICE)) == 1


@pytest.mark.parametrize("opts", [None, Opts(1, 4, 0), Opts(0, 0, 0)], ids=["auto", "one-pass", "unpartitioned"])
def test_the_all_ones_key_among_five_thousand_others(eng, opts):
    """the word of the all-ones key lies beside the table: it is seeded and biased like a slot's"""
    n = 5_001
    rng = np.random.default_rng(5)
    v = rng.integers(1, 1 << 62, n, dtype=np.uint64)
    v[::9] = np.uint64(MASK64)
    v[4::9] = np.uint64(unmix64(MASK64))                                   # (a partition holds mix64(value): this one becomes all ones)
    rows, cols = np.arange(n), full_range_cols(n)
    for ops in ([AGG_MIN_U64, AGG_MIN_I64, AGG_MAX_I64, AGG_SUM], [AGG_MAX_U64, AGG_SUM, AGG_MIN_I64, AGG_MIN_U64]):
        run_ops(eng, v, None, cols, ops, side_oracle(v, rows, cols, ops), opts=opts)
    zero = np.zeros(n, dtype=np.uint64)                                    # ... and a zero reaches its minimum
    run_ops(eng, v, None, [zero, zero], [AGG_MIN_U64, AGG_MAX_I64], side_oracle(v, rows, [zero, zero], [AGG_MIN_U64, AGG_MAX_I64]),
            opts=opts)


# ---- more distinct keys than a table: the class walk -------------------------------------------------------------------------
def test_the_class_walk_with_mixed_ops(eng, inputs):
    v, opts = beyond_a_table("unpartitioned")                              # 40,000 distinct values twice over, one partition
    n = len(v)
    rows, cols = np.arange(n), full_range_cols(n)
    eng.set_option("partition.narrow", -1)
    run_ops(eng, v, None, cols, MIXED, side_oracle(v, rows, cols, MIXED), opts=opts)
    assert eng.info("last.group_rounds") >= 9                              # 40,000 keys over tables of 4608: at least 5 leaves, 9 builds
    run_ops(eng, v, None, [cols[1], cols[1]], TWICE, side_oracle(v, rows, [cols[1], cols[1]], TWICE), opts=opts)
    assert eng.info("last.group_rounds") >= 9
    v, rid, rows, cols, exp = inputs("quarter", 3_000)                     # ... and one table again
    run_ops(eng, v, rid, cols, MIXED, exp([0, 1, 2, 3], MIXED))
    assert eng.info("last.group_rounds") == 1


# ---- every op a sum: the sum entry's arrays ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,opts,narrow", SIZES[:2] + [(80_000, Opts(0, 0, 0), -1)], ids=SIZE_IDS[:2] + ["classes"])
def test_all_sum_is_the_sum_entry(eng, inputs, n, opts, narrow):
    if opts is None:
        v, rid, rows, cols, _ = inputs("quarter", n, True)
    else:
        v, rid, cols = beyond_a_table("unpartitioned")[0], None, full_range_cols(n)
    eng.set_option("partition.narrow", narrow)
    dev = Uploaded(eng, v, rid, cols)
    G = eng.group_sum_cols_dev(dev.v, dev.i, n, opts=opts)
    ref = Outputs(eng, G, 4)
    try:
        assert eng.group_sum_cols_dev(dev.v, dev.i, n, dev.c, n, ref.keys, ref.counts, ref.sums, ref.cap, opts=opts) == G
        want = ref.read(G)
        for ops in (None, [AGG_SUM] * 4):
            out = Outputs(eng, G, 4)
            try:
                assert eng.group_agg_cols_dev(dev.v, dev.i, n, dev.c, ops, n, out.keys, out.counts, out.sums, out.cap, opts=opts) == G
                check_exact(out.read(G), want)
            finally:
                out.free()
    finally:
        ref.free()
        dev.free()


# ---- capacity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3_000, 70_000])
def test_capacity(eng, inputs, n):
    v, rid, rows, cols, exp = inputs("quarter", n)
    e = exp([0, 1, 2, 3], MIXED)
    G = len(e[0])
    eng.set_option("partition.narrow", -1)
    dev = Uploaded(eng, v, None, cols)
    try:
        assert eng.group_agg_cols_dev(dev.v, None, n, (), ()) == G         # count only, NULL outputs
        # ... with columns and ops given: no sweep, no column read -- col_rows = 0 would refuse every row of a sweep
        assert eng.group_agg_cols_dev(dev.v, None, n, dev.c, MIXED, 0) == G
        out = Outputs(eng, G - 1, 4)
        with pytest.raises(RhjError) as err:
            eng.group_agg_cols_dev(dev.v, None, n, dev.c, MIXED, n, out.keys, out.counts, out.sums, out.cap)
        assert err.value.code == RHJ_E_OVERFLOW
        groups = eng.group_agg_cols_dev(dev.v, None, n, dev.c, MIXED, n, out.keys, out.counts, out.sums, out.cap, allow_overflow=True)
        assert groups == G                                                 # the exact count
        keys, counts, aggs = out.read(groups)                              # (asserts the guard words behind every array)
        out.free()
        assert len(keys) == G - 1 and len(np.unique(keys)) == G - 1        # complete, distinct groups of the result
        pos = np.searchsorted(e[0], keys)
        assert np.array_equal(e[0][pos], keys) and np.array_equal(e[1][pos], counts)
        for j in range(4):
            assert np.array_equal(e[2][j][pos], aggs[j]), j
        out = Outputs(eng, G, 4, counts=False)                             # exactly enough; no counts array
        assert eng.group_agg_cols_dev(dev.v, None, n, dev.c, MIXED, n, out.keys, None, out.sums, out.cap) == G
        got = out.read(G)
        out.free()
        assert got[1] is None
        check_exact(got, e)
    finally:
        dev.free()


# ---- guards and arguments ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3_000, 70_000])
def test_a_row_at_col_rows_is_refused_under_a_min_column(eng, inputs, n):
    v, rid, rows, cols, exp = inputs("quarter", n, True)
    bad = rid.copy()
    bad[n // 2] = np.uint64(n)                                             # == col_rows
    eng.set_option("partition.narrow", -1)
    dev, out = Uploaded(eng, v, bad, cols[:1]), Outputs(eng, n, 1)
    try:
        for op in (AGG_MIN_U64, AGG_MIN_I64, AGG_MAX_I64):
            with pytest.raises(RhjError) as err:
                eng.group_agg_cols_dev(dev.v, dev.i, n, dev.c, [op], n, out.keys, out.counts, out.sums, out.cap)
            assert err.value.code == RHJ_E_INVALID and "col_rows" in str(err.value)
        assert eng.group_agg_cols_dev(dev.v, dev.i, n, dev.c, [AGG_MIN_U64], n) == len(exp([0], [AGG_MIN_U64])[0])   # count only: no column read
    finally:
        dev.free()
        out.free()
    run_ops(eng, v, rid, cols, MIXED, exp([0, 1, 2, 3], MIXED))            # a valid call on the same context is exact


def test_invalid_ops_and_arguments(eng):
    n = 100
    v = np.arange(n, dtype=np.uint64)
    R = np.empty(n, dtype=TUPLE)
    R["key"], R["payload"] = v, v
    dv, dR, dc, dk, ds = eng.to_device(v), eng.to_device(R), eng.to_device(v), eng.alloc(8 * n), eng.alloc(8 * n)
    cols = (C.c_void_p * 5)(*[dc.ptr] * 5)
    aggs = (C.c_void_p * 5)(*[ds.ptr] * 5)
    good = (C.c_uint32 * 5)(AGG_SUM, AGG_MIN_U64, AGG_MAX_U64, AGG_MIN_I64, AGG_MAX_I64)
    five = (C.c_uint32 * 5)(AGG_SUM, AGG_MIN_U64, 5, AGG_MAX_I64, 0)
    g = C.c_uint64()
    lib, ctx = eng.lib, eng.ctx

    def cols_call(val, nR, ops, ncols, keys, cap):
        return lib.rhj_group_agg_cols_dev(ctx, val, None, nR, cols, ops, ncols, n, None, keys, None, aggs, cap, C.byref(g))

    def aos_call(rel, nR, ops, ncols, keys, cap):
        return lib.rhj_group_agg_dev(ctx, rel, nR, cols, ops, ncols, n, None, keys, None, aggs, cap, C.byref(g))
    for call, rel in ((cols_call, dv.ptr), (aos_call, dR.ptr)):
        assert call(rel, n, five, 4, dk.ptr, n) == RHJ_E_INVALID                                # an op of 5 ...
        msg = lib.rhj_last_error(ctx).decode()
        assert "ops[2]" in msg and "column 2" in msg and "RHJ_AGG_MAX_I64" in msg, msg          # ... names the column
        assert call(rel, n, five, 4, None, 0) == RHJ_E_INVALID                                  # ... also when only counting
        assert "column 2" in lib.rhj_last_error(ctx).decode()
        assert call(rel, n, five, 2, dk.ptr, n) == 0 and g.value == n                           # (the columns before it are fine)
        assert call(rel, n, good, GROUP_MAX_COLS + 1, dk.ptr, n) == RHJ_E_INVALID               # too many columns
        assert call(rel, n, good, GROUP_MAX_COLS + 1, None, 0) == RHJ_E_INVALID
        assert call(rel, n, good, 4, None, n) == RHJ_E_INVALID                                  # NULL d_out_keys with capacity
        assert call(None, n, good, 1, dk.ptr, n) == RHJ_E_INVALID                               # NULL values with nR > 0
        assert call(rel, n, None, 4, dk.ptr, n) == 0 and g.value == n                           # ops == NULL: sums
        assert call(rel, n, good, 4, dk.ptr, n) == 0 and g.value == n
    for b in (dv, dR, dc, dk, ds):
        b.free()


def test_empty_and_single_row(eng):
    cols = full_range_cols(1, 2)
    ops = [AGG_MIN_I64, AGG_MAX_U64]
    out = Outputs(eng, 4, 2)
    dc = [eng.to_device(c) for c in cols]
    try:
        assert eng.group_agg_cols_dev(None, None, 0, dc, ops, 1, out.keys, out.counts, out.sums, out.cap) == 0
        assert eng.info("last.join_kernel") == -1 and eng.info("last.group_rounds") == 0 and eng.timings()["ntasks"] == 0
        assert eng.group_agg_cols_dev(None, None, 0) == 0 and eng.group_agg_dev(None, 0) == 0
        assert len(out.read(0)[0]) == 0
    finally:
        for b in dc:
            b.free()
        out.free()
    for value in (0, 7, MASK64):
        v = np.array([value], dtype=np.uint64)
        exp = side_oracle(v, np.arange(1), cols, ops)
        assert np.array_equal(exp[2][0], cols[0]) and np.array_equal(exp[2][1], cols[1])        # one tuple: its own words
        assert run_ops(eng, v, None, cols, ops, exp) == 1


# ---- Engine.group_by_columns(ops=...) ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1_000, 300_000])
def test_group_by_columns_with_ops_against_torch(n):
    rng = np.random.default_rng(n)
    k = rng.integers(-(1 << 62), 1 << 62, max(n // 5, 1), dtype=np.int64)[rng.integers(0, max(n // 5, 1), n)]
    k[0], k[1], k[2] = -1, np.iinfo(np.int64).min, 0                       # (-1: the all-ones word)
    w = [rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64) for _ in range(3)]
    w[0][::3] = 0                                                          # zeros among negative and positive weights
    e = Engine(0)
    try:
        tk, tw = torch.from_numpy(k).cuda(), [torch.from_numpy(x).cuda() for x in w]
        uk, inv, cnt = torch.unique(tk, return_inverse=True, return_counts=True)
        exp = [torch.zeros_like(uk).scatter_reduce_(0, inv, tw[0], "amin", include_self=False),
               torch.zeros_like(uk).scatter_reduce_(0, inv, tw[1], "amax", include_self=False),
               torch.zeros_like(uk).index_add_(0, inv, tw[2])]
        keys, counts, aggs = e.group_by_columns(tk, tw, ops=["min", "max", "sum"])
        assert keys.dtype == counts.dtype == torch.int64 and keys.device == tk.device and len(aggs) == 3
        order = torch.argsort(keys)
        assert torch.equal(keys[order], uk) and torch.equal(counts[order], cnt)
        for j in range(3):
            assert aggs[j].dtype == torch.int64 and torch.equal(aggs[j][order], exp[j]), j
        keys2, _, (lo, hi) = e.group_by_columns(tk, [tw[0], tw[0]], ops=("min", "max"))         # one tensor twice
        assert torch.equal(lo[torch.argsort(keys2)], exp[0]) and bool((lo <= hi).all())
        # ops=None is what it was: sums through the sum entry
        keys0, counts0, sums0 = e.group_by_columns(tk, tw)
        keys1, counts1, sums1 = e.group_by_columns(tk, tw, ops=["sum"] * 3)
        o0, o1 = torch.argsort(keys0), torch.argsort(keys1)
        assert torch.equal(keys0[o0], uk) and torch.equal(counts0[o0], cnt) and torch.equal(keys1[o1], uk)
        for j in range(3):
            want = torch.zeros_like(uk).index_add_(0, inv, tw[j])
            assert torch.equal(sums0[j][o0], want) and torch.equal(sums1[j][o1], want)
        keys, counts, aggs = e.group_by_columns(tk[:0].contiguous(), [tw[0][:0].contiguous()], ops=["min"])
        assert keys.shape == counts.shape == aggs[0].shape == (0,)
    finally:
        e.close()


def test_group_by_columns_refuses_wrong_ops_before_any_launch():
    e = Engine(0)
    try:
        good = torch.arange(100, device="cuda", dtype=torch.int64)
        e.group_by_columns(good, [good])
        launches = e.timings()["ntasks"], e.info("last.join_kernel")
        for ops in (["min"], ["min", "max", "sum"], [], ["min", "avg"], ["MIN", "max"], [3, 4], ["min", None]):
            with pytest.raises(ValueError):
                e.group_by_columns(good, [good, good], ops=ops)
        with pytest.raises(ValueError):
            e.group_by_columns(good, (), ops=["sum"])
        assert (e.timings()["ntasks"], e.info("last.join_kernel")) == launches
        keys, counts, aggs = e.group_by_columns(good, [good, good], ops=["min", "max"])
        order = torch.argsort(keys)
        assert torch.equal(keys[order], good) and torch.equal(aggs[0][order], good) and torch.equal(aggs[1][order], good)
    finally:
        e.close()
