"""GPU suite: which row holds each group's minimum or maximum -- rhj_group_arg_cols_dev / rhj_group_arg_dev (include/rhj.h, DESIGN
4.23), Engine.group_by_columns_arg and Engine.drop_duplicates_columns.

The oracle is numpy only (group_arg_cases.arg_oracle): per column one lexicographic sort by (key, column word in the op's order,
rowID in the tie's order).  Every comparison is exact, on groups sorted by key, with guard words behind every output array -- the
rows arrays included, which the kernel fills with global atomics.  A row column is given a value array all the same: it must come
back untouched.  What the cases are built around: the tie rule (rowID order, not position order), the extreme that equals the word a
minimum / maximum sweep starts from (the value sweep skips it, the row sweep must not), the word of the all-ones key, the class walk,
and the capacity."""
import ctypes as C

import numpy as np
import pytest
import torch

from group_agg_cases import ADVERSARIAL, adversarial_col, full_range_cols, side_oracle
from group_arg_cases import IDENTITY, MASK64, VALUE_OPS, arg_oracle, tying_groups
from oracle.pyoracle import TUPLE
from radixhashjoin_amd import (AGG_MAX_I64, AGG_MAX_U64, AGG_MIN_I64, AGG_MIN_U64, ARG_MAX_I64, ARG_MAX_U64, ARG_MIN_I64, ARG_MIN_U64,
                               ARG_ROW, ARG_TIE_FIRST, ARG_TIE_LAST, GROUP_ARG_MAX_COLS, Engine, Opts, RhjError, unmix64)
from radixhashjoin_amd.binding import RHJ_E_INVALID, RHJ_E_OVERFLOW, plan as resolve_plan
from test_gpu_group_sum import GUARD, NGUARD, Outputs, make_values

pytestmark = pytest.mark.gpu
PLAN = Opts(2, 8, 8)
JK_GROUP = 15
F, L = ARG_TIE_FIRST, ARG_TIE_LAST
FOUR = [ARG_MIN_I64, ARG_MAX_U64, ARG_ROW, ARG_ROW]                        # MIN and MAX of ONE pointer, the group's first and last row
FOUR_TIES = [F, L, F, L]
SIZES = [(3_000, None, -1), (70_000, None, -1), (3_000_000, PLAN, 2)]
SIZE_IDS = ["3000-unpartitioned", "70000-one-pass", "3000000-narrow"]
AGG_OF = {ARG_MIN_U64: AGG_MIN_U64, ARG_MAX_U64: AGG_MAX_U64, ARG_MIN_I64: AGG_MIN_I64, ARG_MAX_I64: AGG_MAX_I64}


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def inputs():
    """(dist, n, permuted ids) -> (values, ids or None, rows, one full-range column, oracle of FOUR): built once, shared, never
    written"""
    cache = {}

    def get(dist, n, ids=False):
        key = (dist, n, ids)
        if key not in cache:
            v = make_values(dist, n)
            rid = np.random.default_rng(n + 7).permutation(n).astype(np.uint64) if ids else None
            rows = rid.astype(np.int64) if ids else np.arange(n)
            col = full_range_cols(n, 1)[0]
            cache[key] = (v, rid, rows, col, arg_oracle(v, rows, [col, col, None, None], FOUR, FOUR_TIES))
        return cache[key]
    return get


class Uploaded:
    """a relation's value column, ids and columns on the device; a numpy column given several times is uploaded once, so that its
    entries are the same pointer; None stays None"""
    def __init__(self, eng, values, ids, cols):
        self.n = len(values)
        self.v = eng.to_device(np.ascontiguousarray(values))
        self.i = eng.to_device(np.ascontiguousarray(ids)) if ids is not None else None
        self.bufs = {}
        for c in cols:
            if c is not None and id(c) not in self.bufs:
                self.bufs[id(c)] = eng.to_device(c)
        self.c = [None if c is None else self.bufs[id(c)] for c in cols]

    def free(self):
        for b in [self.v] + ([self.i] if self.i is not None else []) + list(self.bufs.values()):
            b.free()


def check_exact(got, exp, ops):
    """got: Outputs.read of 2k columns -- k value arrays, k rows arrays; exp: arg_oracle's"""
    keys, counts, arrs = got
    ek, ec, ev, er = exp
    k = len(ops)
    wrong = int((keys != ek).sum()) if len(keys) == len(ek) else -1
    print(f"groups {len(keys)} expected {len(ek)} wrong keys {wrong}")
    assert len(keys) == len(ek) and np.array_equal(keys, ek)
    if counts is not None:
        assert np.array_equal(counts, ec)
    for j in range(k):
        if ops[j] == ARG_ROW:
            assert (arrs[j] == GUARD).all(), f"column {j}: the value array of a row column was written"
        else:
            assert np.array_equal(arrs[j], ev[j]), f"values of column {j}"
        bad = np.flatnonzero(arrs[k + j] != er[j])
        if len(bad):
            print(f"column {j} op {ops[j]}: {len(bad)} wrong rows, first at key {keys[bad[0]]:#x}: got {arrs[k + j][bad[0]]:#x} "
                  f"expected {er[j][bad[0]]:#x}")
        assert len(bad) == 0, f"rows of column {j}"


def call_cols(eng, dev, ops, ties, col_rows, out, opts=None, **kw):
    k = len(ops)
    return eng.group_arg_cols_dev(dev.v, dev.i, dev.n, dev.c, ops, ties, col_rows, out.keys, out.counts, out.sums[:k], out.sums[k:],
                                  out.cap, opts=opts, **kw)


def run_arg(eng, values, ids, cols, ops, ties, exp, opts=None, dev=None, twice=False):
    """the columnar entry against the oracle with capacity = the number of groups; returns the group count"""
    own = dev is None
    dev = Uploaded(eng, values, ids, cols) if own else dev
    out = Outputs(eng, len(exp[0]), 2 * len(ops))
    try:
        groups = call_cols(eng, dev, ops, ties, dev.n, out, opts)
        print(f"n {dev.n} ops {ops} ties {ties} groups {groups} kernel {eng.info('last.join_kernel')} rounds "
              f"{eng.info('last.group_rounds')} narrow {eng.info('last.narrow')} passes {eng.timings()['passes']}")
        assert groups == len(exp[0])
        got = out.read(groups)
        check_exact(got, exp, ops)
        assert eng.info("last.join_kernel") == JK_GROUP
        if twice:                                                          # bit-identical from run to run
            again = Outputs(eng, len(exp[0]), 2 * len(ops))
            try:
                assert call_cols(eng, dev, ops, ties, dev.n, again, opts) == groups
                check_exact(again.read(groups), exp, ops)
            finally:
                again.free()
    finally:
        out.free()
        if own:
            dev.free()
    return groups


def members_holding_the_extreme(values, rows, col, exp, j):
    """every row the oracle (hence the kernel) names is a tuple of its group and holds the group's extreme -- never a default word"""
    key_of_row = np.empty(len(values), dtype=np.uint64)
    key_of_row[rows] = values
    r = exp[3][j].astype(np.int64)
    assert (r >= 0).all() and (r < len(values)).all()
    assert np.array_equal(key_of_row[r], exp[0]) and np.array_equal(col[r], exp[2][j])


# ---- paths by size -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", [False, True], ids=["null", "ids"])
@pytest.mark.parametrize("dist", ["distinct", "quarter", "zipf"])
@pytest.mark.parametrize("n,opts,narrow", SIZES, ids=SIZE_IDS)
def test_paths_by_size(eng, inputs, n, opts, narrow, dist, ids):
    v, rid, rows, col, exp = inputs(dist, n, ids)
    if opts is None:
        assert resolve_plan(n, n).passes == (0 if n == 3_000 else 1)
    eng.set_option("partition.narrow", narrow)
    if opts is not None:
        eng.set_option("partition.countfree", 0)
    try:
        run_arg(eng, v, rid, [col, col, None, None], FOUR, FOUR_TIES, exp, opts=opts, twice=n < 3_000_000)
        assert eng.timings()["passes"] == (0 if n == 3_000 else 1 if opts is None else 2)
        assert eng.info("last.narrow") == max(narrow, 0) and eng.info("last.group_rounds") == 1
    finally:
        eng.set_option("partition.narrow", -1)
        eng.set_option("partition.countfree", -1)


@pytest.mark.parametrize("n,opts,narrow", SIZES, ids=SIZE_IDS)
def test_aos_entry(eng, inputs, n, opts, narrow):
    v, rid, rows, col, exp = inputs("quarter", n, True)
    R = np.empty(n, dtype=TUPLE)
    R["key"], R["payload"] = rid, v
    dR, dc, out = eng.to_device(R), eng.to_device(col), Outputs(eng, len(exp[0]), 8)
    eng.set_option("partition.narrow", narrow)
    try:
        groups = eng.group_arg_dev(dR, n, [dc, dc, None, None], FOUR, FOUR_TIES, n, out.keys, out.counts, out.sums[:4], out.sums[4:],
                                   out.cap, opts=opts)
        assert groups == len(exp[0])
        check_exact(out.read(groups), exp, FOUR)                           # ... which the columnar entry returns on the same data
        assert eng.info("last.join_kernel") == JK_GROUP and eng.info("last.narrow") == max(narrow, 0)
        assert np.array_equal(dR.to_numpy(TUPLE, n), R)                    # the input stands as it was
    finally:
        eng.set_option("partition.narrow", -1)
        for b in (dR, dc):
            b.free()
        out.free()


# ---- ties are the rule -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3_000, 70_000])
def test_ties_are_the_rule(eng, inputs, n):
    v, rid, rows, _, _ = inputs("quarter", n, True)                        # permuted ids: rowID order is not position order
    col = np.random.default_rng(n + 3).integers(0, 2, n, dtype=np.uint64)
    ops, ties = [ARG_MAX_U64, ARG_MAX_U64, ARG_MIN_I64, ARG_MIN_I64], [F, L, F, L]
    exp = arg_oracle(v, rows, [col] * 4, ops, ties)
    for op in (ARG_MAX_U64, ARG_MIN_I64):                                  # a condition on the input: ties are what most groups have
        tied = tying_groups(v, rows, col, op) >= 2
        print(f"n {n} op {op}: {int(tied.sum())} of {len(tied)} groups hold their extreme at least twice")
        assert 2 * int(tied.sum()) >= len(tied)
        a, b = (0, 1) if op == ARG_MAX_U64 else (2, 3)
        assert np.array_equal(exp[3][a] != exp[3][b], tied) and (exp[3][a] <= exp[3][b]).all()
    out = Outputs(eng, len(exp[0]), 8)
    dev = Uploaded(eng, v, rid, [col] * 4)
    try:
        assert call_cols(eng, dev, ops, ties, n, out) == len(exp[0])
        got = out.read(len(exp[0]))
        check_exact(got, exp, ops)
        for a, b, op in ((0, 1, ARG_MAX_U64), (2, 3, ARG_MIN_I64)):        # FIRST and LAST differ for exactly the groups that tie
            assert np.array_equal(got[2][4 + a] != got[2][4 + b], tying_groups(v, rows, col, op) >= 2)
    finally:
        out.free()
        dev.free()


# ---- the extreme equals the word the sweep starts from -------------------------------------------------------------------------
@pytest.mark.parametrize("ids", [False, True], ids=["null", "ids"])
@pytest.mark.parametrize("n", [3_000, 70_000])
def test_the_extreme_is_the_identity_of_its_op(eng, inputs, n, ids):
    v, rid, rows, _, _ = inputs("quarter", n, ids)
    cols = [np.full(n, IDENTITY[op], dtype=np.uint64) for op in VALUE_OPS]  # all ones, 0, INT64_MAX, INT64_MIN in every row
    for ties in ([F] * 4, [L] * 4):
        exp = arg_oracle(v, rows, cols, VALUE_OPS, ties)
        for j in range(4):
            assert (exp[2][j] == IDENTITY[VALUE_OPS[j]]).all()
            members_holding_the_extreme(v, rows, cols[j], exp, j)
        run_arg(eng, v, rid, cols, VALUE_OPS, ties, exp)


@pytest.mark.parametrize("ids", [False, True], ids=["null", "ids"])
@pytest.mark.parametrize("n", [3_000, 70_000])
@pytest.mark.parametrize("kind", ADVERSARIAL)
def test_adversarial_column_under_every_op(eng, inputs, kind, n, ids):
    v, rid, rows, _, _ = inputs("quarter", n, ids)
    col = adversarial_col(kind, v, rows)
    dev = Uploaded(eng, v, rid, [col] * 4)
    try:
        for ties in ([F, L, L, F], [L, F, F, L]):
            exp = arg_oracle(v, rows, [col] * 4, VALUE_OPS, ties)
            for j in range(4):
                members_holding_the_extreme(v, rows, col, exp, j)
            run_arg(eng, v, rid, [col] * 4, VALUE_OPS, ties, exp, dev=dev)
    finally:
        dev.free()


# ---- heavy and special keys --------------------------------------------------------------------------------------------------
def test_one_value_seventy_thousand_times(eng):
    n = 70_000
    v = np.full(n, 0x0FEDCBA987654321, dtype=np.uint64)
    rid = np.random.default_rng(n + 7).permutation(n).astype(np.uint64)
    rows = rid.astype(np.int64)
    const = np.full(n, 42, dtype=np.uint64)                                # 70,000 tying tuples on one word
    rising = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(1)   # strictly increasing by rowID: exactly one tying tuple
    cols, ops, ties = [const, const, rising, rising], [ARG_MIN_U64, ARG_MAX_I64, ARG_MIN_I64, ARG_MAX_U64], [F, L, L, F]
    exp = arg_oracle(v, rows, cols, ops, ties)
    assert [int(r[0]) for r in exp[3]] == [0, n - 1, 0, n - 1]             # the smallest and the largest rowID; the one row that holds it
    assert run_arg(eng, v, rid, cols, ops, ties, exp, twice=True) == 1


@pytest.mark.parametrize("opts", [None, Opts(1, 4, 0), Opts(0, 0, 0)], ids=["auto", "one-pass", "unpartitioned"])
def test_the_all_ones_key_among_five_thousand_others(eng, opts):
    """the words of the all-ones key lie beside the table: its group index, its value and its rows come through them"""
    n = 5_001
    rng = np.random.default_rng(5)
    v = rng.integers(1, 1 << 62, n, dtype=np.uint64)
    v[::9] = np.uint64(MASK64)
    v[4::9] = np.uint64(unmix64(MASK64))                                   # (a partition holds mix64(value): this one becomes all ones)
    rows, col = np.arange(n), full_range_cols(n, 1)[0]
    run_arg(eng, v, None, [col, col, None, None], FOUR, FOUR_TIES, arg_oracle(v, rows, [col, col, None, None], FOUR, FOUR_TIES), opts=opts)
    same = np.full(n, MASK64, dtype=np.uint64)                             # ... with ties, at the identity of a minimum
    ops, ties = [ARG_MIN_U64, ARG_MIN_U64, ARG_MAX_I64, ARG_ROW], [F, L, L, L]
    exp = arg_oracle(v, rows, [same, same, same, None], ops, ties)
    at = int(np.searchsorted(exp[0], np.uint64(MASK64)))
    assert exp[0][at] == MASK64 and exp[3][0][at] == 0 and exp[3][1][at] == exp[3][3][at] == 4995
    run_arg(eng, v, None, [same, same, same, None], ops, ties, exp, opts=opts)


# ---- more distinct keys than a table: the class walk -------------------------------------------------------------------------
def test_the_class_walk(eng, inputs):
    n, opts = 80_000, Opts(0, 0, 0)
    v, rid, rows, col, exp = inputs("distinct", n, True)
    run_arg(eng, v, rid, [col, col, None, None], FOUR, FOUR_TIES, exp, opts=opts)
    assert eng.info("last.group_rounds") > 1
    v, rid, rows, col, exp = inputs("quarter", n, True)                    # the same table swept with groups of four
    run_arg(eng, v, rid, [col, col, None, None], FOUR, FOUR_TIES, exp, opts=opts)
    assert eng.info("last.group_rounds") > 1
    tie = np.random.default_rng(8).integers(0, 2, n, dtype=np.uint64)
    ops, ties = [ARG_MAX_U64, ARG_MAX_U64, ARG_MIN_U64, ARG_MIN_U64], [F, L, F, L]
    run_arg(eng, v, rid, [tie] * 4, ops, ties, arg_oracle(v, rows, [tie] * 4, ops, ties), opts=opts)


# ---- capacity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3_000, 70_000])
def test_capacity(eng, inputs, n):
    v, rid, rows, col, exp = inputs("quarter", n, True)
    G = len(exp[0])
    cap = G // 2
    dev = Uploaded(eng, v, rid, [col, col, None, None])
    out = Outputs(eng, cap, 8)
    try:
        with pytest.raises(RhjError) as err:
            call_cols(eng, dev, FOUR, FOUR_TIES, n, out)
        assert err.value.code == RHJ_E_OVERFLOW
        groups = call_cols(eng, dev, FOUR, FOUR_TIES, n, out, allow_overflow=True)
        assert groups == G                                                 # the exact count
        keys, counts, arrs = out.read(groups)                              # (asserts the guard words behind all ten arrays)
        assert len(keys) == cap and len(np.unique(keys)) == cap            # complete, distinct groups of the result
        pos = np.searchsorted(exp[0], keys)
        assert np.array_equal(exp[0][pos], keys) and np.array_equal(exp[1][pos], counts)
        for j in range(4):
            if FOUR[j] != ARG_ROW:
                assert np.array_equal(exp[2][j][pos], arrs[j]), j
            assert np.array_equal(exp[3][j][pos], arrs[4 + j]), j
        # count only: the same count, and no array is touched -- col_rows = 0 would refuse every row of a sweep
        before = [b.to_numpy(np.uint64, cap + NGUARD).copy() for b in out.all()]
        assert eng.group_arg_cols_dev(dev.v, dev.i, n, dev.c, FOUR, FOUR_TIES, 0, None, None, out.sums[:4], out.sums[4:], 0) == G
        assert eng.group_arg_cols_dev(dev.v, dev.i, n, (), (), None) == G
        for b, a in zip(out.all(), before):
            assert np.array_equal(b.to_numpy(np.uint64, cap + NGUARD), a)
    finally:
        out.free()
        dev.free()


# ---- guards and arguments ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3_000, 70_000])
def test_a_row_at_col_rows_is_refused_under_a_min_column(eng, inputs, n):
    v, rid, rows, col, exp = inputs("quarter", n, True)
    bad = rid.copy()
    bad[n // 2] = np.uint64(n)                                             # == col_rows
    dev, out = Uploaded(eng, v, bad, [col, None]), Outputs(eng, n, 4)
    try:
        with pytest.raises(RhjError) as err:
            call_cols(eng, dev, [ARG_MIN_U64, ARG_ROW], [F, F], n, out)
        assert err.value.code == RHJ_E_INVALID and "col_rows" in str(err.value)
        dev.c = [None, None]                                               # row columns only: no column is read, the relation is fine
        e2 = arg_oracle(v, bad.astype(np.int64), [None, None], [ARG_ROW, ARG_ROW], [F, L])
        out2 = Outputs(eng, len(e2[0]), 4)
        try:
            assert call_cols(eng, dev, [ARG_ROW, ARG_ROW], [F, L], n, out2) == len(e2[0])
            check_exact(out2.read(len(e2[0])), e2, [ARG_ROW, ARG_ROW])
        finally:
            out2.free()
    finally:
        dev.free()
        out.free()
    run_arg(eng, v, rid, [col, col, None, None], FOUR, FOUR_TIES, exp)     # a valid call on the same context is exact


def test_invalid_arguments(eng):
    n = 100
    v = np.arange(n, dtype=np.uint64)
    R = np.empty(n, dtype=TUPLE)
    R["key"], R["payload"] = v, v
    dv, dR, dc, dk, ds, dr = eng.to_device(v), eng.to_device(R), eng.to_device(v), eng.alloc(8 * n), eng.alloc(8 * n), eng.alloc(8 * n)
    cols = (C.c_void_p * 5)(*[dc.ptr] * 5)
    vals = (C.c_void_p * 5)(*[ds.ptr] * 5)
    rows = (C.c_void_p * 5)(*[dr.ptr] * 5)
    no_row = (C.c_void_p * 5)(dr.ptr, None, dr.ptr, dr.ptr, dr.ptr)
    no_col = (C.c_void_p * 5)(dc.ptr, dc.ptr, None, dc.ptr, dc.ptr)
    no_col3 = (C.c_void_p * 5)(dc.ptr, dc.ptr, dc.ptr, None, dc.ptr)
    no_val = (C.c_void_p * 5)(ds.ptr, ds.ptr, ds.ptr, None, ds.ptr)
    good = (C.c_uint32 * 5)(ARG_MIN_U64, ARG_MAX_U64, ARG_ROW, ARG_MAX_I64, ARG_MIN_I64)
    five = (C.c_uint32 * 5)(ARG_MIN_U64, ARG_ROW, 5, ARG_MAX_I64, 0)
    tie2 = (C.c_uint32 * 5)(F, L, L, 2, F)
    tie_ok = (C.c_uint32 * 5)(F, L, L, F, L)
    g = C.c_uint64()
    lib, ctx = eng.lib, eng.ctx

    def cols_call(rel, ops, ties, ncols, keys, cap, c=cols, va=vals, ro=rows):
        return lib.rhj_group_arg_cols_dev(ctx, rel, None, n, c, ops, ties, ncols, n, None, keys, None, va, ro, cap, C.byref(g))

    def aos_call(rel, ops, ties, ncols, keys, cap, c=cols, va=vals, ro=rows):
        return lib.rhj_group_arg_dev(ctx, rel, n, c, ops, ties, ncols, n, None, keys, None, va, ro, cap, C.byref(g))
    for call, rel in ((cols_call, dv.ptr), (aos_call, dR.ptr)):
        assert call(rel, five, None, 4, dk.ptr, n) == RHJ_E_INVALID                             # an op of 5 ...
        msg = lib.rhj_last_error(ctx).decode()
        assert "ops[2]" in msg and "column 2" in msg and "RHJ_ARG_ROW" in msg, msg              # ... names the column
        assert call(rel, five, None, 4, None, 0) == RHJ_E_INVALID                               # ... also when only counting
        assert "column 2" in lib.rhj_last_error(ctx).decode()
        assert call(rel, five, None, 2, dk.ptr, n) == 0 and g.value == n                        # (the columns before it are fine)
        assert call(rel, good, tie2, 4, dk.ptr, n) == RHJ_E_INVALID                             # a tie of 2
        msg = lib.rhj_last_error(ctx).decode()
        assert "ties[3]" in msg and "column 3" in msg, msg
        assert call(rel, good, tie2, 4, None, 0) == RHJ_E_INVALID
        assert call(rel, good, tie2, 3, dk.ptr, n) == 0 and g.value == n
        assert call(rel, good, tie_ok, GROUP_ARG_MAX_COLS + 1, dk.ptr, n) == RHJ_E_INVALID      # five columns
        assert call(rel, good, tie_ok, GROUP_ARG_MAX_COLS + 1, None, 0) == RHJ_E_INVALID
        assert call(rel, good, tie_ok, 4, dk.ptr, n, ro=no_row) == RHJ_E_INVALID                # a NULL rows pointer with capacity
        assert "column 1" in lib.rhj_last_error(ctx).decode()
        assert call(rel, good, tie_ok, 4, None, 0, ro=no_row) == 0 and g.value == n             # ... is nothing a count needs
        assert call(rel, good, tie_ok, 4, dk.ptr, n, c=no_col) == 0 and g.value == n            # column 2 is a row column: no column needed
        assert call(rel, good, tie_ok, 4, dk.ptr, n, c=no_col3) == RHJ_E_INVALID                # a NULL column under a value op
        assert "column 3" in lib.rhj_last_error(ctx).decode()
        assert call(rel, good, tie_ok, 4, dk.ptr, n, va=no_val) == RHJ_E_INVALID                # ... or a NULL value array
        assert call(rel, good, tie_ok, 4, None, n) == RHJ_E_INVALID                             # NULL d_out_keys with capacity
        assert call(None, good, tie_ok, 1, dk.ptr, n) == RHJ_E_INVALID                          # NULL values with nR > 0
        assert call(rel, good, None, 4, dk.ptr, n) == 0 and g.value == n                        # ties == NULL: every column FIRST
        assert call(rel, good, tie_ok, 0, dk.ptr, n) == 0 and g.value == n                      # no column: keys and counts only
    for b in (dv, dR, dc, dk, ds, dr):
        b.free()


def test_empty_and_single_row(eng):
    col = full_range_cols(1, 1)[0]
    out = Outputs(eng, 4, 8)
    dc = eng.to_device(col)
    try:
        assert eng.group_arg_cols_dev(None, None, 0, [dc, dc, None, None], FOUR, FOUR_TIES, 1, out.keys, out.counts, out.sums[:4],
                                      out.sums[4:], out.cap) == 0
        assert eng.info("last.join_kernel") == -1 and eng.info("last.group_rounds") == 0 and eng.timings()["ntasks"] == 0
        assert eng.group_arg_cols_dev(None, None, 0) == 0 and eng.group_arg_dev(None, 0) == 0
        assert len(out.read(0)[0]) == 0
        for b in out.all():
            assert (b.to_numpy(np.uint64, 4 + NGUARD) == GUARD).all()
    finally:
        dc.free()
        out.free()
    for value in (0, 7, MASK64):                                           # one row: its own argmin under every op and tie
        v = np.array([value], dtype=np.uint64)
        for word in (col[0], 0, MASK64, 1 << 63, (1 << 63) - 1):
            c = np.array([word], dtype=np.uint64)
            for ties in ([F] * 4, [L] * 4):
                exp = arg_oracle(v, np.arange(1), [c] * 4, VALUE_OPS, ties)
                assert all(int(r[0]) == 0 for r in exp[3]) and all(int(x[0]) == int(word) for x in exp[2])
                assert run_arg(eng, v, None, [c] * 4, VALUE_OPS, ties, exp) == 1
        exp = arg_oracle(v, np.arange(1), [None, None], [ARG_ROW, ARG_ROW], [F, L])
        assert run_arg(eng, v, None, [None, None], [ARG_ROW, ARG_ROW], [F, L], exp) == 1


# ---- the values are the aggregate entry's ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,opts,narrow", SIZES[:2] + [(80_000, Opts(0, 0, 0), -1)], ids=SIZE_IDS[:2] + ["classes"])
def test_values_are_the_aggregate_entry_s(eng, inputs, n, opts, narrow):
    v, rid, rows, col, _ = inputs("quarter", n, True)
    dev = Uploaded(eng, v, rid, [col] * 4)
    G = eng.group_agg_cols_dev(dev.v, dev.i, n, opts=opts)
    ref, out = Outputs(eng, G, 4), Outputs(eng, G, 8)
    try:
        assert eng.group_agg_cols_dev(dev.v, dev.i, n, dev.c, [AGG_OF[o] for o in VALUE_OPS], n, ref.keys, ref.counts, ref.sums, ref.cap,
                                      opts=opts) == G
        assert call_cols(eng, dev, VALUE_OPS, [F, L, F, L], n, out, opts) == G
        want, got = ref.read(G), out.read(G)
        assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])
        for j in range(4):
            assert np.array_equal(want[2][j], got[2][j]), j                # bit for bit
        assert np.array_equal(side_oracle(v, rows, [col] * 4, [AGG_OF[o] for o in VALUE_OPS])[2][0], got[2][0])
    finally:
        ref.free()
        out.free()
        dev.free()


# ---- Engine.group_by_columns_arg / drop_duplicates_columns -------------------------------------------------------------------
@pytest.mark.parametrize("n", [1_000, 300_000])
def test_group_by_columns_arg_against_the_oracle(n):
    rng = np.random.default_rng(n)
    k = rng.integers(-(1 << 62), 1 << 62, max(n // 5, 1), dtype=np.int64)[rng.integers(0, max(n // 5, 1), n)]
    k[0], k[1], k[2] = -1, np.iinfo(np.int64).min, 0                       # (-1: the all-ones word)
    t = rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64)
    few = rng.integers(-1, 2, n, dtype=np.int64)                           # ties, and a sign
    names, ties = ["min", "max", "max_u64", "row"], ["first", "last", "first", "last"]
    ops, tw = [ARG_MIN_I64, ARG_MAX_I64, ARG_MAX_U64, ARG_ROW], [F, L, F, L]
    exp = arg_oracle(k.view(np.uint64), np.arange(n), [t.view(np.uint64), few.view(np.uint64), few.view(np.uint64), None], ops, tw)
    e = Engine(0)
    try:
        tk, tt, tf = torch.from_numpy(k).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(few).cuda()
        keys, counts, vals, rows = e.group_by_columns_arg(tk, [tt, tf, tf, None], names, ties)
        assert keys.dtype == counts.dtype == torch.int64 and keys.device == tk.device and len(vals) == len(rows) == 4 and vals[3] is None
        order = np.argsort(keys.cpu().numpy().view(np.uint64), kind="stable")
        assert np.array_equal(keys.cpu().numpy().view(np.uint64)[order], exp[0])
        assert np.array_equal(counts.cpu().numpy().view(np.uint64)[order], exp[1])
        for j in range(4):
            assert rows[j].dtype == torch.int64 and np.array_equal(rows[j].cpu().numpy().view(np.uint64)[order], exp[3][j]), j
            if vals[j] is not None:
                assert np.array_equal(vals[j].cpu().numpy().view(np.uint64)[order], exp[2][j]), j
        assert torch.equal(tt[rows[0]], vals[0]) and torch.equal(tk[rows[3]], keys)             # idxmin: the row holds the value
        # ties as one string; a two-tensor composite key: (a, b) with a * 7 + b the single key's classes
        a, b = rng.integers(-3, 4, n, dtype=np.int64), rng.integers(0, max(n // 40, 1), n, dtype=np.int64)
        ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        (ua, ub), cnt, (lo,), (r,) = e.group_by_columns_arg([ta, tb], [tt], ["min"], "last")
        single = (a + 3) + b * 7
        exp2 = arg_oracle(single.view(np.uint64), np.arange(n), [t.view(np.uint64)], [ARG_MIN_I64], [L])
        got_key = ((ua + 3) + ub * 7).cpu().numpy().view(np.uint64)
        order = np.argsort(got_key, kind="stable")
        assert np.array_equal(got_key[order], exp2[0]) and np.array_equal(cnt.cpu().numpy().view(np.uint64)[order], exp2[1])
        assert np.array_equal(lo.cpu().numpy().view(np.uint64)[order], exp2[2][0])
        assert np.array_equal(r.cpu().numpy().view(np.uint64)[order], exp2[3][0])
        keys, counts, vals, rows = e.group_by_columns_arg(tk[:0].contiguous(), [tt[:0].contiguous()], ["min"])
        assert keys.shape == counts.shape == vals[0].shape == rows[0].shape == (0,)
    finally:
        e.close()


@pytest.mark.parametrize("n", [1_000, 300_000])
def test_drop_duplicates_columns_against_numpy(n):
    rng = np.random.default_rng(n + 1)
    k = rng.integers(-(1 << 40), 1 << 40, max(n // 3, 1), dtype=np.int64)[rng.integers(0, max(n // 3, 1), n)]
    e = Engine(0)
    try:
        tk = torch.from_numpy(k).cuda()
        first = e.drop_duplicates_columns(tk).cpu().numpy()
        want = np.sort(np.unique(k, return_index=True)[1])
        assert first.dtype == np.int64 and np.array_equal(first, want) and (np.diff(first) > 0).all()
        last = e.drop_duplicates_columns(tk, keep="last").cpu().numpy()
        want = np.sort(n - 1 - np.unique(k[::-1], return_index=True)[1])   # the first of the reverse is the last
        assert np.array_equal(last, want) and (np.diff(last) > 0).all()
        assert np.array_equal(np.sort(k[first]), np.unique(k)) and np.array_equal(np.sort(k[last]), np.unique(k))
        a, b = torch.from_numpy(k % 5).cuda(), torch.from_numpy(k // 5).cuda()                   # a composite key: the same rows
        assert np.array_equal(e.drop_duplicates_columns([a, b], keep="first").cpu().numpy(), first)
    finally:
        e.close()
