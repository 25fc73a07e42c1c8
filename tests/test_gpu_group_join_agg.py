"""GPU suite: MIN and MAX beside SUM in the join with GROUP BY on the key, rhj_group_join_agg_cols_dev / rhj_group_join_agg_dev
(include/rhj.h) and Engine.join_group_by_columns(ops_R=..., ops_S=...): one output row per join value -- the value, how
many tuples of each side carry it, and per column and side the RAW aggregate its op names.

The oracle is numpy only: group_agg_cases.side_oracle per side (a stable sort by value, then np.add / np.minimum / np.maximum
.reduceat on the uint64 or int64 view), the key sets intersected (RHJ_GJ_INNER) or R's (RHJ_GJ_LEFT); under LEFT a group that no
tuple of S carries holds, in S's columns, the identity of the column's op and 0 for a sum.  Every comparison is exact, on groups
sorted by key, with guard words behind every output array.
  * paths by size: 3,000 x 3,000 unpartitioned, 70,000 x 50,000 one pass, 3,000,000 x 2,000,000 under Opts(2, 8, 8) narrow; half of
    S's keys are absent from R and a third of R's from S; [MIN_I64, SUM] on R and [MAX_U64, MIN_U64, SUM] on S; both modes; the
    weights avoid the identity words, so under INNER none appears anywhere and under LEFT exactly the unmatched groups hold them;
  * 70,000 x 70,000 rows of one value; the class walk on R with S holding half of its keys; LEFT over an empty S;
  * every op a sum: the arrays of rhj_group_join_cols_dev; capacity one too few; the row guard names the side; an invalid op on
    S's side; the AoS entry;
  * join_group_by_columns(ops_R=["min"], ops_S=["max"]) against torch for both hows: minimum and maximum come back unmultiplied."""
import ctypes as C

import numpy as np
import pytest
import torch

from group_agg_cases import IDENTITY, full_range_cols, side_oracle
from oracle.pyoracle import TUPLE
from radixhashjoin_amd import AGG_MAX_I64, AGG_MAX_U64, AGG_MIN_I64, AGG_MIN_U64, AGG_SUM, GJ_INNER, GJ_LEFT, Engine, Opts, RhjError
from radixhashjoin_amd.binding import RHJ_E_INVALID, RHJ_E_OVERFLOW, plan as resolve_plan
from test_gpu_group_join import Device, Outputs, same

pytestmark = pytest.mark.gpu
PLAN = Opts(2, 8, 8)
JK_GJOIN = 16
MODES = [GJ_INNER, GJ_LEFT]
MODE_IDS = ["inner", "left"]
OPS_R = [AGG_MIN_I64, AGG_SUM]
OPS_S = [AGG_MAX_U64, AGG_MIN_U64, AGG_SUM]
ONE_PASS = Opts(1, 5, 0)                                                   # what 70,000 x 70,000 resolves to; x 50,000 alone would not partition
SIZES = [(3_000, 3_000, None, -1), (70_000, 50_000, ONE_PASS, -1), (3_000_000, 2_000_000, PLAN, 2)]
SIZE_IDS = ["3000x3000-unpartitioned", "70000x50000-one-pass", "3000000x2000000-narrow"]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


# ---- inputs and the oracle ---------------------------------------------------------------------------------------------------
def clean_cols(rows, k, seed):
    """k full-range columns without the four identity words (0, all ones, INT64_MAX, INT64_MIN)"""
    cols = full_range_cols(max(rows, 1), k, seed)
    for c in cols:
        c[np.isin(c, np.array([IDENTITY[AGG_MIN_U64], IDENTITY[AGG_MIN_I64], IDENTITY[AGG_MAX_I64], 0], dtype=np.uint64))] = np.uint64(12345)
    return cols


class Side:
    """one relation of a case: values, ids (or None: rowID = index), weight columns indexed by rowID; its oracle per list of ops"""
    def __init__(self, values, ids=None, cols=None, ncols=3, seed=1):
        self.v, self.ids, self.n = np.ascontiguousarray(values), ids, len(values)
        self.cols = cols if cols is not None else clean_cols(self.n, ncols, seed)
        self.rows = ids.astype(np.int64) if ids is not None else np.arange(self.n)
        self.memo = {}

    def oracle(self, ops):
        if tuple(ops) not in self.memo:
            self.memo[tuple(ops)] = side_oracle(self.v, self.rows, self.cols[:len(ops)], ops)
        return self.memo[tuple(ops)]


def make_sides(nR, nS, ids=False, seed=0):
    """R draws from a pool of nR / 4 keys.  S's key set is the pool without its first third -- a third of R's keys are absent from
    S -- and as many foreign keys again: half of S's keys are absent from R."""
    rng = np.random.default_rng(nR * 31 + nS + seed)
    P = max(nR // 4, 12)
    u = rng.permutation(np.unique(rng.integers(1, 1 << 63, 2 * P + 64, dtype=np.uint64)))
    pool = u[:P]
    shared = pool[P // 3:]
    foreign = u[P:P + len(shared)]
    assert len(foreign) == len(shared)
    src = np.concatenate([shared, foreign])
    assert nR >= P and nS >= len(src)                                      # every key once, the other rows drawn: the fractions are exact
    vR = rng.permutation(np.concatenate([pool, pool[rng.integers(0, P, nR - P)]]))
    vS = rng.permutation(np.concatenate([src, src[rng.integers(0, len(src), nS - len(src))]]))
    idR = rng.permutation(nR).astype(np.uint64) if ids else None
    idS = rng.permutation(nS).astype(np.uint64) if ids else None
    return Side(vR, idR, ncols=2, seed=1), Side(vS, idS, ncols=3, seed=2)


def oracle(R, S, mode, opsR, opsS):
    """(keys ascending, cntR, cntS, [aggsR], [aggsS])"""
    kR, cR, aR = R.oracle(opsR)
    kS, cS, aS = S.oracle(opsS)
    if mode == GJ_INNER:
        keys = np.intersect1d(kR, kS)
        iR, iS = np.searchsorted(kR, keys), np.searchsorted(kS, keys)
        return keys, cR[iR], cS[iS], [a[iR] for a in aR], [a[iS] for a in aS]
    ident = [np.full(len(kR), IDENTITY[op], dtype=np.uint64) for op in opsS]
    zero = np.zeros(len(kR), dtype=np.uint64)
    if len(kS) == 0:
        return kR, cR, zero, list(aR), ident
    pos = np.minimum(np.searchsorted(kS, kR), len(kS) - 1)
    hit = kS[pos] == kR
    return kR, cR, np.where(hit, cS[pos], zero), list(aR), [np.where(hit, a[pos], i) for a, i in zip(aS, ident)]


@pytest.fixture(scope="module")
def inputs():
    cache = {}

    def get(nR, nS, ids=False):
        if (nR, nS, ids) not in cache:
            cache[(nR, nS, ids)] = make_sides(nR, nS, ids)
        return cache[(nR, nS, ids)]
    return get


def key_sets_as_the_case_says(R, S):
    kR, kS = np.unique(R.v), np.unique(S.v)
    both = len(np.intersect1d(kR, kS))
    return 0.32 < 1 - both / len(kR) < 0.35 and 0.49 < 1 - both / len(kS) < 0.51


def call(eng, dev, R, S, opsR, opsS, mode, out, opts=None, **kw):
    return eng.group_join_agg_cols_dev(dev.vR, dev.iR, R.n, dev.vS, dev.iS, S.n, dev.cR[:len(opsR)], opsR, len(R.cols[0]),
                                       dev.cS[:len(opsS)], opsS, len(S.cols[0]), mode, out.keys, out.cntR, out.cntS, out.sumsR,
                                       out.sumsS, out.cap, opts=opts, **kw)


def identities_where_they_belong(got, mode, opsR, opsS):
    """LEFT: every group without a tuple of S holds the identity of the op in S's MIN / MAX columns and 0 in its SUM columns, and
    no other group does; INNER: no identity anywhere (the weights avoid them)"""
    keys, cR, cS, aR, aS = got
    lonely = cS == 0
    assert (cR > 0).all() and (mode == GJ_LEFT or not lonely.any())
    for op, a in zip(opsS, aS):
        if op == AGG_SUM:
            assert not a[lonely].any()
        else:
            assert np.array_equal(a == np.uint64(IDENTITY[op]), lonely), op
    for op, a in zip(opsR, aR):
        if op != AGG_SUM:
            assert not (a == np.uint64(IDENTITY[op])).any(), op
    return int(lonely.sum())


def run_case(eng, R, S, opsR, opsS, mode, opts=None, dev=None):
    """the columnar entry against the oracle with capacity = the number of groups, twice (bit-identical); returns (groups, rounds)"""
    exp = oracle(R, S, mode, opsR, opsS)
    G = len(exp[0])
    own = dev is None
    dev = Device(eng, R, S) if own else dev
    out, again = Outputs(eng, G, len(opsR), len(opsS)), Outputs(eng, G, len(opsR), len(opsS))
    try:
        groups = call(eng, dev, R, S, opsR, opsS, mode, out, opts)
        t = eng.timings()
        print(f"nR {R.n} nS {S.n} mode {mode} groups {groups} kernel {eng.info('last.join_kernel')} rounds {eng.info('last.group_rounds')} "
              f"narrow {eng.info('last.narrow')} tasks {t['ntasks']} passes {t['passes']}")
        assert groups == G
        got = out.read(groups)
        same(got, exp)
        assert eng.info("last.join_kernel") == JK_GJOIN and eng.info("last.semi_tables") == 0
        rounds = eng.info("last.group_rounds")
        assert call(eng, dev, R, S, opsR, opsS, mode, again, opts) == G
        same(again.read(G), got)
    finally:
        out.free()
        again.free()
        if own:
            dev.free()
    return groups, rounds, got


# ---- paths by size -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", [False, True], ids=["null", "ids"])
@pytest.mark.parametrize("nR,nS,opts,narrow", SIZES, ids=SIZE_IDS)
def test_paths_by_size_in_both_modes(eng, inputs, nR, nS, opts, narrow, ids):
    R, S = inputs(nR, nS, ids)
    assert key_sets_as_the_case_says(R, S)
    assert resolve_plan(nR, nS, opts).passes == (0 if opts is None else opts.passes)
    eng.set_option("partition.narrow", narrow)
    if narrow > 0:
        eng.set_option("partition.countfree", 0)
    dev = Device(eng, R, S)
    try:
        for mode in MODES:
            _, rounds, got = run_case(eng, R, S, OPS_R, OPS_S, mode, opts=opts, dev=dev)
            assert rounds == 1 and eng.info("last.narrow") == max(narrow, 0)
            assert eng.timings()["passes"] == (0 if opts is None else opts.passes)
            lonely = identities_where_they_belong(got, mode, OPS_R, OPS_S)
            assert (lonely > 0) == (mode == GJ_LEFT)
    finally:
        eng.set_option("partition.narrow", -1)
        eng.set_option("partition.countfree", -1)
        dev.free()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("nR,nS,opts,narrow", SIZES, ids=SIZE_IDS)
def test_aos_entry(eng, inputs, nR, nS, opts, narrow, mode):
    R, S = inputs(nR, nS, True)
    exp = oracle(R, S, mode, OPS_R, OPS_S)
    tR, tS = np.empty(nR, dtype=TUPLE), np.empty(nS, dtype=TUPLE)
    tR["key"], tR["payload"], tS["key"], tS["payload"] = R.ids, R.v, S.ids, S.v
    dR, dS = eng.to_device(tR), eng.to_device(tS)
    cR, cS = [eng.to_device(c) for c in R.cols], [eng.to_device(c) for c in S.cols]
    out = Outputs(eng, len(exp[0]), 2, 3)
    eng.set_option("partition.narrow", narrow)
    try:
        groups = eng.group_join_agg_dev(dR, nR, dS, nS, cR, OPS_R, nR, cS, OPS_S, nS, mode, out.keys, out.cntR, out.cntS, out.sumsR,
                                        out.sumsS, out.cap, opts=opts)
        assert groups == len(exp[0])
        same(out.read(groups), exp)
        assert eng.info("last.join_kernel") == JK_GJOIN and eng.info("last.cols_R") == 0 and eng.info("last.narrow") == max(narrow, 0)
    finally:
        eng.set_option("partition.narrow", -1)
        for b in [dR, dS] + cR + cS:
            b.free()
        out.free()


# ---- one group, many classes, no S -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_seventy_thousand_rows_of_one_value_on_both_sides(eng, mode):
    n = 70_000
    v = np.full(n, 0x0FEDCBA987654321, dtype=np.uint64)
    R, S = Side(v, ncols=4, seed=1), Side(v, ncols=4, seed=2)
    opsR = [AGG_MIN_U64, AGG_MAX_U64, AGG_MIN_I64, AGG_MAX_I64]
    opsS = [AGG_MAX_I64, AGG_MIN_I64, AGG_MAX_U64, AGG_MIN_U64]
    groups, _, got = run_case(eng, R, S, opsR, opsS, mode)
    assert groups == 1 and int(got[1][0]) == n and int(got[2][0]) == n
    assert int(got[3][0][0]) == int(R.cols[0].min()) and int(got[3][1][0]) == int(R.cols[1].max())
    assert int(got[3][2].view(np.int64)[0]) == int(R.cols[2].view(np.int64).min())
    assert int(got[4][0].view(np.int64)[0]) == int(S.cols[0].view(np.int64).max()) and int(got[4][3][0]) == int(S.cols[3].min())


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_the_class_walk_on_r_with_s_holding_half_of_its_keys(eng, inputs, mode):
    rng = np.random.default_rng(40)
    keys = rng.permutation(np.arange(1, 160_000, 4, dtype=np.uint64))       # 40,000 distinct keys of R in the one partition
    half = keys[:20_000]
    R, S = Side(keys, ncols=2, seed=1), Side(rng.permutation(np.concatenate([half, half])), ncols=3, seed=2)
    eng.set_option("partition.narrow", -1)
    groups, rounds, got = run_case(eng, R, S, OPS_R, OPS_S, mode, opts=Opts(0, 0, 0))
    assert groups == (20_000 if mode == GJ_INNER else 40_000)
    assert rounds >= 9                                                     # 40,000 keys over tables of 4608: at least 5 leaves, 9 builds
    assert identities_where_they_belong(got, mode, OPS_R, OPS_S) == (0 if mode == GJ_INNER else 20_000)
    r, s = inputs(3_000, 3_000)                                            # ... and one table again
    assert run_case(eng, r, s, OPS_R, OPS_S, mode)[1] == 1


def test_left_over_an_empty_s(eng, inputs):
    R, S = inputs(3_000, 3_000, True)
    empty = Side(np.zeros(0, dtype=np.uint64), cols=S.cols)
    exp = oracle(R, empty, GJ_LEFT, OPS_R, OPS_S)
    dev, out = Device(eng, R, S), Outputs(eng, 3_000, 2, 3)
    try:
        for opts in (None, Opts(1, 4, 0)):
            groups = eng.group_join_agg_cols_dev(dev.vR, dev.iR, R.n, None, None, 0, dev.cR, OPS_R, R.n, dev.cS, OPS_S, 0, GJ_LEFT,
                                                 out.keys, out.cntR, out.cntS, out.sumsR, out.sumsS, out.cap, opts=opts)
            assert groups == len(np.unique(R.v)) and eng.info("last.join_kernel") == JK_GJOIN
            got = out.read(groups)
            same(got, exp)
            assert identities_where_they_belong(got, GJ_LEFT, OPS_R, OPS_S) == groups
        assert eng.group_join_agg_cols_dev(dev.vR, dev.iR, R.n, None, None, 0, dev.cR, OPS_R, R.n, dev.cS, OPS_S, 0, GJ_INNER,
                                           out.keys, out.cntR, out.cntS, out.sumsR, out.sumsS, out.cap) == 0
        assert eng.info("last.join_kernel") == -1 and eng.timings()["ntasks"] == 0
    finally:
        dev.free()
        out.free()


# ---- every op a sum: the sum entry's arrays ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("nR,nS,opts", [(3_000, 3_000, None), (70_000, 50_000, ONE_PASS)], ids=SIZE_IDS[:2])
def test_all_sum_is_the_sum_entry(eng, inputs, nR, nS, opts, mode):
    R, S = inputs(nR, nS, True)
    eng.set_option("partition.narrow", -1)
    dev = Device(eng, R, S)
    G = eng.group_join_cols_dev(dev.vR, dev.iR, nR, dev.vS, dev.iS, nS, mode=mode, opts=opts)
    ref = Outputs(eng, G, 2, 3)
    try:
        assert eng.group_join_cols_dev(dev.vR, dev.iR, nR, dev.vS, dev.iS, nS, dev.cR, nR, dev.cS, nS, mode, ref.keys, ref.cntR, ref.cntS,
                                       ref.sumsR, ref.sumsS, ref.cap, opts=opts) == G
        want = ref.read(G)
        for opsR, opsS in ((None, None), ([AGG_SUM] * 2, [AGG_SUM] * 3), (None, [AGG_SUM] * 3)):
            out = Outputs(eng, G, 2, 3)
            try:
                assert eng.group_join_agg_cols_dev(dev.vR, dev.iR, nR, dev.vS, dev.iS, nS, dev.cR, opsR, nR, dev.cS, opsS, nS, mode, out.keys,
                                                   out.cntR, out.cntS, out.sumsR, out.sumsS, out.cap, opts=opts) == G
                same(out.read(G), want)
            finally:
                out.free()
    finally:
        ref.free()
        dev.free()


# ---- capacity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("nR,nS,opts", [(3_000, 3_000, None), (70_000, 50_000, ONE_PASS)], ids=SIZE_IDS[:2])
def test_capacity_one_too_few(eng, inputs, nR, nS, opts, mode):
    R, S = inputs(nR, nS, True)
    exp = oracle(R, S, mode, OPS_R, OPS_S)
    G = len(exp[0])
    eng.set_option("partition.narrow", -1)
    dev = Device(eng, R, S)
    try:
        # count only with ops given: colR_rows = colS_rows = 0 and real ids -- a column read would be refused
        assert eng.group_join_agg_cols_dev(dev.vR, dev.iR, nR, dev.vS, dev.iS, nS, dev.cR, OPS_R, 0, dev.cS, OPS_S, 0, mode, opts=opts) == G
        out = Outputs(eng, G - 1, 2, 3)
        with pytest.raises(RhjError) as err:
            call(eng, dev, R, S, OPS_R, OPS_S, mode, out, opts)
        assert err.value.code == RHJ_E_OVERFLOW
        groups = call(eng, dev, R, S, OPS_R, OPS_S, mode, out, opts, allow_overflow=True)
        assert groups == G                                                 # the exact count
        got = out.read(groups)                                             # (asserts the guard words behind every array)
        out.free()
        assert len(got[0]) == G - 1 and len(np.unique(got[0])) == G - 1    # complete, distinct groups of the result
        pos = np.searchsorted(exp[0], got[0])
        same(got, (exp[0][pos], exp[1][pos], exp[2][pos], [a[pos] for a in exp[3]], [a[pos] for a in exp[4]]))
    finally:
        dev.free()


# ---- guards and arguments ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("side", ["R", "S"])
def test_the_row_guard_names_the_side(eng, inputs, side, mode):
    n = 3_000
    R, S = inputs(n, n, True)
    shared = np.intersect1d(R.v, S.v)[3]                                   # a key both sides hold: every mode sweeps its tuples
    bad_side = R if side == "R" else S
    bad = bad_side.ids.copy()
    bad[int(np.flatnonzero(bad_side.v == shared)[0])] = np.uint64(n)       # == colR_rows / colS_rows
    eng.set_option("partition.narrow", -1)
    dev, out = Device(eng, R, S), Outputs(eng, n, 1, 1)
    db = eng.to_device(bad)
    iR, iS = (db, dev.iS) if side == "R" else (dev.iR, db)
    try:
        with pytest.raises(RhjError) as err:
            eng.group_join_agg_cols_dev(dev.vR, iR, n, dev.vS, iS, n, dev.cR[:1], [AGG_MIN_I64], n, dev.cS[:1], [AGG_MIN_U64], n, mode,
                                        out.keys, out.cntR, out.cntS, out.sumsR, out.sumsS, out.cap)
        assert err.value.code == RHJ_E_INVALID and f"a rowID of {side} " in str(err.value)
        run_case(eng, R, S, OPS_R, OPS_S, mode, dev=dev)                   # a valid call on the same context is exact
    finally:
        db.free()
        dev.free()
        out.free()


def test_an_invalid_op_on_either_side(eng):
    n = 100
    v = np.arange(n, dtype=np.uint64)
    T = np.empty(n, dtype=TUPLE)
    T["key"], T["payload"] = v, v
    dv, dT, dc, dk, ds = eng.to_device(v), eng.to_device(T), eng.to_device(v), eng.alloc(8 * n), eng.alloc(8 * n)
    cols = (C.c_void_p * 4)(*[dc.ptr] * 4)
    aggs = (C.c_void_p * 4)(*[ds.ptr] * 4)
    good = (C.c_uint32 * 4)(AGG_MIN_U64, AGG_MAX_U64, AGG_MIN_I64, AGG_MAX_I64)
    five = (C.c_uint32 * 4)(AGG_SUM, 5, AGG_SUM, AGG_SUM)
    huge = (C.c_uint32 * 4)(AGG_SUM, AGG_SUM, AGG_SUM, 0xFFFFFFFF)
    g = C.c_uint64()
    lib, ctx = eng.lib, eng.ctx

    def cols_call(opsR, opsS, keys, cap, nc=4):
        return lib.rhj_group_join_agg_cols_dev(ctx, dv.ptr, None, n, dv.ptr, None, n, cols, opsR, nc, n, cols, opsS, nc, n, GJ_INNER, None,
                                               keys, None, None, aggs, aggs, cap, C.byref(g))

    def aos_call(opsR, opsS, keys, cap, nc=4):
        return lib.rhj_group_join_agg_dev(ctx, dT.ptr, n, dT.ptr, n, cols, opsR, nc, n, cols, opsS, nc, n, GJ_INNER, None, keys, None, None,
                                          aggs, aggs, cap, C.byref(g))
    for f in (cols_call, aos_call):
        assert f(good, five, dk.ptr, n) == RHJ_E_INVALID                   # an op of 5 on S's side ...
        msg = lib.rhj_last_error(ctx).decode()
        assert "opsS[1]" in msg and "column 1 of S" in msg, msg            # ... names the side and the column
        assert f(good, five, None, 0) == RHJ_E_INVALID                     # ... also when only counting
        assert "column 1 of S" in lib.rhj_last_error(ctx).decode()
        assert f(huge, good, dk.ptr, n) == RHJ_E_INVALID
        assert "column 3 of R" in lib.rhj_last_error(ctx).decode()
        assert f(good, five, dk.ptr, n, nc=1) == 0 and g.value == n        # (the column before it is fine)
        assert f(good, good, dk.ptr, n, nc=5) == RHJ_E_INVALID             # too many columns
        assert f(None, None, dk.ptr, n) == 0 and g.value == n              # NULL ops: sums
        assert f(good, good, dk.ptr, n) == 0 and g.value == n
    for b in (dv, dT, dc, dk, ds):
        b.free()


# ---- Engine.join_group_by_columns(ops_R=..., ops_S=...) ------------------------------------------------------------------------
def sql_reference(kR, kS, wR, wS, how):
    """SELECT key, COUNT(*), MIN(r.w), SUM(r.w2), MAX(s.w) FROM R [LEFT] JOIN S USING (key) GROUP BY key by torch.unique and
    scatter_reduce_ / index_add_ per side, an intersection or a left lookup by numpy: minimum and maximum over the pairs of a group
    are the per-side ones, the sum is multiplied by the other side's count; an unmatched key of R under LEFT counts once and has
    INT64_MIN for S's maximum"""
    uR, invR, cR = torch.unique(kR, return_inverse=True, return_counts=True)
    uS, invS, cS = torch.unique(kS, return_inverse=True, return_counts=True)
    minR = torch.zeros_like(uR).scatter_reduce_(0, invR, wR[0], "amin", include_self=False).cpu().numpy()
    sumR = torch.zeros_like(uR).index_add_(0, invR, wR[1]).cpu().numpy()
    maxS = torch.zeros_like(uS).scatter_reduce_(0, invS, wS[0], "amax", include_self=False).cpu().numpy()
    nR, nS, cR, cS = uR.cpu().numpy(), uS.cpu().numpy(), cR.cpu().numpy(), cS.cpu().numpy()
    with np.errstate(over="ignore"):
        if how == "inner":
            keys, iR, iS = np.intersect1d(nR, nS, return_indices=True)
            return keys, cR[iR] * cS[iS], minR[iR], sumR[iR] * cS[iS], maxS[iS]
        pos = np.minimum(np.searchsorted(nS, nR), len(nS) - 1)
        hit = nS[pos] == nR
        mS = np.where(hit, cS[pos], 1)
        return nR, cR * mS, minR, sumR * mS, np.where(hit, maxS[pos], np.iinfo(np.int64).min)


@pytest.mark.parametrize("how", ["inner", "left"])
@pytest.mark.parametrize("n", [1_000, 300_000])
def test_join_group_by_columns_with_ops_against_torch(n, how):
    rng = np.random.default_rng(n)
    D = max(n // 5, 4)
    pool = rng.integers(-(1 << 62), 1 << 62, D + D // 4, dtype=np.int64)
    kR = pool[rng.integers(0, D, n)]                                       # R: the first D keys; S: all but the first D / 4, and D / 4 more
    kS = pool[rng.integers(D // 4, len(pool), n + n // 3)]
    kR[0], kR[1], kR[2] = -1, np.iinfo(np.int64).min, 0                    # (-1: the all-ones word)
    kS[0], kS[1] = -1, 0
    assert len(np.setdiff1d(kR, kS)) > 0 and len(np.setdiff1d(kS, kR)) > 0 and len(np.intersect1d(kR, kS)) > 0
    wR = [rng.integers(-(1 << 63), (1 << 63) - 1, len(kR), dtype=np.int64) for _ in range(2)]
    wS = [rng.integers(-(1 << 63), -1, len(kS), dtype=np.int64)]           # all negative: a maximum that starts at 0 is wrong
    e = Engine(0)
    try:
        tR, tS = torch.from_numpy(kR).cuda(), torch.from_numpy(kS).cuda()
        twR, twS = [torch.from_numpy(x).cuda() for x in wR], [torch.from_numpy(x).cuda() for x in wS]
        keys, count, aggs_R, aggs_S = e.join_group_by_columns(tR, tS, twR, twS, how=how, ops_R=["min", "sum"], ops_S=["max"])
        exp = sql_reference(tR, tS, twR, twS, how)
        assert keys.dtype == count.dtype == torch.int64 and keys.device == tR.device and len(aggs_R) == 2 and len(aggs_S) == 1
        order = torch.argsort(keys).cpu().numpy()
        pick = lambda t: t.cpu().numpy()[order]
        assert np.array_equal(pick(keys), exp[0]) and np.array_equal(pick(count), exp[1])
        assert np.array_equal(pick(aggs_R[0]), exp[2]), "MIN(r.w) comes back unmultiplied"
        assert np.array_equal(pick(aggs_R[1]), exp[3]) and np.array_equal(pick(aggs_S[0]), exp[4])
        # one side with ops, the other without: its columns are sums, multiplied as ever
        k2, c2, r2, s2 = e.join_group_by_columns(tR, tS, twR[:1], twS, how=how, ops_R=["min"])
        k0, c0, r0, s0 = e.join_group_by_columns(tR, tS, twR[:1], twS, how=how)
        o2, o0 = torch.argsort(k2), torch.argsort(k0)
        assert torch.equal(k2[o2], k0[o0]) and torch.equal(c2[o2], c0[o0]) and torch.equal(s2[0][o2], s0[0][o0])
        assert np.array_equal(r2[0][o2].cpu().numpy(), exp[2])
        zS = tS[:0].contiguous()                                           # an empty S: nothing, or R's group-by with identities for S
        got = e.join_group_by_columns(tR, zS, twR[:1], [zS], how=how, ops_R=["min"], ops_S=["max"])
        assert len(got[0]) == (0 if how == "inner" else len(np.unique(kR)))
        assert bool((got[3][0] == np.iinfo(np.int64).min).all())
        for bad in (dict(ops_R=["min"]), dict(ops_S=["max", "min"]), dict(ops_R=["min", "median"]), dict(ops_S=["MAX"])):
            with pytest.raises(ValueError):
                e.join_group_by_columns(tR, tS, twR, twS, how=how, **bad)
    finally:
        e.close()
