"""GPU suite: the join with GROUP BY on the key, rhj_group_join_cols_dev / rhj_group_join_dev (include/rhj.h) and
Engine.join_group_by_columns: one output row per join value of R join S -- the value, how many tuples of R and of S carry it, up to
four sums per side over those tuples -- under RHJ_GJ_INNER (the values both sides have) and RHJ_GJ_LEFT (every value of R).

The oracle is numpy and uses nothing of the product: per side np.unique(values, return_counts=True) and the sums by a stable sort on
the values and np.add.reduceat in wrapping uint64; INNER rows are np.intersect1d of the two key sets, LEFT rows are R's keys with
zeros where S has none.  Weights are drawn from the full 64-bit range, so the sums wrap.  The returned groups are sorted by key and
every comparison is exact; every output array carries 64 guard words behind its capacity.  Wherever a case runs through run_case
it is also checked against code this kernel shares nothing with: the sum of cntR * cntS is join_sum_cols_dev's count and the sums of
sumsR[j] * cntS its sums, LEFT's (keys, cntR, sumsR) is group_sum_cols_dev of R, INNER with the sides exchanged returns the same
keys with the fields swapped, and a second run is bit-identical after the sort.
  * paths by size: 3,000 rows per side unpartitioned, 70,000 one pass, 3,000,000 under Opts(2, 8, 8) in the narrow format; n/4
    distinct and Zipf 0.9 values, S over three quarters of R's keys plus a quarter of rows on foreign keys; NULL and permuted ids on
    both sides; (0,0), (1,0), (0,1) and (4,4) columns; both modes; the AoS entry once per size;
  * multiplicity: one value 70,000 x 70,000; the all-ones key and unmix64 of it in R only, in S only and in both, among 5,000
    others and (nearly) alone, under three plans.  "alone" is literal where both sides hold the key; where one side lacks it, three
    ordinary keys stand beside it (one shared, one per side), so that no mode's result is empty;
  * more distinct keys of R than one LDS table in a partition: the class walk (last.group_rounds >= 9), then one table again;
  * capacity: count-only with colR_rows = colS_rows = 0, one slot too few (RHJ_E_OVERFLOW, exact count, complete groups, guard words
    untouched), exactly enough (every run_case call; without the count arrays here);
  * the repeats inside a call: a count-free region that overflows, one rowID of 2^32 on R only and on S only in the narrow format;
  * the row guards of both sides, empty sides and single rows, every invalid argument;
  * join_group_by_columns on int64 tensors: negative keys and weights, how="left", refused tensors, queued work on a side stream."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.pyoracle import TUPLE
from radixhashjoin_amd import GJ_INNER, GJ_LEFT, GROUP_JOIN_MAX_COLS, Engine, Opts, RhjError, unmix64
from radixhashjoin_amd.binding import RHJ_E_INVALID, RHJ_E_OVERFLOW, plan as resolve_plan

pytestmark = pytest.mark.gpu
PLAN = Opts(2, 8, 8)
JK_GJOIN = 16
AGG_FILL = 4608                                                            # rhj_internal.h: distinct keys one LDS table takes
MASK64 = (1 << 64) - 1
GUARD, NGUARD = np.uint64(0xFEEDFACECAFEBEEF), 64                          # words behind every output array
MODES = [GJ_INNER, GJ_LEFT]
MODE_IDS = ["inner", "left"]
COLS = [(0, 0), (1, 0), (0, 1), (4, 4)]
COLS_IDS = ["c00", "c10", "c01", "c44"]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


# ---- inputs and the oracle (numpy alone: tools and CPU checks import them without a GPU) ----------------------------------------
def zipf_ranks(rng, n, D, theta=0.9):
    e = 1.0 - theta
    span = (D + 1.0) ** e - 1.0
    r = np.floor((1.0 + rng.random(n) * span) ** (1.0 / e)).astype(np.int64)
    return np.clip(r, 1, D)


def make_sides(dist, n, seed=0):
    """(values of R, values of S), n each.  R draws from a pool of n/4 keys; S draws three quarters of its rows from the pool without
    its first quarter -- those keys are R's alone -- and a quarter of its rows from foreign keys, which are S's alone."""
    rng = np.random.default_rng(n * 31 + seed)
    P = max(n // 4, 4)
    F = max(P // 4, 1)
    u = np.unique(rng.integers(1, 1 << 63, P + F + 64, dtype=np.uint64))
    assert len(u) >= P + F
    u = rng.permutation(u)
    pool, foreign = u[:P], u[P:P + F]
    shared = pool[P // 4:]

    def draw(src, m):
        if dist == "quarter":
            return src[rng.integers(0, len(src), m)]
        if dist == "zipf":
            return src[zipf_ranks(rng, m, len(src)) - 1]
        raise ValueError(dist)
    nf = n // 4
    vS = np.concatenate([draw(shared, n - nf), draw(foreign, nf)])[rng.permutation(n)]
    return draw(pool, n), vS


def weight_cols(rows, k=GROUP_JOIN_MAX_COLS, seed=1):
    rng = np.random.default_rng(rows + seed)
    return [rng.integers(0, 1 << 64, rows, dtype=np.uint64) for _ in range(k)]


def side_oracle(values, rows, cols):
    """one side: (keys ascending, counts, [sums]).  rows: the rowID of every tuple (int64); cols: uint64 columns indexed by rowID"""
    keys, counts = np.unique(values, return_counts=True)
    if len(keys) == 0:
        return keys, counts.astype(np.uint64), [np.zeros(0, dtype=np.uint64) for _ in cols]
    order = np.argsort(values, kind="stable")
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return keys, counts.astype(np.uint64), [np.add.reduceat(c[rows][order], starts) for c in cols]


def oracle(oR, oS, mode, ncR, ncS):
    """(keys ascending, cntR, cntS, [sumsR], [sumsS]) from the two sides' oracles"""
    kR, cR, sR = oR
    kS, cS, sS = oS
    if mode == GJ_INNER:
        keys = np.intersect1d(kR, kS)
        iR, iS = np.searchsorted(kR, keys), np.searchsorted(kS, keys)
        return keys, cR[iR], cS[iS], [s[iR] for s in sR[:ncR]], [s[iS] for s in sS[:ncS]]
    zero = np.zeros(len(kR), dtype=np.uint64)
    if len(kS) == 0:
        return kR, cR, zero, list(sR[:ncR]), [zero for _ in sS[:ncS]]
    pos = np.minimum(np.searchsorted(kS, kR), len(kS) - 1)
    hit = kS[pos] == kR
    return kR, cR, np.where(hit, cS[pos], zero), list(sR[:ncR]), [np.where(hit, s[pos], zero) for s in sS[:ncS]]


class Side:
    """one relation of a case: values, ids (or None: rowID = index), weight columns indexed by rowID, and its oracle"""
    def __init__(self, values, ids=None, cols=None, col_seed=1):
        self.v, self.ids, self.n = np.ascontiguousarray(values), ids, len(values)
        self.cols = cols if cols is not None else weight_cols(max(self.n, 1), seed=col_seed)
        self.rows = ids.astype(np.int64) if ids is not None else np.arange(self.n)
        self.oracle = side_oracle(self.v, self.rows, self.cols)


@pytest.fixture(scope="module")
def inputs():
    """(dist, n, permuted ids) -> (Side R, Side S): built once, shared, never written"""
    cache = {}

    def get(dist, n, ids=False, seed=0):
        key = (dist, n, ids, seed)
        if key not in cache:
            vR, vS = make_sides(dist, n, seed)
            rng = np.random.default_rng(n + 7)
            idR = rng.permutation(n).astype(np.uint64) if ids else None
            idS = rng.permutation(n).astype(np.uint64) if ids else None
            cache[key] = (Side(vR, idR, col_seed=1), Side(vS, idS, col_seed=2))
        return cache[key]
    return get


class Outputs:
    """capacity + NGUARD words per output array, the tail filled with GUARD"""
    def __init__(self, eng, capacity, ncR, ncS, cntR=True, cntS=True):
        self.cap = capacity
        fill = np.full(capacity + NGUARD, GUARD, dtype=np.uint64)
        self.keys = eng.to_device(fill)
        self.cntR = eng.to_device(fill) if cntR else None
        self.cntS = eng.to_device(fill) if cntS else None
        self.sumsR = [eng.to_device(fill) for _ in range(ncR)]
        self.sumsS = [eng.to_device(fill) for _ in range(ncS)]

    def all(self):
        return [b for b in [self.keys, self.cntR, self.cntS] + self.sumsR + self.sumsS if b is not None]

    def read(self, groups):
        """the first min(groups, capacity) groups sorted by key: (keys, cntR, cntS, [sumsR], [sumsS]); asserts the guard words"""
        k = min(groups, self.cap)
        get = lambda b: None if b is None else b.to_numpy(np.uint64, self.cap + NGUARD)
        keys, cR, cS = get(self.keys), get(self.cntR), get(self.cntS)
        sR, sS = [get(b) for b in self.sumsR], [get(b) for b in self.sumsS]
        for a in [keys, cR, cS] + sR + sS:
            assert a is None or (a[self.cap:] == GUARD).all(), "a word at or past capacity was written"
        order = np.argsort(keys[:k], kind="stable")
        cut = lambda a: None if a is None else a[:k][order]
        return cut(keys), cut(cR), cut(cS), [cut(a) for a in sR], [cut(a) for a in sS]

    def free(self):
        for b in self.all():
            b.free()


def same(got, exp):
    """exact equality of two (keys, cntR, cntS, [sumsR], [sumsS]); a None count array is not compared"""
    wrong = int((got[0] != exp[0]).sum()) if len(got[0]) == len(exp[0]) else -1
    print(f"groups {len(got[0])} expected {len(exp[0])} wrong keys {wrong}")
    assert len(got[0]) == len(exp[0]) and np.array_equal(got[0], exp[0])
    for i in (1, 2):
        if got[i] is not None:
            assert np.array_equal(got[i], exp[i]), ("cntR", "cntS")[i - 1]
    for i in (3, 4):
        assert len(got[i]) == len(exp[i])
        for j, (a, b) in enumerate(zip(got[i], exp[i])):
            assert np.array_equal(a, b), (("sumsR", "sumsS")[i - 3], j)


class Device:
    """both relations of a case on the device"""
    def __init__(self, eng, R, S):
        up = lambda a: eng.to_device(np.ascontiguousarray(a)) if a is not None and len(a) else None
        self.vR, self.iR, self.vS, self.iS = up(R.v), up(R.ids), up(S.v), up(S.ids)
        self.cR, self.cS = [eng.to_device(c) for c in R.cols], [eng.to_device(c) for c in S.cols]

    def free(self):
        for b in [self.vR, self.iR, self.vS, self.iS] + self.cR + self.cS:
            if b is not None:
                b.free()


def call(eng, dev, R, S, ncR, ncS, mode, out, opts=None, exchanged=False, **kw):
    if exchanged:
        return eng.group_join_cols_dev(dev.vS, dev.iS, S.n, dev.vR, dev.iR, R.n, dev.cS[:ncS], len(S.cols[0]), dev.cR[:ncR], len(R.cols[0]),
                                       mode, out.keys, out.cntR, out.cntS, out.sumsR, out.sumsS, out.cap, opts=opts, **kw)
    return eng.group_join_cols_dev(dev.vR, dev.iR, R.n, dev.vS, dev.iS, S.n, dev.cR[:ncR], len(R.cols[0]), dev.cS[:ncS], len(S.cols[0]),
                                   mode, out.keys, out.cntR, out.cntS, out.sumsR, out.sumsS, out.cap, opts=opts, **kw)


def run_case(eng, R, S, ncR, ncS, mode, opts=None, dev=None):
    """the columnar entry against the oracle with capacity = the number of groups, then the cross-checks; returns the group count"""
    exp = oracle(R.oracle, S.oracle, mode, ncR, ncS)
    G = len(exp[0])
    own = dev is None
    dev = Device(eng, R, S) if own else dev
    out = Outputs(eng, G, ncR, ncS)
    try:
        groups = call(eng, dev, R, S, ncR, ncS, mode, out, opts)
        t = eng.timings()
        print(f"nR {R.n} nS {S.n} mode {mode} groups {groups} kernel {eng.info('last.join_kernel')} rounds {eng.info('last.group_rounds')} "
              f"narrow {eng.info('last.narrow')} tasks {t['ntasks']} passes {t['passes']}")
        assert groups == G
        got = out.read(groups)
        same(got, exp)
        assert eng.info("last.join_kernel") == JK_GJOIN and eng.info("last.semi_tables") == 0
        rounds, narrow = eng.info("last.group_rounds"), eng.info("last.narrow")
        # a second run: bit-identical after the sort
        out2 = Outputs(eng, G, ncR, ncS)
        try:
            assert call(eng, dev, R, S, ncR, ncS, mode, out2, opts) == G
            same(out2.read(G), got)
        finally:
            out2.free()
        # SUM over the groups of the products = the aggregating join of the same inputs
        with np.errstate(over="ignore"):
            count, sums = eng.join_sum_cols_dev(dev.vR, dev.iR, R.n, dev.vS, S.n, dev.cR[:ncR], len(R.cols[0]), opts=opts)
            assert count == int((got[1] * got[2]).sum(dtype=np.uint64))
            for j in range(ncR):
                assert sums[j] == int((got[3][j] * got[2]).sum(dtype=np.uint64)), j
        if mode == GJ_LEFT:                                                # (keys, cntR, sumsR) = the group-by of R
            g = Outputs(eng, G, ncR, 0, cntS=False)
            try:
                assert eng.group_sum_cols_dev(dev.vR, dev.iR, R.n, dev.cR[:ncR], len(R.cols[0]), g.keys, g.cntR, g.sumsR, g.cap, opts=opts) == G
                gk, gc, _, gs, _ = g.read(G)
                same((gk, gc, None, gs, []), (got[0], got[1], None, got[3], []))
            finally:
                g.free()
        else:                                                              # the sides exchanged: the same keys, the fields swapped
            x = Outputs(eng, G, ncS, ncR)
            try:
                assert call(eng, dev, R, S, ncR, ncS, mode, x, opts, exchanged=True) == G
                xk, xcR, xcS, xsR, xsS = x.read(G)
                same((xk, xcS, xcR, xsS, xsR), got)
            finally:
                x.free()
    finally:
        out.free()
        if own:
            dev.free()
    return groups, rounds, narrow


def has_both_kinds_of_lonely_keys(R, S):
    """the case means something: a non-empty result in both modes, a key of R that S lacks and a key of S that R lacks"""
    kR, kS = R.oracle[0], S.oracle[0]
    both = len(np.intersect1d(kR, kS))
    return both > 0 and len(kR) > both and len(kS) > both


# ---- paths by size -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("nc", COLS, ids=COLS_IDS)
@pytest.mark.parametrize("ids", [False, True], ids=["null", "ids"])
@pytest.mark.parametrize("dist", ["quarter", "zipf"])
def test_three_thousand_unpartitioned(eng, inputs, dist, ids, nc, mode):
    R, S = inputs(dist, 3_000, ids)
    assert has_both_kinds_of_lonely_keys(R, S)
    eng.set_option("partition.narrow", -1)
    _, rounds, _ = run_case(eng, R, S, nc[0], nc[1], mode)
    assert rounds == 1 and resolve_plan(3_000, 3_000).passes == 0


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("nc", COLS, ids=COLS_IDS)
@pytest.mark.parametrize("ids", [False, True], ids=["null", "ids"])
@pytest.mark.parametrize("dist", ["quarter", "zipf"])
def test_seventy_thousand_one_pass(eng, inputs, dist, ids, nc, mode):
    n = 70_000
    assert resolve_plan(n, n).passes == 1
    R, S = inputs(dist, n, ids)
    assert has_both_kinds_of_lonely_keys(R, S)
    eng.set_option("partition.narrow", -1)
    _, rounds, narrow = run_case(eng, R, S, nc[0], nc[1], mode)
    assert rounds == 1 and narrow == 0


@pytest.fixture(scope="module")
def big_device(eng, inputs):
    """the 3,000,000-row relations on the device, uploaded once per (dist, ids)"""
    cache = {}

    def get(dist, ids):
        if (dist, ids) not in cache:
            cache[(dist, ids)] = Device(eng, *inputs(dist, 3_000_000, ids))
        return cache[(dist, ids)]
    yield get
    for d in cache.values():
        d.free()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("nc", COLS, ids=COLS_IDS)
@pytest.mark.parametrize("ids", [False, True], ids=["null", "ids"])
@pytest.mark.parametrize("dist", ["quarter", "zipf"])
def test_three_million_narrow_two_pass(eng, inputs, big_device, dist, ids, nc, mode):
    R, S = inputs(dist, 3_000_000, ids)
    assert has_both_kinds_of_lonely_keys(R, S)
    eng.set_option("partition.narrow", 2)
    eng.set_option("partition.countfree", 0)
    try:
        _, _, narrow = run_case(eng, R, S, nc[0], nc[1], mode, opts=PLAN, dev=big_device(dist, ids))
        assert narrow == 2
    finally:
        eng.set_option("partition.narrow", -1)
        eng.set_option("partition.countfree", -1)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("n,opts,narrow", [(3_000, None, -1), (70_000, None, -1), (3_000_000, PLAN, 2)])
def test_aos_entry(eng, inputs, n, opts, narrow, mode):
    R, S = inputs("quarter", n, True)
    exp = oracle(R.oracle, S.oracle, mode, 4, 4)
    tR, tS = np.empty(n, dtype=TUPLE), np.empty(n, dtype=TUPLE)
    tR["key"], tR["payload"], tS["key"], tS["payload"] = R.ids, R.v, S.ids, S.v
    dR, dS = eng.to_device(tR), eng.to_device(tS)
    cR, cS = [eng.to_device(c) for c in R.cols], [eng.to_device(c) for c in S.cols]
    out = Outputs(eng, len(exp[0]), 4, 4)
    eng.set_option("partition.narrow", narrow)
    try:
        groups = eng.group_join_dev(dR, n, dS, n, cR, n, cS, n, mode, out.keys, out.cntR, out.cntS, out.sumsR, out.sumsS, out.cap, opts=opts)
        assert groups == len(exp[0])
        same(out.read(groups), exp)
        assert eng.info("last.join_kernel") == JK_GJOIN and eng.info("last.cols_R") == 0 and eng.info("last.cols_S") == 0
        assert eng.info("last.narrow") == max(narrow, 0)
        assert np.array_equal(dR.to_numpy(TUPLE, n), tR) and np.array_equal(dS.to_numpy(TUPLE, n), tS)   # the inputs stand as they were
    finally:
        eng.set_option("partition.narrow", -1)
        for b in [dR, dS] + cR + cS:
            b.free()
        out.free()


# ---- multiplicity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("value", [0x0FEDCBA987654321, MASK64, unmix64(MASK64)], ids=["one-value", "all-ones", "all-ones-mixed"])
def test_one_value_seventy_thousand_times_on_both_sides(eng, value, mode):
    n = 70_000
    R, S = Side(np.full(n, value, dtype=np.uint64), col_seed=1), Side(np.full(n, value, dtype=np.uint64), col_seed=2)
    exp = oracle(R.oracle, S.oracle, mode, 4, 4)
    assert len(exp[0]) == 1 and int(exp[1][0]) == n and int(exp[2][0]) == n
    assert run_case(eng, R, S, 4, 4, mode)[0] == 1


def special_key_sides(value, where, setting):
    """the special key in R only, in S only or in both; "among": 5,000 ordinary keys per side, 4,000 of them shared; "alone": no
    other key where both sides hold it, else one shared ordinary key and one ordinary key per side"""
    rng = np.random.default_rng(5)
    if setting == "among":
        pool = np.unique(rng.integers(1, 1 << 62, 6_100, dtype=np.uint64))[:6_000]
        pool = rng.permutation(pool)
        oR, oS = pool[:5_000], pool[1_000:]
    elif where == "both":
        oR = oS = np.zeros(0, dtype=np.uint64)
    else:
        oR, oS = np.array([11, 22, 22, 11], dtype=np.uint64), np.array([11, 33, 11], dtype=np.uint64)
    sp = np.full(7, value, dtype=np.uint64)
    vR = np.concatenate([oR, sp[:5]]) if where in ("R", "both") else oR
    vS = np.concatenate([oS, sp]) if where in ("S", "both") else oS
    return Side(rng.permutation(vR), col_seed=1), Side(rng.permutation(vS), col_seed=2)


@pytest.mark.parametrize("opts", [None, Opts(1, 4, 0), Opts(0, 0, 0)], ids=["auto", "one-pass", "unpartitioned"])
@pytest.mark.parametrize("setting", ["alone", "among"])
@pytest.mark.parametrize("where", ["R", "S", "both"])
@pytest.mark.parametrize("value", [MASK64, unmix64(MASK64)], ids=["all-ones", "all-ones-mixed"])
def test_the_all_ones_key(eng, value, where, setting, opts):
    R, S = special_key_sides(value, where, setting)
    eng.set_option("partition.narrow", -1)
    for mode in MODES:
        exp = oracle(R.oracle, S.oracle, mode, 1, 1)
        assert len(exp[0]) > 0
        assert (np.uint64(value) in exp[0]) == (where == "both" or (where == "R" and mode == GJ_LEFT))
        run_case(eng, R, S, 1, 1, mode, opts=opts)


# ---- more distinct keys of R than a table: the class walk ----------------------------------------------------------------------
def beyond_a_table(case):
    """(Side R, Side S, opts): R's distinct keys, more than a table takes in one partition; S holds half of them twice each plus
    10,000 foreign keys"""
    rng = np.random.default_rng(40)
    if case == "unpartitioned":                                            # 80,000 distinct values in the one partition
        keys, opts = rng.permutation(np.arange(1, 320_000, 4, dtype=np.uint64)), Opts(0, 0, 0)
        foreign = np.arange(2, 40_000, 4, dtype=np.uint64)
    else:                                                                  # the mix defeated: 20,000 values whose mix64 ends in sixteen
        keys = np.array([unmix64(k << 16) for k in range(1, 20_001)], dtype=np.uint64)[rng.permutation(20_000)]   # zero bits
        foreign = np.concatenate([np.array([unmix64(k << 16) for k in range(20_001, 25_001)], dtype=np.uint64),    # ... same partition
                                  rng.integers(1, 1 << 62, 5_000, dtype=np.uint64)])
        opts = Opts(2, 8, 8)
    assert len(foreign) == 10_000 and len(np.intersect1d(keys, foreign)) == 0
    half = keys[: len(keys) // 2]
    vS = rng.permutation(np.concatenate([half, half, foreign]))
    return Side(keys, col_seed=1), Side(vS, col_seed=2), opts


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("nc", [(4, 4), (0, 0)], ids=["c44", "c00"])
@pytest.mark.parametrize("case", ["unpartitioned", "one-partition-of-65536"])
def test_more_distinct_keys_than_a_table(eng, inputs, case, nc, mode):
    R, S, opts = beyond_a_table(case)
    assert len(R.oracle[0]) > 4 * AGG_FILL and has_both_kinds_of_lonely_keys(R, S)
    eng.set_option("partition.narrow", -1)
    assert eng.info("partition.mix") == 1
    _, rounds, _ = run_case(eng, R, S, nc[0], nc[1], mode, opts=opts)     # (capacity: exactly enough)
    # 20,000 keys of R or more in one partition over tables of 4608: at least 5 leaves, hence 9 builds of the binary walk
    assert rounds >= 9
    r, s = inputs("quarter", 3_000)                                        # ... and one table again
    assert run_case(eng, r, s, nc[0], nc[1], mode)[1] == 1


# ---- capacity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("n", [3_000, 70_000, 80_000], ids=["3000", "70000", "classes"])
def test_capacity(eng, inputs, n, mode):
    if n == 80_000:
        R, S, opts = beyond_a_table("unpartitioned")
        rng = np.random.default_rng(8)
        R = Side(R.v, rng.permutation(R.n).astype(np.uint64), R.cols)
        S = Side(S.v, rng.permutation(S.n).astype(np.uint64), S.cols)
    else:
        (R, S), opts = inputs("quarter", n, True), None
    exp = oracle(R.oracle, S.oracle, mode, 4, 4)
    G = len(exp[0])
    eng.set_option("partition.narrow", -1)
    dev = Device(eng, R, S)
    try:
        # count only: NULL outputs; then the columns given with colR_rows = colS_rows = 0 and real ids -- a column read would be refused
        assert eng.group_join_cols_dev(dev.vR, dev.iR, R.n, dev.vS, dev.iS, S.n, mode=mode, opts=opts) == G
        assert eng.group_join_cols_dev(dev.vR, dev.iR, R.n, dev.vS, dev.iS, S.n, dev.cR, 0, dev.cS, 0, mode, opts=opts) == G
        out = Outputs(eng, G - 1, 4, 4)
        with pytest.raises(RhjError) as err:
            call(eng, dev, R, S, 4, 4, mode, out, opts)
        assert err.value.code == RHJ_E_OVERFLOW
        groups = call(eng, dev, R, S, 4, 4, mode, out, opts, allow_overflow=True)
        assert groups == G                                                 # the exact count
        got = out.read(groups)                                             # (asserts the guard words behind every array)
        out.free()
        assert len(got[0]) == G - 1 and len(np.unique(got[0])) == G - 1    # complete, distinct groups of the result
        pos = np.searchsorted(exp[0], got[0])
        same(got, (exp[0][pos], exp[1][pos], exp[2][pos], [s[pos] for s in exp[3]], [s[pos] for s in exp[4]]))
        out = Outputs(eng, G, 4, 4, cntR=False, cntS=False)                # exactly enough; no count arrays
        assert call(eng, dev, R, S, 4, 4, mode, out, opts) == G
        got = out.read(G)
        out.free()
        assert got[1] is None and got[2] is None
        same(got, exp)
    finally:
        dev.free()


# ---- the repeats inside a call -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_count_free_overflow_repeats_with_exact_cursors(inputs, mode):
    n = 3_000_000
    R0, S = inputs("quarter", n)
    v = R0.v.copy()
    v[np.random.default_rng(3).permutation(n)[: n // 4]] = v[0]            # one value on a quarter of R's rows: no count-free region holds it
    R = Side(v, cols=R0.cols[:1])
    e = Engine(0)
    try:
        e.set_option("partition.narrow", 2)
        e.set_option("partition.countfree", 1)
        run_case(e, R, S, 1, 1, mode, opts=PLAN)
    finally:
        e.close()


def test_a_count_free_overflow_is_reported():
    """what the case above relies on, asked of the call alone (run_case's cross-checks run other calls behind it)"""
    n = 3_000_000
    vR, vS = make_sides("quarter", n)
    vR[np.random.default_rng(3).permutation(n)[: n // 4]] = vR[0]
    e = Engine(0)
    try:
        e.set_option("partition.narrow", 2)
        e.set_option("partition.countfree", 1)
        dR, dS = e.to_device(vR), e.to_device(vS)
        exp = len(np.intersect1d(vR, vS))
        assert e.group_join_cols_dev(dR, None, n, dS, None, n, opts=PLAN) == exp
        print(f"countfree R {e.info('last.countfree_R')} S {e.info('last.countfree_S')}")
        assert e.info("last.narrow") == 2 and e.info("last.countfree_R") == 2 and e.info("last.join_kernel") == JK_GJOIN
    finally:
        e.close()


@pytest.mark.parametrize("side", ["R", "S"])
def test_one_wide_id_repeats_at_sixteen_bytes_for_that_call_only(inputs, side):
    n = 90_000
    vR, vS = make_sides("quarter", n, seed=9)
    ids = np.arange(n, dtype=np.uint64)
    wide = ids.copy()
    wide[n // 3] = np.uint64(1 << 32)
    e = Engine(0)
    try:
        e.set_option("partition.narrow", 2)                                # set once, never re-armed below
        for rid, narrow in ((ids, 2), (wide, 0), (ids, 2)):
            R = Side(vR, rid if side == "R" else ids, cols=[])
            S = Side(vS, rid if side == "S" else ids, cols=[])
            for mode in MODES:
                exp = oracle(R.oracle, S.oracle, mode, 0, 0)
                dev, out = Device(e, R, S), Outputs(e, len(exp[0]), 0, 0)
                groups = e.group_join_cols_dev(dev.vR, dev.iR, n, dev.vS, dev.iS, n, (), 0, (), 0, mode, out.keys, out.cntR, out.cntS,
                                               (), (), out.cap, opts=PLAN)    # no column: the ids travel all the same
                same(out.read(groups), exp)
                assert e.info("last.narrow") == narrow and e.info("last.join_kernel") == JK_GJOIN, (side, narrow)
                if narrow:
                    assert e.info("last.cols_R") == 1 and e.info("last.cols_S") == 1
                dev.free()
                out.free()
    finally:
        e.close()


# ---- the row guards ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("side", ["R", "S"])
@pytest.mark.parametrize("n", [3_000, 70_000])
def test_a_row_at_col_rows_is_refused_and_the_context_goes_on(eng, inputs, n, side, mode):
    R, S = inputs("quarter", n, True)
    shared = np.intersect1d(R.oracle[0], S.oracle[0])[3]                   # a key both sides hold: every mode sums over its tuples
    bad_side = R if side == "R" else S
    bad = bad_side.ids.copy()
    bad[int(np.flatnonzero(bad_side.v == shared)[0])] = np.uint64(n)       # == colR_rows / colS_rows
    eng.set_option("partition.narrow", -1)
    dev, out = Device(eng, R, S), Outputs(eng, n, 1, 1)
    db = eng.to_device(bad)
    iR, iS = (db, dev.iS) if side == "R" else (dev.iR, db)
    G = len(oracle(R.oracle, S.oracle, mode, 0, 0)[0])
    try:
        with pytest.raises(RhjError) as err:
            eng.group_join_cols_dev(dev.vR, iR, n, dev.vS, iS, n, dev.cR[:1], n, dev.cS[:1], n, mode, out.keys, out.cntR, out.cntS,
                                    out.sumsR, out.sumsS, out.cap)
        assert err.value.code == RHJ_E_INVALID and f"a rowID of {side} " in str(err.value)
        # the other side's columns alone: that row is not looked at; no column, and count only: no guard
        cR, cS = ((), dev.cS[:1]) if side == "R" else (dev.cR[:1], ())
        sR, sS = ((), out.sumsS) if side == "R" else (out.sumsR, ())
        assert eng.group_join_cols_dev(dev.vR, iR, n, dev.vS, iS, n, cR, n, cS, n, mode, out.keys, out.cntR, out.cntS, sR, sS, out.cap) == G
        assert eng.group_join_cols_dev(dev.vR, iR, n, dev.vS, iS, n, (), 0, (), 0, mode, out.keys, out.cntR, out.cntS, (), (), out.cap) == G
        assert eng.group_join_cols_dev(dev.vR, iR, n, dev.vS, iS, n, dev.cR[:1], n, dev.cS[:1], n, mode) == G
        run_case(eng, R, S, 1, 1, mode, dev=dev)                           # a valid call on the same context is exact
    finally:
        db.free()
        dev.free()
        out.free()


# ---- edges -------------------------------------------------------------------------------------------------------------------
def test_empty_sides(eng, inputs):
    R, S = inputs("quarter", 3_000, True)
    dev, out = Device(eng, R, S), Outputs(eng, 3_000, 2, 2)
    args = (out.keys, out.cntR, out.cntS, out.sumsR, out.sumsS, out.cap)
    try:
        for mode in MODES:                                                 # nR == 0: nothing, no launch
            assert eng.group_join_cols_dev(None, None, 0, dev.vS, dev.iS, S.n, dev.cR[:2], 0, dev.cS[:2], S.n, mode, *args) == 0
            assert eng.info("last.join_kernel") == -1 and eng.info("last.group_rounds") == 0 and eng.timings()["ntasks"] == 0
            assert eng.group_join_cols_dev(None, None, 0, None, None, 0, mode=mode) == 0
            assert eng.group_join_dev(None, 0, None, 0, mode=mode) == 0
        assert eng.group_join_cols_dev(dev.vR, dev.iR, R.n, None, None, 0, dev.cR[:2], R.n, dev.cS[:2], 0, GJ_INNER, *args) == 0
        assert eng.info("last.join_kernel") == -1 and eng.timings()["ntasks"] == 0
        assert len(out.read(0)[0]) == 0                                    # (nothing was written anywhere)
        # nS == 0 under LEFT: the group-by of R with zero S fields
        empty = Side(np.zeros(0, dtype=np.uint64), cols=S.cols)
        exp = oracle(R.oracle, empty.oracle, GJ_LEFT, 2, 2)
        for opts in (None, Opts(1, 4, 0)):
            groups = eng.group_join_cols_dev(dev.vR, dev.iR, R.n, None, None, 0, dev.cR[:2], R.n, dev.cS[:2], 0, GJ_LEFT, *args, opts=opts)
            assert groups == len(R.oracle[0]) and eng.info("last.join_kernel") == JK_GJOIN
            got = out.read(groups)
            same(got, exp)
            assert not got[2].any() and not got[4][0].any() and not got[4][1].any()
        tR = np.empty(R.n, dtype=TUPLE)
        tR["key"], tR["payload"] = R.ids, R.v
        dR = eng.to_device(tR)
        groups = eng.group_join_dev(dR, R.n, None, 0, dev.cR[:2], R.n, dev.cS[:2], 0, GJ_LEFT, *args)
        same(out.read(groups), exp)
        dR.free()
    finally:
        dev.free()
        out.free()


@pytest.mark.parametrize("a,b", [(7, 7), (7, 8), (MASK64, MASK64), (0, MASK64), (0, 0)])
def test_one_row_per_side(eng, a, b):
    R, S = Side(np.array([a], dtype=np.uint64), col_seed=1), Side(np.array([b], dtype=np.uint64), col_seed=2)
    dev = Device(eng, R, S)
    try:
        for mode in MODES:
            exp = oracle(R.oracle, S.oracle, mode, 2, 2)
            assert len(exp[0]) == (1 if a == b or mode == GJ_LEFT else 0)
            groups, rounds, _ = run_case(eng, R, S, 2, 2, mode, dev=dev)
            assert rounds == (1 if groups or mode == GJ_LEFT else rounds)
    finally:
        dev.free()
    dk = eng.to_device(np.arange(10, dtype=np.uint64))
    assert eng.join_sum_cols_dev(dk, None, 10, dk, 10)[0] == 10
    assert eng.info("last.group_rounds") == 0                              # ... and 0 after a call that is neither
    dk.free()


def test_invalid_arguments(eng):
    n = 100
    v = np.arange(n, dtype=np.uint64)
    T = np.empty(n, dtype=TUPLE)
    T["key"], T["payload"] = v, v
    dv, dT, dc, dk, ds = eng.to_device(v), eng.to_device(T), eng.to_device(v), eng.alloc(8 * n), eng.alloc(8 * n)
    cols = (C.c_void_p * 5)(*[dc.ptr] * 5)
    sums = (C.c_void_p * 5)(*[ds.ptr] * 5)
    holes = (C.c_void_p * 5)(dc.ptr, None, dc.ptr, dc.ptr, dc.ptr)
    g = C.c_uint64()
    lib, ctx = eng.lib, eng.ctx
    K = dict(valR=None, valS=None, nR=n, nS=n, cR=cols, ncR=1, cS=cols, ncS=1, mode=GJ_INNER, keys=dk.ptr, sR=sums, sS=sums, cap=n, og=g)

    def cols_call(**kw):
        a = dict(K, valR=dv.ptr, valS=dv.ptr)
        a.update(kw)
        return lib.rhj_group_join_cols_dev(ctx, a["valR"], None, a["nR"], a["valS"], None, a["nS"], a["cR"], a["ncR"], n, a["cS"], a["ncS"], n,
                                           a["mode"], None, a["keys"], None, None, a["sR"], a["sS"], a["cap"],
                                           C.byref(a["og"]) if a["og"] is not None else None)

    def aos_call(**kw):
        a = dict(K, valR=dT.ptr, valS=dT.ptr)
        a.update(kw)
        return lib.rhj_group_join_dev(ctx, a["valR"], a["nR"], a["valS"], a["nS"], a["cR"], a["ncR"], n, a["cS"], a["ncS"], n, a["mode"],
                                      None, a["keys"], None, None, a["sR"], a["sS"], a["cap"], C.byref(a["og"]) if a["og"] is not None else None)
    for f in (cols_call, aos_call):
        assert f(mode=2) == RHJ_E_INVALID and f(mode=-1) == RHJ_E_INVALID                       # an unknown mode
        for s in ("R", "S"):
            assert f(**{"nc" + s: GROUP_JOIN_MAX_COLS + 1}) == RHJ_E_INVALID                    # too many columns
            assert f(**{"nc" + s: GROUP_JOIN_MAX_COLS + 1}, keys=None, cap=0) == RHJ_E_INVALID  # ... also when only counting
            assert f(**{"c" + s: None}) == RHJ_E_INVALID                                        # NULL d_cols*
            assert f(**{"s" + s: None}) == RHJ_E_INVALID                                        # NULL d_out_sums*
            assert f(**{"c" + s: holes, "nc" + s: 2}) == RHJ_E_INVALID                          # a NULL column
            assert f(**{"s" + s: holes, "nc" + s: 2}) == RHJ_E_INVALID                          # a NULL sum column
            assert f(**{"val" + s: None}) == RHJ_E_INVALID                                      # NULL values with rows
        assert f(og=None) == RHJ_E_INVALID                                                      # NULL out_groups
        assert f(keys=None) == RHJ_E_INVALID                                                    # NULL d_out_keys with capacity
        assert f(cR=None, cS=None, sR=None, sS=None, keys=None, cap=0) == 0 and g.value == n    # count only: no column array is read
        assert f(ncR=4, ncS=4) == 0 and g.value == n
        assert f(mode=GJ_LEFT, ncR=0, ncS=0, cR=None, cS=None, sR=None, sS=None) == 0 and g.value == n
    with pytest.raises(RhjError) as err:
        eng.group_join_cols_dev(dv, None, n, dv, None, n, opts=Opts(3, 0, 0))
    assert err.value.code == RHJ_E_INVALID
    with pytest.raises(RhjError) as err:
        eng.group_join_cols_dev(dv, None, n, dv, None, n, [dc], n, (), 0, GJ_INNER, dk, None, None, (), (), n)   # one column, no sum column
    assert err.value.code == RHJ_E_INVALID
    for b in (dv, dT, dc, dk, ds):
        b.free()


# ---- Engine.join_group_by_columns --------------------------------------------------------------------------------------------
def sql_reference(kR, kS, wR, wS, how):
    """SELECT key, COUNT(*), SUM(r.w).., SUM(s.w).. FROM R [LEFT] JOIN S USING (key) GROUP BY key by torch.unique per side, an
    intersection or a left lookup by numpy, and wrapping int64 products"""
    uR, invR, cR = torch.unique(kR, return_inverse=True, return_counts=True)
    uS, invS, cS = torch.unique(kS, return_inverse=True, return_counts=True)
    sR = [torch.zeros_like(uR).index_add_(0, invR, x) for x in wR]
    sS = [torch.zeros_like(uS).index_add_(0, invS, x) for x in wS]
    nR, nS = uR.cpu().numpy(), uS.cpu().numpy()
    cR, cS = cR.cpu().numpy(), cS.cpu().numpy()
    sR, sS = [x.cpu().numpy() for x in sR], [x.cpu().numpy() for x in sS]
    with np.errstate(over="ignore"):
        if how == "inner":
            keys, iR, iS = np.intersect1d(nR, nS, return_indices=True)
            return keys, cR[iR] * cS[iS], [x[iR] * cS[iS] for x in sR], [x[iS] * cR[iR] for x in sS]
        if len(nS) == 0:                                                   # every row of R unmatched: counted once, NULLs for S
            return nR, cR, sR, [np.zeros(len(nR), dtype=np.int64) for _ in sS]
        pos = np.minimum(np.searchsorted(nS, nR), len(nS) - 1)
        hit = nS[pos] == nR
        mS = np.where(hit, cS[pos], 1)
        return nR, cR * mS, [x * mS for x in sR], [np.where(hit, x[pos] * cR, 0) for x in sS]


def check_sql(got, exp, nwR, nwS):
    keys, count, sums_R, sums_S = got
    assert keys.dtype == count.dtype == torch.int64 and len(sums_R) == nwR and len(sums_S) == nwS
    order = torch.argsort(keys).cpu().numpy()
    pick = lambda t: t.cpu().numpy()[order]
    assert np.array_equal(pick(keys), exp[0]) and np.array_equal(pick(count), exp[1])
    for j in range(nwR):
        assert sums_R[j].dtype == torch.int64 and np.array_equal(pick(sums_R[j]), exp[2][j]), j
    for j in range(nwS):
        assert sums_S[j].dtype == torch.int64 and np.array_equal(pick(sums_S[j]), exp[3][j]), j


def sql_inputs(n):
    rng = np.random.default_rng(n)
    D = max(n // 5, 4)
    pool = rng.integers(-(1 << 62), 1 << 62, D + D // 4, dtype=np.int64)
    kR = pool[rng.integers(0, D, n)]                                       # R: the first D keys; S: all but the first D / 4, and D / 4 more
    kS = pool[rng.integers(D // 4, len(pool), n + n // 3)]
    kR[0], kR[1], kR[2] = -1, np.iinfo(np.int64).min, 0                    # (-1: the all-ones word)
    kS[0], kS[1] = -1, 0
    wR = [rng.integers(-(1 << 63), (1 << 63) - 1, len(kR), dtype=np.int64) for _ in range(3)]
    wS = [rng.integers(-(1 << 63), (1 << 63) - 1, len(kS), dtype=np.int64) for _ in range(2)]
    return kR, kS, wR, wS


@pytest.mark.parametrize("how", ["inner", "left"])
@pytest.mark.parametrize("n", [1_000, 300_000])
def test_join_group_by_columns_against_torch(n, how):
    kR, kS, wR, wS = sql_inputs(n)
    assert len(np.setdiff1d(kR, kS)) > 0 and len(np.setdiff1d(kS, kR)) > 0 and len(np.intersect1d(kR, kS)) > 0
    e = Engine(0)
    try:
        tR, tS = torch.from_numpy(kR).cuda(), torch.from_numpy(kS).cuda()
        twR, twS = [torch.from_numpy(x).cuda() for x in wR], [torch.from_numpy(x).cuda() for x in wS]
        for nwR, nwS in ((0, 0), (3, 2), (1, 0), (0, 1)):
            got = e.join_group_by_columns(tR, tS, twR[:nwR], twS[:nwS], how=how)
            assert got[0].device == tR.device
            check_sql(got, sql_reference(tR, tS, twR[:nwR], twS[:nwS], how), nwR, nwS)
        z = tR[:0].contiguous()
        keys, count, sums_R, sums_S = e.join_group_by_columns(z, tS, [z], [twS[0]], how=how)
        assert keys.shape == count.shape == sums_R[0].shape == sums_S[0].shape == (0,)
        zS = tS[:0].contiguous()
        got = e.join_group_by_columns(tR, zS, twR[:1], [zS], how=how)      # an empty S: nothing, or R's group-by with zero S sums
        check_sql(got, sql_reference(tR, zS, twR[:1], [zS], how), 1, 1)
        assert len(got[0]) == (0 if how == "inner" else len(np.unique(kR)))
    finally:
        e.close()


def test_join_group_by_columns_refuses_what_it_cannot_read():
    e = Engine(0)
    try:
        good = torch.arange(100, device="cuda", dtype=torch.int64)
        for bad in (good.to(torch.int32), good.to(torch.float64), torch.arange(200, device="cuda")[::2], good.cpu(),
                    good.reshape(10, 10), list(range(5))):
            for args in ((bad, good), (good, bad), (good, good, [bad]), (good, good, (), [bad])):
                with pytest.raises(ValueError):
                    e.join_group_by_columns(*args)
        short = good[:50].contiguous()
        for args in ((good, short, [short]), (good, short, (), [good]), (good, good, [good] * (GROUP_JOIN_MAX_COLS + 1)),
                     (good, good, (), [good] * (GROUP_JOIN_MAX_COLS + 1))):
            with pytest.raises(ValueError):
                e.join_group_by_columns(*args)
        with pytest.raises(ValueError):
            e.join_group_by_columns(good, good, how="outer")
        keys, count, sums_R, sums_S = e.join_group_by_columns(good, short, [good], [short])
        order = torch.argsort(keys)
        assert torch.equal(keys[order], short) and bool((count == 1).all())
        assert torch.equal(sums_R[0][order], short) and torch.equal(sums_S[0][order], short)
    finally:
        e.close()


def test_join_group_by_columns_is_ordered_behind_queued_torch_work():
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
            kR = filler[:n].clone() >> 3                                   # (a few rows per key)
            kS = filler[n // 2: n // 2 + n].clone() >> 3                   # ... half of them shared
            wR, wS = filler[F - n:].clone(), filler[F - 2 * n: F - n].clone()
            got = e.join_group_by_columns(kR, kS, [wR], [wS], how="left")
        torch.cuda.synchronize()
        x = [np.arange(n, dtype=np.uint64), np.arange(n // 2, n // 2 + n, dtype=np.uint64), np.arange(F - n, F, dtype=np.uint64),
             np.arange(F - 2 * n, F - n, dtype=np.uint64)]
        with np.errstate(over="ignore"):
            for _ in range(rounds):
                x = [a * np.uint64(3) + np.uint64(1) for a in x]
        t = lambda a: torch.from_numpy(a.view(np.int64).copy())
        exp = sql_reference(t(x[0]) >> 3, t(x[1]) >> 3, [t(x[2])], [t(x[3])], "left")
        check_sql(got, exp, 1, 1)
        assert e.bound_stream is None
    finally:
        e.close()
