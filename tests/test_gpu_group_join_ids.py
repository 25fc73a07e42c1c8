"""GPU suite: the group of every row of either side of a group-by join, rhj_group_join_agg_ids_cols_dev / rhj_group_join_agg_ids_dev
(include/rhj.h) and Engine.join_group_by_columns_with_inverse: the group-by join's outputs and, per tuple of R and of S,
the index of its group in them -- all ones where the tuple's value has none.

The oracle is numpy only (test_gpu_group_join_agg.oracle: np.unique, intersect1d, searchsorted, reduceat).  Ids are checked against
the call's OWN outputs: the rows whose value is among the oracle's keys have ids below the group count with keys[gid] == v on both
sides, cntR / cntS are the bincounts of those ids, every other word is all ones, the guard words behind both arrays stand, and the
sorted outputs equal the oracle.  Every case runs twice and is checked twice.
  * RHJ_GJ_INNER and RHJ_GJ_LEFT over partial overlap (a third of R's keys absent from S, half of S's absent from R, duplicates on
    both sides) on the three paths, NULL and permuted ids; columns on both sides with mixed ops against the _agg_ entry;
  * 70,000 x 300 one pass: most partitions get no task under INNER; nS == 0 in both modes; nR == 0; either pointer alone;
  * the class walk over R with every fourth of its values twice in S; the all-ones key on both sides, on R only, on S only;
  * the row guard on each side; join_group_by_columns_with_inverse against a numpy restatement."""
import numpy as np
import pytest
import torch

from group_ids_cases import NO_GROUP, IdArray, check_ids, raw
from radixhashjoin_amd import AGG_MAX_U64, AGG_MIN_I64, AGG_MIN_U64, AGG_SUM, GJ_INNER, GJ_LEFT, Engine, Opts, RhjError, unmix64
from radixhashjoin_amd.binding import RHJ_E_INVALID
from test_gpu_group_join import Device, Outputs, same
from test_gpu_group_join_agg import MODE_IDS, MODES, ONE_PASS, SIZE_IDS, SIZES, Side, make_sides, oracle
from test_gpu_group_sum import beyond_a_table

pytestmark = pytest.mark.gpu
JK_GJOIN = 16
MASK64 = (1 << 64) - 1
OPS_R = [AGG_MIN_I64, AGG_SUM]
OPS_S = [AGG_MAX_U64, AGG_MIN_U64, AGG_SUM]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def inputs():
    cache = {}

    def get(nR, nS, ids=False):
        if (nR, nS, ids) not in cache:
            cache[(nR, nS, ids)] = make_sides(nR, nS, ids)
        return cache[(nR, nS, ids)]
    return get


def call(eng, dev, R, S, opsR, opsS, mode, out, gR, gS, opts=None, iR=None, iS=None):
    iR, iS = dev.iR if iR is None else iR, dev.iS if iS is None else iS
    return eng.group_join_agg_ids_cols_dev(dev.vR, iR, R.n, dev.vS, iS, S.n, dev.cR[:len(opsR)], opsR, len(R.cols[0]),
                                           dev.cS[:len(opsS)], opsS, len(S.cols[0]), mode, out.keys, out.cntR, out.cntS, out.sumsR,
                                           out.sumsS, out.cap, gR.buf if gR else None, gR.rows if gR else 0, gS.buf if gS else None,
                                           gS.rows if gS else 0, opts=opts)


def check_side(g, side, group_keys, keys, cnt, groups, name):
    """the rows of `side` whose value is among the oracle's keys carry their group; every other word of the array is all ones"""
    has = np.isin(side.v, group_keys)
    print(f"{name}: {int(has.sum())} of {side.n} rows have a group")
    check_ids(g, side.rows[has], side.v[has], keys, cnt, groups)
    rest = np.ones(len(g), dtype=bool)
    rest[side.rows[has]] = False
    assert (g[rest] == NO_GROUP).all(), f"{name}: a word without a group is not all ones"
    return int(has.sum())


def run_ids(eng, R, S, opsR, opsS, mode, opts=None, dev=None, sides="RS"):
    """the columnar entry with ids, capacity = the number of groups, twice; returns (groups, rows of R with a group, rows of S with one)"""
    exp = oracle(R, S, mode, opsR, opsS)
    G = len(exp[0])
    own = dev is None
    dev = Device(eng, R, S) if own else dev
    try:
        for _ in range(2):
            out = Outputs(eng, G, len(opsR), len(opsS))
            gR = IdArray(eng, R.n) if "R" in sides else None
            gS = IdArray(eng, S.n) if "S" in sides and S.n else None
            try:
                groups = call(eng, dev, R, S, opsR, opsS, mode, out, gR, gS, opts)
                print(f"nR {R.n} nS {S.n} mode {mode} groups {groups} kernel {eng.info('last.join_kernel')} rounds "
                      f"{eng.info('last.group_rounds')} narrow {eng.info('last.narrow')} tasks {eng.timings()['ntasks']}")
                assert groups == G
                same(out.read(groups), exp)
                keys = raw(out.keys, groups)
                hasR = check_side(gR.read(), R, exp[0], keys, raw(out.cntR, groups), groups, "R") if gR else -1
                hasS = check_side(gS.read(), S, exp[0], keys, raw(out.cntS, groups), groups, "S") if gS else -1
                if mode == GJ_LEFT:
                    assert hasR in (-1, R.n)                               # under LEFT every row of R has a group
                assert eng.info("last.join_kernel") == JK_GJOIN and eng.info("last.semi_tables") == 0
            finally:
                out.free()
                for g in (gR, gS):
                    if g:
                        g.free()
    finally:
        if own:
            dev.free()
    return G, hasR, hasS


# ---- modes and overlap -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("ids", [False, True], ids=["null", "ids"])
@pytest.mark.parametrize("nR,nS,opts,narrow", SIZES, ids=SIZE_IDS)
def test_paths_by_size_in_both_modes(eng, inputs, nR, nS, opts, narrow, ids, mode):
    R, S = inputs(nR, nS, ids)
    eng.set_option("partition.narrow", narrow)
    if narrow == 2:
        eng.set_option("partition.countfree", 0)
    try:
        G, hasR, hasS = run_ids(eng, R, S, [], [], mode, opts=opts)
        assert eng.timings()["passes"] == (0 if nR == 3_000 else 1 if narrow != 2 else 2) and eng.info("last.narrow") == max(narrow, 0)
        assert eng.info("last.group_rounds") == 1
        assert 0 < hasS < S.n and (hasR == R.n if mode == GJ_LEFT else 0 < hasR < R.n)   # rows without a partner on either side
    finally:
        eng.set_option("partition.narrow", -1)
        eng.set_option("partition.countfree", -1)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("nR,nS,opts,narrow", SIZES, ids=SIZE_IDS)
def test_columns_on_both_sides_with_mixed_ops(eng, inputs, nR, nS, opts, narrow, mode):
    """the id sweeps follow the last op sweep of S; the outputs are the _agg_ entry's"""
    R, S = inputs(nR, nS, True)
    eng.set_option("partition.narrow", narrow)
    dev = Device(eng, R, S)
    try:
        G, _, _ = run_ids(eng, R, S, OPS_R, OPS_S, mode, opts=opts, dev=dev)
        a, b = Outputs(eng, G, 2, 3), Outputs(eng, G, 2, 3)
        gR, gS = IdArray(eng, nR), IdArray(eng, nS)
        try:
            assert eng.group_join_agg_cols_dev(dev.vR, dev.iR, nR, dev.vS, dev.iS, nS, dev.cR[:2], OPS_R, nR, dev.cS[:3], OPS_S, nS, mode,
                                               a.keys, a.cntR, a.cntS, a.sumsR, a.sumsS, a.cap, opts=opts) == G
            assert call(eng, dev, R, S, OPS_R, OPS_S, mode, b, gR, gS, opts) == G
            same(b.read(G), a.read(G))
            assert call(eng, dev, R, S, OPS_R, OPS_S, mode, b, None, None, opts) == G     # both pointers NULL: the _agg_ entry
            same(b.read(G), a.read(G))
        finally:
            for x in (a, b, gR, gS):
                x.free()
    finally:
        eng.set_option("partition.narrow", -1)
        dev.free()


# ---- partitions without a task, empty sides, one pointer ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_few_tuples_of_s(eng, mode):
    """70,000 x 300 in 32 partitions: under INNER the rows of R in a partition S has nothing in are never seen by the kernel"""
    rng = np.random.default_rng(17)
    pool = np.unique(rng.integers(1, 1 << 63, 18_000, dtype=np.uint64))[:17_500]
    R = Side(pool[rng.integers(0, len(pool), 70_000)], ncols=1)
    few = np.unique(R.v)[:4]                                               # S: four of R's values and foreign ones, 300 tuples
    S = Side(np.concatenate([few[rng.integers(0, 4, 200)], rng.integers(1 << 63, 1 << 64, 100, dtype=np.uint64)]), ncols=1)
    eng.set_option("partition.narrow", -1)
    G, hasR, hasS = run_ids(eng, R, S, [], [], mode, opts=ONE_PASS)
    assert eng.timings()["passes"] == 1 and hasS == 200
    if mode == GJ_INNER:
        assert G == 4 and 0 < hasR < 100 and eng.timings()["ntasks"] <= 32
    run_ids(eng, R, S, [AGG_MIN_I64], [AGG_SUM], mode, opts=ONE_PASS)


def test_an_empty_s(eng, inputs):
    R, _ = inputs(3_000, 3_000, True)
    S = Side(np.zeros(0, dtype=np.uint64), ncols=1)
    dev = Device(eng, R, S)
    try:
        for _ in range(2):
            out, gR, gS = Outputs(eng, R.n, 0, 0), IdArray(eng, R.n), IdArray(eng, 5)
            launches = eng.timings()["ntasks"]
            assert call(eng, dev, R, S, [], [], GJ_INNER, out, gR, gS) == 0  # INNER: 0 groups, no launch, and still "no group" everywhere
            assert eng.info("last.join_kernel") == -1 and eng.timings()["ntasks"] in (0, launches)
            assert (gR.read() == NO_GROUP).all() and (gS.read() == NO_GROUP).all()
            for x in (out, gR, gS):
                x.free()
        G, hasR, _ = run_ids(eng, R, S, [AGG_MIN_I64, AGG_SUM], [], GJ_LEFT, dev=dev)   # LEFT: the group-by of R with ids
        assert G == len(np.unique(R.v)) and hasR == R.n
        out, gS = Outputs(eng, 4, 0, 0), IdArray(eng, 7)
        assert eng.group_join_agg_ids_cols_dev(None, None, 0, dev.vR, dev.iR, R.n, d_out_keys=out.keys, capacity=4, d_out_gidS=gS.buf,
                                               gidS_rows=7) == 0           # nR == 0: nothing of S has a group
        assert (gS.read() == NO_GROUP).all()
        out.free()
        gS.free()
    finally:
        dev.free()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("sides", ["R", "S"])
def test_either_pointer_on_its_own(eng, inputs, sides, mode):
    R, S = inputs(70_000, 50_000, True)
    eng.set_option("partition.narrow", -1)
    run_ids(eng, R, S, [AGG_SUM], [AGG_MIN_U64], mode, opts=ONE_PASS, sides=sides)


# ---- the class walk and the all-ones key -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_the_class_walk(eng, mode):
    v, opts = beyond_a_table("two-bits")                                   # 100,000 distinct values over four partitions
    rng = np.random.default_rng(41)
    R = Side(v, ncols=1)
    S = Side(rng.permutation(np.concatenate([v[::4], v[::4]])), ncols=1)   # every fourth value of R, twice
    eng.set_option("partition.narrow", -1)
    G, hasR, hasS = run_ids(eng, R, S, [], [], mode, opts=opts)
    assert eng.info("last.group_rounds") >= 9                              # 25,000 keys of R per partition over tables of 4608
    assert hasS == S.n and hasR == (R.n if mode == GJ_LEFT else R.n // 4)
    run_ids(eng, R, S, [AGG_MIN_I64], [AGG_SUM], mode, opts=opts)
    assert eng.info("last.group_rounds") >= 9


@pytest.mark.parametrize("opts", [None, Opts(0, 0, 0)], ids=["auto", "unpartitioned"])
@pytest.mark.parametrize("where", ["both", "R", "S"])
@pytest.mark.parametrize("value", [MASK64, unmix64(MASK64)], ids=["all-ones", "all-ones-mixed"])
def test_the_all_ones_key(eng, value, where, opts):
    """its id waits beside the table; where R lacks it, the word says "no group" and S's tuples store nothing"""
    rng = np.random.default_rng(5)
    pool = rng.permutation(np.unique(rng.integers(1, 1 << 62, 6_100, dtype=np.uint64))[:6_000])
    sp = np.full(7, value, dtype=np.uint64)
    vR = np.concatenate([pool[:5_000], sp[:5]]) if where in ("R", "both") else pool[:5_000]
    vS = np.concatenate([pool[1_000:], sp]) if where in ("S", "both") else pool[1_000:]
    R, S = Side(rng.permutation(vR), ncols=1), Side(rng.permutation(vS), ncols=1)
    eng.set_option("partition.narrow", -1)
    for mode in MODES:
        exp = oracle(R, S, mode, [], [])
        assert (np.uint64(value) in exp[0]) == (where == "both" or (where == "R" and mode == GJ_LEFT))
        run_ids(eng, R, S, [], [], mode, opts=opts)
        run_ids(eng, R, S, [AGG_MIN_I64], [AGG_MAX_U64], mode, opts=opts)


# ---- the row guard -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("side", ["R", "S"])
def test_the_row_guard_names_the_array(eng, inputs, side, mode):
    n = 3_000
    R, S = inputs(n, n, True)
    shared = np.intersect1d(R.v, S.v)[3]                                   # a key both sides hold: every mode sweeps its tuples
    bad_side = R if side == "R" else S
    bad = bad_side.ids.copy()
    bad[int(np.flatnonzero(bad_side.v == shared)[0])] = np.uint64(n)       # == gidR_rows / gidS_rows
    eng.set_option("partition.narrow", -1)
    dev, db = Device(eng, R, S), eng.to_device(bad)
    try:
        for _ in range(2):
            out, gR, gS = Outputs(eng, n, 0, 0), IdArray(eng, n), IdArray(eng, n)
            with pytest.raises(RhjError) as err:
                call(eng, dev, R, S, [], [], mode, out, gR, gS, iR=db if side == "R" else None, iS=db if side == "S" else None)
            assert err.value.code == RHJ_E_INVALID and f"a rowID of {side} " in str(err.value) and f"d_out_gid{side}" in str(err.value)
            gR.read()                                                      # the guard words behind both arrays are intact
            gS.read()
            for x in (out, gR, gS):
                x.free()
        run_ids(eng, R, S, OPS_R, OPS_S, mode, dev=dev)                    # a valid call on the same context is exact
    finally:
        db.free()
        dev.free()


# ---- Engine.join_group_by_columns_with_inverse -------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["inner", "left"])
@pytest.mark.parametrize("n", [1_000, 300_000])
def test_join_group_by_columns_with_inverse_against_numpy(n, how):
    rng = np.random.default_rng(n + 1)
    pool = rng.integers(-(1 << 62), 1 << 62, max(n // 4, 4), dtype=np.int64)
    pool[0], pool[1] = -1, np.iinfo(np.int64).min                          # negative keys; -1 is the all-ones word
    half = len(pool) // 2
    kR = pool[rng.integers(0, half + half // 2, n)]                        # the sides share the middle of the pool
    kS = pool[rng.integers(half // 2, len(pool), n // 2)]
    wR = rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64)
    e = Engine(0)
    try:
        tR, tS, tw = torch.from_numpy(kR).cuda(), torch.from_numpy(kS).cuda(), torch.from_numpy(wR).cuda()
        for _ in range(2):
            keys, count, sums_R, sums_S, (inv_R, inv_S) = e.join_group_by_columns_with_inverse(tR, tS, [tw], how=how)
            plain = e.join_group_by_columns(tR, tS, [tw], how=how)         # the entry without the inverse returns what it returned
            assert len(plain) == 4 and torch.equal(torch.sort(plain[0]).values, torch.sort(keys).values)
            assert inv_R.dtype == inv_S.dtype == torch.int64 and inv_R.shape == tR.shape and inv_S.shape == tS.shape
            gk, iR, iS = keys.cpu().numpy(), inv_R.cpu().numpy(), inv_S.cpu().numpy()
            want = np.intersect1d(kR, kS) if how == "inner" else np.unique(kR)
            assert np.array_equal(np.sort(gk), want)
            order = np.argsort(gk)                                         # sorted rank -> this call's group index
            for k, inv in ((kR, iR), (kS, iS)):
                pos = np.minimum(np.searchsorted(want, k), len(want) - 1)
                hit = want[pos] == k
                assert np.array_equal(inv[hit], order[pos[hit]]) and (inv[~hit] == -1).all()
                assert np.array_equal(gk[inv[hit]], k[hit])
            assert (iR >= 0).all() if how == "left" else (iR < 0).any()
            assert (iS < 0).any()
            cR, cS = np.bincount(iR[iR >= 0], minlength=len(gk)), np.bincount(iS[iS >= 0], minlength=len(gk))
            assert np.array_equal(count.cpu().numpy(), cR * (np.maximum(cS, 1) if how == "left" else cS))
        keys, count, sums_R, sums_S, (inv_R, inv_S) = e.join_group_by_columns_with_inverse(tR, tS[:0].contiguous(), how=how)
        assert inv_S.shape == (0,) and len(keys) == (0 if how == "inner" else len(np.unique(kR)))
        assert bool((inv_R == -1).all()) if how == "inner" else torch.equal(keys[inv_R], tR)
        keys, count, sums_R, sums_S, (inv_R, inv_S) = e.join_group_by_columns_with_inverse(tR[:0].contiguous(), tS, how=how)
        assert len(keys) == 0 and inv_R.shape == (0,) and bool((inv_S == -1).all())
    finally:
        e.close()
