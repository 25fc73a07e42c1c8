"""GPU suite: the outer-join entries rhj_outer_join_cols_dev / rhj_outer_join_dev (include/rhj.h) and Engine.outer_join_columns.

The oracle is numpy: a sort-merge join gives the matched pairs, ~np.isin(valR, valS) the rowIDs of R without a partner and the same
with the sides exchanged those of S.  Every case runs the three modes; what is checked of every result:
  * the sections are where the contract puts them: [0, matched) holds no NO_ROW and is the inner join's pair multiset, the second
    section holds {id, NO_ROW} only and exactly the unmatched ids of R, the third {NO_ROW, id} only and the unmatched ids of S;
  * total == the sum of the sections, a section the mode does not ask for is 0.
Cases:
  * paths by size: 3,000 rows per side (unpartitioned), 70,000 (one-pass automatic plan), 3,000,000 under Opts(2, 8, 8) in the narrow
    format; uniform, duplicate-heavy and Zipf 0.9 inputs with foreign values on both sides; NULL and explicit ids; the section counts
    against join_cols_dev and semi_join_cols_dev(ANTI) in both directions;
  * one value on 1,000 rows of each side (10^6 pairs) beside values repeated 1,000 times on one side only;
  * partitions of the table side far beyond one LDS table, in both sweep directions: "last.semi_tables" >= 2, then 1, then 0;
  * the all-ones join value (the table's empty marker) and unmix64 of it (the marker of a partitioned plan) on both sides, on R only, on
    S only; keys 0 and 1 << 63;
  * partitions without a tuple of the other side; disjoint sides; n = 0 and n = 1; invalid arguments;
  * the repeats inside a call: a count-free region that overflows, one rowID of 2^32 on either side in a narrow format;
  * count-only mode and buffers that end inside each section; the AoS entry;
  * outer_join_columns on int64 tensors: negative keys, empty tensors, refused tensors and modes, queued torch work, a bound stream."""
import numpy as np
import pytest
import torch

import cf_cases
from oracle.pyoracle import TUPLE
from radixhashjoin_amd import ANTI, NO_ROW, OUTER_FULL, OUTER_LEFT, OUTER_RIGHT, PAIR, Engine, Opts, RhjError
from radixhashjoin_amd.binding import RHJ_E_INVALID, RHJ_E_OVERFLOW, mix64, plan as resolve_plan, unmix64

pytestmark = pytest.mark.gpu
PLAN = Opts(2, 8, 8)
NO = np.uint64(NO_ROW)
SENTINEL = np.uint64(0x5A5A5A5A5A5A5A5A)
JK_SEMI = 12
MODES = (OUTER_LEFT, OUTER_RIGHT, OUTER_FULL)
SWEEPS = {OUTER_LEFT: 1, OUTER_RIGHT: 1, OUTER_FULL: 2}
SEMI_MAX_SPLIT = 32768                                       # tuples of the probed side per sweep task at most


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


# ---- input builders (those of test_gpu_semi_join.py, with foreign values on R's side too) --------------------------------------
def rel(rng, n, values):
    t = np.empty(n, dtype=TUPLE)
    t["key"] = rng.permutation(n).astype(np.uint64)
    t["payload"] = values
    return t


def zipf_ranks(rng, n, D, theta=0.9):
    e = 1.0 - theta
    span = (D + 1.0) ** e - 1.0
    r = np.floor((1.0 + rng.random(n) * span) ** (1.0 / e)).astype(np.int64)
    return np.clip(r, 1, D)


def make(dist, nR, nS, seed=0):
    """R values; S values sampled from R, every 97th made foreign; then every 89th value of R made foreign; ids a permutation"""
    rng = np.random.default_rng(nR * 31 + nS + seed)
    if dist == "dups":
        rv = rng.integers(1, 1 << 61, max(nR // 4, 1), dtype=np.uint64)[rng.integers(0, max(nR // 4, 1), nR)]
    else:
        rv = rng.integers(1, 1 << 61, nR, dtype=np.uint64)
    if dist == "zipf":
        sv = rv[zipf_ranks(rng, nS, nR) - 1]
    else:
        sv = rv[rng.integers(0, nR, nS)]
        if dist == "quarter":
            sv[rng.permutation(nS)[: nS // 4]] = rv[0]         # one value on a quarter of the rows: no count-free region holds it
    sv[::97] ^= np.uint64(1 << 62)
    rv[5::89] ^= np.uint64(1 << 61)                            # (rv[0], the heavy value of "quarter", keeps its partners)
    return rel(rng, nR, rv), rel(rng, nS, sv)


def with_ids(T, ids):
    if ids:
        return T
    t = T.copy()
    t["key"] = np.arange(len(T), dtype=np.uint64)
    return t


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def sort_pairs(p):
    if len(p) and max(int(p["keyR"].max()), int(p["keyS"].max())) < 1 << 32:         # one 64-bit sort key where the ids allow it
        return p[np.argsort((p["keyR"] << np.uint64(32)) | p["keyS"])]
    return p[np.lexsort((p["keyS"], p["keyR"]))]


class Expected:
    """sort-merge equi-join on .payload (both sides sorted once, sorted needles: a search with 3 * 10^6 unsorted ones takes seconds):
    .pairs the sorted (R.key, S.key) pairs, .r_only / .s_only the sorted rowIDs of the tuples whose value the other side lacks"""

    def __init__(self, R, S):
        ro, so = np.argsort(R["payload"], kind="stable"), np.argsort(S["payload"], kind="stable")
        rs, ss = R["payload"][ro], S["payload"][so]
        lo = np.searchsorted(ss, rs, "left")
        cnt = np.searchsorted(ss, rs, "right") - lo                          # partners of the tuples of R, in sorted order
        ri = np.repeat(np.arange(len(R)), cnt)
        within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        si = np.repeat(lo, cnt) + within
        pairs = np.empty(len(ri), dtype=PAIR)
        pairs["keyR"], pairs["keyS"] = R["key"][ro[ri]], S["key"][so[si]]
        self.pairs = sort_pairs(pairs)
        self.r_only = np.sort(R["key"][ro[cnt == 0]])
        self.s_only = np.sort(S["key"][so[np.searchsorted(rs, ss, "right") == np.searchsorted(rs, ss, "left")]])

    def sections(self, how):
        return (len(self.pairs), len(self.r_only) if how & OUTER_LEFT else 0, len(self.s_only) if how & OUTER_RIGHT else 0)


@pytest.fixture(scope="module")
def inputs():
    """(dist, n, nS, seed, ids) -> (R, S, Expected): built once, shared, never written"""
    cache = {}

    def get(dist, n, nS=None, seed=0, ids=True):
        key = (dist, n, nS, seed, ids)
        if key not in cache:
            R, S = make(dist, n, nS or n, seed)
            R, S = with_ids(R, ids), with_ids(S, ids)
            cache[key] = (R, S, Expected(R, S))
        return cache[key]
    return get


def check(got, total, sec, how, exp):
    """the whole contract of one filled result"""
    m, ro, so = sec
    print(f"how {how}: total {total} sections {sec} expected {exp.sections(how)}")
    assert tuple(sec) == exp.sections(how) and total == m + ro + so == len(got)
    first, second, third = got[:m], got[m: m + ro], got[m + ro:]
    assert not (first["keyR"] == NO).any() and not (first["keyS"] == NO).any()
    assert np.array_equal(sort_pairs(first), exp.pairs)
    assert (second["keyS"] == NO).all() and np.array_equal(np.sort(second["keyR"]), exp.r_only[: ro])
    assert (third["keyR"] == NO).all() and np.array_equal(np.sort(third["keyS"]), exp.s_only[: so])


def run_cols(eng, R, S, exp, ids=True, opts=None, after=None, modes=MODES):
    """the modes through the columnar entry against the oracle; after(how): further assertions on the engine's state"""
    cols = [eng.to_device(np.ascontiguousarray(a)) if (ids or name == "payload") and len(T) else None
            for T in (R, S) for name, a in (("payload", T["payload"]), ("key", T["key"]))]
    dvR, diR, dvS, diS = cols
    cap = max(sum(exp.sections(OUTER_FULL)), 1)
    out = eng.alloc(16 * cap)
    result = {}
    try:
        for how in modes:
            n, sec = eng.outer_join_cols_dev(dvR, diR, len(R), dvS, diS, len(S), how, out, cap, opts=opts)
            print(f"kernel {eng.info('last.join_kernel')} sweeps {eng.info('last.outer_sweeps')} tables {eng.info('last.semi_tables')} "
                  f"narrow {eng.info('last.narrow')} ntasks {eng.timings()['ntasks']}")
            check(out.to_numpy(PAIR, n), n, sec, how, exp)
            if after is not None:
                after(how)
            result[how] = sec
    finally:
        for b in cols + [out]:
            if b is not None:
                b.free()
    return result


# ---- paths by size -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", [False, True], ids=["null", "ids"])
@pytest.mark.parametrize("dist", ["uniform", "dups", "zipf"])
@pytest.mark.parametrize("n,passes", [(3_000, 0), (70_000, 1)])
def test_small_sizes_automatic_plan(eng, inputs, n, passes, dist, ids):
    assert resolve_plan(n, n).passes == passes
    R, S, exp = inputs(dist, n, ids=ids)
    assert all(x > 0 for x in exp.sections(OUTER_FULL))
    eng.set_option("partition.narrow", -1)

    def after(how):
        assert eng.info("last.outer_sweeps") == SWEEPS[how] and eng.info("last.semi_tables") == 1 and eng.info("last.narrow") == 0
        assert eng.timings()["passes"] == passes and eng.info("last.join_kernel") != JK_SEMI
    sec = run_cols(eng, R, S, exp, ids, after=after)[OUTER_FULL]
    # the sections against the entries that count each of them alone
    dv, ds = eng.to_device(np.ascontiguousarray(R["payload"])), eng.to_device(np.ascontiguousarray(S["payload"]))
    inner = eng.join_cols_dev(dv, None, n, ds, None, n)
    kernel = eng.info("last.join_kernel")
    assert sec[0] == inner
    assert sec[1] == eng.semi_join_cols_dev(dv, None, n, ds, n, ANTI)
    assert sec[2] == eng.semi_join_cols_dev(ds, None, n, dv, n, ANTI)
    assert eng.outer_join_cols_dev(dv, None, n, ds, None, n, OUTER_FULL) == (sum(sec), sec)
    assert passes == 1 or eng.info("last.join_kernel") == kernel            # (a one-pass pair join alone may run fused: another kernel)
    dv.free()
    ds.free()


@pytest.mark.parametrize("dist", ["uniform", "zipf"])
def test_three_million_narrow_two_pass(eng, inputs, dist):
    R, S, exp = inputs(dist, 3_000_000, ids=False)
    eng.set_option("partition.narrow", 2)
    eng.set_option("partition.countfree", 0)

    def after(how):
        assert eng.info("last.narrow") == 2 and eng.info("last.cols_R") == 1 and eng.info("last.cols_S") == 1
        assert eng.info("last.outer_sweeps") == SWEEPS[how] and eng.info("last.semi_tables") == 1
    try:
        run_cols(eng, R, S, exp, ids=False, opts=PLAN, after=after)
    finally:
        eng.set_option("partition.narrow", -1)
        eng.set_option("partition.countfree", -1)


# ---- duplicates ------------------------------------------------------------------------------------------------------------------
def test_heavy_values_matched_and_unmatched(eng, inputs):
    R0, S0, _ = inputs("uniform", 70_000)
    rng = np.random.default_rng(5)
    both, r_heavy, s_heavy = np.uint64(0x123456789ABCDEF), np.uint64(0x2222222222222222), np.uint64(0x3333333333333333)
    rv = np.concatenate([R0["payload"][: 68_000], np.full(1_000, both, dtype=np.uint64), np.full(1_000, r_heavy, dtype=np.uint64)])
    sv = np.concatenate([S0["payload"][: 68_000], np.full(1_000, both, dtype=np.uint64), np.full(1_000, s_heavy, dtype=np.uint64)])
    R, S = rel(rng, len(rv), rv[rng.permutation(len(rv))]), rel(rng, len(sv), sv[rng.permutation(len(sv))])
    exp = Expected(R, S)
    assert len(R) == len(S) == 70_000 and len(exp.pairs) >= 1_000_000
    assert np.isin(R["key"][R["payload"] == r_heavy], exp.r_only).all() and np.isin(S["key"][S["payload"] == s_heavy], exp.s_only).all()
    eng.set_option("partition.narrow", -1)
    run_cols(eng, R, S, exp, ids=True)


# ---- several tables per task, several tasks per partition, in both sweep directions ----------------------------------------------
@pytest.mark.parametrize("table_side", ["S", "R"])
@pytest.mark.parametrize("opts,nT", [(Opts(1, 1, 0), 200_000), (Opts(0, 0, 0), 100_000)], ids=["one-bit", "unpartitioned"])
def test_partitions_beyond_one_table(eng, opts, nT, table_side):
    rng = np.random.default_rng(nT)
    nP = 300_000
    tv = rng.permutation(np.arange(1, 4 * nT, 4, dtype=np.uint64))           # distinct
    pv = np.concatenate([tv[rng.integers(0, nT, nP // 2)], rng.integers(0, nT, nP - nP // 2).astype(np.uint64) * np.uint64(4) + np.uint64(2)])
    P, T = rel(rng, nP, pv[rng.permutation(nP)]), rel(rng, nT, tv)
    R, S = (P, T) if table_side == "S" else (T, P)
    exp = Expected(R, S)
    mine = OUTER_LEFT if table_side == "S" else OUTER_RIGHT                  # the sweep that probes P against tables on T
    assert exp.sections(mine)[0] == nP // 2 and sum(exp.sections(mine)[1:]) == nP - nP // 2
    eng.set_option("partition.narrow", -1)
    ntasks = {}

    def after(how):
        ntasks[how] = eng.timings()["ntasks"]
        if how & mine:
            assert eng.info("last.semi_tables") >= 2
    run_cols(eng, R, S, exp, ids=True, opts=opts, after=after)
    sweep_tasks = ntasks[OUTER_FULL] - ntasks[OUTER_FULL & ~mine]           # (the pair join and the other sweep are in both)
    print(f"tasks {ntasks}: {sweep_tasks} of the sweep over P")
    assert sweep_tasks >= max(2 * (1 << opts.bits1), -(-nP // SEMI_MAX_SPLIT))   # several tasks per partition
    small = make("uniform", 3_000, 3_000)

    def one_table(how):
        assert eng.info("last.semi_tables") == 1
    run_cols(eng, *small, Expected(*small), ids=True, after=one_table)
    dv, ds = eng.to_device(np.ascontiguousarray(small[0]["payload"])), eng.to_device(np.ascontiguousarray(small[1]["payload"]))
    assert eng.join_cols_dev(dv, None, 3_000, ds, None, 3_000) > 0
    assert eng.info("last.semi_tables") == 0 and eng.info("last.outer_sweeps") == 0
    dv.free()
    ds.free()


# ---- the all-ones join value, 0 and 1 << 63 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3_000, 70_000])
@pytest.mark.parametrize("ones_on", ["both", "R", "S", "both-unmixed", "R-unmixed", "S-unmixed"])
def test_all_ones_value(eng, inputs, n, ones_on):
    """the raw all-ones value is the tables' empty marker at 3,000 rows only (unpartitioned: the kernels see the payloads); under the
    one-pass plan of 70,000 rows they see rhj_mix64(payload), the marker there is unmix64(all ones) -- the "-unmixed" cases -- and
    each value is an ordinary key on the other path"""
    assert resolve_plan(n, n).passes == (0 if n == 3_000 else 1)
    ones_on, _, unmixed = ones_on.partition("-")
    R0, S0, _ = inputs("uniform", n)
    R, S = R0.copy(), S0.copy()
    ones, top = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(1 << 63)
    if unmixed:
        ones = unmix64(ones)
        assert int(mix64(ones)) == 0xFFFFFFFFFFFFFFFF
    if ones_on in ("both", "R"):
        R["payload"][[3, 1_500]] = ones
    if ones_on in ("both", "S"):
        S["payload"][[7, 8, 2_000]] = ones
    R["payload"][[10, 11]], S["payload"][[12]] = np.uint64(0), np.uint64(0)      # 0 on both sides
    R["payload"][[20]], S["payload"][[21, 22]] = top, top                       # 1 << 63 on both sides
    R["payload"][[30]], S["payload"][[31]] = top | np.uint64(1), top | np.uint64(2)   # ... and neighbours of it on one side each
    exp = Expected(R, S)
    ones_R, ones_S = R["key"][R["payload"] == ones], S["key"][S["payload"] == ones]
    if ones_on == "both":
        assert len(ones_R) == 2 and len(ones_S) == 3 and not np.isin(ones_R, exp.r_only).any() and not np.isin(ones_S, exp.s_only).any()
    elif ones_on == "R":
        assert len(ones_R) == 2 and np.isin(ones_R, exp.r_only).all()
    else:
        assert len(ones_S) == 3 and np.isin(ones_S, exp.s_only).all()
    eng.set_option("partition.narrow", -1)
    run_cols(eng, R, S, exp, ids=True)


# ---- partitions without the other side, disjoint sides, degenerate sizes, invalid arguments -------------------------------------
@pytest.mark.parametrize("small_side", ["S", "R"])
def test_empty_partitions_of_the_other_side(eng, inputs, small_side):
    big, _, _ = inputs("uniform", 3_000_000, ids=False)
    rng = np.random.default_rng(11)
    v = big["payload"][rng.integers(0, len(big), 70_000)]
    v[::97] ^= np.uint64(1 << 62)
    small = with_ids(rel(rng, len(v), v), False)
    R, S = (big, small) if small_side == "S" else (small, big)
    exp = Expected(R, S)
    eng.set_option("partition.narrow", -1)
    sec = run_cols(eng, R, S, exp, ids=False, opts=PLAN)[OUTER_FULL]
    assert sec[1 if small_side == "S" else 2] > 2_900_000 and sec[2 if small_side == "S" else 1] > 500
    assert 0 < eng.info(f"last.max_part_{small_side}") < 20                  # ~1.07 tuples per partition: a third have none


def test_disjoint_sides(eng, inputs):
    R, S0, _ = inputs("uniform", 70_000)
    S = S0.copy()
    S["payload"] |= np.uint64(1 << 63)
    exp = Expected(R, S)
    assert exp.sections(OUTER_FULL) == (0, len(R), len(S))
    eng.set_option("partition.narrow", -1)
    assert run_cols(eng, R, S, exp, ids=True) == {OUTER_LEFT: (0, len(R), 0), OUTER_RIGHT: (0, 0, len(S)), OUTER_FULL: (0, len(R), len(S))}


def test_degenerate_sizes(eng, inputs):
    R, S, exp = inputs("uniform", 3_000)
    big, _, _ = inputs("uniform", 70_000)
    eng.set_option("partition.narrow", -1)

    def only_a_sweep(preserved):
        def after(how):
            ran = bool(how & preserved)
            assert eng.info("last.join_kernel") == (JK_SEMI if ran else -1)
            assert eng.info("last.outer_sweeps") == (1 if ran else 0) and eng.info("last.semi_tables") == (1 if ran else 0)
        return after
    for ids in (True, False):
        r, s = with_ids(R, ids), with_ids(S, ids)
        got = run_cols(eng, r, s[:0], Expected(r, s[:0]), ids, after=only_a_sweep(OUTER_LEFT))          # nS == 0
        assert got == {OUTER_LEFT: (0, len(R), 0), OUTER_RIGHT: (0, 0, 0), OUTER_FULL: (0, len(R), 0)}
        got = run_cols(eng, r[:0], s, Expected(r[:0], s), ids, after=only_a_sweep(OUTER_RIGHT))         # nR == 0
        assert got == {OUTER_LEFT: (0, 0, 0), OUTER_RIGHT: (0, 0, len(S)), OUTER_FULL: (0, 0, len(S))}

    def nothing(how):
        assert eng.info("last.join_kernel") == -1 and eng.info("last.outer_sweeps") == 0 and eng.info("last.semi_tables") == 0
    assert set(run_cols(eng, R[:0], S[:0], Expected(R[:0], S[:0]), after=nothing).values()) == {(0, 0, 0)}
    # a large side against an empty one: every id, through several tasks
    def several_tasks(how):
        assert eng.timings()["ntasks"] >= 3
    assert run_cols(eng, big, S[:0], Expected(big, S[:0]), after=several_tasks, modes=(OUTER_LEFT, OUTER_FULL))[OUTER_FULL] == (0, len(big), 0)
    assert run_cols(eng, R[:0], big, Expected(R[:0], big), after=several_tasks, modes=(OUTER_RIGHT, OUTER_FULL))[OUTER_FULL] == (0, 0, len(big))
    # n = 1 on either side, with and without a partner
    hit_R = int(np.flatnonzero(np.isin(R["payload"], S["payload"]))[0])
    miss_R = int(np.flatnonzero(~np.isin(R["payload"], S["payload"]))[0])
    hit_S = int(np.flatnonzero(np.isin(S["payload"], R["payload"]))[0])
    miss_S = int(np.flatnonzero(~np.isin(S["payload"], R["payload"]))[0])
    for r, s in ((R[hit_R: hit_R + 1], S), (R[miss_R: miss_R + 1], S), (R, S[hit_S: hit_S + 1]), (R, S[miss_S: miss_S + 1]),
                 (R[hit_R: hit_R + 1], S[S["payload"] == R["payload"][hit_R]][:1]), (R[miss_R: miss_R + 1], S[miss_S: miss_S + 1])):
        run_cols(eng, r, s, Expected(r, s), ids=True)
    r1, s1 = with_ids(R[miss_R: miss_R + 1], False), with_ids(S[miss_S: miss_S + 1], False)
    assert run_cols(eng, r1, s1, Expected(r1, s1), ids=False)[OUTER_FULL] == (0, 1, 1)


def test_invalid_arguments(eng, inputs):
    R, S, exp = inputs("uniform", 3_000)
    n = 3_000
    dvR, dvS = eng.to_device(np.ascontiguousarray(R["payload"])), eng.to_device(np.ascontiguousarray(S["payload"]))
    dR, dS, out = eng.to_device(R), eng.to_device(S), eng.alloc(16 * 3 * n)
    for how in (0, 4, -1):
        with pytest.raises(RhjError) as err:
            eng.outer_join_cols_dev(dvR, None, n, dvS, None, n, how, out, 3 * n)
        assert err.value.code == RHJ_E_INVALID
        with pytest.raises(RhjError) as err:
            eng.outer_join_dev(dR, n, dS, n, how, out, 3 * n)
        assert err.value.code == RHJ_E_INVALID
    for how in MODES:
        for args in ((None, None, n, dvS, None, n), (dvR, None, n, None, None, n), (None, dvR, n, dvS, None, n), (dvR, None, n, None, dvS, n),
                     (None, None, 5, None, None, 0), (None, None, 0, None, None, 5)):
            with pytest.raises(RhjError) as err:
                eng.outer_join_cols_dev(*args, how, out, 3 * n)
            assert err.value.code == RHJ_E_INVALID
        for args in ((None, n, dS, n), (dR, n, None, n), (None, 5, None, 0), (None, 0, None, 5)):
            with pytest.raises(RhjError) as err:
                eng.outer_join_dev(*args, how, out, 3 * n)
            assert err.value.code == RHJ_E_INVALID
    assert eng.lib.rhj_outer_join_cols_dev(eng.ctx, dvR.ptr, None, n, dvS.ptr, None, n, OUTER_FULL, None, None, 0, None, None) == RHJ_E_INVALID
    assert eng.lib.rhj_outer_join_dev(eng.ctx, dR.ptr, n, dS.ptr, n, OUTER_FULL, None, None, 0, None, None) == RHJ_E_INVALID
    # the context is usable afterwards
    total, sec = eng.outer_join_dev(dR, n, dS, n, OUTER_FULL, out, 3 * n)
    check(out.to_numpy(PAIR, total), total, sec, OUTER_FULL, exp)
    for b in (dvR, dvS, dR, dS, out):
        b.free()


# ---- the repeats inside a call -----------------------------------------------------------------------------------------------
def test_count_free_overflow_repeats_S(inputs):
    R, S, exp = inputs("quarter", 3_000_000, ids=False)
    # R fits its count-free regions (its largest pass-1 piece is 36 or 37 of 64 slots), S does not: R stands, "last.countfree_R" is 1
    assert int(cf_cases.piece_lengths(R).max()) <= cf_cases.cap(cf_cases.unit_len(len(R)), 8) < int(cf_cases.piece_lengths(S).max())
    e = Engine(0)
    try:
        e.set_option("partition.narrow", 2)

        def after(how):
            assert e.info("last.narrow") == 2 and e.info("last.countfree_S") == 2 and e.info("last.countfree_R") == 1
            assert e.info("last.outer_sweeps") == SWEEPS[how]
            e.set_option("partition.countfree", 1)                         # re-arm the back-off for the next mode
        e.set_option("partition.countfree", 1)
        run_cols(e, R, S, exp, ids=False, opts=PLAN, after=after)
    finally:
        e.close()


def test_one_wide_id_falls_back_for_that_call_only(inputs):
    R0, S0, _ = inputs("uniform", 90_000, 120_000, seed=2)
    in_S, in_R = np.isin(R0["payload"], S0["payload"]), np.isin(S0["payload"], R0["payload"])
    e = Engine(0)
    try:
        e.set_option("partition.narrow", 2)                                # set once, never re-armed below
        cases = ((None, None), ("R", int(np.flatnonzero(in_S)[7])), ("R", int(np.flatnonzero(~in_S)[7])), (None, None),
                 ("S", int(np.flatnonzero(in_R)[7])), ("S", int(np.flatnonzero(~in_R)[7])), (None, None))
        for side, row in cases:
            R, S = R0.copy(), S0.copy()
            if side is not None:
                (R if side == "R" else S)["key"][row] = np.uint64(1 << 32)   # reported in the matched section / as an unmatched row
            exp = Expected(R, S)

            def after(how):
                assert e.info("last.narrow") == (0 if side else 2)
                assert e.info("last.cols_R") == (2 if side else 1) and e.info("last.cols_S") == (2 if side else 1)
                assert e.info("last.outer_sweeps") == SWEEPS[how]
            run_cols(e, R, S, exp, ids=True, opts=PLAN, after=after)
    finally:
        e.close()


# ---- count-only and small buffers ----------------------------------------------------------------------------------------------
def test_count_only_and_small_buffers(eng, inputs):
    R, S, exp = inputs("dups", 70_000)
    m, ro, so = sections = exp.sections(OUTER_FULL)
    total, pad = m + ro + so, 64
    assert m > 100 and ro > 100 and so > 100
    eng.set_option("partition.narrow", -1)
    cols = [eng.to_device(np.ascontiguousarray(a)) for a in (R["payload"], R["key"], S["payload"], S["key"])]
    args = (cols[0], cols[1], len(R), cols[2], cols[3], len(S), OUTER_FULL)
    assert eng.outer_join_cols_dev(*args) == (total, sections)                                # d_out NULL, capacity 0
    full = eng.alloc(16 * total)
    assert eng.outer_join_cols_dev(*args, full, total) == (total, sections)
    check(full.to_numpy(PAIR, total), total, sections, OUTER_FULL, exp)
    full.free()

    def key(p):                                                            # (ids are below 2^32 here)
        return (p["keyR"] << np.uint64(32)) | p["keyS"]
    for cap in (total - 5, m + ro // 2, m // 2):
        fill = np.empty(cap + pad, dtype=PAIR)
        fill["keyR"] = fill["keyS"] = SENTINEL
        out = eng.to_device(fill)
        with pytest.raises(RhjError) as err:
            eng.outer_join_cols_dev(*args, out, cap)
        assert err.value.code == RHJ_E_OVERFLOW
        assert eng.outer_join_cols_dev(*args, out, cap, allow_overflow=True) == (total, sections)
        back = out.to_numpy(PAIR, cap + pad)
        out.free()
        assert (back["keyR"][cap:] == SENTINEL).all() and (back["keyS"][cap:] == SENTINEL).all(), "a row was written at or past capacity"
        first, second, third = back[: min(cap, m)], back[min(cap, m): min(cap, m + ro)], back[min(cap, m + ro): cap]
        print(f"capacity {cap}: {len(first)} + {len(second)} + {len(third)} rows of {sections}")
        assert len(first) + len(second) + len(third) == cap
        assert len(np.unique(key(first))) == len(first) and np.isin(key(first), key(exp.pairs)).all()
        assert (second["keyS"] == NO).all() and len(np.unique(second["keyR"])) == len(second) and np.isin(second["keyR"], exp.r_only).all()
        assert (third["keyR"] == NO).all() and len(np.unique(third["keyS"])) == len(third) and np.isin(third["keyS"], exp.s_only).all()
    for b in cols:
        b.free()


# ---- the AoS entry -------------------------------------------------------------------------------------------------------------
def test_aos_entry_agrees(eng, inputs):
    R, S, exp = inputs("dups", 70_000)
    cap = sum(exp.sections(OUTER_FULL))
    eng.set_option("partition.narrow", -1)
    dR, dS, out = eng.to_device(R), eng.to_device(S), eng.alloc(16 * cap)
    secs = {}
    for how in MODES:
        n, secs[how] = eng.outer_join_dev(dR, len(R), dS, len(S), how, out, cap)
        check(out.to_numpy(PAIR, n), n, secs[how], how, exp)
        assert eng.info("last.cols_R") == 0 and eng.info("last.cols_S") == 0 and eng.info("last.outer_sweeps") == SWEEPS[how]
        assert eng.outer_join_dev(dR, len(R), dS, len(S), how) == (n, secs[how])
    assert secs == run_cols(eng, R, S, exp, ids=True)
    for b in (dR, dS, out):
        b.free()


# ---- Engine.outer_join_columns -------------------------------------------------------------------------------------------------
def as_rel(keys):
    t = np.empty(len(keys), dtype=TUPLE)
    t["key"], t["payload"] = np.arange(len(keys), dtype=np.uint64), keys.view(np.uint64)
    return t


def check_columns(idx_R, idx_S, how, exp):
    assert idx_R.dtype == torch.int64 and idx_S.dtype == torch.int64 and idx_R.is_cuda and idx_R.dim() == 1 and idx_R.shape == idx_S.shape
    got = np.empty(idx_R.numel(), dtype=PAIR)
    got["keyR"], got["keyS"] = idx_R.cpu().numpy().view(np.uint64), idx_S.cpu().numpy().view(np.uint64)
    sec = exp.sections({"left": OUTER_LEFT, "right": OUTER_RIGHT, "full": OUTER_FULL}[how])
    check(got, len(got), sec, {"left": OUTER_LEFT, "right": OUTER_RIGHT, "full": OUTER_FULL}[how], exp)
    m, ro, _ = sec
    assert (idx_S[m: m + ro] == -1).all() and (idx_R[m + ro:] == -1).all()
    assert (idx_R[: m + ro] >= 0).all() and (idx_S[:m] >= 0).all() and (idx_S[m + ro:] >= 0).all()


@pytest.mark.parametrize("nR,nS", [(1_000, 3_000), (200_000, 300_000)])
def test_outer_join_columns_against_numpy(nR, nS):
    rng = np.random.default_rng(nR)
    kR = rng.integers(-(1 << 62), 1 << 62, nR, dtype=np.int64)
    kR[: nR // 10] = kR[nR // 2: nR // 2 + nR // 10]
    kR[0], kR[1] = -1, np.iinfo(np.int64).min                              # (-1: the all-ones word)
    kS = kR[rng.integers(0, nR, nS)]
    kS[::13] = rng.integers(-(1 << 62), 1 << 62, len(kS[::13]), dtype=np.int64)
    kS[5], kS[6] = -1, np.iinfo(np.int64).min
    exp, mirrored = Expected(as_rel(kR), as_rel(kS)), Expected(as_rel(kS), as_rel(kR))
    assert all(x > 0 for x in exp.sections(OUTER_FULL))
    e = Engine(0)
    try:
        tR, tS = torch.from_numpy(kR).cuda(), torch.from_numpy(kS).cuda()
        for how in ("left", "right", "full"):
            check_columns(*e.outer_join_columns(tR, tS, how), how, exp)
        check_columns(*e.outer_join_columns(tR, tS), "left", exp)                           # the default
        # "right" is "left" with the arguments and the outputs exchanged
        iS, iR = e.outer_join_columns(tS, tR, "left")
        check_columns(iR, iS, "right", exp)
        check_columns(iS, iR, "left", mirrored)
        # empty tensors on either side
        noR, noS = tR[:0].contiguous(), tS[:0].contiguous()
        for how in ("left", "right", "full"):
            check_columns(*e.outer_join_columns(tR, noS, how), how, Expected(as_rel(kR), as_rel(kS[:0])))
            check_columns(*e.outer_join_columns(noR, tS, how), how, Expected(as_rel(kR[:0]), as_rel(kS)))
            iR, iS = e.outer_join_columns(noR, noS, how)
            assert iR.numel() == 0 and iS.numel() == 0 and iR.dtype == torch.int64
    finally:
        e.close()


def test_outer_join_columns_refuses_what_it_cannot_read():
    e = Engine(0)
    try:
        good = torch.arange(100, device="cuda", dtype=torch.int64)
        for bad in (good.to(torch.int32), good.to(torch.float64), torch.arange(200, device="cuda")[::2], good.cpu(),
                    good.reshape(10, 10), list(range(5))):
            for how in ("left", "right", "full"):
                with pytest.raises(ValueError):
                    e.outer_join_columns(bad, good, how)
                with pytest.raises(ValueError):
                    e.outer_join_columns(good, bad, how)
        for how in ("inner", "outer", "LEFT", None, 1):
            with pytest.raises(ValueError):
                e.outer_join_columns(good, good, how)
        iR, iS = e.outer_join_columns(good, good, "full")
        assert torch.equal(iR.sort().values, good) and torch.equal(iR, iS)
    finally:
        e.close()


def test_outer_join_columns_is_ordered_behind_queued_torch_work():
    """the keys are the last product of a queue of torch kernels issued right before the call, on a stream of its own"""
    F, nR, nS, rounds = 50_000_000, 300_000, 250_000, 20
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
            kR = filler[:nR].clone()
            kS = filler[nR // 2: nR // 2 + nS].clone()                     # distinct values: S = rows nR/2 ... of R and beyond
            iR, iS = e.outer_join_columns(kR, kS, "full")
        torch.cuda.synchronize()
        m, ro, so = nR - nR // 2, nR // 2, nS - (nR - nR // 2)
        assert iR.numel() == m + ro + so
        assert torch.equal(iR[:m].sort().values, torch.arange(nR // 2, nR, device="cuda"))
        assert torch.equal(iR[:m] - nR // 2, iS[:m])                       # row i of R is row i - nR/2 of S
        assert torch.equal(iR[m: m + ro].sort().values, torch.arange(0, nR // 2, device="cuda")) and (iS[m: m + ro] == -1).all()
        assert torch.equal(iS[m + ro:].sort().values, torch.arange(m, nS, device="cuda")) and (iR[m + ro:] == -1).all()
        x = np.arange(nR, dtype=np.uint64)
        with np.errstate(over="ignore"):
            for _ in range(rounds):
                x = x * np.uint64(3) + np.uint64(1)
        assert np.array_equal(kR.cpu().numpy().view(np.uint64), x)
        assert e.bound_stream is None
    finally:
        e.close()


def test_outer_join_columns_keeps_the_callers_stream_binding():
    e = Engine(0)
    try:
        mine, other = torch.cuda.Stream(), torch.cuda.Stream()
        e.set_stream(mine.cuda_stream)
        keys = torch.arange(5_000, device="cuda", dtype=torch.int64)
        torch.cuda.synchronize()
        assert e.outer_join_columns(keys, keys, "full")[0].numel() == 5_000 and e.bound_stream == mine.cuda_stream
        with torch.cuda.stream(other):
            iR, iS = e.outer_join_columns(keys, keys[:100].contiguous(), "left")
            assert iR.numel() == 5_000 and int((iS == -1).sum()) == 4_900
        assert e.bound_stream == mine.cuda_stream
        with torch.cuda.stream(mine):
            iR, iS = e.outer_join_columns(keys, keys, "right")
        assert torch.equal(iR.sort().values, keys) and torch.equal(iR, iS) and e.bound_stream == mine.cuda_stream
        e.set_stream(None)
        assert e.bound_stream is None
    finally:
        e.close()
