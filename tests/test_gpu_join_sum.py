"""GPU suite: the aggregating join rhj_join_sum_cols_dev / rhj_join_sum_dev (include/rhj.h) and Engine.join_sum_columns: COUNT(*)
and SUM(column of R) over R join S, without the pairs.

The oracle is numpy: np.unique(valS, return_counts=True) + searchsorted give mult, the number of partners of every tuple of R;
count = mult.sum(), sums[j] = (mult * w[j][id]).sum() in wrapping uint64.  Weights are drawn from the full 64-bit range, so the
sums wrap.  Every comparison is exact.
  * paths by size: 3,000 rows per side (unpartitioned), 70,000 (one-pass automatic plan), 3,000,000 under Opts(2, 8, 8) in the
    narrow format (columns read directly); uniform, duplicate-heavy and Zipf 0.9 inputs; NULL and explicit ids; 0, 1 and 4 columns;
  * multiplicities the pair join cannot afford: 1,000 x 10^6 rows of one value (10^9 pairs), 70,000 x 70,000 (4.9 * 10^9 > 2^32
    pairs, every tuple in one slot), the all-ones key on both sides;
  * partitions of S far beyond one LDS table with R cut into several tasks ("last.semi_tables" >= 2), then one table;
  * the repeats inside a call: a count-free region that overflows; one rowID of 2^32 in a narrow format (with ncols = 0: a column
    that reaches row 2^32 would be 32 GiB, or a base pointer outside its allocation);
  * the guard: a rowID equal to col_rows is RHJ_E_INVALID, and the context goes on;
  * n = 0 and n = 1, a disjoint S, invalid arguments; the AoS entry; the pair join's pairs summed in numpy;
  * join_sum_columns on int64 tensors: negative keys and weights, refused tensors, queued torch work on a side stream."""
import numpy as np
import pytest
import torch

import cf_cases
from oracle.pyoracle import TUPLE
from radixhashjoin_amd import Engine, Opts, RhjError, SUM_MAX_COLS, unmix64
from radixhashjoin_amd.binding import RHJ_E_INVALID, plan as resolve_plan

pytestmark = pytest.mark.gpu
PLAN = Opts(2, 8, 8)
JK_AGG = 13
MASK64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


# ---- input builders (those of test_gpu_semi_join.py) -------------------------------------------------------------------------
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
    """R values; S values sampled from R, every 97th made foreign; ids a permutation"""
    rng = np.random.default_rng(nR * 31 + nS + seed)
    if dist == "dups":
        rv = rng.integers(1, 1 << 62, max(nR // 4, 1), dtype=np.uint64)[rng.integers(0, max(nR // 4, 1), nR)]
    else:
        rv = rng.integers(1, 1 << 62, nR, dtype=np.uint64)
    if dist == "zipf":
        sv = rv[zipf_ranks(rng, nS, nR) - 1]
    else:
        sv = rv[rng.integers(0, nR, nS)]
        if dist == "quarter":
            sv[rng.permutation(nS)[: nS // 4]] = rv[0]         # one value on a quarter of the rows: no count-free region holds it
    sv[::97] ^= np.uint64(1 << 62)
    return rel(rng, nR, rv), rel(rng, nS, sv)


def with_ids(T, ids):
    if ids:
        return T
    t = T.copy()
    t["key"] = np.arange(len(T), dtype=np.uint64)
    return t


def weights(rows, seed=1):
    """SUM_MAX_COLS columns of `rows` words from the full 64-bit range"""
    rng = np.random.default_rng(rows + seed)
    return [rng.integers(0, 1 << 64, rows, dtype=np.uint64) for _ in range(SUM_MAX_COLS)]


def multiplicity(rv, sv):
    """partners in sv of every value of rv"""
    if len(sv) == 0 or len(rv) == 0:
        return np.zeros(len(rv), dtype=np.uint64)
    u, c = np.unique(sv, return_counts=True)
    pos = np.minimum(np.searchsorted(u, rv), len(u) - 1)
    return np.where(u[pos] == rv, c[pos], 0).astype(np.uint64)


def oracle(mult, ids, W, ncols):
    return int(mult.sum(dtype=np.uint64)), [int((mult * W[j][ids]).sum(dtype=np.uint64)) for j in range(ncols)]


@pytest.fixture(scope="module")
def inputs():
    """(dist, n) -> (R, S, mult, W): built once, shared, never written"""
    cache = {}

    def get(dist, n, nS=None, seed=0):
        key = (dist, n, nS, seed)
        if key not in cache:
            R, S = make(dist, n, nS or n, seed)
            cache[key] = (R, S, multiplicity(R["payload"], S["payload"]), weights(n))
        return cache[key]
    return get


def run_cols(eng, R, S, mult, W, ncols, ids=True, opts=None):
    """the columnar entry against the oracle; returns (count, sums)"""
    R = with_ids(R, ids)
    dv, di = eng.to_device(np.ascontiguousarray(R["payload"])), eng.to_device(np.ascontiguousarray(R["key"])) if ids else None
    ds = eng.to_device(np.ascontiguousarray(S["payload"]))
    dw = [eng.to_device(W[j]) for j in range(ncols)]
    try:
        got = eng.join_sum_cols_dev(dv, di, len(R), ds, len(S), dw, len(W[0]) if ncols else 0, opts=opts)
        exp = oracle(mult, R["key"].astype(np.int64), W, ncols)
        print(f"count {got[0]} expected {exp[0]} sums {got[1]} expected {exp[1]} kernel {eng.info('last.join_kernel')} "
              f"tables {eng.info('last.semi_tables')} narrow {eng.info('last.narrow')} tasks {eng.timings()['ntasks']}")
        assert got == exp
    finally:
        for b in [dv, di, ds] + dw:
            if b is not None:
                b.free()
    return got


# ---- paths by size -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncols", [0, 1, 4])
@pytest.mark.parametrize("ids", [False, True], ids=["null", "ids"])
@pytest.mark.parametrize("dist", ["uniform", "dups", "zipf"])
@pytest.mark.parametrize("n,passes", [(3_000, 0), (70_000, 1)])
def test_small_sizes_automatic_plan(eng, inputs, n, passes, dist, ids, ncols):
    assert resolve_plan(n, n).passes == passes
    R, S, mult, W = inputs(dist, n)
    eng.set_option("partition.narrow", -1)
    count, _ = run_cols(eng, R, S, mult, W, ncols, ids)
    assert count > 0
    assert eng.info("last.join_kernel") == JK_AGG and eng.info("last.semi_tables") == 1 and eng.info("last.narrow") == 0
    assert eng.timings()["passes"] == passes


@pytest.mark.parametrize("dist,ncols,ids", [("uniform", 4, False), ("zipf", 1, False), ("dups", 0, True)])
def test_three_million_narrow_two_pass(eng, inputs, dist, ncols, ids):
    R, S, mult, W = inputs(dist, 3_000_000)
    eng.set_option("partition.narrow", 2)
    eng.set_option("partition.countfree", 0)
    try:
        run_cols(eng, R, S, mult, W, ncols, ids=ids, opts=PLAN)
        assert eng.info("last.narrow") == 2 and eng.info("last.cols_R") == 1 and eng.info("last.cols_S") == 1
        assert eng.info("last.join_kernel") == JK_AGG and eng.info("last.semi_tables") == 1
    finally:
        eng.set_option("partition.narrow", -1)
        eng.set_option("partition.countfree", -1)


# ---- multiplicity the pair join cannot afford --------------------------------------------------------------------------------
def test_a_value_on_a_thousand_rows_of_R_and_a_million_of_S(eng):
    heavy = np.uint64(0x123456789ABCDEF)
    rng = np.random.default_rng(5)
    R, S = rel(rng, 1_000, np.full(1_000, heavy, dtype=np.uint64)), rel(rng, 1_000_000, np.full(1_000_000, heavy, dtype=np.uint64))
    W = weights(1_000)
    eng.set_option("partition.narrow", -1)
    count, sums = run_cols(eng, R, S, multiplicity(R["payload"], S["payload"]), W, 2)
    assert count == 10**9
    assert sums == [(10**6 * sum(int(x) for x in W[j])) & MASK64 for j in range(2)]


@pytest.mark.parametrize("value", [0x0FEDCBA987654321, MASK64, unmix64(MASK64)], ids=["one-value", "all-ones", "mixes-to-all-ones"])
def test_one_value_seventy_thousand_times_on_both_sides(eng, value):
    n = 70_000
    rng = np.random.default_rng(6)
    R, S = rel(rng, n, np.full(n, value, dtype=np.uint64)), rel(rng, n, np.full(n, value, dtype=np.uint64))
    count, _ = run_cols(eng, R, S, np.full(n, n, dtype=np.uint64), weights(n), 4)
    assert count == n * n > 1 << 32


def test_the_all_ones_key_among_others(eng, inputs):
    R0, S0, _, W = inputs("uniform", 3_000)
    R, S = R0.copy(), S0.copy()
    R["payload"][::7] = np.uint64(MASK64)
    S["payload"][::5] = np.uint64(MASK64)
    R["payload"][::11] = np.uint64(unmix64(MASK64))                        # (joins compare mix64(value): this one becomes all ones)
    S["payload"][::13] = np.uint64(unmix64(MASK64))
    count, _ = run_cols(eng, R, S, multiplicity(R["payload"], S["payload"]), W, 4)
    assert count >= 2 * (3_000 // 77) * (3_000 // 65)


# ---- several tables per task, several tasks per partition --------------------------------------------------------------------
def test_partitions_beyond_one_table(eng):
    n = 70_000
    rng = np.random.default_rng(n)
    sv = rng.permutation(np.arange(1, 4 * n, 4, dtype=np.uint64))            # distinct
    rv = np.concatenate([sv[rng.integers(0, n, n // 2)], rng.integers(0, n, n - n // 2).astype(np.uint64) * np.uint64(4) + np.uint64(2)])
    R, S = rel(rng, n, rv[rng.permutation(n)]), rel(rng, n, sv)
    mult, W = multiplicity(R["payload"], S["payload"]), weights(n)
    assert int(mult.sum()) == n // 2
    eng.set_option("partition.narrow", -1)
    forced = run_cols(eng, R, S, mult, W, 4, opts=Opts(1, 2, 0, 4096))       # four partitions of ~17,500 keys; R in tasks of 4096
    assert eng.info("last.semi_tables") >= 2 and eng.timings()["ntasks"] >= 2 * 4
    auto = run_cols(eng, R, S, mult, W, 4)
    assert eng.info("last.semi_tables") == 1
    assert auto == forced
    big_tasks = run_cols(eng, R, S, mult, W, 4, opts=Opts(0, 0, 0, 1 << 30))  # one task of 70,000 tuples of R: beyond 32768
    assert eng.timings()["ntasks"] == 1 and eng.info("last.semi_tables") >= 2 and big_tasks == forced


# ---- the repeats inside a call -----------------------------------------------------------------------------------------------
def test_count_free_overflow_repeats_S(inputs):
    R, S, mult, W = inputs("quarter", 3_000_000)
    # R fits its count-free regions (its largest pass-1 piece is 36 or 37 of 64 slots), S does not: R stands, "last.countfree_R" is 1
    assert int(cf_cases.piece_lengths(R).max()) <= cf_cases.cap(cf_cases.unit_len(len(R)), 8) < int(cf_cases.piece_lengths(S).max())
    e = Engine(0)
    try:
        e.set_option("partition.narrow", 2)
        e.set_option("partition.countfree", 1)
        run_cols(e, R, S, mult, W, 4, ids=False, opts=PLAN)
        assert e.info("last.narrow") == 2 and e.info("last.countfree_S") == 2 and e.info("last.countfree_R") == 1
        assert e.info("last.join_kernel") == JK_AGG
    finally:
        e.close()


def test_one_wide_id_of_R_falls_back_for_that_call_only(inputs):
    R0, S, mult, W = inputs("uniform", 90_000, 120_000, seed=2)
    e = Engine(0)
    try:
        e.set_option("partition.narrow", 2)                                # set once, never re-armed below
        for wide in (False, True, False):
            R = R0.copy()
            if wide:
                R["key"][int(np.flatnonzero(mult)[7])] = np.uint64(1 << 32)    # on a tuple with partners
            run_cols(e, R, S, mult, W, 0, ids=True, opts=PLAN)             # (ncols = 0: col_rows is ignored)
            assert e.info("last.narrow") == (0 if wide else 2) and e.info("last.cols_R") == (2 if wide else 1)
        run_cols(e, R0, S, mult, W, 4, ids=True, opts=PLAN)
    finally:
        e.close()


# ---- the guard ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3_000, 70_000])
def test_a_rowid_at_col_rows_is_refused_and_the_context_goes_on(eng, inputs, n):
    R0, S, mult, W = inputs("uniform", n)
    R = R0.copy()
    R["key"][int(np.flatnonzero(mult)[3])] = np.uint64(n)                  # == col_rows, on a tuple that matches
    dv, di, ds = (eng.to_device(np.ascontiguousarray(a)) for a in (R["payload"], R["key"], S["payload"]))
    dw = [eng.to_device(w) for w in W]
    for cols in (dw[:1], dw):
        with pytest.raises(RhjError) as err:
            eng.join_sum_cols_dev(dv, di, n, ds, n, cols, n)
        assert err.value.code == RHJ_E_INVALID
    assert eng.join_sum_cols_dev(dv, di, n, ds, n) == (int(mult.sum()), [])  # ncols = 0: no column, no guard
    for b in [dv, di, ds] + dw:
        b.free()
    run_cols(eng, R0, S, mult, W, 4)


# ---- degenerate sizes, a disjoint S, invalid arguments -------------------------------------------------------------------------
def test_degenerate_sizes(eng, inputs):
    R, S, mult, W = inputs("uniform", 3_000)
    none = np.zeros(len(R), dtype=np.uint64)
    assert run_cols(eng, R, S[:0], none, W, 4) == (0, [0, 0, 0, 0])                      # nS == 0
    assert eng.info("last.join_kernel") == -1 and eng.info("last.semi_tables") == 0
    assert run_cols(eng, R[:0], S, none[:0], W, 4, ids=False) == (0, [0, 0, 0, 0])       # nR == 0
    assert run_cols(eng, R[:0], S[:0], none[:0], W, 0) == (0, [])
    hit, miss = int(np.flatnonzero(mult)[0]), int(np.flatnonzero(mult == 0)[0])
    one_s = S[S["payload"] == R["payload"][hit]][:1]
    assert run_cols(eng, R, one_s, multiplicity(R["payload"], one_s["payload"]), W, 4)[0] >= 1   # n = 1 on either side
    assert run_cols(eng, R[hit: hit + 1], S, mult[hit: hit + 1], W, 4)[0] == int(mult[hit])
    assert run_cols(eng, R[miss: miss + 1], S, mult[miss: miss + 1], W, 4) == (0, [0, 0, 0, 0])
    assert run_cols(eng, R[hit: hit + 1], one_s, np.ones(1, dtype=np.uint64), W, 1)[0] == 1
    assert run_cols(eng, R[miss: miss + 1], one_s, np.zeros(1, dtype=np.uint64), W, 1) == (0, [0])


def test_disjoint_S(eng, inputs):
    R, S0, _, W = inputs("uniform", 70_000)
    S = S0.copy()
    S["payload"] |= np.uint64(1 << 63)
    assert run_cols(eng, R, S, np.zeros(len(R), dtype=np.uint64), W, 4) == (0, [0, 0, 0, 0])
    assert eng.info("last.join_kernel") == JK_AGG


def test_invalid_arguments(eng, inputs):
    R, S, _, W = inputs("uniform", 3_000)
    n = 3_000
    dv, ds = eng.to_device(np.ascontiguousarray(R["payload"])), eng.to_device(np.ascontiguousarray(S["payload"]))
    dR, dS = eng.to_device(R), eng.to_device(S)
    dw = [eng.to_device(w) for w in W]
    bad_cols = ([dw[0]] * (SUM_MAX_COLS + 1), [dw[0], None], [None])
    for cols in bad_cols:
        with pytest.raises(RhjError) as err:
            eng.join_sum_cols_dev(dv, None, n, ds, n, cols, n)
        assert err.value.code == RHJ_E_INVALID
        with pytest.raises(RhjError) as err:
            eng.join_sum_dev(dR, n, dS, n, cols, n)
        assert err.value.code == RHJ_E_INVALID
    for args in ((None, None, n, ds, n), (dv, None, n, None, n), (None, dv, n, ds, n), (None, None, 5, None, 0)):
        with pytest.raises(RhjError) as err:
            eng.join_sum_cols_dev(*args, dw[:1], n)
        assert err.value.code == RHJ_E_INVALID
    for args in ((None, n, dS, n), (dR, n, None, n)):
        with pytest.raises(RhjError) as err:
            eng.join_sum_dev(*args, dw[:1], n)
        assert err.value.code == RHJ_E_INVALID
    assert eng.lib.rhj_join_sum_cols_dev(eng.ctx, dv.ptr, None, n, ds.ptr, n, None, 0, 0, None, None, None) == RHJ_E_INVALID   # NULL out_count
    assert eng.lib.rhj_join_sum_dev(eng.ctx, dR.ptr, n, dS.ptr, n, None, 0, 0, None, None, None) == RHJ_E_INVALID
    for b in [dv, ds, dR, dS] + dw:
        b.free()


# ---- the AoS entry, and the pair join ----------------------------------------------------------------------------------------
def test_aos_entry_agrees(eng, inputs):
    R, S, mult, W = inputs("dups", 70_000)
    dR, dS, dw = eng.to_device(R), eng.to_device(S), [eng.to_device(w) for w in W]
    got = eng.join_sum_dev(dR, len(R), dS, len(S), dw, len(R))
    assert eng.info("last.cols_R") == 0 and eng.info("last.join_kernel") == JK_AGG
    assert got == oracle(mult, R["key"].astype(np.int64), W, 4) == run_cols(eng, R, S, mult, W, 4)
    assert eng.join_sum_dev(dR, len(R), dS, len(S)) == (got[0], [])
    for b in [dR, dS] + dw:
        b.free()


def test_the_pair_joins_pairs_summed_in_numpy(eng, inputs):
    R, S, mult, W = inputs("dups", 70_000)
    dv, di, ds = (eng.to_device(np.ascontiguousarray(a)) for a in (R["payload"], R["key"], S["payload"]))
    count = eng.join_cols_dev(dv, di, len(R), ds, None, len(S))
    out = eng.alloc(16 * count)
    assert eng.join_cols_dev(dv, di, len(R), ds, None, len(S), out, count) == count
    assert eng.info("last.join_kernel") != JK_AGG and eng.info("last.semi_tables") == 0
    row_r = out.to_numpy(np.uint64, 2 * count).reshape(count, 2)[:, 0].astype(np.int64)
    exp = (count, [int(W[j][row_r].sum(dtype=np.uint64)) for j in range(4)])
    for b in (dv, di, ds, out):
        b.free()
    assert run_cols(eng, R, S, mult, W, 4) == exp


# ---- Engine.join_sum_columns -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nR,nS", [(1_000, 3_000), (200_000, 300_000)])
def test_join_sum_columns_against_numpy(nR, nS):
    rng = np.random.default_rng(nR)
    kR = rng.integers(-(1 << 62), 1 << 62, nR, dtype=np.int64)
    kR[: nR // 10] = kR[nR // 2: nR // 2 + nR // 10]
    kR[0], kR[1] = -1, np.iinfo(np.int64).min                              # (-1: the all-ones word)
    kS = kR[rng.integers(0, nR, nS)]
    kS[::13] = rng.integers(-(1 << 62), 1 << 62, len(kS[::13]), dtype=np.int64)
    kS[5], kS[6] = -1, np.iinfo(np.int64).min
    w = [rng.integers(-(1 << 63), (1 << 63) - 1, nR, dtype=np.int64) for _ in range(2)]
    mult = multiplicity(kR.view(np.uint64), kS.view(np.uint64))
    exp = oracle(mult, np.arange(nR), [x.view(np.uint64) for x in w], 2)
    assert sum(int(m) * int(x) for m, x in zip(mult[:2000], w[0][:2000])) & MASK64 == \
        int((mult[:2000] * w[0][:2000].view(np.uint64)).sum(dtype=np.uint64))     # two's complement: the same sum mod 2^64
    e = Engine(0)
    try:
        tR, tS, tw = torch.from_numpy(kR).cuda(), torch.from_numpy(kS).cuda(), [torch.from_numpy(x).cuda() for x in w]
        got = e.join_sum_columns(tR, tS, tw)
        assert got == exp and all(isinstance(v, int) and 0 <= v <= MASK64 for v in [got[0]] + got[1])
        assert e.join_sum_columns(tR, tS) == (exp[0], [])
        assert e.join_sum_columns(tR, tS[:0].contiguous(), tw) == (0, [0, 0])
        assert e.join_sum_columns(tR[:0].contiguous(), tS) == (0, [])
    finally:
        e.close()


def test_join_sum_columns_refuses_what_it_cannot_read():
    e = Engine(0)
    try:
        good = torch.arange(100, device="cuda", dtype=torch.int64)
        for bad in (good.to(torch.int32), good.to(torch.float64), torch.arange(200, device="cuda")[::2], good.cpu(),
                    good.reshape(10, 10), list(range(5))):
            with pytest.raises(ValueError):
                e.join_sum_columns(bad, good)
            with pytest.raises(ValueError):
                e.join_sum_columns(good, bad)
            with pytest.raises(ValueError):
                e.join_sum_columns(good, good, [good, bad])
        with pytest.raises(ValueError):
            e.join_sum_columns(good, good, [good[:99].contiguous()])         # the wrong length
        with pytest.raises(ValueError):
            e.join_sum_columns(good, good, [good] * (SUM_MAX_COLS + 1))
        assert e.join_sum_columns(good, good, [good]) == (100, [4950])
    finally:
        e.close()


def test_join_sum_columns_is_ordered_behind_queued_torch_work():
    """the keys and the weights are the last products of a queue of torch kernels issued right before the call, on a stream of its own"""
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
            wt = filler[F - nR:].clone()
            got = e.join_sum_columns(kR, kS, [wt])
        torch.cuda.synchronize()
        x = np.arange(F - nR, F, dtype=np.uint64)
        with np.errstate(over="ignore"):
            for _ in range(rounds):
                x = x * np.uint64(3) + np.uint64(1)
        assert got == (nR - nR // 2, [int(x[nR // 2:].sum(dtype=np.uint64))])
        assert e.bound_stream is None
    finally:
        e.close()
