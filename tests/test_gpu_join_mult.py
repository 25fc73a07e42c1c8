"""GPU suite: the multiplicity join rhj_join_mult_cols_dev / rhj_join_mult_dev (include/rhj.h) and Engine.join_multiplicity_columns:
for every tuple of R, out[rowR] += the number of tuples of S with its join value, or the sum of their weights.

The oracle is numpy, all in uint64: np.unique on S's values, np.add.at of the weights per distinct value, searchsorted for R, then
np.add.at into out by R's rowID.  Weights are drawn from the full 64-bit range, so the sums wrap.  Every comparison is exact.
  * paths by size: 1, 65, 3,001 and 30,011 rows with the automatic plan, 70,001 rows, 3,000,000 under Opts(2, 8, 8) in the narrow
    format; unweighted and weighted; NULL ids and id columns on either side; uniform and Zipf 0.9;
  * rowIDs of R that repeat (out accumulates) under an out_rows beyond every rowID (the tail stays 0);
  * the all-ones key among others; one value 70,000 times on both sides;
  * partitions of S beyond three LDS tables whose keys repeat, so that a key's weight is split among tables: the additive-tables case;
  * the repeats inside a call: a count-free region that overflows (out is not added twice); one rowID of 2^32 on S, and on R;
  * the guards: rowS == wS_rows and rowR == out_rows are RHJ_E_INVALID, and the context goes on;
  * n = 0 and n = 1, a disjoint S, invalid arguments; the AoS entry; the aggregating join's count and sums;
  * join_multiplicity_columns on int64 tensors: refused tensors, queued torch work on a side stream."""
import numpy as np
import pytest
import torch

import cf_cases
from oracle.pyoracle import TUPLE
from radixhashjoin_amd import Engine, Opts, RhjError, unmix64
from radixhashjoin_amd.binding import RHJ_E_INVALID, plan as resolve_plan

pytestmark = pytest.mark.gpu
PLAN = Opts(2, 8, 8)
JK_MULT = 14
AGG_FILL = 4608                                                            # rhj_internal.h: distinct keys one LDS table takes
DIRECT_DEV = 5 * 4224                                                      # device-resident inputs up to here are joined unpartitioned
MASK64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


# ---- input builders (those of test_gpu_join_sum.py) --------------------------------------------------------------------------
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


def weights(rows, seed=1):
    return np.random.default_rng(rows + seed).integers(0, 1 << 64, rows, dtype=np.uint64)


def oracle(rv, rid, sv, sid, w, out_rows):
    """(out, total).  rid / sid: the rowIDs (int64 index arrays); w: the weight column indexed by S's rowID, or None"""
    out = np.zeros(out_rows, dtype=np.uint64)
    if len(rv) and len(sv):
        u, inv = np.unique(sv, return_inverse=True)
        share = np.zeros(len(u), dtype=np.uint64)
        np.add.at(share, inv.reshape(-1), w[sid] if w is not None else np.uint64(1))
        pos = np.minimum(np.searchsorted(u, rv), len(u) - 1)
        np.add.at(out, rid, np.where(u[pos] == rv, share[pos], np.uint64(0)))
    return out, int(out.sum(dtype=np.uint64))


@pytest.fixture(scope="module")
def inputs():
    """(dist, nR, nS, seed) -> (R, S, W): built once, shared, never written.  W: nS words, indexed by S's rowID"""
    cache = {}

    def get(dist, n, nS=None, seed=0):
        key = (dist, n, nS, seed)
        if key not in cache:
            R, S = make(dist, n, nS or n, seed)
            cache[key] = (R, S, weights(len(S)))
        return cache[key]
    return get


def run_cols(eng, R, S, W=None, ids_R=True, ids_S=True, out_rows=None, opts=None, e_code=None):
    """the columnar entry against the oracle; returns (out, total).  ids_*: False = NULL id column, rowID = position.
    e_code: the call must fail with this code instead"""
    nR, nS = len(R), len(S)
    rid = R["key"].astype(np.int64) if ids_R else np.arange(nR)
    sid = S["key"].astype(np.int64) if ids_S else np.arange(nS)
    if out_rows is None:
        out_rows = nR
    bufs = [eng.to_device(np.ascontiguousarray(R["payload"])), eng.to_device(np.ascontiguousarray(R["key"])) if ids_R else None,
            eng.to_device(np.ascontiguousarray(S["payload"])), eng.to_device(np.ascontiguousarray(S["key"])) if ids_S else None,
            eng.to_device(W) if W is not None else None,
            eng.to_device(np.full(max(out_rows, 1), 0xDEADBEEF, dtype=np.uint64))]   # the call zeroes out itself
    dv, di, ds, dsi, dw, dout = bufs
    try:
        if e_code is not None:
            with pytest.raises(RhjError) as err:
                eng.join_mult_cols_dev(dv, di, nR, ds, dsi, nS, dout, out_rows, dw, len(W) if W is not None else 0, opts=opts)
            assert err.value.code == e_code
            return None
        total = eng.join_mult_cols_dev(dv, di, nR, ds, dsi, nS, dout, out_rows, dw, len(W) if W is not None else 0, opts=opts)
        out = dout.to_numpy(np.uint64, out_rows) if out_rows else np.zeros(0, dtype=np.uint64)
        exp_out, exp_total = oracle(R["payload"], rid, S["payload"], sid, W, out_rows)
        print(f"total {total} expected {exp_total} kernel {eng.info('last.join_kernel')} tables {eng.info('last.semi_tables')} "
              f"narrow {eng.info('last.narrow')} tasks {eng.timings()['ntasks']} wrong words {int((out != exp_out).sum())}")
        assert total == exp_total
        assert np.array_equal(out, exp_out)
    finally:
        for b in bufs:
            if b is not None:
                b.free()
    return out, total


# ---- paths by size -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["count", "weighted"])
@pytest.mark.parametrize("ids", [False, True], ids=["null", "ids"])
@pytest.mark.parametrize("dist", ["uniform", "zipf"])
@pytest.mark.parametrize("n", [1, 65, 3_001, 30_011])
def test_small_sizes_automatic_plan(eng, inputs, n, dist, ids, weighted):
    R, S, W = inputs(dist, n)
    eng.set_option("partition.narrow", -1)
    run_cols(eng, R, S, W if weighted else None, ids, ids)
    assert eng.info("last.join_kernel") == JK_MULT and eng.info("last.narrow") == 0
    assert eng.timings()["passes"] == (0 if n <= DIRECT_DEV else 1)


@pytest.mark.parametrize("weighted", [False, True], ids=["count", "weighted"])
@pytest.mark.parametrize("dist,ids_R,ids_S", [("uniform", True, False), ("zipf", False, True), ("dups", True, True)])
def test_seventy_thousand_one_pass(eng, inputs, dist, ids_R, ids_S, weighted):
    n = 70_001
    assert resolve_plan(n, n).passes == 1
    R, S, W = inputs(dist, n)
    eng.set_option("partition.narrow", -1)
    _, total = run_cols(eng, R, S, W if weighted else None, ids_R, ids_S)
    assert total > 0
    assert eng.info("last.join_kernel") == JK_MULT and eng.info("last.semi_tables") == 1 and eng.timings()["passes"] == 1


@pytest.mark.parametrize("dist,weighted,ids_R,ids_S", [("uniform", True, False, False), ("zipf", False, True, False), ("dups", True, True, True)])
def test_three_million_narrow_two_pass(eng, inputs, dist, weighted, ids_R, ids_S):
    R, S, W = inputs(dist, 3_000_000)
    eng.set_option("partition.narrow", 2)
    eng.set_option("partition.countfree", 0)
    try:
        run_cols(eng, R, S, W if weighted else None, ids_R, ids_S, opts=PLAN)
        assert eng.info("last.narrow") == 2 and eng.info("last.cols_R") == 1 and eng.info("last.cols_S") == 1
        assert eng.info("last.join_kernel") == JK_MULT and eng.info("last.semi_tables") == 1
    finally:
        eng.set_option("partition.narrow", -1)
        eng.set_option("partition.countfree", -1)


# ---- out accumulates; its tail stays zero ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3_001, 70_001])
@pytest.mark.parametrize("weighted", [False, True], ids=["count", "weighted"])
def test_repeated_rowids_of_R_accumulate_and_the_tail_is_zero(eng, inputs, n, weighted):
    R0, S, W = inputs("dups", n)
    R = R0.copy()
    R["key"] = np.random.default_rng(n).integers(0, n // 3, n).astype(np.uint64)       # about three tuples per row
    out, total = run_cols(eng, R, S, W if weighted else None, True, True, out_rows=n + 1_000)
    assert total > 0 and not out[n // 3:].any()


# ---- keys and multiplicities -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["count", "weighted"])
def test_the_all_ones_key_among_others(eng, inputs, weighted):
    R0, S0, W = inputs("uniform", 3_001)
    R, S = R0.copy(), S0.copy()
    R["payload"][::7] = np.uint64(MASK64)
    S["payload"][::5] = np.uint64(MASK64)
    R["payload"][::11] = np.uint64(unmix64(MASK64))                        # (joins compare mix64(value): this one becomes all ones)
    S["payload"][::13] = np.uint64(unmix64(MASK64))
    out, total = run_cols(eng, R, S, W if weighted else None)
    if not weighted:
        assert total >= 2 * (3_001 // 77) * (3_001 // 65)


@pytest.mark.parametrize("value", [0x0FEDCBA987654321, MASK64], ids=["one-value", "all-ones"])
def test_one_value_seventy_thousand_times_on_both_sides(eng, value):
    n = 70_000
    rng = np.random.default_rng(6)
    R, S = rel(rng, n, np.full(n, value, dtype=np.uint64)), rel(rng, n, np.full(n, value, dtype=np.uint64))
    out, total = run_cols(eng, R, S)
    assert total == n * n > 1 << 32 and (out == n).all()
    W = weights(n)
    out, total = run_cols(eng, R, S, W)
    assert (out == W.sum(dtype=np.uint64)).all()


# ---- additive tables: a key's weight split among the tables of one task --------------------------------------------------------
@pytest.mark.parametrize("opts,parts", [(Opts(0, 0, 0, 1 << 30), 1), (Opts(1, 1, 0, 4096), 2)], ids=["unpartitioned", "one-pass"])
def test_partitions_beyond_three_tables_with_keys_in_several_of_them(eng, opts, parts):
    n = 70_000
    rng = np.random.default_rng(n)
    keys = rng.permutation(np.arange(1, 2 * n, 4, dtype=np.uint64))         # 35,000 distinct keys, each twice in S
    assert len(keys) // parts > 3 * AGG_FILL
    sv = np.concatenate([keys, keys])[rng.permutation(n)]
    rv = np.concatenate([keys[rng.integers(0, len(keys), n // 2)], rng.integers(0, n, n - n // 2).astype(np.uint64) * np.uint64(4) + np.uint64(2)])
    R, S, W = rel(rng, n, rv[rng.permutation(n)]), rel(rng, n, sv), weights(n)
    eng.set_option("partition.narrow", -1)
    for w in (None, W):
        _, total = run_cols(eng, R, S, w, opts=opts)
        assert eng.info("last.semi_tables") >= 3 and eng.info("last.join_kernel") == JK_MULT
        if w is None:
            assert total == 2 * (n // 2)


# ---- the repeats inside a call -----------------------------------------------------------------------------------------------
def test_count_free_overflow_repeats_S_and_out_is_not_added_twice(inputs):
    R, S, W = inputs("quarter", 3_000_000)
    # R fits its count-free regions (its largest pass-1 piece is 36 or 37 of 64 slots), S does not: R stands, "last.countfree_R" is 1
    assert int(cf_cases.piece_lengths(R).max()) <= cf_cases.cap(cf_cases.unit_len(len(R)), 8) < int(cf_cases.piece_lengths(S).max())
    e = Engine(0)
    try:
        e.set_option("partition.narrow", 2)
        e.set_option("partition.countfree", 1)
        run_cols(e, R, S, W, ids_R=False, ids_S=False, opts=PLAN)
        assert e.info("last.narrow") == 2 and e.info("last.countfree_S") == 2 and e.info("last.countfree_R") == 1
        assert e.info("last.join_kernel") == JK_MULT
    finally:
        e.close()


def test_one_wide_id_falls_back_for_that_call_only(inputs):
    """a rowID of 2^32 in a narrow format repeats the call at 16 bytes: on S (unweighted: the rowID is read, never used as an address)
    the result is exact; on R, and on S under weights, the row lies beyond out_rows / wS_rows and the guard answers"""
    R0, S0, W = inputs("uniform", 90_000, 120_000, seed=2)
    exp, _ = oracle(R0["payload"], np.arange(len(R0)), S0["payload"], np.arange(len(S0)), None, len(R0))
    hit_R = int(np.flatnonzero(exp)[7])                                    # a tuple of R with partners ...
    hit_S = int(np.flatnonzero(S0["payload"] == R0["payload"][hit_R])[0])  # ... and one of them
    e = Engine(0)
    try:
        e.set_option("partition.narrow", 2)                                # set once, never re-armed below
        for side, weighted in ((None, True), ("S", False), (None, False), ("S", True), (None, True), ("R", False), (None, True)):
            R, S = R0.copy(), S0.copy()
            if side == "R":
                R["key"][hit_R] = np.uint64(1 << 32)
            if side == "S":
                S["key"][hit_S] = np.uint64(1 << 32)
            refused = side == "R" or (side == "S" and weighted)
            run_cols(e, R, S, W if weighted else None, opts=PLAN, e_code=RHJ_E_INVALID if refused else None)
            assert e.info("last.narrow") == (0 if side else 2), (side, weighted)
            if side is None:
                assert e.info("last.cols_R") == 1 and e.info("last.cols_S") == 1
    finally:
        e.close()


# ---- the guards --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3_001, 70_001])
def test_rows_at_the_bounds_are_refused_and_the_context_goes_on(eng, inputs, n):
    R0, S0, W = inputs("uniform", n)
    exp, _ = oracle(R0["payload"], R0["key"].astype(np.int64), S0["payload"], S0["key"].astype(np.int64), None, n)
    hit_R = int(np.flatnonzero(R0["key"] == np.flatnonzero(exp)[3])[0])    # a tuple of R that matches ...
    hit_S = int(np.flatnonzero(S0["payload"] == R0["payload"][hit_R])[0])  # ... and a partner
    eng.set_option("partition.narrow", -1)
    R = R0.copy()
    R["key"][hit_R] = np.uint64(n)                                         # == out_rows
    for w in (None, W):
        run_cols(eng, R, S0, w, e_code=RHJ_E_INVALID)
    run_cols(eng, R, S0, W, out_rows=n + 1)                                # one more word: the same call is fine
    S = S0.copy()
    S["key"][hit_S] = np.uint64(n)                                         # == wS_rows
    run_cols(eng, R0, S, W, e_code=RHJ_E_INVALID)
    run_cols(eng, R0, S, None, ids_S=True)                                 # unweighted: no weight column, no guard
    run_cols(eng, R0, S0, W)                                               # a correct call on the same context is exact


# ---- degenerate sizes, a disjoint S, invalid arguments -------------------------------------------------------------------------
def test_degenerate_sizes(eng, inputs):
    R, S, W = inputs("uniform", 3_001)
    for w in (None, W):
        out, total = run_cols(eng, R, S[:0], None if w is None else W[:0], ids_S=False)          # nS == 0: out all zero, no launch
        assert total == 0 and not out.any()
        assert eng.info("last.join_kernel") == -1 and eng.info("last.semi_tables") == 0
        assert run_cols(eng, R[:0], S, w, ids_R=False, out_rows=0)[1] == 0                        # nR == 0, no output word
        out, total = run_cols(eng, R[:0], S, w, ids_R=False, out_rows=77)                         # nR == 0: the words are zeroed
        assert total == 0 and not out.any()
        assert run_cols(eng, R[:0], S[:0], None, False, False, out_rows=0)[1] == 0
    exp, _ = oracle(R["payload"], np.arange(len(R)), S["payload"], np.arange(len(S)), None, len(R))
    hit, miss = int(np.flatnonzero(exp)[0]), int(np.flatnonzero(exp == 0)[0])
    one_s = S[S["payload"] == R["payload"][hit]][:1]
    assert run_cols(eng, R, one_s, W)[1] == int(W[int(one_s["key"][0])]) * int((R["payload"] == one_s["payload"][0]).sum()) & MASK64
    one_r = R[hit: hit + 1]
    assert run_cols(eng, one_r, S, None, out_rows=len(R))[1] == int(exp[hit])
    assert run_cols(eng, R[miss: miss + 1], S, W, out_rows=len(R))[1] == 0
    assert run_cols(eng, one_r, one_s, None, ids_R=False, ids_S=False, out_rows=1)[1] == 1


def test_disjoint_S(eng, inputs):
    R, S0, W = inputs("uniform", 70_001)
    S = S0.copy()
    S["payload"] |= np.uint64(1 << 63)
    for w in (None, W):
        out, total = run_cols(eng, R, S, w)
        assert total == 0 and not out.any()
        assert eng.info("last.join_kernel") == JK_MULT


def test_invalid_arguments(eng, inputs):
    R, S, W = inputs("uniform", 3_001)
    n = len(R)
    dv, ds = eng.to_device(np.ascontiguousarray(R["payload"])), eng.to_device(np.ascontiguousarray(S["payload"]))
    dR, dS, dout = eng.to_device(R), eng.to_device(S), eng.alloc(8 * n)
    for args in ((None, None, n, ds, None, n, dout, n), (dv, None, n, None, None, n, dout, n), (None, dv, n, ds, None, n, dout, n),
                 (None, None, 5, None, None, 0, dout, n), (dv, None, n, ds, None, n, None, n), (dv, None, 0, ds, None, n, None, n)):
        with pytest.raises(RhjError) as err:
            eng.join_mult_cols_dev(*args)
        assert err.value.code == RHJ_E_INVALID
    for args in ((None, n, dS, n, dout, n), (dR, n, None, n, dout, n), (dR, n, dS, n, None, n)):
        with pytest.raises(RhjError) as err:
            eng.join_mult_dev(*args)
        assert err.value.code == RHJ_E_INVALID
    assert eng.lib.rhj_join_mult_cols_dev(eng.ctx, dv.ptr, None, n, ds.ptr, None, n, None, 0, None, dout.ptr, n, None) == RHJ_E_INVALID   # NULL out_total
    assert eng.lib.rhj_join_mult_dev(eng.ctx, dR.ptr, n, dS.ptr, n, None, 0, None, dout.ptr, n, None) == RHJ_E_INVALID
    with pytest.raises(RhjError) as err:                                   # out_rows == 0 with tuples that match: every row is beyond
        eng.join_mult_cols_dev(dv, None, n, ds, None, n, None, 0)
    assert err.value.code == RHJ_E_INVALID
    for b in (dv, ds, dR, dS, dout):
        b.free()


# ---- the AoS entry, and the aggregating join -----------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["count", "weighted"])
def test_aos_entry_agrees(eng, inputs, weighted):
    R, S, W = inputs("dups", 70_001)
    n = len(R)
    w = W if weighted else None
    dR, dS, dw, dout = eng.to_device(R), eng.to_device(S), eng.to_device(W) if weighted else None, eng.alloc(8 * n)
    total = eng.join_mult_dev(dR, n, dS, len(S), dout, n, dw, len(W) if weighted else 0)
    assert eng.info("last.cols_R") == 0 and eng.info("last.join_kernel") == JK_MULT
    out = dout.to_numpy(np.uint64, n)
    for b in (dR, dS, dw, dout):
        if b is not None:
            b.free()
    cols_out, cols_total = run_cols(eng, R, S, w)
    assert total == cols_total and np.array_equal(out, cols_out)


def test_total_and_weighted_sums_are_the_aggregating_joins(eng, inputs):
    """total = join_sum_cols_dev's count; the sum over R's rows of out[r] * x[r] = its sum of the column x"""
    R, S, _ = inputs("dups", 70_001)
    n = len(R)
    out, total = run_cols(eng, R, S, None, ids_R=True, ids_S=False)
    x = [weights(n, seed=s) for s in (2, 3)]
    dv, di, ds = (eng.to_device(np.ascontiguousarray(a)) for a in (R["payload"], R["key"], S["payload"]))
    dx = [eng.to_device(c) for c in x]
    count, sums = eng.join_sum_cols_dev(dv, di, n, ds, len(S), dx, n)
    for b in [dv, di, ds] + dx:
        b.free()
    assert total == count
    assert [int((out * c).sum(dtype=np.uint64)) for c in x] == sums


# ---- Engine.join_multiplicity_columns ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nR,nS", [(1_000, 3_000), (200_000, 300_000)])
def test_join_multiplicity_columns_against_numpy(nR, nS):
    rng = np.random.default_rng(nR)
    kR = rng.integers(-(1 << 62), 1 << 62, nR, dtype=np.int64)
    kR[: nR // 10] = kR[nR // 2: nR // 2 + nR // 10]
    kR[0], kR[1] = -1, np.iinfo(np.int64).min                              # (-1: the all-ones word)
    kS = kR[rng.integers(0, nR, nS)]
    kS[::13] = rng.integers(-(1 << 62), 1 << 62, len(kS[::13]), dtype=np.int64)
    kS[5], kS[6] = -1, np.iinfo(np.int64).min
    w = rng.integers(-(1 << 63), (1 << 63) - 1, nS, dtype=np.int64)
    e = Engine(0)
    try:
        tR, tS, tw = torch.from_numpy(kR).cuda(), torch.from_numpy(kS).cuda(), torch.from_numpy(w).cuda()
        for weight, tensor in ((None, None), (w.view(np.uint64), tw)):
            exp_out, exp_total = oracle(kR.view(np.uint64), np.arange(nR), kS.view(np.uint64), np.arange(nS), weight, nR)
            mult, total = e.join_multiplicity_columns(tR, tS, tensor)
            assert mult.dtype == torch.int64 and mult.device == tR.device and mult.shape == (nR,)
            assert isinstance(total, int) and total == exp_total
            assert np.array_equal(mult.cpu().numpy().view(np.uint64), exp_out)
        mult, total = e.join_multiplicity_columns(tR, tS[:0].contiguous(), tw[:0].contiguous())
        assert total == 0 and mult.shape == (nR,) and not mult.any()
        mult, total = e.join_multiplicity_columns(tR[:0].contiguous(), tS)
        assert total == 0 and mult.shape == (0,)
    finally:
        e.close()


def test_join_multiplicity_columns_refuses_what_it_cannot_read():
    e = Engine(0)
    try:
        good = torch.arange(100, device="cuda", dtype=torch.int64)
        for bad in (good.to(torch.int32), good.to(torch.float64), torch.arange(200, device="cuda")[::2], good.cpu(),
                    good.reshape(10, 10), list(range(5))):
            with pytest.raises(ValueError):
                e.join_multiplicity_columns(bad, good)
            with pytest.raises(ValueError):
                e.join_multiplicity_columns(good, bad)
            with pytest.raises(ValueError):
                e.join_multiplicity_columns(good, good, bad)
        with pytest.raises(ValueError):
            e.join_multiplicity_columns(good, good[:50].contiguous(), good)  # weights as long as R, not as S
        mult, total = e.join_multiplicity_columns(good, good, good)
        assert total == 4950 and torch.equal(mult, good)
    finally:
        e.close()


def test_join_multiplicity_columns_is_ordered_behind_queued_torch_work():
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
            wt = filler[F - nS:].clone()
            mult, total = e.join_multiplicity_columns(kR, kS, wt)
        torch.cuda.synchronize()
        x = np.arange(F - nS, F, dtype=np.uint64)
        with np.errstate(over="ignore"):
            for _ in range(rounds):
                x = x * np.uint64(3) + np.uint64(1)
        exp = np.zeros(nR, dtype=np.uint64)
        exp[nR // 2:] = x[: nR - nR // 2]                                  # row nR/2 + i of R meets row i of S alone
        assert np.array_equal(mult.cpu().numpy().view(np.uint64), exp) and total == int(exp.sum(dtype=np.uint64))
        assert e.bound_stream is None
    finally:
        e.close()
