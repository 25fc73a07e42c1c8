"""GPU suite: the lookup join rhj_lookup_cols_dev / rhj_lookup_dev, the gather rhj_gather_cols_fill (include/rhj.h) and
Engine.lookup_columns: for every row of R the smallest (first) or largest (last) rowID of S among the tuples of S with its join value,
all ones where there is none.

The oracle is numpy: one stable lexsort((rowS, valS)), the first or last rowS of every run of equal values through searchsorted, then
np.minimum.at (unsigned) / np.maximum.at (signed) into an all-ones array by R's rowID; matched = the words that are not all ones.
Every comparison is exact and covers the whole of d_out, under both `which` values unless noted.  d_out is allocated SLACK words
longer than out_rows and the slack must stay as it was: a broken guard shows as a wrong answer.
  * paths by size: 1, 65, 3,001 and 30,011 rows with the automatic plan, 70,001 rows in one pass, 3,000,000 under Opts(2, 8, 8) in the
    narrow format; NULL ids and id columns; uniform, Zipf 0.9 and repeated values;
  * a partition of S beyond three LDS tables where every key sits in S twice: the smaller rowS of a key is in a LATER table than the
    larger one for thousands of keys -- a kernel that stores, or keeps the first table's answer, fails;
  * rowIDs of R that repeat; values the table can mistake for its empty marker, and the builders of keyed_table_cases.py;
  * rowS 0, 2^63 - 1 and 2^63; rowR == out_rows; the repeats inside a call; degenerate sizes and invalid arguments;
  * agreement with the 16-byte entry, the semi join and the multiplicity join; two runs give the same bytes;
  * rhj_gather_cols_fill against numpy, its guard and its arguments; Engine.lookup_columns on int64 tensors."""
import numpy as np
import pytest
import torch

import cf_cases
import keyed_table_cases as K
from oracle.pyoracle import TUPLE
from radixhashjoin_amd import LOOKUP_FIRST, LOOKUP_LAST, LOOKUP_MAX_COLS, NO_ROW, SEMI, Engine, Opts, RhjError, unmix64
from radixhashjoin_amd.binding import RHJ_E_INVALID, plan as resolve_plan
from test_gpu_join_mult import make, rel

pytestmark = pytest.mark.gpu
PLAN = Opts(2, 8, 8)
JK_LOOKUP = 17
AGG_FILL = 4608                                                            # rhj_internal.h: distinct keys one LDS table takes
BUILD_TILE = 1024                                                          # ... and the tuples of one build tile
DIRECT_DEV = 5 * 4224                                                      # device-resident inputs up to here are joined unpartitioned
U64 = np.uint64
ONES = U64(NO_ROW)
SLACK = 8                                                                  # words of d_out behind out_rows
STAMP = U64(0xDEADBEEFDEADBEEF)
WHICH = [LOOKUP_FIRST, LOOKUP_LAST]
which_ids = pytest.mark.parametrize("which", WHICH, ids=["first", "last"])


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def inputs():
    """(dist, nR, nS, seed) -> (R, S): built once, shared, never written"""
    cache = {}

    def get(dist, n, nS=None, seed=0):
        key = (dist, n, nS, seed)
        if key not in cache:
            cache[key] = make(dist, n, nS or n, seed)
        return cache[key]
    return get


def oracle(rv, rid, sv, sid, which, out_rows):
    """(out, matched).  rid: R's rowIDs as an int64 index array; sid: S's rowIDs as uint64"""
    out = np.full(out_rows, ONES, dtype=U64)
    if len(rv) and len(sv):
        sid = np.asarray(sid, dtype=U64)
        order = np.lexsort((sid, sv))
        vals, rows = sv[order], sid[order]
        lo, hi = np.searchsorted(vals, rv, "left"), np.searchsorted(vals, rv, "right")
        hit = hi > lo
        if which == LOOKUP_FIRST:
            np.minimum.at(out, rid[hit], rows[lo[hit]])
        else:
            np.maximum.at(out.view(np.int64), rid[hit], rows[hi[hit] - 1].view(np.int64))
    return out, int((out != ONES).sum())


def run_cols(eng, R, S, which, ids_R=True, ids_S=True, out_rows=None, opts=None, e_code=None):
    """the columnar entry against the oracle; returns (out, matched).  ids_*: False = NULL id column, rowID = position.
    e_code: the call must fail with this code instead"""
    nR, nS = len(R), len(S)
    rid = R["key"].astype(np.int64) if ids_R else np.arange(nR)
    sid = S["key"] if ids_S else np.arange(nS, dtype=U64)
    if out_rows is None:
        out_rows = nR
    bufs = [eng.to_device(np.ascontiguousarray(R["payload"])), eng.to_device(np.ascontiguousarray(R["key"])) if ids_R else None,
            eng.to_device(np.ascontiguousarray(S["payload"])), eng.to_device(np.ascontiguousarray(S["key"])) if ids_S else None,
            eng.to_device(np.full(out_rows + SLACK, STAMP, dtype=U64))]    # the call fills out itself
    dv, di, ds, dsi, dout = bufs
    try:
        if e_code is not None:
            with pytest.raises(RhjError) as err:
                eng.lookup_cols_dev(dv, di, nR, ds, dsi, nS, dout, out_rows, which, opts=opts)
            assert err.value.code == e_code
            assert (dout.to_numpy(U64, out_rows + SLACK)[out_rows:] == STAMP).all()
            return None
        matched = eng.lookup_cols_dev(dv, di, nR, ds, dsi, nS, dout, out_rows, which, opts=opts)
        got = dout.to_numpy(U64, out_rows + SLACK)
        out, slack = got[:out_rows], got[out_rows:]
        exp_out, exp_matched = oracle(R["payload"], rid, S["payload"], sid, which, out_rows)
        print(f"which {which} matched {matched} expected {exp_matched} kernel {eng.info('last.join_kernel')} tables "
              f"{eng.info('last.semi_tables')} narrow {eng.info('last.narrow')} tasks {eng.timings()['ntasks']} wrong words "
              f"{int((out != exp_out).sum())}")
        assert (slack == STAMP).all()
        assert matched == exp_matched
        assert np.array_equal(out, exp_out)
    finally:
        for b in bufs:
            if b is not None:
                b.free()
    return out, matched


# ---- paths by size -----------------------------------------------------------------------------------------------------------
@which_ids
@pytest.mark.parametrize("ids", [False, True], ids=["null", "ids"])
@pytest.mark.parametrize("dist", ["uniform", "zipf", "dups"])
@pytest.mark.parametrize("n", [1, 65, 3_001, 30_011])
def test_small_sizes_automatic_plan(eng, inputs, n, dist, ids, which):
    R, S = inputs(dist, n)
    eng.set_option("partition.narrow", -1)
    run_cols(eng, R, S, which, ids, ids)
    assert eng.info("last.join_kernel") == JK_LOOKUP and eng.info("last.narrow") == 0
    assert eng.timings()["passes"] == (0 if n <= DIRECT_DEV else 1)


@which_ids
@pytest.mark.parametrize("dist,ids_R,ids_S", [("uniform", True, False), ("zipf", False, True), ("dups", True, True)])
def test_seventy_thousand_one_pass(eng, inputs, dist, ids_R, ids_S, which):
    n = 70_001
    assert resolve_plan(n, n).passes == 1
    R, S = inputs(dist, n)
    eng.set_option("partition.narrow", -1)
    _, matched = run_cols(eng, R, S, which, ids_R, ids_S)
    assert matched > 0
    assert eng.info("last.join_kernel") == JK_LOOKUP and eng.info("last.semi_tables") == 1 and eng.timings()["passes"] == 1


@pytest.mark.parametrize("dist,which,ids_R,ids_S", [("uniform", LOOKUP_FIRST, False, False), ("zipf", LOOKUP_LAST, True, False),
                                                    ("dups", LOOKUP_FIRST, True, True), ("dups", LOOKUP_LAST, True, True)])
def test_three_million_narrow_two_pass(eng, inputs, dist, which, ids_R, ids_S):
    R, S = inputs(dist, 3_000_000)
    eng.set_option("partition.narrow", 2)
    eng.set_option("partition.countfree", 0)
    try:
        run_cols(eng, R, S, which, ids_R, ids_S, opts=PLAN)
        assert eng.info("last.narrow") == 2 and eng.info("last.cols_R") == 1 and eng.info("last.cols_S") == 1
        assert eng.info("last.join_kernel") == JK_LOOKUP and eng.info("last.semi_tables") == 1
    finally:
        eng.set_option("partition.narrow", -1)
        eng.set_option("partition.countfree", -1)


# ---- the minimum in a later table ----------------------------------------------------------------------------------------------
def table_of_rows(keys_in_order):
    """per tuple of one task's table side, read in this order, the number of the LDS table that takes it: the close rule of
    keyed_table_cases.tables_closed (whole tiles of BUILD_TILE tuples while filled + BUILD_TILE <= AGG_FILL distinct keys)"""
    keys = np.asarray(keys_in_order, dtype=U64)
    table = np.empty(len(keys), dtype=np.int64)
    done, tables = 0, 0
    while done < len(keys):
        inside, filled = set(), 0
        while done < len(keys) and filled + BUILD_TILE <= AGG_FILL:
            tile = keys[done: done + BUILD_TILE]
            inside.update(tile[tile != ONES].tolist())
            filled = len(inside)
            table[done: done + len(tile)] = tables
            done += len(tile)
        tables += 1
    return table, tables


@pytest.mark.parametrize("opts,parts", [(Opts(0, 0, 0, 1 << 30), 1), (Opts(1, 1, 0, 4096), 2)], ids=["unpartitioned", "one-pass"])
def test_the_smaller_rowid_of_a_key_sits_in_a_later_table(eng, opts, parts):
    n = 70_000
    rng = np.random.default_rng(n)
    keys = rng.permutation(np.arange(1, 2 * n, 4, dtype=U64))               # 35,000 distinct keys, each twice in S
    assert len(keys) // parts > 3 * AGG_FILL
    sv = np.concatenate([keys, keys])[rng.permutation(n)]
    rv = np.concatenate([keys[rng.integers(0, len(keys), n // 2)], rng.integers(0, n, n - n // 2).astype(U64) * U64(4) + U64(2)])
    R, S = rel(rng, n, rv[rng.permutation(n)]), rel(rng, n, sv)             # S's ids: a random permutation
    if parts == 1:                                                          # the one task reads S in input order
        table, tables = table_of_rows(S["payload"])
        assert tables == K.tables_closed(S["payload"])
        order = np.lexsort((S["key"], S["payload"]))                        # per key: the row with the smaller id, then the other
        small, large = order[0::2], order[1::2]
        assert np.array_equal(S["payload"][small], S["payload"][large])
        later = int((table[small] > table[large]).sum())
        print(f"{tables} tables; {later} of {len(keys)} keys have their smaller rowS in a later table than their larger one")
        assert later >= 10_000 and int((table[small] < table[large]).sum()) >= 10_000
    eng.set_option("partition.narrow", -1)
    for which in WHICH:
        _, matched = run_cols(eng, R, S, which, opts=opts)
        assert eng.info("last.semi_tables") >= 3 and eng.info("last.join_kernel") == JK_LOOKUP
        assert matched == len(np.unique(R["key"][np.isin(R["payload"], keys)]))
        if parts == 1:
            assert eng.info("last.semi_tables") == tables


# ---- rowIDs of R that repeat ---------------------------------------------------------------------------------------------------
@which_ids
@pytest.mark.parametrize("n", [3_001, 70_001])
def test_repeated_rowids_of_R_take_the_extreme_over_all_their_tuples(eng, inputs, n, which):
    R0, S = inputs("dups", n)
    R = R0.copy()
    R["key"] = np.random.default_rng(n).integers(0, n // 3, n).astype(U64)  # about three tuples per row, with different values
    out, matched = run_cols(eng, R, S, which, True, True, out_rows=n + 1_000)
    assert (out[n // 3:] == ONES).all() and 0 < matched <= n // 3 < int(np.isin(R["payload"], S["payload"]).sum())


# ---- values the table can mistake ------------------------------------------------------------------------------------------------
@which_ids
@pytest.mark.parametrize("where", ["R", "S", "both"])
def test_the_all_ones_key_among_others(eng, inputs, where, which):
    R0, S0 = inputs("uniform", 3_001)
    R, S = R0.copy(), S0.copy()
    if where in ("R", "both"):
        R["payload"][::7] = ONES
        R["payload"][::11] = U64(unmix64(NO_ROW))                           # (joins compare mix64(value): this one becomes all ones)
    if where in ("S", "both"):
        S["payload"][::5] = ONES
        S["payload"][::13] = U64(unmix64(NO_ROW))
    for opts in (None, Opts(1, 4, 0)):                                      # unpartitioned (raw values) and one pass (mixed values)
        out, matched = run_cols(eng, R, S, which, opts=opts)
        if where == "both":
            for marker in (ONES, U64(unmix64(NO_ROW))):
                extreme = (min if which == LOOKUP_FIRST else max)(S["key"][S["payload"] == marker].tolist())
                assert (out[R["key"][R["payload"] == marker].astype(np.int64)] == U64(extreme)).all()


@which_ids
@pytest.mark.parametrize("value", [0x0FEDCBA987654321, NO_ROW], ids=["one-value", "all-ones"])
def test_one_value_seventy_thousand_times_on_both_sides(eng, value, which):
    n = 70_000
    rng = np.random.default_rng(6)
    R, S = rel(rng, n, np.full(n, value, dtype=U64)), rel(rng, n, np.full(n, value, dtype=U64))
    out, matched = run_cols(eng, R, S, which)
    assert matched == n and (out == U64(0 if which == LOOKUP_FIRST else n - 1)).all()


def as_rel(val, ids):
    t = np.empty(len(val), dtype=TUPLE)
    t["key"], t["payload"] = ids, val
    return t


PATHS = {"unpartitioned": (Opts(0, 0, 0), -1, -1), "one-pass": (Opts(1, 4, 0), -1, -1), "two-pass-narrow2": (Opts(2, 8, 8), 2, 0)}
PATTERN = {0: 0, 4: 9, 16: 0xBEEF}


def run_case(eng, case, path, tables=None):
    plan, narrow, countfree = PATHS[path]
    R, S = as_rel(case.valR, case.idR), as_rel(case.valS, case.idS)
    try:
        for which in WHICH:
            for ids in (True, False):
                eng.set_option("partition.narrow", narrow)
                eng.set_option("partition.countfree", countfree)
                run_cols(eng, R, S, which, ids, ids, opts=plan)
                assert eng.info("last.join_kernel") == JK_LOOKUP and eng.timings()["passes"] == plan.passes
                assert eng.info("last.narrow") == max(narrow, 0)
                if tables is not None:
                    assert eng.info("last.semi_tables") == tables
    finally:
        eng.set_option("partition.narrow", -1)
        eng.set_option("partition.countfree", -1)


@pytest.mark.parametrize("variant", K.MARKER_VARIANTS)
@pytest.mark.parametrize("path", list(PATHS))
def test_markers(eng, path, variant):
    rb = K.radix_bits(PATHS[path][0])
    case = K.markers(rb, PATTERN[rb], rb != 0, variant)
    run_case(eng, case, path, tables=K.tables_closed(case.valS) if rb == 0 else 1)


@pytest.mark.parametrize("variant", K.CHAIN_VARIANTS)
@pytest.mark.parametrize("path", list(PATHS))
def test_chain(eng, path, variant):
    rb = K.radix_bits(PATHS[path][0])
    case = K.chain(rb, PATTERN[rb], rb != 0, variant)
    run_case(eng, case, path, tables=K.tables_closed(case.valS) if rb == 0 else 1)


@pytest.mark.parametrize("probes", K.MARKER_PROBES)
@pytest.mark.parametrize("position", K.MARKER_POSITIONS)
def test_marker_and_tables(eng, position, probes):
    case = K.marker_and_tables(position, probes)
    run_case(eng, case, "unpartitioned", tables=K.tables_closed(case.valS))


@pytest.mark.parametrize("edge", K.FILL_EDGES, ids=[str(x) for x in K.FILL_EDGES])
def test_fill_edge(eng, edge):
    case = K.fill_edge(edge)
    run_case(eng, case, "unpartitioned", tables=K.tables_closed(case.valS))


# ---- rowS at the edges -------------------------------------------------------------------------------------------------------------
def single_partner(R, S):
    """(index in R, index in S): a tuple of R whose value occurs exactly once in S, and that tuple of S"""
    vals, first, counts = np.unique(S["payload"], return_index=True, return_counts=True)
    once = first[counts == 1]
    j = int(once[np.isin(S["payload"][once], R["payload"])][0])
    return int(np.flatnonzero(R["payload"] == S["payload"][j])[0]), j


@pytest.mark.parametrize("n", [3_001, 70_001])
def test_rowids_of_S_at_the_edges(eng, inputs, n):
    R, S0 = inputs("uniform", n)
    i, j = single_partner(R, S0)
    eng.set_option("partition.narrow", -1)
    S = S0.copy()                                                           # rowS 0 as the only partner: the word is 0, not "none"
    S["key"][S["key"] == 0] = S["key"][j]
    S["key"][j] = 0
    for which in WHICH:
        out, _ = run_cols(eng, R, S, which)
        assert out[int(R["key"][i])] == 0
    S = S0.copy()
    S["key"][j] = U64((1 << 63) - 1)                                        # the largest rowS a signed maximum orders
    for which in WHICH:
        out, _ = run_cols(eng, R, S, which)
        assert out[int(R["key"][i])] == U64((1 << 63) - 1)
    S["key"][j] = U64(1 << 63)
    run_cols(eng, R, S, LOOKUP_LAST, e_code=RHJ_E_INVALID)                  # ... and the first it cannot
    run_cols(eng, R, S0, LOOKUP_LAST)                                       # the context goes on
    out, _ = run_cols(eng, R, S, LOOKUP_FIRST)                              # an unsigned minimum orders every rowS
    assert out[int(R["key"][i])] == U64(1 << 63)


# ---- the guards --------------------------------------------------------------------------------------------------------------------
@which_ids
@pytest.mark.parametrize("n", [3_001, 70_001])
def test_a_row_at_out_rows_is_refused_and_the_context_goes_on(eng, inputs, n, which):
    R0, S = inputs("uniform", n)
    i, _ = single_partner(R0, S)
    eng.set_option("partition.narrow", -1)
    R = R0.copy()
    R["key"][i] = U64(n)                                                    # == out_rows, on a tuple that matches
    run_cols(eng, R, S, which, e_code=RHJ_E_INVALID)
    run_cols(eng, R, S, which, out_rows=n + 1)                              # one more word: the same call is fine
    run_cols(eng, R0, S, which)                                             # a correct call on the same context is exact


# ---- the repeats inside a call -------------------------------------------------------------------------------------------------------
@which_ids
def test_count_free_overflow_repeats_S_and_starts_from_nothing(inputs, which):
    R, S = inputs("quarter", 3_000_000)
    # R fits its count-free regions (its largest pass-1 piece is 36 or 37 of 64 slots), S does not: R stands, "last.countfree_R" is 1
    assert int(cf_cases.piece_lengths(R).max()) <= cf_cases.cap(cf_cases.unit_len(len(R)), 8) < int(cf_cases.piece_lengths(S).max())
    e = Engine(0)
    try:
        e.set_option("partition.narrow", 2)
        e.set_option("partition.countfree", 1)
        run_cols(e, R, S, which, ids_R=False, ids_S=False, opts=PLAN)
        assert e.info("last.narrow") == 2 and e.info("last.countfree_S") == 2 and e.info("last.countfree_R") == 1
        assert e.info("last.join_kernel") == JK_LOOKUP
    finally:
        e.close()


def test_one_wide_id_falls_back_for_that_call_only(inputs):
    """a rowID of 2^32 in a narrow format repeats the call at 16 bytes: on S the result is exact (the rowID is the answer); on R the
    row lies beyond out_rows and the guard answers"""
    R0, S0 = inputs("uniform", 90_000, 120_000, seed=2)
    i, j = single_partner(R0, S0)
    e = Engine(0)
    try:
        e.set_option("partition.narrow", 2)                                # set once, never re-armed below
        for side, which in ((None, LOOKUP_FIRST), ("S", LOOKUP_FIRST), (None, LOOKUP_LAST), ("S", LOOKUP_LAST), ("R", LOOKUP_FIRST),
                            (None, LOOKUP_LAST), ("R", LOOKUP_LAST), (None, LOOKUP_FIRST)):
            R, S = R0.copy(), S0.copy()
            if side == "R":
                R["key"][i] = U64(1 << 32)
            if side == "S":
                S["key"][j] = U64(1 << 32)
            res = run_cols(e, R, S, which, opts=PLAN, e_code=RHJ_E_INVALID if side == "R" else None)
            assert e.info("last.narrow") == (0 if side else 2), (side, which)
            if side == "S":
                assert res[0][int(R["key"][i])] == U64(1 << 32)
            if side is None:
                assert e.info("last.cols_R") == 1 and e.info("last.cols_S") == 1
    finally:
        e.close()


# ---- degenerate sizes, a disjoint S, invalid arguments ---------------------------------------------------------------------------------
@which_ids
def test_degenerate_sizes(eng, inputs, which):
    R, S = inputs("uniform", 3_001)
    out, matched = run_cols(eng, R, S[:0], which, ids_S=False)             # nS == 0: out all ones, no launch
    assert matched == 0 and (out == ONES).all()
    assert eng.info("last.join_kernel") == -1 and eng.info("last.semi_tables") == 0
    assert run_cols(eng, R[:0], S, which, ids_R=False, out_rows=0)[1] == 0
    out, matched = run_cols(eng, R[:0], S, which, ids_R=False, out_rows=77)   # nR == 0: the words are filled
    assert matched == 0 and len(out) == 77 and (out == ONES).all() and eng.info("last.join_kernel") == -1
    out, matched = run_cols(eng, R[:0], S[:0], which, False, False, out_rows=77)
    assert matched == 0 and (out == ONES).all() and eng.info("last.join_kernel") == -1
    i, j = single_partner(R, S)
    assert run_cols(eng, R, S[j: j + 1], which)[1] == int((R["payload"] == S["payload"][j]).sum())
    assert run_cols(eng, R[i: i + 1], S, which, out_rows=len(R))[1] == 1
    miss = int(np.flatnonzero(~np.isin(R["payload"], S["payload"]))[0])
    assert run_cols(eng, R[miss: miss + 1], S, which, out_rows=len(R))[1] == 0
    out, matched = run_cols(eng, R[i: i + 1], S[j: j + 1], which, ids_R=False, ids_S=False, out_rows=1)   # one tuple per side
    assert matched == 1 and out[0] == 0


@which_ids
def test_disjoint_S(eng, inputs, which):
    R, S0 = inputs("uniform", 70_001)
    S = S0.copy()
    S["payload"] |= U64(1 << 63)
    out, matched = run_cols(eng, R, S, which)
    assert matched == 0 and (out == ONES).all() and eng.info("last.join_kernel") == JK_LOOKUP


def test_invalid_arguments(eng, inputs):
    R, S = inputs("uniform", 3_001)
    n = len(R)
    dv, ds = eng.to_device(np.ascontiguousarray(R["payload"])), eng.to_device(np.ascontiguousarray(S["payload"]))
    dR, dS, dout = eng.to_device(R), eng.to_device(S), eng.alloc(8 * n)
    for args in ((None, None, n, ds, None, n, dout, n), (dv, None, n, None, None, n, dout, n), (None, dv, n, ds, None, n, dout, n),
                 (None, None, 5, None, None, 0, dout, n), (dv, None, n, ds, None, n, None, n), (dv, None, 0, ds, None, n, None, n),
                 (dv, None, n, ds, None, n, dout, n, 2), (dv, None, n, ds, None, n, dout, n, -1), (dv, None, 0, ds, None, n, dout, n, 2)):
        with pytest.raises(RhjError) as err:
            eng.lookup_cols_dev(*args)
        assert err.value.code == RHJ_E_INVALID
    for args in ((None, n, dS, n, dout, n), (dR, n, None, n, dout, n), (dR, n, dS, n, None, n), (dR, n, dS, n, dout, n, 2)):
        with pytest.raises(RhjError) as err:
            eng.lookup_dev(*args)
        assert err.value.code == RHJ_E_INVALID
    assert eng.lib.rhj_lookup_cols_dev(eng.ctx, dv.ptr, None, n, ds.ptr, None, n, 0, None, dout.ptr, n, None) == RHJ_E_INVALID   # NULL out_matched
    assert eng.lib.rhj_lookup_dev(eng.ctx, dR.ptr, n, dS.ptr, n, 0, None, dout.ptr, n, None) == RHJ_E_INVALID
    with pytest.raises(RhjError) as err:                                   # out_rows == 0 with tuples that match: every row is beyond
        eng.lookup_cols_dev(dv, None, n, ds, None, n, None, 0)
    assert err.value.code == RHJ_E_INVALID
    assert eng.lookup_cols_dev(dv, None, n, ds, None, n, dout, n) > 0      # the context goes on
    for b in (dv, ds, dR, dS, dout):
        b.free()


# ---- agreement with what exists --------------------------------------------------------------------------------------------------------
@which_ids
def test_agrees_with_the_aos_entry_the_semi_join_and_the_multiplicity_join(eng, inputs, which):
    R, S = inputs("dups", 70_001)
    n = len(R)
    cols_out, cols_matched = run_cols(eng, R, S, which)
    again, _ = run_cols(eng, R, S, which)
    assert cols_out.tobytes() == again.tobytes()                           # two runs: the same bytes
    dR, dS, dout = eng.to_device(R), eng.to_device(S), eng.alloc(8 * n)
    matched = eng.lookup_dev(dR, n, dS, len(S), dout, n, which)
    assert eng.info("last.cols_R") == 0 and eng.info("last.join_kernel") == JK_LOOKUP
    assert matched == cols_matched and np.array_equal(dout.to_numpy(U64, n), cols_out)
    dv, di, ds, dsi = (eng.to_device(np.ascontiguousarray(a)) for a in (R["payload"], R["key"], S["payload"], S["key"]))
    count = eng.semi_join_cols_dev(dv, di, n, ds, len(S), SEMI, dout, n)
    rows = np.sort(dout.to_numpy(U64, count))
    assert np.array_equal(rows, np.flatnonzero(cols_out != ONES).astype(U64))
    eng.join_mult_cols_dev(dv, di, n, ds, dsi, len(S), dout, n)
    assert np.array_equal(dout.to_numpy(U64, n) != 0, cols_out != ONES)
    for b in (dR, dS, dout, dv, di, ds, dsi):
        b.free()


# ---- rhj_gather_cols_fill ------------------------------------------------------------------------------------------------------------------
GATHER_SLACK = 5                                                           # rows the sources are allocated beyond src_rows


def run_gather(eng, srcs, src_rows, idx, fills, e_code=None):
    n, k = len(idx), len(srcs)
    d_srcs = [eng.to_device(np.concatenate([s, np.full(GATHER_SLACK, 0xBAD, dtype=U64)])) for s in srcs]
    d_idx = eng.to_device(idx) if n else None
    d_dsts = [eng.to_device(np.full(n + 1, STAMP, dtype=U64)) for _ in range(k)]
    try:
        if e_code is not None:
            with pytest.raises(RhjError) as err:
                eng.gather_cols_fill(d_srcs, src_rows, d_idx, n, fills, d_dsts)
            assert err.value.code == e_code
            return None
        eng.gather_cols_fill(d_srcs, src_rows, d_idx, n, fills, d_dsts)
        got = [d.to_numpy(U64, n + 1) for d in d_dsts]
        for j in range(k):
            none = idx == ONES
            src = srcs[j] if len(srcs[j]) else np.zeros(1, dtype=U64)           # (src_rows 0: every index is "no row")
            exp = np.where(none, U64(fills[j] & NO_ROW), src[np.where(none, 0, idx).astype(np.int64)])
            assert np.array_equal(got[j][:n], exp) and got[j][n] == STAMP, j
        return got
    finally:
        for b in d_srcs + d_dsts + [d_idx]:
            if b is not None:
                b.free()


@pytest.mark.parametrize("ncols", [1, 4])
@pytest.mark.parametrize("n", [1, 257, 100_003])
def test_gather_cols_fill_against_numpy(eng, n, ncols):
    rng = np.random.default_rng(n + ncols)
    src_rows = 50_000
    srcs = [rng.integers(0, 1 << 64, src_rows, dtype=U64) for _ in range(ncols)]
    idx = rng.integers(0, src_rows, n, dtype=U64)
    idx[::3] = ONES
    idx[-1] = U64(src_rows - 1)
    fills = [-1, 0, 1 << 63, 0x1234][:ncols]
    run_gather(eng, srcs, src_rows, idx, fills)
    run_gather(eng, srcs, src_rows, np.full(n, ONES, dtype=U64), fills)    # nothing but "no row"
    run_gather(eng, [s[:0] for s in srcs], 0, np.full(n, ONES, dtype=U64), fills)


def test_gather_cols_fill_guard_and_arguments(eng):
    rng = np.random.default_rng(5)
    src_rows, n = 1_000, 5_000
    srcs = [rng.integers(0, 1 << 64, src_rows, dtype=U64) for _ in range(2)]
    idx = rng.integers(0, src_rows, n, dtype=U64)
    bad = idx.copy()
    bad[n // 2] = U64(src_rows)                                            # (the sources are allocated longer: nothing strays)
    run_gather(eng, srcs, src_rows, bad, [7, 8], e_code=RHJ_E_INVALID)
    bad[n // 2] = ONES - U64(1)
    run_gather(eng, srcs, src_rows, bad, [7, 8], e_code=RHJ_E_INVALID)
    run_gather(eng, srcs, src_rows, idx, [7, 8])                           # the context goes on
    d_src, d_idx, d_dst = eng.to_device(srcs[0]), eng.to_device(idx), eng.alloc(8 * n)
    for k in (0, LOOKUP_MAX_COLS + 1):
        with pytest.raises(RhjError) as err:
            eng.gather_cols_fill([d_src] * k, src_rows, d_idx, n, [0] * k, [d_dst] * k)
        assert err.value.code == RHJ_E_INVALID
    for args in ((None, src_rows, d_idx, n, [0], [d_dst]), ([d_src], src_rows, None, n, [0], [d_dst]), ([d_src], src_rows, d_idx, n, None, [d_dst]),
                 ([d_src], src_rows, d_idx, n, [0], None), ([None], src_rows, d_idx, n, [0], [d_dst]), ([d_src], src_rows, d_idx, n, [0], [None])):
        with pytest.raises(RhjError) as err:
            eng.gather_cols_fill(*args)
        assert err.value.code == RHJ_E_INVALID
    eng.gather_cols_fill([d_src], src_rows, None, 0, [0], [d_dst])         # n == 0: accepted, no launch
    eng.gather_cols_fill([None], 0, None, 0, [0], [None])
    for b in (d_src, d_idx, d_dst):
        b.free()


# ---- Engine.lookup_columns -----------------------------------------------------------------------------------------------------------------
def columns_oracle(kR, kS, vals, fills, which):
    out, matched = oracle(kR.view(U64), np.arange(len(kR)), kS.view(U64), np.arange(len(kS), dtype=U64), which, len(kR))
    idx = out.view(np.int64)
    return idx, matched, [np.where(idx < 0, np.int64(f), v[np.maximum(idx, 0)]) if len(kS) else np.full(len(kR), f, dtype=np.int64)
                          for v, f in zip(vals, fills)]


@pytest.mark.parametrize("nR,nS", [(1_000, 3_000), (200_000, 300_000)])
def test_lookup_columns_against_numpy(nR, nS):
    rng = np.random.default_rng(nR)
    kR = rng.integers(-(1 << 62), 1 << 62, nR, dtype=np.int64)
    kR[: nR // 10] = kR[nR // 2: nR // 2 + nR // 10]
    kR[0], kR[1] = -1, np.iinfo(np.int64).min                              # (-1: the all-ones word)
    kS = kR[rng.integers(0, nR, nS)]
    kS[::13] = rng.integers(-(1 << 62), 1 << 62, len(kS[::13]), dtype=np.int64)
    kS[5], kS[6] = -1, np.iinfo(np.int64).min
    vals = [rng.integers(-(1 << 63), (1 << 63) - 1, nS, dtype=np.int64) for _ in range(2)]
    fills = [-7, 1 << 40]
    e = Engine(0)
    try:
        tR, tS, tv = torch.from_numpy(kR).cuda(), torch.from_numpy(kS).cuda(), [torch.from_numpy(v).cuda() for v in vals]
        for name, which in (("first", LOOKUP_FIRST), ("last", LOOKUP_LAST)):
            exp_idx, exp_matched, exp_vals = columns_oracle(kR, kS, vals, fills, which)
            idx, matched, values = e.lookup_columns(tR, tS, tv, fills, name)
            assert idx.dtype == torch.int64 and idx.device == tR.device and idx.shape == (nR,)
            assert isinstance(matched, int) and matched == exp_matched and 0 < matched < nR
            assert np.array_equal(idx.cpu().numpy(), exp_idx)
            assert isinstance(values, list) and len(values) == 2
            for v, ev in zip(values, exp_vals):
                assert v.dtype == torch.int64 and v.device == tR.device and v.shape == (nR,)
                assert np.array_equal(v.cpu().numpy(), ev)
        idx, matched, values = e.lookup_columns(tR, tS)                    # defaults: first, no values
        assert values == [] and np.array_equal(idx.cpu().numpy(), columns_oracle(kR, kS, [], [], LOOKUP_FIRST)[0])
        one = e.lookup_columns(tR, tS, tv[:1], 5)[2]                       # one fill for every tensor
        assert np.array_equal(one[0].cpu().numpy(), columns_oracle(kR, kS, vals[:1], [5], LOOKUP_FIRST)[2][0])
        idx, matched, values = e.lookup_columns(tR, tS[:0].contiguous(), [v[:0].contiguous() for v in tv], fills)   # empty sides
        assert matched == 0 and idx.shape == (nR,) and bool((idx == -1).all())
        assert [bool((v == f).all()) and v.shape == (nR,) for v, f in zip(values, fills)] == [True, True]
        idx, matched, values = e.lookup_columns(tR[:0].contiguous(), tS, tv, fills)
        assert matched == 0 and idx.shape == (0,) and [v.shape for v in values] == [(0,), (0,)]
    finally:
        e.close()


def test_lookup_columns_on_two_key_columns():
    rng = np.random.default_rng(11)
    nR, nS = 20_000, 30_000
    a, b = rng.integers(-50, 50, nS, dtype=np.int64), rng.integers(0, 400, nS, dtype=np.int64)
    pick = rng.integers(0, nS, nR)
    ra, rb = a[pick].copy(), b[pick].copy()
    rb[::4] += 1_000                                                        # a quarter of R's rows: no such tuple in S
    val = rng.integers(-(1 << 63), (1 << 63) - 1, nS, dtype=np.int64)
    first, last = {}, {}
    for j, t in enumerate(zip(a.tolist(), b.tolist())):
        first.setdefault(t, j)
        last[t] = j
    e = Engine(0)
    try:
        dev = [torch.from_numpy(x).cuda() for x in (ra, rb, a, b, val)]
        for name, table in (("first", first), ("last", last)):
            exp = np.array([table.get(t, -1) for t in zip(ra.tolist(), rb.tolist())], dtype=np.int64)
            idx, matched, values = e.lookup_columns([dev[0], dev[1]], [dev[2], dev[3]], [dev[4]], -1, name)
            assert matched == int((exp >= 0).sum()) and np.array_equal(idx.cpu().numpy(), exp)
            assert np.array_equal(values[0].cpu().numpy(), np.where(exp < 0, np.int64(-1), val[np.maximum(exp, 0)]))
    finally:
        e.close()


def test_lookup_columns_refuses_what_it_cannot_read():
    e = Engine(0)
    try:
        good = torch.arange(100, device="cuda", dtype=torch.int64)
        for bad in (good.to(torch.int32), good.to(torch.float64), torch.arange(200, device="cuda")[::2], good.cpu(),
                    good.reshape(10, 10), list(range(5))):
            with pytest.raises(ValueError):
                e.lookup_columns(bad, good)
            with pytest.raises(ValueError):
                e.lookup_columns(good, bad)
            with pytest.raises(ValueError):
                e.lookup_columns(good, good, [bad])
            with pytest.raises(ValueError):
                e.lookup_columns(good, good, [good, bad], [0, 0])
        with pytest.raises(ValueError):
            e.lookup_columns(good[:50].contiguous(), good, [good[:50].contiguous()])   # values as long as R, not as S
        for kwargs in ({"which": "any"}, {"which": 1}, {"values_S": [good] * (LOOKUP_MAX_COLS + 1)}, {"values_S": [good], "fill": [1, 2]},
                       {"values_S": [good], "fill": 1.5}):
            with pytest.raises(ValueError):
                e.lookup_columns(good, good, **kwargs)
        idx, matched, values = e.lookup_columns(good, good, [good * 2])
        assert matched == 100 and torch.equal(idx, good) and torch.equal(values[0], good * 2)
    finally:
        e.close()


def test_lookup_columns_is_ordered_behind_queued_torch_work():
    """the keys and the values are the last products of a queue of torch kernels issued right before the call, on a stream of its own"""
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
            vS = filler[F - nS:].clone()
            idx, matched, values = e.lookup_columns(kR, kS, [vS], -5, "last")
        torch.cuda.synchronize()
        x = np.arange(F - nS, F, dtype=U64)
        with np.errstate(over="ignore"):
            for _ in range(rounds):
                x = x * U64(3) + U64(1)
        exp_idx = np.full(nR, -1, dtype=np.int64)
        exp_idx[nR // 2:] = np.arange(nR - nR // 2)                        # row nR/2 + i of R meets row i of S alone
        exp_val = np.full(nR, -5, dtype=np.int64)
        exp_val[nR // 2:] = x[: nR - nR // 2].view(np.int64)
        assert matched == nR - nR // 2 and np.array_equal(idx.cpu().numpy(), exp_idx)
        assert np.array_equal(values[0].cpu().numpy(), exp_val)
        assert e.bound_stream is None
    finally:
        e.close()
