"""GPU suite: the group of every row, rhj_group_agg_ids_cols_dev / rhj_group_agg_ids_dev (include/rhj.h) and
Engine.group_by_columns_with_inverse / factorize_columns: the group-by's outputs and, per tuple of R, the index of its group in them.

The oracle is numpy only (np.unique; group_agg_cases.side_oracle for the aggregates).  Ids are checked against the call's OWN outputs,
so nothing depends on the order of groups: groups == len(np.unique(v)); gid[rows] < groups; keys[gid[rows]] == v; the bincount of the
ids is the count column; keys, counts and aggregates sorted by key equal the oracle.  Every id array has guard words behind it and a
sentinel in every word, so "untouched" is asserted; every case runs twice and is checked twice.
  * paths by size: 3,000 rows unpartitioned, 70,000 one pass, 3,000,000 under Opts(2, 8, 8) narrow; all-distinct, n/4 distinct and
    Zipf values; NULL and permuted ids; no column (the id sweep follows emission) and [SUM, MIN_I64, MAX_U64, SUM] (it follows an op
    sweep); the AoS entry once per size;
  * the all-ones key and unmix64(all ones) among 5,000 others under three plans; one value 70,000 times;
  * the class walk (last.group_rounds >= 9): ids across classes with different bases, then one table again;
  * capacity: one slot too few (ids stay exact indices, the rows of the group that was not stored carry one value), ids only;
  * the count-free overflow repeated with exact cursors; the row guard at gid_rows and at 2^32, narrow and not; a NULL id array
    against the _agg_ entry; nR 0 and 1; sparse explicit ids;
  * the torch entries against torch.unique(return_inverse=True), negative keys, queued torch work on a side stream."""
import numpy as np
import pytest
import torch

from group_agg_cases import MASK64, full_range_cols, side_oracle
from group_ids_cases import SENTINEL, IdArray, check_ids, raw
from oracle.pyoracle import TUPLE
from radixhashjoin_amd import AGG_MAX_U64, AGG_MIN_I64, AGG_SUM, Engine, Opts, RhjError, unmix64
from radixhashjoin_amd.binding import RHJ_E_INVALID, RHJ_E_OVERFLOW, plan as resolve_plan
from test_gpu_group_agg import SIZE_IDS, SIZES, Uploaded, check_exact
from test_gpu_group_sum import Outputs, beyond_a_table, make_values

pytestmark = pytest.mark.gpu
PLAN = Opts(2, 8, 8)
JK_GROUP = 15
MIXED = [AGG_SUM, AGG_MIN_I64, AGG_MAX_U64, AGG_SUM]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def inputs():
    """(dist, n, permuted ids) -> (values, ids or None, rows, four full-range columns, {with columns: oracle}): built once, shared,
    never written"""
    cache = {}

    def get(dist, n, ids=False):
        if (dist, n, ids) not in cache:
            v = make_values(dist, n)
            rid = np.random.default_rng(n + 7).permutation(n).astype(np.uint64) if ids else None
            rows = rid.astype(np.int64) if ids else np.arange(n)
            cols = full_range_cols(n)
            cache[(dist, n, ids)] = (v, rid, rows, cols, {False: side_oracle(v, rows, [], []), True: side_oracle(v, rows, cols, MIXED)})
        return cache[(dist, n, ids)]
    return get


def run_ids(eng, values, ids, cols, ops, exp, opts=None, dev=None, id_rows=None, after_first=None):
    """the columnar entry with ids, capacity = the number of groups, twice; each time the sorted outputs against the oracle, the ids
    against the call's own outputs, and the sentinel in every word no tuple names.  after_first: called between the two runs.
    Returns the group count."""
    n = len(values)
    rows = ids.astype(np.int64) if ids is not None else np.arange(n)
    id_rows = n if id_rows is None else id_rows
    own = dev is None
    dev = Uploaded(eng, values, ids, cols) if own else dev
    unnamed = np.ones(id_rows, dtype=bool)
    unnamed[rows] = False
    try:
        for attempt in range(2):
            if attempt and after_first:
                after_first()
            out, gid = Outputs(eng, len(exp[0]), len(cols)), IdArray(eng, id_rows)
            try:
                groups = eng.group_agg_ids_cols_dev(dev.v, dev.i, n, dev.c[:len(cols)], ops if cols else None, len(cols[0]) if cols else 0,
                                                    out.keys, out.counts, out.sums, out.cap, gid.buf, gid.rows, opts=opts)
                print(f"n {n} ops {ops if cols else None} groups {groups} kernel {eng.info('last.join_kernel')} rounds "
                      f"{eng.info('last.group_rounds')} narrow {eng.info('last.narrow')} passes {eng.timings()['passes']}")
                assert groups == len(exp[0]) == len(np.unique(values))
                check_exact(out.read(groups), exp)
                g = gid.read()
                check_ids(g, rows, values, raw(out.keys, groups), raw(out.counts, groups), groups)
                assert (g[unnamed] == SENTINEL).all(), "a word no tuple names was written"
                assert eng.info("last.join_kernel") == JK_GROUP and eng.info("last.cols_S") == 0 and eng.info("last.semi_tables") == 0
            finally:
                out.free()
                gid.free()
    finally:
        if own:
            dev.free()
    return groups


# ---- paths by size -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_cols", [False, True], ids=["no-column", "mixed-ops"])
@pytest.mark.parametrize("ids", [False, True], ids=["null", "ids"])
@pytest.mark.parametrize("dist", ["distinct", "quarter", "zipf"])
@pytest.mark.parametrize("n,opts,narrow", SIZES, ids=SIZE_IDS)
def test_paths_by_size(eng, inputs, n, opts, narrow, dist, ids, with_cols):
    v, rid, rows, cols, exp = inputs(dist, n, ids)
    if opts is None:
        assert resolve_plan(n, n).passes == (0 if n == 3_000 else 1)
    eng.set_option("partition.narrow", narrow)
    if opts is not None:
        eng.set_option("partition.countfree", 0)
    try:
        run_ids(eng, v, rid, cols if with_cols else [], MIXED, exp[with_cols], opts=opts)
        assert eng.timings()["passes"] == (0 if n == 3_000 else 1 if opts is None else 2)
        assert eng.info("last.narrow") == max(narrow, 0) and eng.info("last.group_rounds") == 1
    finally:
        eng.set_option("partition.narrow", -1)
        eng.set_option("partition.countfree", -1)


@pytest.mark.parametrize("n,opts,narrow", SIZES, ids=SIZE_IDS)
def test_aos_entry(eng, inputs, n, opts, narrow):
    v, rid, rows, cols, exp = inputs("quarter", n, True)
    e = exp[True]
    R = np.empty(n, dtype=TUPLE)
    R["key"], R["payload"] = rid, v
    dR, dc, out, gid = eng.to_device(R), [eng.to_device(c) for c in cols], Outputs(eng, len(e[0]), 4), IdArray(eng, n)
    eng.set_option("partition.narrow", narrow)
    try:
        groups = eng.group_agg_ids_dev(dR, n, dc, MIXED, n, out.keys, out.counts, out.sums, out.cap, gid.buf, n, opts=opts)
        assert groups == len(e[0])
        check_exact(out.read(groups), e)
        check_ids(gid.read(), rows, v, raw(out.keys, groups), raw(out.counts, groups), groups)
        assert eng.info("last.join_kernel") == JK_GROUP and eng.info("last.cols_R") == 0 and eng.info("last.narrow") == max(narrow, 0)
        assert np.array_equal(dR.to_numpy(TUPLE, n), R)                     # the input stands as it was
    finally:
        eng.set_option("partition.narrow", -1)
        for b in [dR] + dc:
            b.free()
        out.free()
        gid.free()


# ---- heavy and special keys --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [None, Opts(1, 4, 0), Opts(0, 0, 0)], ids=["auto", "one-pass", "unpartitioned"])
def test_the_all_ones_key_among_five_thousand_others(eng, opts):
    """the id of the all-ones key waits in the word beside the table, as its count does"""
    n = 5_001
    rng = np.random.default_rng(5)
    v = rng.integers(1, 1 << 62, n, dtype=np.uint64)
    v[::9] = np.uint64(MASK64)
    v[4::9] = np.uint64(unmix64(MASK64))                                   # (a partition holds mix64(value): this one becomes all ones)
    rows, cols = np.arange(n), full_range_cols(n)
    run_ids(eng, v, None, [], MIXED, side_oracle(v, rows, [], []), opts=opts)
    run_ids(eng, v, None, cols, MIXED, side_oracle(v, rows, cols, MIXED), opts=opts)


def test_one_value_seventy_thousand_times(eng):
    n = 70_000
    v = np.full(n, 0x0FEDCBA987654321, dtype=np.uint64)
    assert run_ids(eng, v, None, [], MIXED, side_oracle(v, np.arange(n), [], [])) == 1
    gid = IdArray(eng, n)
    dv = eng.to_device(v)
    try:
        assert eng.group_agg_ids_cols_dev(dv, None, n, d_out_gid=gid.buf, gid_rows=n) == 1
        assert not gid.read().any()                                        # every id is equal: the one group is group 0
    finally:
        dv.free()
        gid.free()


# ---- more distinct keys than a table: the class walk -------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["unpartitioned", "two-bits", "one-partition-of-65536"])
def test_the_class_walk(eng, inputs, case):
    """every class that survives its build claims its own base: an id is base + rank of a class, never of the table alone"""
    v, opts = beyond_a_table(case)
    n = len(v)
    rows, cols = np.arange(n), full_range_cols(n)
    eng.set_option("partition.narrow", -1)
    run_ids(eng, v, None, [], MIXED, side_oracle(v, rows, [], []), opts=opts)
    assert eng.info("last.group_rounds") >= 9                              # 20,000 keys or more over tables of 4608: at least 5 leaves, 9 builds
    run_ids(eng, v, None, cols, MIXED, side_oracle(v, rows, cols, MIXED), opts=opts)
    assert eng.info("last.group_rounds") >= 9
    v, rid, rows, cols, exp = inputs("quarter", 3_000)                     # ... and one table again
    run_ids(eng, v, rid, cols, MIXED, exp[True])
    assert eng.info("last.group_rounds") == 1


# ---- capacity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,opts", [(3_000, None), (70_000, None), (80_000, Opts(0, 0, 0))], ids=["3000", "70000", "classes"])
def test_one_slot_too_few_and_ids_only(eng, inputs, n, opts):
    if opts is None:
        v, _, rows, cols, exp = inputs("quarter", n)
        e = exp[True]
    else:
        v = beyond_a_table("unpartitioned")[0]
        rows, cols = np.arange(n), full_range_cols(n)
        e = side_oracle(v, rows, cols, MIXED)
    G = len(e[0])
    eng.set_option("partition.narrow", -1)
    dev = Uploaded(eng, v, None, cols)
    try:
        for _ in range(2):
            out, gid = Outputs(eng, G - 1, 4), IdArray(eng, n)
            with pytest.raises(RhjError) as err:
                eng.group_agg_ids_cols_dev(dev.v, None, n, dev.c, MIXED, n, out.keys, out.counts, out.sums, out.cap, gid.buf, n, opts=opts)
            assert err.value.code == RHJ_E_OVERFLOW
            gid.free()
            gid = IdArray(eng, n)
            groups = eng.group_agg_ids_cols_dev(dev.v, None, n, dev.c, MIXED, n, out.keys, out.counts, out.sums, out.cap, gid.buf, n,
                                                opts=opts, allow_overflow=True)
            assert groups == G                                             # the exact count
            out.read(groups)                                               # (asserts the guard words behind every output array)
            keys, counts, g = raw(out.keys, G - 1), raw(out.counts, G - 1), gid.read()
            assert (g < np.uint64(G)).all()                                # exact group indices, never compared with the capacity
            stored = g < np.uint64(G - 1)
            assert np.array_equal(keys[g[stored].astype(np.int64)], v[stored])
            assert np.array_equal(np.bincount(g.astype(np.int64), minlength=G)[:G - 1].astype(np.uint64), counts)
            lost = v[~stored]                                              # the rows of the group that was not stored carry the one value
            assert len(lost) and (lost == lost[0]).all() and lost[0] not in keys and len(np.unique(keys)) == G - 1
            out.free()
            gid.free()
            gid = IdArray(eng, n)                                          # ids only: a dense labelling without the dictionary
            assert eng.group_agg_ids_cols_dev(dev.v, None, n, dev.c, MIXED, 0, d_out_gid=gid.buf, gid_rows=n, opts=opts) == G   # (col_rows 0: no column is read)
            g = gid.read()
            gid.free()
            assert len(np.unique(g)) == G and int(g.max()) == G - 1
            assert len(np.unique(np.stack([v, g], axis=1), axis=0)) == G   # the pairs (value, id) have exactly G distinct values
    finally:
        dev.free()


# ---- the repeats inside a call -----------------------------------------------------------------------------------------------
def test_count_free_overflow_repeats_with_exact_cursors():
    n = 3_000_000
    v = make_values("quarter", n, seed=3)
    v[np.random.default_rng(3).permutation(n)[: n // 4]] = v[0]            # one value on a quarter of the rows: no count-free region holds it
    cols = full_range_cols(n, 1)
    e = Engine(0)
    try:
        e.set_option("partition.narrow", 2)
        e.set_option("partition.countfree", 1)
        def repeated():                                                    # (the context counts the overflow: its next call starts with exact cursors)
            assert e.info("last.narrow") == 2 and e.info("last.countfree_R") == 2 and e.info("last.cols_R") == 1
        run_ids(e, v, None, cols, [AGG_MIN_I64], side_oracle(v, np.arange(n), cols, [AGG_MIN_I64]), opts=PLAN, after_first=repeated)
        assert e.info("last.narrow") == 2
    finally:
        e.close()


# ---- the row guard -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["at-gid-rows", "two-to-the-32"])
@pytest.mark.parametrize("n", [3_000, 70_000])
def test_a_row_beyond_the_id_array_is_refused_and_the_context_goes_on(eng, inputs, n, where):
    v, rid, rows, cols, exp = inputs("quarter", n, True)
    bad = rid.copy()
    bad[n // 2] = np.uint64(n if where == "at-gid-rows" else 1 << 32)
    eng.set_option("partition.narrow", -1)
    dev = Uploaded(eng, v, bad, [])
    try:
        for _ in range(2):
            gid, out = IdArray(eng, n), Outputs(eng, n, 0)
            with pytest.raises(RhjError) as err:
                eng.group_agg_ids_cols_dev(dev.v, dev.i, n, (), None, 0, out.keys, out.counts, (), out.cap, gid.buf, n)
            assert err.value.code == RHJ_E_INVALID and "d_out_gid" in str(err.value) and "gid_rows" in str(err.value)
            gid.read()                                                     # the guard words are intact
            gid.free()
            out.free()
            assert eng.group_agg_cols_dev(dev.v, dev.i, n) == len(exp[False][0])   # without an id array the same tuples are fine
    finally:
        dev.free()
    run_ids(eng, v, rid, cols, MIXED, exp[True])                           # a valid call on the same context is exact


def test_one_wide_id_repeats_at_sixteen_bytes_and_meets_the_guard_there(inputs):
    """narrow partitions cannot hold a rowID of 2^32: the call repeats at 16 bytes, where the guard sees the rowID and no address does"""
    n = 90_000
    v, _, rows, cols, exp = inputs("quarter", n)
    ids = np.arange(n, dtype=np.uint64)
    wide = ids.copy()
    wide[n // 3] = np.uint64(1 << 32)
    e = Engine(0)
    try:
        e.set_option("partition.narrow", 2)                                # set once, never re-armed below
        for rid, ok in ((ids, True), (wide, False), (ids, True)):
            dev, gid, out = Uploaded(e, v, rid, []), IdArray(e, n), Outputs(e, len(exp[False][0]), 0)
            try:
                if ok:
                    groups = e.group_agg_ids_cols_dev(dev.v, dev.i, n, (), None, 0, out.keys, out.counts, (), out.cap, gid.buf, n, opts=PLAN)
                    check_exact(out.read(groups), exp[False])
                    check_ids(gid.read(), rows, v, raw(out.keys, groups), raw(out.counts, groups), groups)
                    assert e.info("last.narrow") == 2
                else:
                    with pytest.raises(RhjError) as err:
                        e.group_agg_ids_cols_dev(dev.v, dev.i, n, (), None, 0, out.keys, out.counts, (), out.cap, gid.buf, n, opts=PLAN)
                    assert err.value.code == RHJ_E_INVALID and "d_out_gid" in str(err.value)
                    assert e.info("last.narrow") == 0                      # the attempt that answered ran at 16 bytes
                    gid.read()
            finally:
                dev.free()
                gid.free()
                out.free()
    finally:
        e.close()


# ---- a NULL id array, small and sparse inputs --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3_000, 70_000])
def test_a_null_id_array_is_the_agg_entry(eng, inputs, n):
    v, rid, rows, cols, exp = inputs("zipf", n, True)
    G = len(exp[True][0])
    dev, a, b = Uploaded(eng, v, rid, cols), Outputs(eng, G, 4), Outputs(eng, G, 4)
    try:
        assert eng.group_agg_cols_dev(dev.v, dev.i, n, dev.c, MIXED, n, a.keys, a.counts, a.sums, a.cap) == G
        assert eng.group_agg_ids_cols_dev(dev.v, dev.i, n, dev.c, MIXED, n, b.keys, b.counts, b.sums, b.cap, None, 12345) == G
        check_exact(b.read(G), a.read(G))
        check_exact(b.read(G), exp[True])
    finally:
        dev.free()
        a.free()
        b.free()


def test_empty_and_single_row(eng):
    gid, out = IdArray(eng, 4), Outputs(eng, 4, 0)
    try:
        assert eng.group_agg_ids_cols_dev(None, None, 0, (), None, 0, out.keys, out.counts, (), out.cap, gid.buf, 4) == 0
        assert eng.info("last.join_kernel") == -1 and eng.info("last.group_rounds") == 0 and eng.timings()["ntasks"] == 0
        assert eng.group_agg_ids_dev(None, 0, d_out_gid=gid.buf, gid_rows=4) == 0
        assert (gid.read() == SENTINEL).all() and len(out.read(0)[0]) == 0
    finally:
        gid.free()
        out.free()
    cols = full_range_cols(1, 2)
    for value in (0, 7, MASK64):
        v = np.array([value], dtype=np.uint64)
        assert run_ids(eng, v, None, cols, [AGG_MIN_I64, AGG_MAX_U64], side_oracle(v, np.arange(1), cols, [AGG_MIN_I64, AGG_MAX_U64])) == 1


def test_sparse_explicit_ids(eng):
    """3,000 tuples that name every third word of a 9,000-word array: the other words keep what they held"""
    n = 3_000
    v = make_values("quarter", n)
    rid = (np.random.default_rng(11).permutation(n) * 3).astype(np.uint64)
    cols = full_range_cols(3 * n)
    exp = side_oracle(v, rid.astype(np.int64), cols, MIXED)
    run_ids(eng, v, rid, cols, MIXED, exp, id_rows=3 * n)                   # (run_ids asserts the sentinel in the 6,000 unnamed words)
    run_ids(eng, v, rid, [], MIXED, side_oracle(v, rid.astype(np.int64), [], []), id_rows=3 * n)


# ---- the torch entries -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1_000, 300_000])
def test_with_inverse_and_factorize_against_torch(n):
    rng = np.random.default_rng(n)
    k = rng.integers(-(1 << 62), 1 << 62, max(n // 5, 1), dtype=np.int64)[rng.integers(0, max(n // 5, 1), n)]
    k[0], k[1], k[2] = -1, np.iinfo(np.int64).min, 0                       # negative keys; -1 is the all-ones word
    w = [rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64) for _ in range(2)]
    e = Engine(0)
    try:
        tk, tw = torch.from_numpy(k).cuda(), [torch.from_numpy(x).cuda() for x in w]
        uk, inv, cnt = torch.unique(tk, return_inverse=True, return_counts=True)
        for _ in range(2):
            keys, counts, aggs, inverse = e.group_by_columns_with_inverse(tk, tw, ops=["min", "sum"])
            assert inverse.dtype == torch.int64 and inverse.shape == tk.shape and inverse.device == tk.device
            assert torch.equal(keys[inverse], tk)                          # unique[inverse] == keys
            assert torch.equal(torch.bincount(inverse, minlength=len(keys)), counts)
            order = torch.argsort(keys)
            assert torch.equal(keys[order], uk) and torch.equal(counts[order], cnt)
            assert torch.equal(order[inv], inverse)                        # torch's inverse, renamed to this call's order of groups
            assert torch.equal(aggs[0][order], torch.zeros_like(uk).scatter_reduce_(0, inv, tw[0], "amin", include_self=False))
            assert torch.equal(aggs[1][order], torch.zeros_like(uk).index_add_(0, inv, tw[1]))
            # what the inverse is for: an aggregate no op covers, as a direct-indexed torch op
            mag = tw[1].double().abs()                                     # (one sign: no cancellation, so the order of the addends costs
            mean = torch.zeros(len(keys), dtype=torch.float64, device="cuda").index_add_(0, inverse, mag) / counts   # a few ulps at most)
            want = torch.zeros(len(uk), dtype=torch.float64, device="cuda").index_add_(0, inv, mag) / cnt
            assert torch.allclose(mean[order], want, rtol=1e-12, atol=0)
            codes, uniques = e.factorize_columns(tk)
            assert codes.dtype == torch.int64 and torch.equal(uniques[codes], tk) and torch.equal(torch.sort(uniques).values, uk)
            assert torch.equal(torch.bincount(codes, minlength=len(uniques))[torch.argsort(uniques)], cnt)
        keys, counts, sums = e.group_by_columns(tk, tw)                     # the entry without the inverse returns what it returned
        assert torch.equal(torch.sort(keys).values, uk) and len(sums) == 2
        keys, counts, aggs, inverse = e.group_by_columns_with_inverse(tk[:0].contiguous())
        assert keys.shape == counts.shape == inverse.shape == (0,) and aggs == []
        codes, uniques = e.factorize_columns(tk[:0].contiguous())
        assert codes.shape == uniques.shape == (0,)
    finally:
        e.close()


def test_with_inverse_is_ordered_behind_queued_torch_work():
    """the keys are the last product of a queue of torch kernels issued right before the call, on a stream of its own"""
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
            keys, counts, _, inverse = e.group_by_columns_with_inverse(k)
        torch.cuda.synchronize()
        x = np.arange(n, dtype=np.uint64)
        with np.errstate(over="ignore"):
            for _ in range(rounds):
                x = x * np.uint64(3) + np.uint64(1)
        want = (x.view(np.int64) >> 3).view(np.uint64)
        ek, ec = np.unique(want, return_counts=True)
        gk, gi = keys.cpu().numpy().view(np.uint64), inverse.cpu().numpy()
        assert np.array_equal(np.sort(gk), ek) and np.array_equal(gk[gi], want)
        assert np.array_equal(np.bincount(gi, minlength=len(gk)), counts.cpu().numpy())
        assert e.bound_stream is None
    finally:
        e.close()
