"""GPU suite: the semi-join / anti-join entries rhj_semi_join_cols_dev / rhj_semi_join_dev (include/rhj.h) and
Engine.semi_join_columns.

The oracle is numpy: np.isin(valR, valS) selects the rowIDs a semi join reports, its complement those of an anti join; the sorted
ids must be equal, every case runs both kinds, and the two counts sum to nR.
  * paths by size: 3,000 rows per side (unpartitioned), 70,000 (one-pass automatic plan), 3,000,000 under Opts(2, 8, 8) in the
    narrow format (columns read directly); uniform, duplicate-heavy and Zipf 0.9 inputs; NULL and explicit ids;
  * one value on 1,000 rows of R and 10^6 rows of S: 10^9 pairs for the inner join, 1,000 ids here;
  * partitions of S far beyond one LDS table, R cut into several tasks: "last.semi_tables" >= 2, then 1, then 0 after an inner join;
  * the all-ones join value and unmix64 of it (the empty marker of the tables under a partitioned plan) on S only, R only, both;
  * partitions without a tuple of S under an anti join; a disjoint S; n = 0 and n = 1; invalid arguments;
  * the repeats inside a call: a count-free region that overflows, one rowID of 2^32 in a narrow format;
  * count-only mode, an undersized buffer; the AoS entry; the inner join's distinct idx_R;
  * semi_join_columns on int64 tensors: negative keys, an empty keys_S, refused tensors, queued torch work, a bound stream."""
import numpy as np
import pytest
import torch

import cf_cases
from oracle.pyoracle import TUPLE
from radixhashjoin_amd import ANTI, SEMI, Engine, Opts, RhjError
from radixhashjoin_amd.binding import RHJ_E_INVALID, RHJ_E_OVERFLOW, mix64, plan as resolve_plan, unmix64

pytestmark = pytest.mark.gpu
PLAN = Opts(2, 8, 8)
SENTINEL = np.uint64(0xFFFFFFFFFFFFFFFF)
JK_SEMI = 12


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


# ---- input builders (those of test_gpu_cols_join.py) -------------------------------------------------------------------------
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


@pytest.fixture(scope="module")
def inputs():
    """(dist, n) -> (R, S, isin mask): built once, shared, never written"""
    cache = {}

    def get(dist, n, nS=None, seed=0):
        key = (dist, n, nS, seed)
        if key not in cache:
            R, S = make(dist, n, nS or n, seed)
            cache[key] = (R, S, np.isin(R["payload"], S["payload"]))
        return cache[key]
    return get


def expected(R, mask, kind):
    return np.sort(R["key"][mask if kind == SEMI else ~mask])


def run_cols(eng, R, S, mask, ids=True, opts=None, after=None):
    """both kinds through the columnar entry against the mask; after(kind): further assertions on the engine's state"""
    R = with_ids(R, ids)
    dv, di = eng.to_device(np.ascontiguousarray(R["payload"])), eng.to_device(np.ascontiguousarray(R["key"])) if ids else None
    ds, out = eng.to_device(np.ascontiguousarray(S["payload"])), eng.alloc(8 * max(len(R), 1))
    counts = {}
    try:
        for kind in (SEMI, ANTI):
            n = eng.semi_join_cols_dev(dv, di, len(R), ds, len(S), kind, out, len(R), opts=opts)
            got = out.to_numpy(np.uint64, n)
            exp = expected(R, mask, kind)
            print(f"kind {kind}: count {n} expected {len(exp)} kernel {eng.info('last.join_kernel')} tables {eng.info('last.semi_tables')} "
                  f"narrow {eng.info('last.narrow')}")
            assert n == len(got) == len(exp)
            assert np.array_equal(np.sort(got), exp)
            if after is not None:
                after(kind)
            counts[kind] = n
        assert counts[SEMI] + counts[ANTI] == len(R)
    finally:
        for b in (dv, di, ds, out):
            if b is not None:
                b.free()
    return counts


# ---- paths by size -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", [False, True], ids=["null", "ids"])
@pytest.mark.parametrize("dist", ["uniform", "dups", "zipf"])
@pytest.mark.parametrize("n,passes", [(3_000, 0), (70_000, 1)])
def test_small_sizes_automatic_plan(eng, inputs, n, passes, dist, ids):
    assert resolve_plan(n, n).passes == passes
    R, S, mask = inputs(dist, n)
    eng.set_option("partition.narrow", -1)

    def after(kind):
        assert eng.info("last.join_kernel") == JK_SEMI and eng.info("last.semi_tables") == 1 and eng.info("last.narrow") == 0
        assert eng.timings()["passes"] == passes
    run_cols(eng, R, S, mask, ids, after=after)


@pytest.mark.parametrize("dist", ["uniform", "zipf"])
def test_three_million_narrow_two_pass(eng, inputs, dist):
    R, S, mask = inputs(dist, 3_000_000)
    eng.set_option("partition.narrow", 2)
    eng.set_option("partition.countfree", 0)

    def after(kind):
        assert eng.info("last.narrow") == 2 and eng.info("last.cols_R") == 1 and eng.info("last.cols_S") == 1
        assert eng.info("last.join_kernel") == JK_SEMI and eng.info("last.semi_tables") == 1
    try:
        run_cols(eng, R, S, mask, ids=False, opts=PLAN, after=after)
    finally:
        eng.set_option("partition.narrow", -1)
        eng.set_option("partition.countfree", -1)


# ---- duplicates do not multiply ----------------------------------------------------------------------------------------------
def test_a_value_repeated_a_million_times_in_S(eng, inputs):
    R0, S0, _ = inputs("uniform", 70_000)
    rng = np.random.default_rng(5)
    heavy = np.uint64(0x123456789ABCDEF)
    rv = np.concatenate([R0["payload"], np.full(1_000, heavy, dtype=np.uint64)])
    sv = np.concatenate([S0["payload"], np.full(1_000_000, heavy, dtype=np.uint64)])
    R, S = rel(rng, len(rv), rv[rng.permutation(len(rv))]), rel(rng, len(sv), sv[rng.permutation(len(sv))])
    mask = np.isin(R["payload"], S["payload"])
    assert int((R["payload"] == heavy).sum()) == 1_000 and mask[R["payload"] == heavy].all()
    eng.set_option("partition.narrow", -1)
    run_cols(eng, R, S, mask, ids=True)


# ---- several tables per task, several tasks per partition --------------------------------------------------------------------
@pytest.mark.parametrize("opts,nS", [(Opts(1, 1, 0), 200_000), (Opts(0, 0, 0), 100_000)], ids=["one-bit", "unpartitioned"])
def test_partitions_beyond_one_table(eng, opts, nS):
    rng = np.random.default_rng(nS)
    nR = 300_000
    sv = rng.permutation(np.arange(1, 4 * nS, 4, dtype=np.uint64))           # distinct
    rv = np.concatenate([sv[rng.integers(0, nS, nR // 2)], rng.integers(0, nS, nR - nR // 2).astype(np.uint64) * np.uint64(4) + np.uint64(2)])
    R, S = rel(rng, nR, rv[rng.permutation(nR)]), rel(rng, nS, sv)
    mask = np.isin(R["payload"], S["payload"])
    assert int(mask.sum()) == nR // 2
    eng.set_option("partition.narrow", -1)

    def after(kind):
        assert eng.info("last.semi_tables") >= 2
        assert eng.timings()["ntasks"] >= 2 * (1 << opts.bits1)              # several tasks per partition
    run_cols(eng, R, S, mask, ids=True, opts=opts, after=after)
    small = make("uniform", 3_000, 3_000)

    def one_table(kind):
        assert eng.info("last.semi_tables") == 1
    run_cols(eng, *small, np.isin(small[0]["payload"], small[1]["payload"]), ids=False, after=one_table)
    dv, ds = eng.to_device(np.ascontiguousarray(small[0]["payload"])), eng.to_device(np.ascontiguousarray(small[1]["payload"]))
    assert eng.join_cols_dev(dv, None, 3_000, ds, None, 3_000) > 0
    assert eng.info("last.semi_tables") == 0 and eng.info("last.join_kernel") != JK_SEMI
    dv.free()
    ds.free()


# ---- the tables' empty marker as a join value ----------------------------------------------------------------------------------
@pytest.mark.parametrize("value", ["raw", "unmixed"])
@pytest.mark.parametrize("ones_on", ["both", "R", "S"])
def test_all_ones_value(eng, inputs, ones_on, value):
    """70,000 rows, a one-pass plan: the kernel sees rhj_mix64(payload), so unmix64(all ones) is the key it keeps beside the table
    (and the raw all-ones payload an ordinary key); on S only, on R only and on both"""
    n = 70_000
    assert resolve_plan(n, n).passes == 1
    R0, S0, _ = inputs("uniform", n)
    R, S = R0.copy(), S0.copy()
    ones = np.uint64(0xFFFFFFFFFFFFFFFF)
    if value == "unmixed":
        ones = unmix64(ones)
        assert int(mix64(ones)) == 0xFFFFFFFFFFFFFFFF
    if ones_on in ("both", "R"):
        R["payload"][[3, 1_500]] = ones
    if ones_on in ("both", "S"):
        S["payload"][[7, 8, 2_000]] = ones
    mask = np.isin(R["payload"], S["payload"])
    is_ones = R["payload"] == ones
    assert int(is_ones.sum()) == (0 if ones_on == "S" else 2) and mask[is_ones].all() == (ones_on == "both" or ones_on == "S")
    eng.set_option("partition.narrow", -1)

    def after(kind):
        assert eng.info("last.join_kernel") == JK_SEMI and eng.info("last.semi_tables") == 1 and eng.timings()["passes"] == 1
    for ids in (True, False):
        run_cols(eng, R, S, mask, ids, after=after)


# ---- partitions without S, a disjoint S, degenerate sizes, invalid arguments -------------------------------------------------
def test_empty_partitions_of_S_under_anti(eng, inputs):
    R, _, _ = inputs("uniform", 3_000_000)
    rng = np.random.default_rng(11)
    sv = R["payload"][rng.integers(0, len(R), 70_000)]
    sv[::97] ^= np.uint64(1 << 62)
    S = rel(rng, len(sv), sv)
    mask = np.isin(R["payload"], sv)
    eng.set_option("partition.narrow", -1)
    counts = run_cols(eng, R, S, mask, ids=False, opts=PLAN)
    assert counts[ANTI] > 2_900_000 and 0 < eng.info("last.max_part_S") < 20     # ~1.07 tuples of S per partition: a third have none


def test_disjoint_S(eng, inputs):
    R, S0, _ = inputs("uniform", 70_000)
    S = S0.copy()
    S["payload"] |= np.uint64(1 << 63)
    counts = run_cols(eng, R, S, np.zeros(len(R), dtype=bool), ids=True)
    assert counts == {SEMI: 0, ANTI: len(R)}


def test_degenerate_sizes(eng, inputs):
    R, S, mask = inputs("uniform", 3_000)
    none = np.zeros(len(R), dtype=bool)
    assert run_cols(eng, R, S[:0], none, ids=True) == {SEMI: 0, ANTI: len(R)}          # nS == 0
    assert eng.info("last.join_kernel") == JK_SEMI                                      # (the anti call ran the kernel over empty tables)
    assert run_cols(eng, R, S[:0], none, ids=False) == {SEMI: 0, ANTI: len(R)}
    assert run_cols(eng, R[:0], S, none[:0]) == {SEMI: 0, ANTI: 0}                      # nR == 0
    assert eng.info("last.join_kernel") == -1 and eng.info("last.semi_tables") == 0
    assert run_cols(eng, R[:0], S[:0], none[:0]) == {SEMI: 0, ANTI: 0}
    hit = int(np.flatnonzero(mask)[0])
    one_s = S[S["payload"] == R["payload"][hit]][:1]
    assert run_cols(eng, R, one_s, R["payload"] == one_s["payload"][0], ids=True)[SEMI] >= 1      # n = 1 on either side
    assert run_cols(eng, R[hit: hit + 1], S, mask[hit: hit + 1], ids=True) == {SEMI: 1, ANTI: 0}
    miss = int(np.flatnonzero(~mask)[0]) if (~mask).any() else None
    if miss is not None:
        assert run_cols(eng, R[miss: miss + 1], S, mask[miss: miss + 1], ids=False) == {SEMI: 0, ANTI: 1}
    assert run_cols(eng, R[hit: hit + 1], one_s, np.ones(1, dtype=bool)) == {SEMI: 1, ANTI: 0}
    # a large R against an empty S: every id, through several tasks
    big, _, _ = inputs("uniform", 70_000)
    assert run_cols(eng, big, S[:0], np.zeros(len(big), dtype=bool), ids=True) == {SEMI: 0, ANTI: len(big)}


def test_invalid_arguments(eng, inputs):
    R, S, _ = inputs("uniform", 3_000)
    dv, ds, out = eng.to_device(np.ascontiguousarray(R["payload"])), eng.to_device(np.ascontiguousarray(S["payload"])), eng.alloc(8 * 3_000)
    dR, dS = eng.to_device(R), eng.to_device(S)
    for kind in (SEMI, ANTI):
        for args in ((None, None, 3_000, ds, 3_000), (dv, None, 3_000, None, 3_000), (None, dv, 3_000, ds, 3_000), (None, None, 5, None, 0)):
            with pytest.raises(RhjError) as err:
                eng.semi_join_cols_dev(*args, kind, out, 3_000)
            assert err.value.code == RHJ_E_INVALID
        for args in ((None, 3_000, dS, 3_000), (dR, 3_000, None, 3_000)):
            with pytest.raises(RhjError) as err:
                eng.semi_join_dev(*args, kind, out, 3_000)
            assert err.value.code == RHJ_E_INVALID
    for kind in (2, -1):
        with pytest.raises(RhjError) as err:
            eng.semi_join_cols_dev(dv, None, 3_000, ds, 3_000, kind, out, 3_000)
        assert err.value.code == RHJ_E_INVALID
        with pytest.raises(RhjError) as err:
            eng.semi_join_dev(dR, 3_000, dS, 3_000, kind, out, 3_000)
        assert err.value.code == RHJ_E_INVALID
    for b in (dv, ds, out, dR, dS):
        b.free()


# ---- the repeats inside a call -----------------------------------------------------------------------------------------------
def test_count_free_overflow_repeats_S(inputs):
    R, S, mask = inputs("quarter", 3_000_000)
    # R fits its count-free regions (its largest pass-1 piece is 36 or 37 of 64 slots), S does not: R stands, "last.countfree_R" is 1
    assert int(cf_cases.piece_lengths(R).max()) <= cf_cases.cap(cf_cases.unit_len(len(R)), 8) < int(cf_cases.piece_lengths(S).max())
    e = Engine(0)
    try:
        e.set_option("partition.narrow", 2)

        def after(kind):
            assert e.info("last.narrow") == 2 and e.info("last.countfree_S") == 2 and e.info("last.countfree_R") == 1
            e.set_option("partition.countfree", 1)                         # re-arm the back-off for the next kind
        e.set_option("partition.countfree", 1)
        run_cols(e, R, S, mask, ids=False, opts=PLAN, after=after)
    finally:
        e.close()


def test_one_wide_id_of_R_falls_back_for_that_call_only(inputs):
    R0, S, mask = inputs("uniform", 90_000, 120_000, seed=2)
    e = Engine(0)
    try:
        e.set_option("partition.narrow", 2)                                # set once, never re-armed below
        for wide, row in ((False, None), (True, int(np.flatnonzero(mask)[7])), (True, int(np.flatnonzero(~mask)[7])), (False, None)):
            R = R0.copy()
            if wide:
                R["key"][row] = np.uint64(1 << 32)                         # reported by the semi join (first row) / the anti join (second)

            def after(kind):
                assert e.info("last.narrow") == (0 if wide else 2)
                assert e.info("last.cols_R") == (2 if wide else 1)
            run_cols(e, R, S, mask, ids=True, opts=PLAN, after=after)
    finally:
        e.close()


# ---- count-only and overflow -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [SEMI, ANTI])
def test_count_only_and_small_buffer(eng, inputs, kind):
    R, S, mask = inputs("dups", 70_000)
    exp = expected(R, mask, kind)
    count, pad = len(exp), 64
    assert count > 100
    dv, di, ds = (eng.to_device(np.ascontiguousarray(a)) for a in (R["payload"], R["key"], S["payload"]))
    assert eng.semi_join_cols_dev(dv, di, len(R), ds, len(S), kind) == count            # d_out NULL, capacity 0
    cap = count - 5
    out = eng.to_device(np.full(cap + pad, SENTINEL, dtype=np.uint64))
    with pytest.raises(RhjError) as err:
        eng.semi_join_cols_dev(dv, di, len(R), ds, len(S), kind, out, cap)
    assert err.value.code == RHJ_E_OVERFLOW
    assert eng.semi_join_cols_dev(dv, di, len(R), ds, len(S), kind, out, cap, allow_overflow=True) == count
    back = out.to_numpy(np.uint64, cap + pad)
    assert (back[cap:] == SENTINEL).all(), "an id was written at or past capacity"
    assert len(np.unique(back[:cap])) == cap and np.isin(back[:cap], exp).all()
    for b in (dv, di, ds, out):
        b.free()


# ---- the AoS entry, and the inner join -----------------------------------------------------------------------------------------
def test_aos_entry_agrees(eng, inputs):
    R, S, mask = inputs("dups", 70_000)
    dR, dS, out = eng.to_device(R), eng.to_device(S), eng.alloc(8 * len(R))
    counts = {}
    for kind in (SEMI, ANTI):
        counts[kind] = eng.semi_join_dev(dR, len(R), dS, len(S), kind, out, len(R))
        assert np.array_equal(np.sort(out.to_numpy(np.uint64, counts[kind])), expected(R, mask, kind))
        assert eng.info("last.cols_R") == 0 and eng.info("last.join_kernel") == JK_SEMI
        assert eng.semi_join_dev(dR, len(R), dS, len(S), kind) == counts[kind]
    assert counts == run_cols(eng, R, S, mask, ids=True)
    for b in (dR, dS, out):
        b.free()


def test_inner_join_distinct_idx_R_is_the_semi_join(inputs):
    R, S, mask = inputs("dups", 70_000)
    e = Engine(0)
    try:
        kR, kS = (torch.from_numpy(np.ascontiguousarray(T["payload"]).view(np.int64)).cuda() for T in (R, S))
        iR, _ = e.join_columns(kR, kS)
        semi = e.semi_join_columns(kR, kS)
        assert np.array_equal(np.unique(iR.cpu().numpy()), np.sort(semi.cpu().numpy()))
        assert np.array_equal(np.sort(semi.cpu().numpy()), np.flatnonzero(mask))
    finally:
        e.close()


# ---- Engine.semi_join_columns ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nR,nS", [(1_000, 3_000), (200_000, 300_000)])
def test_semi_join_columns_against_numpy(nR, nS):
    rng = np.random.default_rng(nR)
    kR = rng.integers(-(1 << 62), 1 << 62, nR, dtype=np.int64)
    kR[: nR // 10] = kR[nR // 2: nR // 2 + nR // 10]
    kR[0], kR[1] = -1, np.iinfo(np.int64).min                              # (-1: the all-ones word)
    kS = kR[rng.integers(0, nR, nS)]
    kS[::13] = rng.integers(-(1 << 62), 1 << 62, len(kS[::13]), dtype=np.int64)
    kS[5], kS[6] = -1, np.iinfo(np.int64).min
    mask = np.isin(kR, kS)
    e = Engine(0)
    try:
        tR, tS = torch.from_numpy(kR).cuda(), torch.from_numpy(kS).cuda()
        semi, anti = e.semi_join_columns(tR, tS), e.semi_join_columns(tR, tS, anti=True)
        assert semi.dtype == torch.int64 and anti.dtype == torch.int64 and semi.is_cuda and semi.dim() == 1
        assert np.array_equal(np.sort(semi.cpu().numpy()), np.flatnonzero(mask))
        assert np.array_equal(np.sort(anti.cpu().numpy()), np.flatnonzero(~mask))
        assert semi.numel() + anti.numel() == nR and mask[0] and mask[1]
        # an empty keys_S, an empty keys_R
        assert e.semi_join_columns(tR, tS[:0].contiguous()).numel() == 0
        everything = e.semi_join_columns(tR, tS[:0].contiguous(), anti=True)
        assert torch.equal(everything.sort().values, torch.arange(nR, device="cuda"))
        for anti_flag in (False, True):
            got = e.semi_join_columns(tR[:0].contiguous(), tS, anti=anti_flag)
            assert got.numel() == 0 and got.dtype == torch.int64
    finally:
        e.close()


def test_semi_join_columns_refuses_what_it_cannot_read():
    e = Engine(0)
    try:
        good = torch.arange(100, device="cuda", dtype=torch.int64)
        for bad in (good.to(torch.int32), good.to(torch.float64), torch.arange(200, device="cuda")[::2], good.cpu(),
                    good.reshape(10, 10), list(range(5))):
            for anti in (False, True):
                with pytest.raises(ValueError):
                    e.semi_join_columns(bad, good, anti=anti)
                with pytest.raises(ValueError):
                    e.semi_join_columns(good, bad, anti=anti)
        assert torch.equal(e.semi_join_columns(good, good).sort().values, good)
        assert e.semi_join_columns(good, good, anti=True).numel() == 0
    finally:
        e.close()


def test_semi_join_columns_is_ordered_behind_queued_torch_work():
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
            semi = e.semi_join_columns(kR, kS)
            anti = e.semi_join_columns(kR, kS, anti=True)
        torch.cuda.synchronize()
        assert torch.equal(semi.sort().values, torch.arange(nR // 2, nR, device="cuda"))
        assert torch.equal(anti.sort().values, torch.arange(0, nR // 2, device="cuda"))
        x = np.arange(nR, dtype=np.uint64)
        with np.errstate(over="ignore"):
            for _ in range(rounds):
                x = x * np.uint64(3) + np.uint64(1)
        assert np.array_equal(kR.cpu().numpy().view(np.uint64), x)
        assert e.bound_stream is None
    finally:
        e.close()


def test_semi_join_columns_keeps_the_callers_stream_binding():
    e = Engine(0)
    try:
        mine, other = torch.cuda.Stream(), torch.cuda.Stream()
        e.set_stream(mine.cuda_stream)
        keys = torch.arange(5_000, device="cuda", dtype=torch.int64)
        torch.cuda.synchronize()
        assert e.semi_join_columns(keys, keys).numel() == 5_000 and e.bound_stream == mine.cuda_stream
        with torch.cuda.stream(other):
            assert e.semi_join_columns(keys, keys[:100].contiguous(), anti=True).numel() == 4_900
        assert e.bound_stream == mine.cuda_stream
        with torch.cuda.stream(mine):
            a = e.semi_join_columns(keys, keys)
        assert torch.equal(a.sort().values, keys) and e.bound_stream == mine.cuda_stream
        e.set_stream(None)
        assert e.bound_stream is None
    finally:
        e.close()
