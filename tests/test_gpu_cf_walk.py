"""GPU suite: the two count-free partition passes on inputs whose piece lengths and partition sizes are SET (tests/cf_cases.py), with
the one-writer pass 2 (k_scatter_wcn_cf2, dev_scatter_wcn with CF == 3) forced at sizes far below its automatic 2^28.

Every join here runs with "partition.narrow" 2, "partition.countfree" 1 and "partition.countfree2" 1 and asserts "last.narrow" == 2
and all four state words against cf_cases.predict, which computes them from the data and the device's compute-unit count: no case can
pass by having taken the exact path unnoticed.
  * set_lengths: every unit carries pieces of 0, 1, 31, 32, 33, 63, 64 (and 65, 95, 96 with two-tile units); a bucket whose first
    five pieces are empty, one whose last five are, one that is empty except for a full region in every 7th unit, one whose prefix
    puts a piece boundary on slot 1024 and on slot 4096; in every bucket of at least cap2 + 254 tuples one final partition at exactly
    cap2 and one empty.  Sizes
    from 4 units (two wholly empty buckets) over 257 units (a bucket is a tile or two) to 4.5 M x 5 M rows (two-tile units, cap 96,
    buckets of five tiles: cursors carried across tiles, the carry-line flush, the walk across prefetch calls and the clamped
    reload of the last tile) and 4,194,299 rows = 1024 units, where every entry of the kernel's prefix table is a piece and the last
    piece's walk ends on the sentinel behind the table.
  * all_full: every live region of both passes filled to the last slot, three quarters of the buckets empty; one tuple too many in
    pass 2 (the workgroup gives up on its fourth tile: nothing of the three stored tiles may show) and in pass 1; the back-off.
  * the plan matrix: seven plans other than 8+8, regions of one 32-slot line and of a few hundred slots.
  * the columnar entry.
Checked: pairs against the CPU oracle; rhj_debug_read_partitions -- boundaries and every partition's sorted {h, rowID} -- against the
run with the option(s) at 0, and against the input's own {mix64(payload), rowID}."""
import ctypes as C

import numpy as np
import pytest
import torch

import cf_cases as CF
from oracle.pyoracle import PAIR, sorted_pairs
from radixhashjoin_amd import Engine, Opts, mix64

pytestmark = pytest.mark.gpu
PLAN88 = Opts(2, 8, 8)


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def eng(cus):
    e = Engine(0)
    fn = e.lib.rhj_debug_read_partitions
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    yield e
    e.close()


@pytest.fixture(scope="module")
def full(oracle):
    """all_full() and its pairs, shared and left unchanged"""
    R, S, _ = CF.all_full()
    return R, S, sorted_pairs(oracle.join(R, S))


def force(eng, cf=1, cf2=1):
    """the options of every join here (setting them also re-arms the per-side back-off of both passes)"""
    eng.set_option("partition.narrow", 2)
    eng.set_option("partition.countfree", cf)
    eng.set_option("partition.countfree2", cf2)


def states(eng):
    """((pass 1, pass 2) of R, (pass 1, pass 2) of S) of the last join"""
    return ((eng.info("last.countfree_R"), eng.info("last.countfree2_R")), (eng.info("last.countfree_S"), eng.info("last.countfree2_S")))


def read_partitions(eng, side, n, nparts):
    """-> ({h} and {rowID} of side `side` in partition order, sorted by rowID inside every partition (rowIDs are distinct here, so that
    IS the sorted {h, rowID}), the nparts + 1 boundaries)"""
    pay, rid, bounds = np.empty(n, np.uint64), np.empty(n, np.uint32), np.full(nparts + 2, 0xABCD, np.uint64)
    rc = eng.lib.rhj_debug_read_partitions(eng.ctx, side, pay.ctypes.data, rid.ctypes.data, bounds.ctypes.data)
    assert rc == 0
    assert bounds[nparts + 1] == 0xABCD                        # the plan's 2^(b1 + b2) + 1 boundaries, not one more
    bounds = bounds[: nparts + 1].astype(np.int64)
    assert bounds[0] == 0 and bounds[-1] == n and (np.diff(bounds) >= 0).all()
    part = np.repeat(np.arange(nparts, dtype=np.uint64), np.diff(bounds))
    order = np.argsort(part << np.uint64(32) | rid.astype(np.uint64))
    return pay[order], rid[order], bounds


def same_partitions(seen0, seen1, X, plan):
    """both runs left the same boundaries and the same sorted {h, rowID} in every partition, every tuple lies in the partition its
    digits name, and together they are the input's own {mix64(payload), rowID}: nothing lost, doubled, stale or altered"""
    (p0, r0, b0), (p1, r1, b1) = seen0, seen1
    n, (k1, k2) = len(X), CF.bits_of(plan)
    assert np.array_equal(b0, b1)
    assert np.array_equal(p0, p1) and np.array_equal(r0, r1)
    part = np.repeat(np.arange(len(b1) - 1, dtype=np.uint64), np.diff(b1))
    d1, d2 = p1 & np.uint64((1 << k1) - 1), (p1 >> np.uint64(k1)) & np.uint64((1 << k2) - 1)
    assert np.array_equal(d1 << np.uint64(k2) | d2, part)
    assert np.array_equal(np.bincount(r1.astype(np.int64), minlength=n), np.ones(n, dtype=np.int64))          # rowIDs: a permutation of 0 .. n - 1
    mine, theirs = np.empty(n, np.uint64), np.empty(n, np.uint64)
    mine[r1] = p1
    theirs[X["key"].astype(np.int64)] = mix64(X["payload"])
    assert np.array_equal(mine, theirs)


def run(eng, A, B, plan, expect, exp_pairs=None, exp_cc=None, cf=1, cf2=1, rearm=True):
    """A x B under the options -> the partitions of both sides; pairs (sorted) or (count, checksum) against the oracle's, "last.narrow"
    and the four state words against `expect`"""
    if rearm:
        force(eng, cf, cf2)
    room = (len(exp_pairs) if exp_pairs is not None else exp_cc[0]) + 64
    dA, dB, out = eng.to_device(A), eng.to_device(B), eng.alloc(room * 16)
    try:
        cnt = eng.join_dev(dA, len(A), dB, len(B), out, room, opts=plan)
        st = (eng.info("last.narrow"),) + states(eng)
        print(f"  {len(A)} x {len(B)} {plan!r} cf {cf} cf2 {cf2}: {cnt} pairs, narrow {st[0]}, states {st[1:]}, expected {expect}")
        if exp_pairs is not None:
            assert cnt == len(exp_pairs) and np.array_equal(sorted_pairs(out.to_numpy(PAIR, cnt)), exp_pairs)
        else:
            assert (cnt, eng.pairs_checksum(out, cnt)) == exp_cc
        assert st == (2,) + tuple(expect)
        nparts = 1 << sum(CF.bits_of(plan))
        return [read_partitions(eng, side, len(X), nparts) for side, X in ((0, A), (1, B))]
    finally:
        for b in (dA, dB, out):
            b.free()


def both_ways(eng, A, B, plan, expect, off, exp_pairs=None, exp_cc=None):
    """the join with the options forced and with `off` = (cf, cf2) -> partitions compared side by side"""
    seen1 = run(eng, A, B, plan, expect, exp_pairs, exp_cc)
    zero = tuple((off[0] * x[0], 0) for x in expect)           # pass 1 is decided by the data, whatever pass 2 may do
    seen0 = run(eng, A, B, plan, zero, exp_pairs, exp_cc, cf=off[0], cf2=off[1])
    for side, X in ((0, A), (1, B)):
        same_partitions(seen0[side], seen1[side], X, plan)
    return seen1


# ---- set piece lengths through CF == 3 ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("nR,nS", [(3 * 4096 + 33, 5 * 4096 + 1), (70_000, 100_031), ((1 << 20) + 17, (1 << 20) + 17),
                                   (4_194_299, 70_000), (4_500_031, 5_000_000)])
def test_set_lengths_through_the_one_writer_pass(eng, oracle, cus, nR, nS):
    R, S, info = CF.set_lengths(nR, nR % 7, nS)
    print(info)
    for A, B in ((R, S), (S, R)):
        expect = (CF.predict(A, PLAN88, cus), CF.predict(B, PLAN88, cus))
        assert expect == ((1, 1), (1, 1))                      # (a device of more than 256 compute units would try no pass 2)
        exp = oracle.join_count_checksum(A, B)
        assert 0 < exp[0] < len(S)                             # matches, and rows that must not match
        seen = both_ways(eng, A, B, PLAN88, expect, (1, 0), exp_cc=exp)
        for side, X in ((0, A), (1, B)):                       # what the case is about reached the kernel: the boundaries say so
            sizes = np.diff(seen[side][2]).reshape(256, 256)
            assert np.array_equal(sizes, CF.partition_sizes(X)) and sizes.max() <= CF.cap2(len(X), 8, 8)
            if len(X) > 1 << 20:
                assert (sizes.max(axis=1) == CF.cap2(len(X), 8, 8)).sum() > 200
            if CF.units(len(X)) <= 5:
                assert sizes[CF.MARK_FRONT].sum() == 0 and sizes[CF.MARK_BACK].sum() == 0


# ---- every live region full ---------------------------------------------------------------------------------------------------

def test_all_full(eng, cus, full):
    R, S, exp = full
    for A, B, e in ((R, S, exp), (S, R, swapped(exp))):
        expect = (CF.predict(A, PLAN88, cus), CF.predict(B, PLAN88, cus))
        assert expect == ((1, 1), (1, 1))
        seen = both_ways(eng, A, B, PLAN88, expect, (1, 0), exp_pairs=e)
        assert (eng.info("last.max_part_R"), eng.info("last.max_part_S")) == (64, 64)
        for side in (0, 1):
            sizes = np.diff(seen[side][2])
            assert set(sizes.tolist()) == {0, 64} and int((sizes == 0).sum()) == 49_152


def swapped(p):
    q = np.empty(len(p), dtype=PAIR)
    q["keyR"], q["keyS"] = p["keyS"], p["keyR"]
    return sorted_pairs(q)


def plain_again(eng, full, side, skipped):
    """the plain all_full join three times on the same context, the options NOT set again: the side that fell back sits out two
    eligible joins (streak 1: 1 << 1, see partition_and_join) in state `skipped`, then is count-free again; the pairs are right
    every time"""
    R, S, exp = full
    seen = []
    for _ in range(3):
        want = [(1, 1), (1, 1)]
        if len(seen) < 2:
            want[side] = skipped
        run(eng, R, S, PLAN88, tuple(want), exp_pairs=exp, rearm=False)
        seen.append(states(eng))
    assert (eng.info("last.max_part_R"), eng.info("last.max_part_S")) == (64, 64)
    return seen


@pytest.mark.parametrize("crafted", ["R", "S"])
def test_all_full_one_too_many_in_pass_2(eng, oracle, cus, full, crafted):
    R, S, info = CF.all_full("over2", crafted)
    side = "RS".index(crafted)
    expect = (CF.predict(R, PLAN88, cus), CF.predict(S, PLAN88, cus))
    assert expect[side] == (1, 2) and expect[1 - side] == (1, 1)
    exp = sorted_pairs(oracle.join(R, S))
    seen1 = run(eng, R, S, PLAN88, expect, exp_pairs=exp)      # gives up on the bucket's fourth tile, repeats that side alone
    assert eng.info("last.max_part_" + crafted) == 65 and eng.info("last.max_part_" + "SR"[side]) == 64
    plain_again(eng, full, side, (1, 0))                  # pass 2 of that side backs off; its pass 1 stays count-free
    seen0 = run(eng, R, S, PLAN88, ((1, 0), (1, 0)), exp_pairs=exp, cf2=0)
    for s, X in ((0, R), (1, S)):                              # nothing of the three stored tiles shows
        same_partitions(seen0[s], seen1[s], X, PLAN88)
    sizes = np.diff(seen1[side][2])
    assert sorted(np.bincount(sizes)[[0, 63, 64, 65]].tolist()) == [1, 1, 16_382, 49_152]


@pytest.mark.parametrize("crafted", ["R", "S"])
def test_all_full_one_too_many_in_pass_1(eng, oracle, cus, full, crafted):
    R, S, info = CF.all_full("over1", crafted)
    side = "RS".index(crafted)
    expect = (CF.predict(R, PLAN88, cus), CF.predict(S, PLAN88, cus))
    assert expect[side] == (2, 0) and expect[1 - side] == (1, 1)
    exp = sorted_pairs(oracle.join(R, S))
    seen1 = run(eng, R, S, PLAN88, expect, exp_pairs=exp)
    plain_again(eng, full, side, (0, 0))                  # that side on the exact path twice, then count-free in both passes
    seen0 = run(eng, R, S, PLAN88, ((0, 0), (0, 0)), exp_pairs=exp, cf=0, cf2=0)
    for s, X in ((0, R), (1, S)):
        same_partitions(seen0[s], seen1[s], X, PLAN88)


# ---- plans other than 8 + 8 ---------------------------------------------------------------------------------------------------

PLANS = [(8, 1), (8, 4), (8, 7), (5, 5), (3, 8), (4, 4), (1, 8)]


def matrix_rows(b1, b2, size):
    """"lines": a mean final partition of 4 (cap2 = 32: regions of a single 32-slot line); "deep": a mean of 200 -- or as near as
    2^21 rows allow, which for the 15-bit plan is 64.  Odd, and no multiple of a tile."""
    nparts = 1 << (b1 + b2)
    return 4 * nparts + 37 if size == "lines" else min(200 * nparts, 1 << 21) - 13


@pytest.mark.parametrize("dist", ["uniform", "dups"])
@pytest.mark.parametrize("size", ["lines", "deep"])
@pytest.mark.parametrize("b1,b2", PLANS)
def test_plan_matrix(eng, oracle, cus, b1, b2, size, dist):
    plan, n = Opts(2, b1, b2), matrix_rows(b1, b2, size)
    R, S = CF.plain(n, dist, b1 * 16 + b2, n - n // 64)
    assert min(len(R), len(S)) > 1024 and max(len(R), len(S)) <= 1 << 21
    if size == "lines":
        assert CF.cap2(len(R), b1, b2) == CF.cap2(len(S), b1, b2) == 32
    exp = sorted_pairs(oracle.join(R, S))
    for A, B, e in ((R, S, exp), (S, R, swapped(exp))):
        expect = (CF.predict(A, plan, cus), CF.predict(B, plan, cus))
        if (1 << b1) < cus:
            assert expect[0][1] == 0 and expect[1][1] == 0     # fewer workgroups than compute units: the histogram pass 2
        if dist == "uniform":
            assert expect[0][0] == 1 and expect[1][0] == 1     # hashed digits fit a region of mean + 10 sigma
        both_ways(eng, A, B, plan, expect, (0, 0), exp_pairs=e)


# ---- the columnar entry -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ids", [False, True])
@pytest.mark.parametrize("case", ["set_lengths", "all_full"])
def test_columnar_entry(eng, oracle, cus, case, ids):
    R, S = CF.set_lengths(70_000, 1, 100_031)[:2] if case == "set_lengths" else CF.all_full()[:2]
    if not ids:                                                # NULL ids: the rowID of a tuple is its index
        R, S = R.copy(), S.copy()
        R["key"], S["key"] = np.arange(len(R), dtype=np.uint64), np.arange(len(S), dtype=np.uint64)
    exp = sorted_pairs(oracle.join(R, S))
    expect = (CF.predict(R, PLAN88, cus), CF.predict(S, PLAN88, cus))
    assert expect == ((1, 1), (1, 1))
    vR, vS = eng.to_device(np.ascontiguousarray(R["payload"])), eng.to_device(np.ascontiguousarray(S["payload"]))
    iR = eng.to_device(np.ascontiguousarray(R["key"])) if ids else None
    iS = eng.to_device(np.ascontiguousarray(S["key"])) if ids else None
    out = eng.alloc((len(exp) + 64) * 16)
    seen = {}
    for cf2 in (1, 0):
        force(eng, 1, cf2)
        cnt = eng.join_cols_dev(vR, iR, len(R), vS, iS, len(S), out, len(exp) + 64, opts=PLAN88)
        assert cnt == len(exp) and np.array_equal(sorted_pairs(out.to_numpy(PAIR, cnt)), exp)
        assert eng.info("last.narrow") == 2 and states(eng) == ((1, cf2), (1, cf2))
        assert (eng.info("last.cols_R"), eng.info("last.cols_S")) == (1, 1)
        seen[cf2] = [read_partitions(eng, side, len(X), 1 << 16) for side, X in ((0, R), (1, S))]
    for side, X in ((0, R), (1, S)):
        same_partitions(seen[0][side], seen[1][side], X, PLAN88)
    for b in (vR, vS, iR, iS, out):
        if b is not None:
            b.free()
