"""GPU suite: the count-free pass 2 with one writer per final partition (rhj_set_option "partition.countfree2").

A side of a pair join whose pass 1 ran count-free is written by pass 2 with one workgroup per pass-1 bucket into a fixed region
of cap2 slots per final partition: no pass-2 histogram, no scan, boundaries with gaps ({start[k] = k * cap2, end[k]}).  Everything
here runs Opts(2, 8, 8) with "partition.narrow" = 2 and both count-free options forced, at sizes where a pass-1 unit is one tile
(cap = 64) and, from 2^20 tuples on, cap2 = 64 for a mean final partition of 16:
  * the pair SET equals the CPU oracle's, both argument orders, count-only mode, a too-small output buffer;
  * rhj_debug_read_partitions returns the boundaries and per-partition multisets of {h, rowID} of "partition.countfree2" = 0;
  * a partition of exactly cap2 - 1 and cap2 tuples stays count-free, cap2 + 1 falls back for THAT side alone;
  * a pass-2-only overflow (one value 200 times) falls back, backs off for two eligible joins and is tried again;
  * a wide rowID, the columnar entry, the entries that must not take the path, two joins of different sizes on one context.
The state a side must report is computed here from the data: 1 where its largest final partition (counted with numpy over the low
16 bits of mix64) fits cap2 = round_up_32(m2 + 10 sqrt(m2) + 1), 2 where it does not.  Primary keys always fit; foreign keys drawn
at random and drawn duplicates pile several equal values into a partition, and at 300,000 tuples (m2 = 4.6 ... 6.1, cap2 = 32)
some inputs exceed it (largest partitions of 35 and 44): those sides must report the fall-back, and the pairs are checked all the same."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle.pyoracle import PAIR, TUPLE, sorted_pairs
from radixhashjoin_amd import SEMI, Engine, Opts
from radixhashjoin_amd.binding import GJ_INNER, mix64, unmix64

pytestmark = pytest.mark.gpu
PLAN = Opts(2, 8, 8)
NP = 1 << 16


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    e.set_option("partition.narrow", 2)
    fn = e.lib.rhj_debug_read_partitions
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    yield e
    e.close()


def force(eng, cf2=1):
    """both options forced (setting them also re-arms the per-side back-off)"""
    eng.set_option("partition.narrow", 2)
    eng.set_option("partition.countfree", 1)
    eng.set_option("partition.countfree2", cf2)


def rel(rng, n, values, key0=0):
    t = np.empty(n, dtype=TUPLE)
    t["key"] = rng.permutation(n).astype(np.uint64) + np.uint64(key0)
    t["payload"] = values
    return t


def make(dist, nR, nS, seed=0):
    rng = np.random.default_rng(nR * 31 + nS + seed)
    if dist == "uniform":                                      # primary key / foreign key
        rv = rng.integers(1, 1 << 62, nR, dtype=np.uint64)
    else:                                                      # uniformly drawn duplicates on both sides
        pool = rng.integers(1, 1 << 62, max(nR // 2, 1), dtype=np.uint64)
        rv = pool[rng.integers(0, len(pool), nR)]
    sv = rv[rng.integers(0, nR, nS)]
    sv[::97] ^= np.uint64(1 << 62)                             # some probe tuples match nothing
    return rel(rng, nR, rv), rel(rng, nS, sv)


def cap2_of(n):
    m = n / NP
    return (int(m + 10.0 * math.sqrt(m)) + 1 + 31) // 32 * 32


def predict2(*rels):
    """"last.countfree2" of each relation under the forced option: 1 if its largest final partition fits its region, else 2"""
    return tuple(1 if int(np.bincount((mix64(X["payload"]) & np.uint64(NP - 1)).astype(np.int64)).max()) <= cap2_of(len(X)) else 2
                 for X in rels)


def states(eng):
    return (eng.info("last.countfree_R"), eng.info("last.countfree_S")), (eng.info("last.countfree2_R"), eng.info("last.countfree2_S"))


def join_pairs(eng, R, S, exp_count=None):
    """the pairs of rhj_join_dev, sorted"""
    dR, dS = eng.to_device(R), eng.to_device(S)
    n = eng.join_dev(dR, len(R), dS, len(S), None, 0, opts=PLAN)           # count-only mode
    st = states(eng)
    if exp_count is not None:
        assert n == exp_count, (n, exp_count)
    out = eng.alloc(max(n, 1) * 16)
    n2 = eng.join_dev(dR, len(R), dS, len(S), out, n, opts=PLAN)
    assert n2 == n
    got = sorted_pairs(out.to_numpy(PAIR, n))
    for b in (dR, dS, out):
        b.free()
    return got, st


def check_join(eng, oracle, R, S, expect2=None, expect1=(1, 1)):
    exp = sorted_pairs(oracle.join(R, S))
    expect2 = predict2(R, S) if expect2 is None else expect2
    force(eng)
    got, st = join_pairs(eng, R, S, len(exp))
    print(f"{len(R)} x {len(S)}: {len(exp)} pairs, countfree {st[0]}, countfree2 {st[1]}")
    assert np.array_equal(got, exp)
    assert st[0] == expect1 and st[1] == expect2, st
    assert eng.info("last.narrow") == 2


@pytest.mark.parametrize("n", [4_097, 300_000, 1_000_003])
@pytest.mark.parametrize("dist", ["uniform", "dups"])
def test_parity_both_orders(eng, oracle, dist, n):
    R, S = make(dist, n, n + n // 3)
    if dist == "uniform":
        assert predict2(R) == (1,)                              # hashed distinct values fit their regions
    check_join(eng, oracle, R, S)
    check_join(eng, oracle, S, R)


def test_output_capacity_overflow(eng, oracle):
    R, S = make("uniform", 300_000, 400_000, seed=1)
    exp = sorted_pairs(oracle.join(R, S))
    force(eng)
    dR, dS = eng.to_device(R), eng.to_device(S)
    cap = len(exp) // 3
    out = eng.alloc(cap * 16)
    n = eng.join_dev(dR, len(R), dS, len(S), out, cap, opts=PLAN, allow_overflow=True)
    assert n == len(exp) and n > cap                           # the full count is reported, nothing is written beyond cap
    assert states(eng)[1] == predict2(R, S)
    got = out.to_numpy(PAIR, cap)
    both = np.concatenate([sorted_pairs(got), exp])            # the pairs that were written are pairs of the join, each once
    assert len(np.unique(both)) == len(exp) and len(np.unique(got)) == cap
    for b in (dR, dS, out):
        b.free()


def read_partitions(eng, side, n):
    pay, rid, bounds = np.empty(n, np.uint64), np.empty(n, np.uint32), np.empty(NP + 1, np.uint64)
    rc = eng.lib.rhj_debug_read_partitions(eng.ctx, side, pay.ctypes.data, rid.ctypes.data, bounds.ctypes.data)
    assert rc == 0
    part = np.repeat(np.arange(NP, dtype=np.int64), np.diff(bounds.astype(np.int64)))
    order = np.lexsort((rid, pay, part))                       # {h, rowID} sorted inside every partition
    return pay[order], rid[order], bounds.astype(np.int64)


@pytest.mark.parametrize("dist,n", [("uniform", 1_000_003), ("dups", 300_000), ("uniform", 4_097)])
def test_same_partitions_as_the_histogram_path(eng, oracle, dist, n):
    R, S = make(dist, n, n, seed=3)
    exp = oracle.join_count_checksum(R, S)
    cap = exp[0] + 1024
    dR, dS, out = eng.to_device(R), eng.to_device(S), eng.alloc(cap * 16)
    seen = {}
    for cf2 in (0, 1):
        force(eng, cf2)
        cnt = eng.join_dev(dR, n, dS, n, out, cap, opts=PLAN)
        assert (cnt, eng.pairs_checksum(out, cnt)) == exp
        assert states(eng) == ((1, 1), tuple(cf2 * x for x in predict2(R, S)))
        seen[cf2] = [read_partitions(eng, side, n) for side in (0, 1)]
    for side in (0, 1):
        p0, r0, b0 = seen[0][side]
        p1, r1, b1 = seen[1][side]
        assert int(b0[-1]) == n and np.array_equal(b0, b1)
        assert np.array_equal(p0, p1) and np.array_equal(r0, r1)
        rel_h = np.sort(mix64((R if side == 0 else S)["payload"]))                    # every h is there, whatever the partition
        assert np.array_equal(np.sort(p1), rel_h)
    for b in (dR, dS, out):
        b.free()


def edge_relations(count, n=1 << 20, d1=0x5A, d2=0xC3, seed=7):
    """A: n distinct join values of which exactly `count` fall into final partition (d1, d2), on rows spread evenly over the
    pass-1 units (so that no pass-1 region overflows); B: foreign keys into A that avoid that partition"""
    rng = np.random.default_rng(seed + count)
    pbits = np.uint64(d1 | d2 << 8)
    h = mix64(rng.integers(1, 1 << 62, n, dtype=np.uint64))
    inside = (h & np.uint64(NP - 1)) == pbits
    h[inside] ^= np.uint64(0x100)                              # the background leaves the partition (for its neighbour in d2)
    rows = (np.arange(count, dtype=np.int64) * n) // count
    h[rows] = (rng.integers(1, 1 << 40, count, dtype=np.uint64) << np.uint64(16)) | pbits
    av = unmix64(h)
    assert len(np.unique(av)) == n and int(((mix64(av) & np.uint64(NP - 1)) == pbits).sum()) == count
    outside = np.flatnonzero((h & np.uint64(NP - 1)) != pbits)
    bv = av[outside[rng.integers(0, len(outside), n)]]
    bv[::97] ^= np.uint64(1 << 62)
    bv = bv[(mix64(bv) & np.uint64(NP - 1)) != pbits]          # (a flipped value may land anywhere)
    A = np.empty(n, dtype=TUPLE)
    A["key"] = np.arange(n, dtype=np.uint64)                   # rowID = row: the chosen rows stay spread over the units
    A["payload"] = av
    return A, rel(rng, len(bv), bv)


@pytest.mark.parametrize("crafted", ["R", "S"])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_region_edges(eng, oracle, delta, crafted):
    cap2 = 64                                                  # n = 2^20: m2 = 16, round_up_32(16 + 40 + 1)
    A, B = edge_relations(cap2 + delta)
    R, S = (A, B) if crafted == "R" else (B, A)
    expect2 = (1, 1) if delta <= 0 else ((2, 1) if crafted == "R" else (1, 2))
    check_join(eng, oracle, R, S, expect2=expect2)             # (the count-free pass 1 of both sides stood: expect1 = (1, 1))
    name = "last.max_part_R" if crafted == "R" else "last.max_part_S"
    if delta <= 0:                                             # (the last join ran on boundaries with gaps)
        assert eng.info(name) == cap2 + delta
    force(eng, 0)
    dR, dS = eng.to_device(R), eng.to_device(S)
    eng.join_dev(dR, len(R), dS, len(S), None, 0, opts=PLAN)
    assert eng.info(name) == cap2 + delta
    for b in (dR, dS):
        b.free()


def test_pass2_only_overflow_and_back_off(eng, oracle):
    n = 1 << 20
    R, S = make("uniform", n, n, seed=5)
    Sk = S.copy()
    Sk["key"] = np.arange(n, dtype=np.uint64)
    Sk["payload"][(np.arange(200, dtype=np.int64) * n) // 200] = R["payload"][12345]      # one value 200 times, rows spread evenly
    exp_k, exp = sorted_pairs(oracle.join(R, Sk)), sorted_pairs(oracle.join(R, S))
    force(eng)
    got, st = join_pairs(eng, R, Sk)                           # two joins: the count, then the pairs
    assert np.array_equal(got, exp_k)
    # the count-only join fell back (2) and started the back-off; the second join of join_pairs was the first of two skipped
    assert st == ((1, 1), (1, 2)), st
    assert states(eng) == ((1, 1), (1, 0))
    dR, dS, out = eng.to_device(R), eng.to_device(S), eng.alloc((len(exp) + 16) * 16)
    seen = []
    for call in range(3):
        cnt = eng.join_dev(dR, n, dS, n, out, len(exp) + 16, opts=PLAN)
        assert np.array_equal(sorted_pairs(out.to_numpy(PAIR, cnt)), exp)
        seen.append(states(eng))
    assert seen == [((1, 1), (1, 0)), ((1, 1), (1, 1)), ((1, 1), (1, 1))], seen
    dK = eng.to_device(Sk)                                     # the skewed relation again: tried, falls back again
    cnt = eng.join_dev(dR, n, dK, n, out, len(exp) + 16, opts=PLAN)
    assert np.array_equal(sorted_pairs(out.to_numpy(PAIR, cnt)), exp_k)
    assert states(eng) == ((1, 1), (1, 2))
    for b in (dR, dS, dK, out):
        b.free()


def test_wide_rowid_ends_in_the_16_byte_repeat(eng, oracle):
    R, S = make("uniform", 90_000, 120_000, seed=2)
    S["key"][4321] = np.uint64((1 << 32) + 5)
    exp = sorted_pairs(oracle.join(R, S))
    force(eng)
    got, st = join_pairs(eng, R, S, len(exp))
    assert np.array_equal(got, exp)
    assert eng.info("last.narrow") == 0 and states(eng) == ((0, 0), (0, 0))


@pytest.mark.parametrize("ids", [False, True])
def test_columnar_entry(eng, oracle, ids):
    n = 300_000
    R, S = make("uniform", n, n + 999, seed=6)
    if not ids:                                                # NULL ids: the rowID of a tuple is its index
        R["key"], S["key"] = np.arange(len(R), dtype=np.uint64), np.arange(len(S), dtype=np.uint64)
    exp = sorted_pairs(oracle.join(R, S))
    force(eng)
    vR, vS = eng.to_device(np.ascontiguousarray(R["payload"])), eng.to_device(np.ascontiguousarray(S["payload"]))
    iR = eng.to_device(np.ascontiguousarray(R["key"])) if ids else None
    iS = eng.to_device(np.ascontiguousarray(S["key"])) if ids else None
    assert eng.join_cols_dev(vR, iR, len(R), vS, iS, len(S), None, 0, opts=PLAN) == len(exp)
    out = eng.alloc(len(exp) * 16)
    cnt = eng.join_cols_dev(vR, iR, len(R), vS, iS, len(S), out, len(exp), opts=PLAN)
    assert cnt == len(exp) and np.array_equal(sorted_pairs(out.to_numpy(PAIR, cnt)), exp)
    assert states(eng) == ((1, 1), predict2(R, S)) and (eng.info("last.cols_R"), eng.info("last.cols_S")) == (1, 1)
    p1 = [read_partitions(eng, side, len(rel_)) for side, rel_ in ((0, R), (1, S))]
    force(eng, 0)
    assert eng.join_cols_dev(vR, iR, len(R), vS, iS, len(S), out, len(exp), opts=PLAN) == len(exp)
    p0 = [read_partitions(eng, side, len(rel_)) for side, rel_ in ((0, R), (1, S))]
    for a, b in zip(p0, p1):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for b in (vR, vS, iR, iS, out):
        if b is not None:
            b.free()


def test_other_entries_keep_exact_boundaries(eng, oracle):
    n = 300_000
    R, S = make("dups", n, n, seed=8)
    dR, dS = eng.to_device(R), eng.to_device(S)
    w = eng.to_device(np.arange(1, n + 1, dtype=np.uint64))
    res = {}
    for cf2 in (0, 1):
        force(eng, cf2)
        ids = eng.alloc(n * 8)
        k = eng.semi_join_dev(dR, n, dS, n, SEMI, ids, n, opts=PLAN)
        st_semi = states(eng)
        semi = np.sort(ids.to_numpy(np.uint64, k))
        total = eng.join_sum_dev(dR, n, dS, n, [w], n, opts=PLAN)
        st_sum = states(eng)
        keys, cR, cS = eng.alloc(n * 8), eng.alloc(n * 8), eng.alloc(n * 8)
        g = eng.group_join_dev(dR, n, dS, n, mode=GJ_INNER, d_out_keys=keys, d_out_cntR=cR, d_out_cntS=cS, capacity=n, opts=PLAN)
        st_gj = states(eng)
        kk, a, b = keys.to_numpy(np.uint64, g), cR.to_numpy(np.uint64, g), cS.to_numpy(np.uint64, g)
        o = np.argsort(kk)
        res[cf2] = (semi, total, kk[o], a[o], b[o])
        for st in (st_semi, st_sum, st_gj):
            assert st == ((1, 1), (0, 0)), (cf2, st)
        for x in (ids, keys, cR, cS):
            x.free()
    assert res[0][1] == res[1][1] and res[0][1][0] == oracle.join_count_checksum(R, S)[0]
    for x, y in zip(res[0], res[1]):
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, y)
    for b in (dR, dS, w):
        b.free()


def test_a_smaller_join_after_a_larger_one(oracle):
    """one context, the larger join first: nothing of its end[] / start[] may reach the smaller join"""
    e = Engine(0)
    big, small = make("uniform", 1_000_003, 800_000, seed=9), make("dups", 5_000, 4_097, seed=9)
    for R, S in (big, small, big):
        check_join(e, oracle, R, S)
    e.close()
