"""GPU suite: the count-free pass 1 of narrow 8+8 joins (rhj_set_option "partition.countfree").

Pass 1 writes every (digit, unit) run into a fixed region instead of at exact cursors, so the 16-byte histogram read is gone;
pass 2 reads the pieces.  Forced on (1) against forced off (0):
  * (count, pairs checksum) equal the CPU oracle's on uniform, dense i + 1, k << 16, duplicate-heavy and Zipf 0.9 inputs, from a
    few thousand rows (one tile per unit: regions far larger than the relation) to a few million, R x S and S x R, rowIDs up
    to 2^32 - 1, and one rowID of 2^32 (the narrow format's own fallback on top);
  * "last.countfree_R/_S" report the path: 1 for a side of hashed distinct (or uniformly drawn) values, 2 for a side built to
    overflow a region (one value on a quarter of the rows), which is repeated with exact cursors inside the call; the context
    then leaves that side on the exact path for the following calls (0) while the other side stays count-free;
  * the layout property the design rests on: the final boundaries are IDENTICAL and every final partition holds the same
    multiset of {h, rowID} under both settings (read back through the test entry rhj_debug_read_partitions)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.pyoracle import TUPLE
from radixhashjoin_amd import Engine, Opts

pytestmark = pytest.mark.gpu
PLAN = Opts(2, 8, 8)
SIZES = [3_000, 70_000, 3_000_000]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    e.set_option("partition.narrow", 2)
    fn = e.lib.rhj_debug_read_partitions
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    yield e
    e.close()


def rel(rng, n, values, key0=0):
    t = np.empty(n, dtype=TUPLE)
    t["key"] = rng.permutation(n).astype(np.uint64) + np.uint64(key0)
    t["payload"] = values
    return t


def zipf_ranks(rng, n, D, theta=0.9):
    """ranks 1..D with P(r) ~ r^-theta (inverse CDF of the continuous form, as the engine's generator)"""
    e = 1.0 - theta
    span = (D + 1.0) ** e - 1.0
    r = np.floor((1.0 + rng.random(n) * span) ** (1.0 / e)).astype(np.int64)
    return np.clip(r, 1, D)


def make(dist, nR, nS, seed=0, key0R=0, key0S=0):
    """-> R, S, (countfree_R, countfree_S) expected under the forced option (None: either 1 or 2)"""
    rng = np.random.default_rng(nR * 31 + nS + seed)
    if dist == "uniform":
        rv = rng.integers(1, 1 << 62, nR, dtype=np.uint64)
    elif dist == "dense":
        rv = np.arange(1, nR + 1, dtype=np.uint64)
    elif dist == "shift16":
        rv = np.arange(1, nR + 1, dtype=np.uint64) << np.uint64(16)
    elif dist == "dups":
        rv = rng.integers(1, 1 << 62, max(nR // 4, 1), dtype=np.uint64)[rng.integers(0, max(nR // 4, 1), nR)]
    elif dist in ("zipf", "quarter"):
        rv = rng.integers(1, 1 << 62, nR, dtype=np.uint64)
    else:
        raise ValueError(dist)
    if dist == "zipf":
        sv = rv[zipf_ranks(rng, nS, nR) - 1]
    elif dist == "quarter":
        sv = rv[rng.integers(0, nR, nS)]
        sv[rng.permutation(nS)[: nS // 4]] = rv[0]            # one value on a quarter of the rows: no region holds its digit
    else:
        sv = rv[rng.integers(0, nR, nS)]
    sv[::97] ^= np.uint64(1 << 62)                             # some probe tuples match nothing
    expect = {"uniform": (1, 1), "dense": (1, 1), "shift16": (1, 1), "dups": (None, None), "zipf": (1, None), "quarter": (1, 2)}[dist]
    return rel(rng, nR, rv, key0R), rel(rng, nS, sv, key0S), expect


def run(eng, R, S, countfree, cap):
    eng.set_option("partition.countfree", countfree)          # (also re-arms the per-side back-off)
    dR, dS = eng.to_device(R), eng.to_device(S)
    out = eng.alloc(cap * 16)
    n = eng.join_dev(dR, len(R), dS, len(S), out, cap, opts=PLAN)
    got = (n, eng.pairs_checksum(out, n))
    state = (eng.info("last.narrow"), eng.info("last.countfree_R"), eng.info("last.countfree_S"))
    for b in (dR, dS, out):
        b.free()
    return got, state


def check_paths(state, expect):
    assert state[0] == 2
    for got, exp in zip(state[1:], expect):
        assert got in (1, 2) if exp is None else got == exp, (state, expect)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dist", ["uniform", "dense", "shift16", "dups", "zipf", "quarter"])
def test_same_result_both_orders(eng, oracle, dist, n):
    nR, nS = n, n + n // 3
    R, S, expect = make(dist, nR, nS)
    exp = oracle.join_count_checksum(R, S)
    print(f"{dist} {nR} x {nS}: oracle count {exp[0]}")
    cap = exp[0] + 1024
    got0, st0 = run(eng, R, S, 0, cap)
    assert got0 == exp and st0 == (2, 0, 0)
    got1, st1 = run(eng, R, S, 1, cap)
    print(f"  R x S: {got1} paths {st1}")
    assert got1 == exp
    check_paths(st1, expect)
    # S x R: the pairs are (rowS, rowR) now, the sides swap
    exps = oracle.join_count_checksum(S, R)
    got0, st0 = run(eng, S, R, 0, cap)
    assert got0 == exps and st0 == (2, 0, 0)
    got1, st1 = run(eng, S, R, 1, cap)
    print(f"  S x R: {got1} paths {st1}")
    assert got1 == exps
    check_paths(st1, expect[::-1])


@pytest.mark.parametrize("n", [70_000, 2_000_000])
def test_rowids_to_the_edge_of_32_bits(eng, oracle, n):
    R, S, expect = make("uniform", n, n, seed=1, key0R=(1 << 32) - n, key0S=(1 << 32) - n)
    assert int(R["key"].max()) == (1 << 32) - 1
    exp = oracle.join_count_checksum(R, S)
    got, st = run(eng, R, S, 1, exp[0] + 1024)
    assert got == exp
    check_paths(st, expect)


@pytest.mark.parametrize("side", ["R", "S"])
def test_one_wide_rowid_falls_back_to_16_bytes(eng, oracle, side):
    R, S, _ = make("uniform", 90_000, 120_000, seed=2)
    (R if side == "R" else S)["key"][12345] = np.uint64(1 << 32)
    exp = oracle.join_count_checksum(R, S)
    got, st = run(eng, R, S, 1, exp[0] + 1024)
    assert got == exp
    assert st == (0, 0, 0)                                    # the repeat ran in the 16-byte format, with exact cursors
    eng.set_option("partition.narrow", 2)                     # re-arm


@pytest.mark.parametrize("n", [200_000, 2_500_000])
def test_overflow_of_S_alone_and_back_off(eng, oracle, n):
    R, S, _ = make("quarter", n, n)
    exp = oracle.join_count_checksum(R, S)
    cap = exp[0] + 1024
    got, st = run(eng, R, S, 1, cap)
    assert got == exp and st == (2, 1, 2)                     # R's partition stood, S was repeated with exact cursors
    dR, dS, out = eng.to_device(R), eng.to_device(S), eng.alloc(cap * 16)
    for call in range(2):                                     # the following calls: S stays on the exact path, R count-free
        cnt = eng.join_dev(dR, len(R), dS, len(S), out, cap, opts=PLAN)
        assert (cnt, eng.pairs_checksum(out, cnt)) == exp
        assert (eng.info("last.countfree_R"), eng.info("last.countfree_S")) == (1, 0), call
    cnt = eng.join_dev(dR, len(R), dS, len(S), out, cap, opts=PLAN)      # the back-off is over: tried again, falls back again
    assert (cnt, eng.pairs_checksum(out, cnt)) == exp
    assert (eng.info("last.countfree_R"), eng.info("last.countfree_S")) == (1, 2)
    for b in (dR, dS, out):
        b.free()


def test_first_join_of_a_context_overflows(oracle):
    """nothing of an earlier join in the scratch tables: the kernels that run after an overflow without testing the skip word
    (the pass-2 scan, the task builder) must find valid loop bounds"""
    R, S, _ = make("quarter", 150_000, 260_000, seed=4)
    exp = oracle.join_count_checksum(S, R)
    e = Engine(0)
    e.set_option("partition.narrow", 2)
    got, st = run(e, S, R, 1, exp[0] + 1024)
    e.close()
    assert got == exp and st == (2, 2, 1)


def read_partitions(eng, side, n):
    pay, rid, bounds = np.empty(n, np.uint64), np.empty(n, np.uint32), np.empty((1 << 16) + 1, np.uint64)
    rc = eng.lib.rhj_debug_read_partitions(eng.ctx, side, pay.ctypes.data, rid.ctypes.data, bounds.ctypes.data)
    assert rc == 0
    part = np.repeat(np.arange(1 << 16, dtype=np.int64), np.diff(bounds.astype(np.int64)))
    order = np.lexsort((rid, pay, part))                       # {h, rowID} sorted inside every partition
    return pay[order], rid[order], bounds


@pytest.mark.parametrize("dist,n", [("uniform", 3_000_000), ("zipf", 2_500_000), ("uniform", 5_000)])
def test_final_partitions_are_those_of_the_exact_path(eng, oracle, dist, n):
    R, S, expect = make(dist, n, n, seed=3)
    exp = oracle.join_count_checksum(R, S)
    cap = exp[0] + 1024
    dR, dS, out = eng.to_device(R), eng.to_device(S), eng.alloc(cap * 16)
    seen = {}
    for cf in (0, 1):
        eng.set_option("partition.countfree", cf)
        cnt = eng.join_dev(dR, n, dS, n, out, cap, opts=PLAN)
        assert (cnt, eng.pairs_checksum(out, cnt)) == exp
        paths = (eng.info("last.countfree_R"), eng.info("last.countfree_S"))
        assert paths == (0, 0) if cf == 0 else paths[0] == 1
        seen[cf] = [read_partitions(eng, side, n) for side in (0, 1)]
    for side in (0, 1):
        p0, r0, b0 = seen[0][side]
        p1, r1, b1 = seen[1][side]
        assert int(b0[-1]) == n
        assert torch.equal(torch.from_numpy(b0.astype(np.int64)), torch.from_numpy(b1.astype(np.int64)))
        assert np.array_equal(p0, p1) and np.array_equal(r0, r1)
    for b in (dR, dS, out):
        b.free()


def test_option_and_reserve(eng):
    eng.set_option("partition.countfree", -1)
    eng.set_option("partition.countfree", 1)
    eng.reserve(5_000, 2_000_000, PLAN)                       # regions of a small relation exceed 16 n bytes: covered
    with pytest.raises(Exception):
        eng.set_option("partition.countfree", 2)
