"""GPU suite: the word-plane layout of the count-free intermediate payload array.

Between the two count-free passes slot a of the payload array keeps the low word of h = mix64(payload) at word
((a >> 5) << 6) | (a & 31) and the high word 32 words further; k_hist_pieces_n reads the low-word lines only, 256 tuples per
wavefront load, and masks the last, partial block of a piece by tuple index.  With "partition.countfree" forced to 1:
  * piece lengths (the run of one digit inside one pass-1 unit) are SET by the input order, not left to chance: every unit
    carries runs of 0, 1, 31, 32, 33, 63, 64 tuples (one tile per unit: regions of 64 slots) and, in the 5 M-row case (two tiles
    per unit: regions of 96 slots), 65, 95 and 96 as well -- the test computes the lengths from the inputs and asserts that
    they are there, and "last.countfree_R/_S" == 1 shows that no run overflowed into the exact path;
  * the join values are built in the mixed space (unmix64): "lowdup" -- many tuples share their low word and differ in the high
    word only, "highdup" -- one high word per 65,536 rows, distinct low words; the probe side adds values that differ from a build
    value in the high word only, and in the upper half of the low word only (same final partition).  A swapped, dropped or
    misplaced half turns up as wrong pairs;
  * (count, pairs checksum) equal the CPU oracle's, R x S and S x R;
  * boundaries and the {h, rowID} multiset of every final partition equal those of the run with the option at 0."""
import ctypes as C

import numpy as np
import pytest

from cf_cases import build_side, probe_side                       # (moved: tests/cf_cases.py, where d2 can be set as well)
from oracle.pyoracle import TUPLE
from radixhashjoin_amd import Engine, Opts, mix64, unmix64

pytestmark = pytest.mark.gpu
PLAN = Opts(2, 8, 8)
U64 = np.uint64
TILE, TARGET_UNITS = 4096, 1024                               # pass-1 unit length: n / 1024 rounded up to whole tiles
SPECIAL = {4096: [0, 1, 31, 32, 33, 63, 64], 8192: [0, 1, 31, 32, 33, 63, 64, 65, 95, 96]}
CAP = {4096: 64, 8192: 96}                                    # round_up_32(m + 10 sqrt(m) + 1), m = L / 256


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    e.set_option("partition.narrow", 2)
    fn = e.lib.rhj_debug_read_partitions
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    yield e
    e.close()


def unit_len(n):
    per = -(-n // TARGET_UNITS)
    return max(TILE, -(-per // TILE) * TILE)


def piece_lengths(t):
    """run lengths per (pass-1 unit, digit), from the relation as the library sees it"""
    n, L = len(t), unit_len(len(t))
    d1 = (mix64(t["payload"]) & U64(255)).astype(np.int64)
    return np.bincount((np.arange(n) // L) * 256 + d1, minlength=-(-n // L) * 256)


def rel(rng, h):
    t = np.empty(len(h), dtype=TUPLE)
    t["key"] = rng.permutation(len(h)).astype(U64)
    t["payload"] = unmix64(h)
    return t


def read_partitions(eng, side, n):
    pay, rid, bounds = np.empty(n, np.uint64), np.empty(n, np.uint32), np.empty((1 << 16) + 1, np.uint64)
    rc = eng.lib.rhj_debug_read_partitions(eng.ctx, side, pay.ctypes.data, rid.ctypes.data, bounds.ctypes.data)
    assert rc == 0
    part = np.repeat(np.arange(1 << 16, dtype=np.int64), np.diff(bounds.astype(np.int64)))
    order = np.lexsort((rid, pay, part))                       # {h, rowID} sorted inside every partition
    return pay[order], rid[order], bounds


def join_both(eng, A, B, exp):
    """A x B with the option at 0 and at 1 -> the partitions of both sides under both settings"""
    cap = exp[0] + 1024
    dA, dB, out = eng.to_device(A), eng.to_device(B), eng.alloc(cap * 16)
    seen = {}
    for cf in (0, 1):
        eng.set_option("partition.countfree", cf)
        cnt = eng.join_dev(dA, len(A), dB, len(B), out, cap, opts=PLAN)
        got = (cnt, eng.pairs_checksum(out, cnt))
        state = (eng.info("last.narrow"), eng.info("last.countfree_R"), eng.info("last.countfree_S"))
        print(f"  countfree={cf}: {got} paths {state}")
        assert got == exp
        assert state == (2, cf, cf)                            # (1, 1): every run fitted its region, nothing was repeated
        seen[cf] = [read_partitions(eng, side, len(X)) for side, X in ((0, A), (1, B))]
    for b in (dA, dB, out):
        b.free()
    return seen


@pytest.mark.parametrize("nR,nS", [(3 * 4096 + 33, 5 * 4096 + 1), (70_000, 100_031), (4096 + 31, 3_000), (5_000_000, 4_500_031)])
@pytest.mark.parametrize("kind", ["lowdup", "highdup"])
def test_planes_keep_both_halves(eng, oracle, kind, nR, nS):
    rng = np.random.default_rng(nR * 7 + nS + len(kind))
    hR = build_side(rng, nR, kind)
    R, S = rel(rng, hR), rel(rng, probe_side(rng, hR, nS))
    for t in (R, S):                                           # the piece lengths the case is about are really there
        lens, L = piece_lengths(t), unit_len(len(t))
        assert lens.max() <= CAP[L]
        if len(t) >= L:
            assert set(SPECIAL[L]) <= set(lens.tolist()), sorted(set(SPECIAL[L]) - set(lens.tolist()))
    exp = oracle.join_count_checksum(R, S)
    print(f"{kind} {nR} x {nS}: oracle count {exp[0]}")
    assert 0 < exp[0] < nS                                     # matches, and probe rows that must not match
    for A, B, e in ((R, S, exp), (S, R, oracle.join_count_checksum(S, R))):
        seen = join_both(eng, A, B, e)
        for side, X in ((0, A), (1, B)):
            p0, r0, b0 = seen[0][side]
            p1, r1, b1 = seen[1][side]
            assert int(b0[-1]) == len(X)
            assert np.array_equal(b0, b1)
            assert np.array_equal(p0, p1) and np.array_equal(r0, r1)
            # and they are the input's own {mix64(payload), rowID}: nothing lost or altered on either path
            o0, o1 = np.lexsort((r1, p1)), np.lexsort((X["key"], mix64(X["payload"])))
            assert np.array_equal(p1[o0], mix64(X["payload"])[o1]) and np.array_equal(r1[o0], X["key"][o1].astype(np.uint32))
