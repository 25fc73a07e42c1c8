"""GPU suite: the edges of the multi-GPU stage calls of include/rhj.h (rhj_shard_stats / _split / _split_peer / _partition / _join).

tests/test_gpu_shard_stages.py and tests/test_gpu_sharded*.py run those calls on one family of inputs; the kernels and template
instantiations only they reach (k_seg_units, the sender-tag scatter's WnTag, the narrow-in 16-byte-out k_scatter_wc_n, and
k_join_bkt<.., TAGGED> with its own compare mask and 2 x 16 rowID bases) could be wrong in these places without one of them failing:

    1. bases      R and S always had the SAME rowID bases (row0[s]); here they differ for every sender, so that reading one side's
                  bases for the other, on whichever side the table is built, shows in every pair
    2. senders    nseg was 2, 3, 4, 5 or 8; here 1, 2, 6 and 7 (12 and 14 unit groups: no power of two), 11, 13 and 16 (one group per
                  sender; tag 15)
    3. segments   no received segment was longer than one tile per unit; here lengths 0, 1, 4095, 4096, 4097, 12345 and, across
                  units_per_seg * 4096 (where a unit becomes two tiles), one more; whole sides of 1, 63 and 1023 tuples; an empty side
    4. values     join values were 24-bit numbers; here random 64-bit values, and the near-miss, fold-collision and extreme-value
                  families of tests/test_gpu_adversarial.py through the TAGGED, GLOBAL16 and PLAIN receivers, TAGGED also with build
                  sides of several table chunks
    5. overflow   rhj_shard_join's RHJ_E_OVERFLOW contract ("count / overflow behaviour of rhj_join_dev"), which
                  radixhashjoin_amd/sharded.py relies on, against a canary guard behind the capacity
    6. senders' calls   only shift, bits = 20, 8 on tens of thousands of rows; here n = 0, 1 and around one tile, 1-4 class bits,
                  class bits at the top of the word, a rowID span of exactly 2^32 - 1 (accepted) against 2^32 (refused), key_base
                  below the smallest rowID

Everything is compared bit for bit.  A join's reference is the CPU oracle on the GLOBAL relations, as sorted (rowR, rowS) pairs.
The receiver tests build the wire format of include/rhj.h directly in numpy -- sender s's segment is P = mix64(payload) (uint64)
and K = rowID - row0[s] (uint32) -- so the oracle's relation is {key = row0[s] + K, payload = P}: mix64 is a bijection, equal P
are equal payloads.  Local rowIDs are a permutation of 0 .. len - 1 inside EVERY segment: all senders use the same local
numbers, a tuple credited to the wrong sender is a wrong pair.  The sender calls are compared with numpy class by class."""
import ctypes as C

import numpy as np
import pytest

from oracle.pyoracle import TUPLE
from radixhashjoin_amd import Engine, Opts
from radixhashjoin_amd.binding import (RHJ_E_INVALID, RHJ_E_OVERFLOW, RHJ_OK, SHARD_GLOBAL16, SHARD_PLAIN, SHARD_TAGGED, RhjError, _addr,
                                       mix64, narrow_bytes, narrow_key_offset)
from test_gpu_adversarial import family, radix_bits

pytestmark = pytest.mark.gpu

U64 = np.uint64
TOP32 = (1 << 32) - 1
BKT, CT, CT_HALF, CT_20, CT_MID = 0, 2, 3, 4, 6          # "last.join_kernel" (include/rhj.h)
ONE_TABLE = 4224                                           # build tuples in the one-table kernel's LDS table (BJ_CHUNK)
MODES = [SHARD_TAGGED, SHARD_GLOBAL16, SHARD_PLAIN]
MODE_NAME = {SHARD_TAGGED: "tagged", SHARD_GLOBAL16: "global16", SHARD_PLAIN: "plain"}
P88, P44, P66, P89 = Opts(2, 8, 8), Opts(2, 4, 4), Opts(2, 6, 6), Opts(2, 8, 9)
PLAN_NAME = {id(P88): "8+8", id(P44): "4+4", id(P66): "6+6", id(P89): "8+9"}


@pytest.fixture(scope="module")
def shared_engine():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture
def eng(shared_engine):
    """the module's context, the kernel options back at their defaults afterwards"""
    yield shared_engine
    for k in ("join.big_tables", "join.big_kernel"):
        shared_engine.set_option(k, -1)


def sort2(a):
    return a[np.lexsort((a[:, 1], a[:, 0]))]


# ---------------------------------------------------------------------------------------------------------------------------
# the receiver: segments in the wire format -> rhj_shard_partition x 2 -> rhj_shard_join
# ---------------------------------------------------------------------------------------------------------------------------
def partition_sides(eng, segsR, row0R, segsS, row0S, plan, mode):
    """uploads the segments [(P, K) per sender] of both sides and partitions them (side 0, side 1); returns the two seg_off"""
    offs = []
    for side, (segs, row0) in enumerate(((segsR, row0R), (segsS, row0S))):
        off = np.concatenate([[0], np.cumsum([len(p) for p, _ in segs])]).astype(np.int64)
        m = int(off[-1])
        P = np.concatenate([p for p, _ in segs]).astype(U64)
        K = np.concatenate([k for _, k in segs]).astype(np.uint32)
        dP, dK = eng.to_device(P if m else np.zeros(1, U64)), eng.to_device(K if m else np.zeros(1, np.uint32))
        eng.shard_partition(side, dP, dK, m, off.tolist(), row0, plan, mode)
        eng.sync()
        dP.free(); dK.free()
        offs.append(off)
    return offs


def join_exact(eng):
    """count only, then the exact capacity: the pairs as an (n, 2) uint64 array"""
    cnt = eng.shard_join(None, 0)
    out = eng.alloc(16 * max(cnt, 1))
    assert eng.shard_join(out, cnt) == cnt
    pairs = out.to_numpy(U64, 2 * cnt).reshape(-1, 2)
    out.free()
    return pairs


def receive_and_join(eng, segsR, row0R, segsS, row0S, plan, mode):
    offs = partition_sides(eng, segsR, row0R, segsS, row0S, plan, mode)
    return join_exact(eng), offs


def global_rel(segs, row0):
    """what the senders held: {key = row0[s] + K, payload = P}"""
    t = np.empty(sum(len(p) for p, _ in segs), dtype=TUPLE)
    if len(t):
        t["key"] = np.concatenate([k.astype(U64) + U64(b) for (_, k), b in zip(segs, row0)])
        t["payload"] = np.concatenate([p for p, _ in segs])
    return t


def expected_pairs(oracle, R, S):
    exp = oracle.join(R, S)
    return sort2(np.stack([exp["keyR"], exp["keyS"]], axis=1))


def allow_one_table(eng, mR, mS, plan, mode):
    """rhj_shard_join refuses RHJ_SHARD_TAGGED ("partitions this large") where the automatic choice (choose_join_kind: the average
    build partition beyond one table) is not the one-table kernel: "join.big_tables" 0, "always the one-table kernel" (rhj.h)"""
    if mode == SHARD_TAGGED and min(mR, mS) >> radix_bits(plan) > ONE_TABLE:
        eng.set_option("join.big_tables", 0)
        return True
    return False


def check_both_orders(eng, oracle, segsR, row0R, segsS, row0S, plan, mode, kernel):
    """(R, S) and then (S, R) as sides 0 and 1 -- the table is built on either side -- against the oracle; returns the (R, S)
    result (sorted) and the seg_off of R and S"""
    R, S = global_rel(segsR, row0R), global_rel(segsS, row0S)
    e = expected_pairs(oracle, R, S)
    ran = kernel if len(R) and len(S) else -1                                 # rhj.h "last.join_kernel": -1 for an empty input
    got, offs = receive_and_join(eng, segsR, row0R, segsS, row0S, plan, mode)
    assert eng.info("last.join_kernel") == ran
    assert len(got) == len(e)
    assert np.array_equal(sort2(got), e)
    got, _ = receive_and_join(eng, segsS, row0S, segsR, row0R, plan, mode)
    assert eng.info("last.join_kernel") == ran
    assert len(got) == len(e)
    assert np.array_equal(sort2(got), sort2(e[:, ::-1]))
    return e, offs


def bases(nseg, mode):
    """rowID bases that differ between R and S for every sender, beyond 2^32 from sender 1 on; PLAIN: zero (rhj.h)"""
    if mode == SHARD_PLAIN:
        return [0] * nseg, [0] * nseg
    return [s * (5 << 30) + 12345 for s in range(nseg)], [(nseg - 1 - s) * (7 << 30) + 999 for s in range(nseg)]


def local_rowids(rng, lens, mode, top_seg=None):
    """K per segment.  TAGGED / GLOBAL16: a permutation of 0 .. len - 1 in every segment (top_seg: that segment's largest becomes
    2^32 - 1).  PLAIN (the rowIDs ARE the global ones): slices of one permutation of 0 .. m - 1, its largest 2^32 - 1."""
    if mode == SHARD_PLAIN:
        k = rng.permutation(sum(lens)).astype(np.uint32)
        if len(k) > 1:
            k[np.argmax(k)] = TOP32
        return np.split(k, np.cumsum(lens)[:-1])
    ks = [rng.permutation(n).astype(np.uint32) for n in lens]
    if top_seg is not None:
        ks[top_seg][np.argmax(ks[top_seg])] = TOP32
    return ks


def join_values(rng, mR, mS):
    """random 64-bit h, each on about two rows per side; S drawn from R's values, every 53rd matching nothing"""
    vals = rng.integers(0, 1 << 64, max(mR // 2, 1), dtype=U64)
    hR, hS = vals[rng.integers(0, len(vals), mR)], vals[rng.integers(0, len(vals), mS)]
    hS[52::53] ^= U64(1 << 45)
    return hR, hS


def segments(h, ks):
    return [(p, k) for p, k in zip(np.split(h, np.cumsum([len(k) for k in ks])[:-1]), ks)]


def units_per_seg(nseg):
    """pass-1 units per sender segment, partition_relation_fused (segmented branch, radixhashjoin_amd/csrc/rhj_api.hip):
    groups_per_seg = max(16 / nseg, 1), ngroups = groups_per_seg * nseg, per = max(1024 / ngroups, 1), units_per_seg =
    groups_per_seg * per; a segment's unit is L = round_up(ceil(len / units_per_seg), 4096) tuples long"""
    groups_per_seg = max(16 // nseg, 1)
    ngroups = groups_per_seg * nseg
    per = max(1024 // ngroups, 1)
    return groups_per_seg * per


SHORT = [0, 1, 4095, 4096, 4097, 12_345]


def rotation(nseg):
    """the segment lengths of R and of S (R's rotated by three: a sender that sent nothing of R sent a full segment of S); the
    two lengths around units_per_seg * 4096 -- L goes from one tile to two -- from 6 senders on (they stay below 700 K there)"""
    ups = units_per_seg(nseg)
    pool = SHORT + ([ups * 4096, ups * 4096 + 1] if nseg >= 6 else [])
    return [pool[s % len(pool)] for s in range(nseg)], [pool[(s + 3) % len(pool)] for s in range(nseg)], pool


def run_lengths(eng, oracle, nseg, lensR, lensS, plan, mode, seed):
    rng = np.random.default_rng(seed)
    row0R, row0S = bases(nseg, mode)
    hR, hS = join_values(rng, sum(lensR), sum(lensS))
    segsR, segsS = segments(hR, local_rowids(rng, lensR, mode)), segments(hS, local_rowids(rng, lensS, mode))
    allow_one_table(eng, sum(lensR), sum(lensS), plan, mode)
    e, (offR, offS) = check_both_orders(eng, oracle, segsR, row0R, segsS, row0S, plan, mode, BKT)
    assert np.diff(offR).tolist() == list(lensR) and np.diff(offS).tolist() == list(lensS)      # the lengths meant are the lengths run
    return e


# ---------------------------------------------------------------------------------------------------------------------------
# A: receiver segment geometry (gaps 1, 2, 3)
# ---------------------------------------------------------------------------------------------------------------------------
GEOMETRY = ([(n, m, P88) for n in (6, 7, 11, 13, 16) for m in MODES] + [(n, SHARD_TAGGED, P44) for n in (7, 16)] +
            [(16, SHARD_PLAIN, P89)])


@pytest.mark.parametrize("nseg,mode,plan", GEOMETRY, ids=[f"{n}-{MODE_NAME[m]}-{PLAN_NAME[id(p)]}" for n, m, p in GEOMETRY])
def test_segment_geometry_many_senders(eng, oracle, nseg, mode, plan):
    """6 and 7 senders (12 and 14 unit groups), 11, 13 and 16 (one group each, tags up to 15), every segment length of the
    rotation, different for R and S; under 4+4 bits the 16-sender case is joined by the one-table kernel in several chunks"""
    lensR, lensS, pool = rotation(nseg)
    assert set(lensR) | set(lensS) == set(pool) and lensR != lensS
    ups = units_per_seg(nseg)
    assert ups * 4096 + 1 in lensR + lensS and ups * 4096 + 1 <= 696_321
    e = run_lengths(eng, oracle, nseg, lensR, lensS, plan, mode, 1000 * nseg + mode)
    assert len(e) > sum(lensS)
    if mode != SHARD_PLAIN:
        assert e[:, 0].max() >= 1 << 32 and e[:, 1].max() >= 1 << 32         # the receiver really had to restore wide rowIDs
        assert not np.array_equal(e[:, 0], e[:, 1])


# (lengths of R's segments, lengths of S's): whole sides of 1, 63 and 1023 tuples (below NARROW_MIN_TUPLES = 1024, which
# rhj_shard_partition does not exclude), an empty side, the lengths around the tile
FEW = {
    1: [([1], [4097]), ([63], [4095]), ([1023], [12_345]), ([0], [4096]), ([4096], [4097]), ([12_345], [1]), ([4097], [0])],
    2: [([0, 1], [4096, 0]), ([63, 0], [4095, 4097]), ([1000, 23], [1, 12_345]), ([0, 0], [4096, 4097]), ([4095, 4096], [4097, 0]),
        ([12_345, 4097], [0, 4095]), ([4096, 1], [0, 0])],
}
FEW_CASES = ([(n, m, P88, c) for n in (1, 2) for m in MODES for c in range(len(FEW[n]))] +
             [(1, SHARD_TAGGED, P44, c) for c in range(len(FEW[1]))] + [(2, SHARD_PLAIN, P89, c) for c in range(len(FEW[2]))])


@pytest.mark.parametrize("nseg,mode,plan,case", FEW_CASES,
                         ids=[f"{n}-{MODE_NAME[m]}-{PLAN_NAME[id(p)]}-{'+'.join(map(str, FEW[n][c][0]))}x{'+'.join(map(str, FEW[n][c][1]))}"
                              for n, m, p, c in FEW_CASES])
def test_segment_geometry_one_and_two_senders(eng, oracle, nseg, mode, plan, case):
    """one sender (16 unit groups of one segment) and two, with a checked pair set: short segments, tiny and empty sides"""
    lensR, lensS = FEW[nseg][case]
    if not (sum(lensR) and sum(lensS)):                                      # an empty side reports no kernel whatever ran before:
        run_lengths(eng, oracle, nseg, [4097] * nseg, [4096] * nseg, plan, mode, 5)     # let one have run
    e = run_lengths(eng, oracle, nseg, lensR, lensS, plan, mode, 100 * nseg + 10 * mode + case)
    assert (len(e) > 0) == (sum(lensR) > 0 and sum(lensS) > 0)


@pytest.mark.parametrize("mode", MODES, ids=[MODE_NAME[m] for m in MODES])
def test_extreme_bases_and_local_rowids(eng, oracle, mode):
    """a sender with row0 = 2^64 - 2^32 that holds local rowID 2^32 - 1 (the global rowID 2^64 - 1 must come back) and one with
    row0 = 0 that holds local rowID 0, other senders for R than for S; PLAIN: the rowIDs 0 and 2^32 - 1 themselves"""
    rng = np.random.default_rng(40 + mode)
    lensR, lensS = [4097, 12_345, 4096], [12_345, 4096, 4097]
    if mode == SHARD_PLAIN:
        row0R, row0S, topR, topS = [0, 0, 0], [0, 0, 0], None, None
        top = TOP32
    else:
        row0R, row0S, topR, topS = [(1 << 64) - (1 << 32), 0, 2 * (5 << 30) + 12345], [7 << 30, (1 << 64) - (1 << 32), 0], 0, 1
        top = (1 << 64) - 1
    hR, hS = join_values(rng, sum(lensR), sum(lensS))
    kR, kS = local_rowids(rng, lensR, mode, topR), local_rowids(rng, lensS, mode, topS)
    gR = np.concatenate([k.astype(U64) + U64(b) for k, b in zip(kR, row0R)])
    gS = np.concatenate([k.astype(U64) + U64(b) for k, b in zip(kS, row0S)])
    for g in (top, 0):                                                       # the extreme rows of R and S are partners
        (iR,), (iS,) = np.flatnonzero(gR == U64(g)), np.flatnonzero(gS == U64(g))
        hS[iS] = hR[iR]
    e, _ = check_both_orders(eng, oracle, segments(hR, kR), row0R, segments(hS, kS), row0S, P88, mode, BKT)
    for g in (top, 0):
        assert np.any((e[:, 0] == U64(g)) & (e[:, 1] == U64(g)))


# ---------------------------------------------------------------------------------------------------------------------------
# B: the value families through the receiver instantiations (gap 4)
# ---------------------------------------------------------------------------------------------------------------------------
# (mode, kernel, plan, "join.big_tables", "join.big_kernel"); the families hold 20 K build tuples in two partitions, so every
# one-table row -- the TAGGED ones among them -- meets build sides of several table chunks
RECEIVERS = [
    (SHARD_TAGGED, BKT, P44, -1, -1),
    (SHARD_TAGGED, BKT, P88, -1, -1),
    (SHARD_GLOBAL16, BKT, P66, -1, -1),
    (SHARD_GLOBAL16, CT, P88, 1, CT),
    (SHARD_GLOBAL16, CT_HALF, P88, 1, CT_HALF),
    (SHARD_GLOBAL16, CT_MID, P88, 1, CT_MID),
    (SHARD_PLAIN, BKT, P88, -1, -1),
    (SHARD_PLAIN, CT, P88, 1, CT),
    (SHARD_PLAIN, CT_20, P88, 1, CT_20),                  # the narrow-only 20-slot geometry
    (SHARD_PLAIN, CT, P89, 1, CT),
]
RECEIVER_IDS = [f"{MODE_NAME[m]}-k{k}-{PLAN_NAME[id(p)]}" for m, k, p, _, _ in RECEIVERS]


def family_values(fam, rb, rng=None, extra=0):
    """(h of R, h of S) in mixed space -- what the wire carries; the raw-payload part of `extreme` goes through mix64"""
    b, p = family(fam, rb)
    if fam == "extreme":
        b, p = np.concatenate([b[0], mix64(b[1])]), np.concatenate([p[0], mix64(p[1])])
    if extra:
        p = np.concatenate([p, b[rng.integers(0, len(b), extra)]])           # probe duplicates: several pairs per build tuple
    return b.copy(), p.copy()


def deal(rng, h, nseg, mode):
    """the tuples dealt to nseg senders at random"""
    sender = rng.integers(0, nseg, len(h))
    order = np.argsort(sender, kind="stable")
    lens = np.bincount(sender, minlength=nseg).tolist()
    return segments(h[order], local_rowids(rng, lens, mode))


@pytest.mark.parametrize("mode,kernel,plan,big_tables,big_kernel", RECEIVERS, ids=RECEIVER_IDS)
@pytest.mark.parametrize("nseg", [3, 16])
@pytest.mark.parametrize("fam", ["near_miss", "fold", "extreme"])
def test_value_families_through_receivers(eng, oracle, fam, nseg, mode, kernel, plan, big_tables, big_kernel):
    rng = np.random.default_rng(sum(map(ord, fam)) * 7 + nseg + 100 * mode + kernel)
    hR, hS = family_values(fam, radix_bits(plan))
    eng.set_option("join.big_tables", big_tables)
    eng.set_option("join.big_kernel", big_kernel)
    row0R, row0S = bases(nseg, mode)
    e, _ = check_both_orders(eng, oracle, deal(rng, hR, nseg, mode), row0R, deal(rng, hS, nseg, mode), row0S, plan, mode, kernel)
    assert len(e) > 10_000


# ---------------------------------------------------------------------------------------------------------------------------
# C: rhj_shard_join's output bound (gap 5)
# ---------------------------------------------------------------------------------------------------------------------------
CANARY = U64(0xC5C5A5A55A5A3C3C)


def shard_join_status(eng, d_out, capacity):
    n = C.c_uint64(0)
    rc = eng.lib.rhj_shard_join(eng.ctx, _addr(d_out), capacity, C.byref(n))
    return rc, n.value


@pytest.mark.parametrize("mode,kernel,plan,big_tables,big_kernel", [RECEIVERS[1], RECEIVERS[3], RECEIVERS[8]],
                         ids=[RECEIVER_IDS[1], RECEIVER_IDS[3], RECEIVER_IDS[8]])
def test_shard_join_output_bound(eng, oracle, mode, kernel, plan, big_tables, big_kernel):
    """capacity 1, n // 2 and n - 1 into a buffer of n + 256 slots filled with a canary: RHJ_E_OVERFLOW with the exact count, every
    slot from `capacity` on untouched, every slot below it a distinct pair of the result (two 64-bit columns: the rowIDs exceed
    32 bits); then, on the SAME partitions, count-only and the exact capacity give the oracle's pairs, the guard intact"""
    nseg = 3
    rng = np.random.default_rng(50 + mode)
    hR, hS = family_values("near_miss", radix_bits(plan), rng, extra=3000)
    eng.set_option("join.big_tables", big_tables)
    eng.set_option("join.big_kernel", big_kernel)
    row0R, row0S = bases(nseg, mode)
    segsR, segsS = deal(rng, hR, nseg, mode), deal(rng, hS, nseg, mode)
    e = expected_pairs(oracle, global_rel(segsR, row0R), global_rel(segsS, row0S))
    n = len(e)
    assert n > 600
    genuine = set(map(tuple, e.tolist()))
    assert len(genuine) == n
    partition_sides(eng, segsR, row0R, segsS, row0S, plan, mode)
    canary = np.empty((n + 256, 2), dtype=U64)
    canary[:, 0], canary[:, 1] = CANARY, ~CANARY
    d_out = eng.alloc(16 * (n + 256))

    def run(cap, d=d_out):
        eng._chk(eng.lib.rhj_copy_h2d(eng.ctx, d_out.ptr, canary.ctypes.data, canary.nbytes))
        rc, cnt = shard_join_status(eng, d, cap)
        assert eng.info("last.join_kernel") == kernel
        out = d_out.to_numpy(U64, 2 * (n + 256)).reshape(-1, 2)
        assert np.array_equal(out[cap:], canary[cap:]), f"a pair past capacity {cap}"
        return rc, cnt, out[:cap]

    for cap in (1, n // 2, n - 1):
        rc, cnt, out = run(cap)
        assert (rc, cnt) == (RHJ_E_OVERFLOW, n), (cap, rc, cnt)
        got = set(map(tuple, out.tolist()))
        assert len(got) == cap, f"holes or repeated pairs below capacity {cap}"
        assert got <= genuine, f"a slot below capacity {cap} is not a pair of the result"
    rc, cnt, _ = run(0, None)                                                # count only
    assert (rc, cnt) == (RHJ_OK, n)
    rc, cnt, out = run(n)
    assert (rc, cnt) == (RHJ_OK, n)
    assert np.array_equal(sort2(out), e)
    d_out.free()


# ---------------------------------------------------------------------------------------------------------------------------
# D: the sender calls against numpy (gap 6)
# ---------------------------------------------------------------------------------------------------------------------------
K_CANARY = np.uint32(0xA5A53C3C)


def shard(rng, n, key0=5 << 30, step=3):
    """random 64-bit payloads, one value on 5 % of the rows; rowIDs with gaps, beyond 2^32"""
    t = np.empty(n, dtype=TUPLE)
    t["payload"] = rng.integers(0, 1 << 64, n, dtype=U64)
    t["payload"][rng.random(n) < 0.05] = U64(0xDEADBEEF12345678)
    t["key"] = rng.permutation(n).astype(U64) * U64(step) + U64(key0)
    return t


def classes_of(P, shift, bits):
    return ((P >> U64(shift)) & U64((1 << bits) - 1)).astype(np.int64)


def assert_class_split(P, K, hist, t, key_base, shift, bits):
    """P / K: what arrived, classes in order, hist[c] tuples each; per class the multiset {mix64(payload), rowID - key_base}"""
    eP, eK = mix64(t["payload"]), (t["key"] - U64(key_base))
    assert len(eK) == 0 or int(eK.max()) <= TOP32
    where = np.repeat(np.arange(1 << bits), hist)                             # the class every position belongs to
    assert np.array_equal(classes_of(P, shift, bits), where)
    g = np.lexsort((K, P, where))
    x = np.lexsort((eK, eP, classes_of(eP, shift, bits)))
    assert np.array_equal(P[g], eP[x]) and np.array_equal(K[g].astype(U64), eK[x])


def split_to_buffer(eng, side, d, t, shift, bits, key_base):
    """rhj_shard_split of the relation the last rhj_shard_stats of this side saw: (P, K, class starts)"""
    n, nb = len(t), 1 << bits
    buf, starts = eng.alloc(max(narrow_bytes(n), 16)), eng.alloc(8 * (nb + 1))
    eng.shard_split(side, d, n, shift, bits, key_base, buf, starts)
    raw = buf.to_numpy(np.uint8, narrow_bytes(n))
    P = raw[:8 * n].view(U64).copy()
    K = raw[narrow_key_offset(n):narrow_key_offset(n) + 4 * n].view(np.uint32).copy()
    st = starts.to_numpy(U64, nb + 1)
    buf.free(); starts.free()
    return P, K, st


def split_to_peers(eng, side, d, t, shift, bits, key_base, hist, expect_refusal=False):
    """rhj_shard_split_peer into two local buffers standing in for two peers: even classes to peer 0, odd ones to peer 1, gaps
    between the classes; every element outside the ranges written keeps its canary.  Returns (P, K) in class order."""
    n, nb = len(t), 1 << bits
    owner = (np.arange(nb) & 1).astype(np.uint8)
    dst, at = np.zeros(nb, dtype=U64), [5, 9]
    for c in range(nb):
        dst[c] = at[owner[c]]
        at[owner[c]] += int(hist[c]) + 3
    size = [a + 7 for a in at]
    dP = [eng.to_device(np.full(s, CANARY, dtype=U64)) for s in size]
    dK = [eng.to_device(np.full(s, K_CANARY, dtype=np.uint32)) for s in size]
    try:
        eng.shard_split_peer(side, d, n, shift, bits, key_base, owner, dst, dP, dK)
        eng.sync()
    finally:
        gotP, gotK = [b.to_numpy(U64, s) for b, s in zip(dP, size)], [b.to_numpy(np.uint32, s) for b, s in zip(dK, size)]
        for b in dP + dK:
            b.free()
        if expect_refusal:                                                   # nothing was launched: nothing was written
            assert all(np.all(p == CANARY) for p in gotP) and all(np.all(k == K_CANARY) for k in gotK)
    written = [np.zeros(s, dtype=bool) for s in size]
    Ps, Ks = [], []
    for c in range(nb):
        o, a, b = int(owner[c]), int(dst[c]), int(dst[c]) + int(hist[c])
        written[o][a:b] = True
        Ps.append(gotP[o][a:b]); Ks.append(gotK[o][a:b])
    for o in (0, 1):
        assert np.all(gotP[o][~written[o]] == CANARY) and np.all(gotK[o][~written[o]] == K_CANARY), "a store outside the classes' ranges"
    return np.concatenate(Ps), np.concatenate(Ks)


def check_sender_calls(eng, side, t, shift, bits, key_base=None):
    n, nb = len(t), 1 << bits
    d = eng.to_device(t)
    hist, kmin, kmax = eng.shard_stats(side, d, n, shift, bits)
    assert np.array_equal(hist, np.bincount(classes_of(mix64(t["payload"]), shift, bits), minlength=nb))
    assert (kmin, kmax) == ((int(t["key"].min()), int(t["key"].max())) if n else (0, 0))
    base = kmin if key_base is None else key_base
    P, K, st = split_to_buffer(eng, side, d, t, shift, bits, base)
    assert np.array_equal(st, np.concatenate([[0], np.cumsum(hist)]).astype(U64))
    assert_class_split(P, K, hist, t, base, shift, bits)
    P2, K2 = split_to_peers(eng, side, d, t, shift, bits, base, hist)
    assert_class_split(P2, K2, hist, t, base, shift, bits)
    d.free()
    return K


@pytest.mark.parametrize("shift,bits", [(20, 8), (16, 1), (29, 3), (56, 8), (60, 4)])
@pytest.mark.parametrize("n", [0, 1, 4095, 4096, 4097, 100_003])
def test_sender_calls_equal_numpy(eng, n, shift, bits):
    """rhj_shard_stats, rhj_shard_split and rhj_shard_split_peer on an empty shard, one tuple, the sizes around one tile and several
    units; 1, 3, 4 and 8 class bits, at the top of the word too"""
    rng = np.random.default_rng(n + 64 * shift + bits)
    for side in (0, 1):
        check_sender_calls(eng, side, shard(rng, n), shift, bits)


def test_rowid_span_limit(eng):
    """max - min of exactly 2^32 - 1 is accepted with key_base = min, and K reaches 0xFFFFFFFF; one rowID one higher is refused by
    both split calls (RHJ_E_INVALID), which then launch nothing"""
    rng = np.random.default_rng(9)
    t = shard(rng, 5000)
    lo = 3 << 33
    t["key"] = np.concatenate([[0, TOP32], 1 + rng.choice(TOP32 - 1, len(t) - 2, replace=False)]).astype(U64) + U64(lo)
    K = check_sender_calls(eng, 0, t, 20, 8)
    assert int(K.max()) == TOP32 and int(K.min()) == 0
    t["key"][1] += U64(1)                                                    # span 2^32
    d = eng.to_device(t)
    hist, kmin, kmax = eng.shard_stats(0, d, len(t), 20, 8)
    assert kmax - kmin == 1 << 32
    buf = eng.to_device(np.full(narrow_bytes(len(t)) // 8, CANARY, dtype=U64))
    with pytest.raises(RhjError) as err:
        eng.shard_split(0, d, len(t), 20, 8, kmin, buf)
    assert err.value.code == RHJ_E_INVALID
    eng.sync()
    assert np.all(buf.to_numpy(U64, narrow_bytes(len(t)) // 8) == CANARY)
    with pytest.raises(RhjError) as err:
        split_to_peers(eng, 0, d, t, 20, 8, kmin, hist, expect_refusal=True)
    assert err.value.code == RHJ_E_INVALID
    d.free(); buf.free()


@pytest.mark.parametrize("below", [None, 7])
def test_key_base_below_the_smallest_rowid(eng, below):
    """key_base = 0 and key_base = min - 7 on a shard with small rowIDs: K = rowID - key_base"""
    rng = np.random.default_rng(3)
    t = shard(rng, 30_000, key0=1000, step=1)
    K = check_sender_calls(eng, 1, t, 29, 3, key_base=0 if below is None else 1000 - below)
    assert int(K.min()) == (1000 if below is None else below)
