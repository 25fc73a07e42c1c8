"""GPU suite: adversarial join values, rowIDs and output bounds for every join kernel.

Every bucket-join kernel stores a PART of the mixed join value h = rhj_mix64(payload): inside a partition of a plan of rb radix
bits the compact-table kernels keep key = h >> rb in an entry {key << KB | arrival index} (KB = 16, 13 or 12) and compare it as
two 32-bit words that meet at key bit 32 - KB; the one-table and compact-table kernels find a bucket by folding the key,
(u32)key ^ (u32)(key >> 32), and hashing the fold.  The values below are built in that mixed space (unmix64 turns them into
payloads; with "partition.mix" 0, and for the unpartitioned direct join, which compares the caller's payloads as they are, they
are the payloads) so that they sit exactly where such a kernel can go wrong:

    a. near misses     h ^ (1 << b) for every b in 0..63, and probes that share a build value's bucket in every geometry while
                       differing from it only in the low compare word, only in the high one, or only in h's upper 32 bits
    b. fold collisions thousands of DISTINCT keys x ^ (d * 0x100000001) in one bucket, with duplicates
    c. extreme values  payloads 0, 1, 2^32 - 1, 2^32, 2^63, 2^64 - 1; mixed values 0 and all ones; keys of all ones and zero
    d. extreme rowIDs  0, 2^32 - 1, 2^32, 2^63, 2^64 - 1 on either side, with the build side on S and on R

They run through every path (the direct one-launch join, the one-table kernel under a one- and a two-pass plan, the chunked
kernel, and the compact-table geometries 2-11 under plans they accept) in every partition format, and every case asserts the
kernel and format that ran (include/rhj.h: "last.join_kernel", "last.narrow").  Expected pairs come from the CPU oracle.
The output-bound contract of rhj_join_dev (RHJ_E_OVERFLOW) is checked on each path against a canary guard behind the
capacity, and rhj_join_batch at its own boundaries (16 joins per launch, the direct-path limits)."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle.pyoracle import PAIR, TUPLE, sorted_pairs
from radixhashjoin_amd import Engine, Opts
from radixhashjoin_amd.binding import RHJ_E_OVERFLOW, RHJ_OK, _addr, unmix64

pytestmark = pytest.mark.gpu

U64 = np.uint64
M32 = U64(0xFFFFFFFF)
FOLD = U64(0x100000001)                    # d * FOLD: equal 32-bit halves, so x ^ (d * FOLD) folds like x
DIRECT_MAX_BUILD, DIRECT_MAX_PROBE = 12 * 4224, 131072

# name -> (kernel forced, plan, "join.big_tables", "join.big_kernel", build tuples per table).  What runs, as every case asserts
# (Forced.assert_ran), for test IDs "<path>-narrow<level asked>":
#   kernel -1 (direct), 1 (chunked), 0 under the one-pass plan: 16-byte tuples, whatever level is asked
#   kernel 0 under the two-pass plan, kernels 2, 3, 6-11: the level asked (1 under the fused 8+8 plan)
#   kernels 4 / 5: the level asked, 1 or 2; asked for 0 they run as kernels 8 / 3
#   any kernel: 16-byte tuples for a join with a rowID >= 2^32 (test_extreme_rowids)
PATHS = {
    "direct": (-1, Opts(0), -1, -1, 4224),
    "one_table_1pass": (0, Opts(1, 7), 0, -1, 4224),
    "one_table_2pass": (0, Opts(2, 8, 8), 0, -1, 4224),
    "chunked": (1, Opts(2, 8, 8), 1, 1, 8448),
    "ct": (2, Opts(2, 8, 8), 1, 2, 16352),
    "ct_half": (3, Opts(2, 8, 8), 1, 3, 8160),
    "ct_20slots": (4, Opts(2, 8, 8), 1, 4, 17920),
    "ct_half_20slots": (5, Opts(2, 8, 8), 1, 5, 8960),
    "ct_mid": (6, Opts(2, 8, 8), 1, 6, 12288),
    "ct_half_mid": (7, Opts(2, 8, 8), 1, 7, 6144),
    "ct_8192_buckets": (8, Opts(2, 8, 8), 1, 8, 17920),
    "ct_half_mid_guards": (9, Opts(2, 8, 8), 1, 9, 6144),
    "ct_13bit_index_13bits": (10, Opts(2, 7, 6), 1, 10, 6144),
    "ct_13bit_index_15bits": (10, Opts(2, 8, 7), 1, 10, 6144),
    "ct_12bit_index": (11, Opts(2, 6, 6), 1, 11, 4096),
}
FUSED_8_8 = Opts(2, 8, 8)


def radix_bits(plan):
    return plan.bits1 + plan.bits2 if plan.passes == 2 else plan.bits1 if plan.passes == 1 else 0


def matrix():
    """(path, narrow level asked for): 0 and 2 under the path's own plan, 1 under the fused 8+8 plan (once per kernel)"""
    out, seen1 = [], set()
    for name, (kind, plan, *_rest) in PATHS.items():
        out += [(name, 0), (name, 2)]
        if plan.passes == 2 and kind not in seen1:
            seen1.add(kind)
            out.append((name, 1))
    return out


MATRIX = matrix()
MATRIX_IDS = [f"{p}-narrow{n}" for p, n in MATRIX]


@pytest.fixture(scope="module")
def engines():
    """one context per path (forced options are set per case and reset in a finally block)"""
    es = {}
    yield lambda name: es.setdefault(name, Engine(0))
    for e in es.values():
        e.close()


class Forced:
    """the options of one path on a context, reset to the defaults on exit"""

    def __init__(self, eng, name, narrow, mix=1):
        self.eng, self.name, self.narrow, self.mix = eng, name, narrow, mix
        self.kind, plan, self.big_tables, self.big_kernel, self.table = PATHS[name]
        self.plan = FUSED_8_8 if narrow == 1 and plan.passes == 2 else plan
        self.rb = radix_bits(self.plan)

    def __enter__(self):
        e = self.eng
        e.set_option("join.big_tables", self.big_tables)
        e.set_option("join.big_kernel", self.big_kernel)
        e.set_option("partition.narrow", self.narrow)
        e.set_option("partition.mix", self.mix)
        return self

    def __exit__(self, *exc):
        for k in ("join.big_tables", "join.big_kernel", "partition.narrow", "partition.mix"):
            self.eng.set_option(k, -1)
        return False

    def rearm(self):
        self.eng.set_option("partition.narrow", self.narrow)      # (a wide rowID turns it off for the join that met it)

    def expected_narrow(self, R, S):
        """the format the join must have run in: the requested level under a fused plan (both passes <= 8 bits) whose bucket join
        reads narrow partitions (not the chunked kernel), for inputs of >= 1024 tuples per side whose rowIDs all fit 32 bits"""
        p = self.plan
        fused = p.passes == 2 and 1 <= p.bits1 <= 8 and 1 <= p.bits2 <= 8 and p.bits1 + p.bits2 <= 16
        wide = any(len(t) and int(t["key"].max()) >= 1 << 32 for t in (R, S))
        ok = fused and self.kind != 1 and min(len(R), len(S)) >= 1024 and not wide
        return self.narrow if ok and self.narrow > 0 else 0

    def expected_kernel(self, narrow_ran):
        # the 20-slot geometries read narrow partitions only: 16-byte tuples take kernels 8 / 3 (include/rhj.h "join.big_kernel")
        if narrow_ran == 0 and self.kind in (4, 5):
            return {4: 8, 5: 3}[self.kind]
        return self.kind

    def assert_ran(self, R, S):
        nar = self.expected_narrow(R, S)
        assert self.eng.info("last.narrow") == nar, (self.name, self.narrow)
        assert self.eng.info("last.join_kernel") == self.expected_kernel(nar), self.name
        self.rearm()

    def payloads(self, h):
        # (the direct join partitions nothing and compares the caller's payloads: the values are crafted for it as they are)
        return unmix64(h) if self.mix and self.kind != -1 else np.asarray(h, dtype=U64)


# ---------------------------------------------------------------------------------------------------------------------------
# value families, in mixed space
# ---------------------------------------------------------------------------------------------------------------------------
def bucket14(key):
    """top 14 bits of the Fibonacci hash of the folded key: bj_bucket / ct_bucket of every geometry (11-14 bucket bits) take the
    top BBITS bits of this same product, so keys that agree here share a bucket in all of them"""
    key = np.asarray(key, dtype=U64)
    f = (key & M32) ^ (key >> U64(32))
    with np.errstate(over="ignore"):
        return ((f * U64(0x9E3779B1)) & M32) >> U64(18)


def rand_keys(rng, n, rb):
    """n distinct keys < 2^(64 - rb), random in all their bits"""
    k = np.unique(rng.integers(0, 1 << 63, 2 * n + 64, dtype=U64) * U64(2) + rng.integers(0, 2, 2 * n + 64, dtype=U64))
    k = rng.permutation(k >> U64(rb))[:n]
    assert len(np.unique(k)) == n
    return k


def lows(rb, nlow, seed=1):
    """nlow partition patterns of rb bits (one for an unpartitioned plan)"""
    if rb == 0:
        return np.zeros(1, dtype=U64)
    return np.random.default_rng(seed).permutation(min(1 << rb, 1 << 16))[:nlow].astype(U64)


def place(keys, rb, pats):
    """h = key << rb | the partition pattern chosen by the key: few, large partitions"""
    keys = np.asarray(keys, dtype=U64)
    if rb == 0:
        return keys
    return (keys << U64(rb)) | pats[(keys % U64(len(pats))).astype(np.int64)]


def same_bucket_near_misses(rng, h, rb, per=2):
    """for every h: up to `per` values h ^ d per window, d confined to one window of bits of h above the radix bits, with the
    SAME bucket in every geometry -- values that only a correct key compare tells apart.  Windows: h bits [rb, rb + 16) (the low
    compare word of every compact-table geometry), [rb + 20, 64) (its high word), [max(32, rb), 64) (h's upper 32 bits)."""
    out = []
    for lo, hi in ((rb, rb + 16), (rb + 20, 64), (max(32, rb), 64)):
        width = hi - lo
        cand = np.arange(1, 1 << width, dtype=U64) if width <= 16 else rng.integers(1, 1 << width, 1 << 16, dtype=U64)
        cand = cand << U64(lo)
        ck = cand >> U64(rb)
        for x in h:
            k = x >> U64(rb)
            hit = ck[bucket14(k ^ ck) == bucket14(k)][:per]
            out.append(x ^ (hit << U64(rb)))
    out = np.concatenate(out)
    assert len(out) >= len(h), "the search found too few same-bucket values"
    return out


def rel(rng, vals, key0=0):
    t = np.empty(len(vals), dtype=TUPLE)
    t["key"] = rng.permutation(len(vals)).astype(U64) + U64(key0)
    t["payload"] = vals
    return t


@functools.lru_cache(maxsize=None)
def family(name, rb, nbuild=20_000, nlow=2, seed=0):
    """(build h, probe h) of a value family for plans of rb radix bits (the build side is the smaller)"""
    rng = np.random.default_rng(seed * 1000 + rb * 7 + len(name))
    pats = lows(rb, nlow, seed + 1)
    if name == "near_miss":
        base = place(rand_keys(rng, nbuild, rb), rb, pats)
        flips = base[:360, None] ^ (U64(1) << np.arange(64, dtype=U64))[None, :]        # every bit of 360 build values
        flipped = flips.ravel()
        bucket = same_bucket_near_misses(rng, base[360:460], rb)
        # some near misses ARE build values (flips above the radix bits: the build side stays in the base values' partitions)
        on_build = np.concatenate([flips[:, rb:].ravel()[5::97], bucket[3::11]])
        build = np.concatenate([base[:nbuild - len(on_build)], on_build])
        probe = np.concatenate([flipped, bucket, base[rng.integers(0, nbuild, nbuild // 2)]])
    elif name == "fold":
        nd = 1200                                                                        # distinct keys per folded bucket
        dmax = 1 << min(32, 32 - rb) if rb < 32 else 1
        groups = []
        for x0 in rand_keys(rng, 3, rb):
            d = rng.choice(np.arange(1, min(dmax, 1 << 20), dtype=U64), nd, replace=False)
            g = np.concatenate([[x0], x0 ^ (d * FOLD)])
            assert rb == 0 or int(g.max()) < 1 << (64 - rb)
            assert len(np.unique(g)) == len(g) and len(np.unique(bucket14(g))) == 1
            groups.append(g)
        # one partition pattern for all three groups: their buckets become one long bucket per group inside ONE partition
        pat = pats[:1]
        keys = [place(g, rb, pat) for g in groups]
        build_k = np.concatenate([k[: 2 * len(k) // 3] for k in keys])                 # two thirds of each bucket on the build side
        dups = np.repeat(build_k[::50], 3)                                               # ... some of them four times
        filler = place(rand_keys(rng, nbuild - len(build_k) - len(dups), rb), rb, pat)   # unrelated keys, same partition
        build = np.concatenate([build_k, dups, filler])
        probe = np.concatenate([np.concatenate(keys),                                    # equal to some keys, fold-colliding with the rest
                                build_k[rng.integers(0, len(build_k), 4000)], filler, filler[:4000]])
    elif name == "extreme":
        ones = ~U64(0)
        pay = np.array([0, 1, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1], dtype=U64)
        kmax = (ones >> U64(rb)) if rb else ones                                         # key = h >> rb of all ones
        special = np.concatenate([[U64(0), ones], place(np.array([kmax, kmax ^ U64(1), U64(0), U64(1)], dtype=U64), rb, pats),
                                  place(kmax ^ (U64(1) << np.arange(64 - rb, dtype=U64)), rb, pats)[::5],
                                  place(U64(1) << np.arange(64 - rb, dtype=U64), rb, pats)[::3]])
        filler = place(rand_keys(rng, nbuild, rb), rb, pats)
        # (build h, payloads) and (probe h, payloads): the second array holds payloads as they are, never unmixed (see relations)
        build = (np.concatenate([np.repeat(special, 3), filler[: nbuild - 3 * len(special)]]), np.repeat(pay, 3))
        probe = (np.concatenate([np.repeat(special, 2), special ^ U64(1 << 40), filler[::2]]), np.repeat(pay, 2))
        return build, probe
    else:
        raise ValueError(name)
    return rng.permutation(build), rng.permutation(probe)


def relations(f, rng, fam, nbuild=20_000, nlow=2, seed=0):
    """R (build side, the smaller) and S of a family under the options f"""
    b, p = family(fam, f.rb, nbuild, nlow, seed)
    if fam == "extreme":
        bv = np.concatenate([f.payloads(b[0]), b[1]])                  # raw payloads 0, 1, 2^32 - 1, ... as they are
        pv = np.concatenate([f.payloads(p[0]), p[1]])
    else:
        bv, pv = f.payloads(b), f.payloads(p)
    return rel(rng, bv), rel(rng, pv, key0=1 << 31)


def check(f, oracle, R, S):
    got = f.eng.join(R, S, opts=f.plan)
    exp = oracle.join(R, S)
    assert len(got) == len(exp), (f.name, len(got), len(exp))
    assert np.array_equal(sorted_pairs(got), sorted_pairs(exp)), f.name
    f.assert_ran(R, S)
    return exp


# ---------------------------------------------------------------------------------------------------------------------------
# 1 + 2: the path matrix x the value families
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,narrow", MATRIX, ids=MATRIX_IDS)
@pytest.mark.parametrize("fam", ["near_miss", "fold", "extreme"])
def test_value_families(engines, oracle, path, narrow, fam):
    """each family in both roles (the build side R, then S: pairs stay (rowR,rowS)); near misses and fold collisions must not
    pair with anything but equal values"""
    with Forced(engines(path), path, narrow) as f:
        rng = np.random.default_rng(sum(map(ord, path + fam)) * 3 + narrow)
        R, S = relations(f, rng, fam)
        exp = check(f, oracle, R, S)
        assert len(exp) > 0
        check(f, oracle, S, R)


@pytest.mark.parametrize("path,narrow", [(p, n) for p, n in MATRIX if n != 1], ids=[i for i, (p, n) in zip(MATRIX_IDS, MATRIX) if n != 1])
def test_table_and_task_boundaries(engines, oracle, path, narrow):
    """near misses in ONE partition whose build side is exactly one table, then one tuple more (a second chunk of one tuple)"""
    with Forced(engines(path), path, narrow) as f:
        rng = np.random.default_rng(7)
        for nb in (f.table, f.table + 1):
            R, S = relations(f, rng, "near_miss", nbuild=nb, nlow=1, seed=1)
            check(f, oracle, R, S)


MIX0 = ["one_table_1pass", "one_table_2pass", "chunked", "ct", "ct_half_mid_guards", "ct_13bit_index_13bits", "ct_12bit_index"]


@pytest.mark.parametrize("path", MIX0)
@pytest.mark.parametrize("fam", ["near_miss", "fold", "extreme"])
def test_value_families_raw_radix_digits(engines, oracle, path, fam):
    """"partition.mix" 0: the same values as raw payloads (radix digits and keys taken from the payload itself)"""
    for narrow in (0, 2):
        with Forced(engines(path), path, narrow, mix=0) as f:
            rng = np.random.default_rng(3)
            R, S = relations(f, rng, fam)
            check(f, oracle, R, S)
            assert f.eng.info("partition.mix") == 0


EXTREME_ROWIDS = np.array([0, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1], dtype=U64)


@pytest.mark.parametrize("path,narrow", MATRIX, ids=MATRIX_IDS)
def test_extreme_rowids(engines, oracle, path, narrow):
    """rowIDs 0, 2^32 - 1, 2^32, 2^63, 2^64 - 1 on either side, build side R and S: 64-bit rowIDs come back intact, in (rowR,rowS)
    order; rowIDs up to 2^32 - 1 keep the narrow format, a larger one sends the join to 16-byte tuples"""
    with Forced(engines(path), path, narrow) as f:
        rng = np.random.default_rng(11)
        R0, S0 = relations(f, rng, "near_miss", nbuild=12_000)
        for side in ("R", "S"):
            for ids in (EXTREME_ROWIDS[:2], EXTREME_ROWIDS):                  # below 2^32 (narrow stays), then all of them
                R, S = R0.copy(), S0.copy()
                T, O = (R, S) if side == "R" else (S, R)
                T["key"] += U64(1)                                            # rowID 0 is free
                rows = rng.choice(len(T), len(ids), replace=False)
                T["key"][rows] = ids
                # the other side gets a partner for every extreme row (and an extreme rowID of its own, S role)
                part = rng.choice(len(O), len(ids), replace=False)
                O["payload"][part] = T["payload"][rows]
                for A, B in ((R, S), (S, R)):                                 # build side R, then S
                    exp = check(f, oracle, A, B)
                    kr = exp["keyR"] if A is T else exp["keyS"]
                    assert np.isin(ids, kr).all()                            # every extreme rowID is in some pair


# ---------------------------------------------------------------------------------------------------------------------------
# 3: the output-bound contract (rhj_join_dev, RHJ_E_OVERFLOW)
# ---------------------------------------------------------------------------------------------------------------------------
CANARY = U64(0xC5C5A5A55A5A3C3C)


def join_dev_status(eng, dR, nR, dS, nS, plan, d_out, capacity):
    n = C.c_uint64(0)
    rc = eng.lib.rhj_join_dev(eng.ctx, _addr(dR), nR, _addr(dS), nS, C.byref(plan), _addr(d_out), capacity, C.byref(n))
    return rc, n.value


def fill(eng, d_buf, host):
    eng._chk(eng.lib.rhj_copy_h2d(eng.ctx, d_buf.ptr, host.ctypes.data, host.nbytes))


def pair_codes(p):
    return (p["keyR"] << U64(32)) | p["keyS"]                                # (rowIDs below 2^32 in these inputs)


@pytest.mark.parametrize("path,narrow", MATRIX, ids=MATRIX_IDS)
def test_output_bound_contract(engines, oracle, path, narrow):
    """capacity 1, exact - 1 and a middle value into a buffer of exact + 256 slots filled with a canary: RHJ_E_OVERFLOW with the
    exact count, the guard (every slot from `capacity` on) untouched, every slot below `capacity` a distinct genuine pair
    (include/rhj.h: pairs beyond capacity are dropped, the first `capacity` slots hold pairs of the result); then count-only and
    the exact capacity on the same context give the oracle's answer"""
    with Forced(engines(path), path, narrow) as f:
        rng = np.random.default_rng(5)
        R, S = relations(f, rng, "near_miss", nbuild=12_000)
        S = np.concatenate([S, R[rng.integers(0, len(R), 3000)]])          # duplicates on the probe side too: several pairs per build tuple
        S["key"] = rng.permutation(len(S)).astype(U64) + U64(1 << 31)
        exp = oracle.join(R, S)
        n = len(exp)
        assert n > 600
        codes = np.sort(pair_codes(exp))
        assert len(np.unique(codes)) == n
        e = f.eng
        dR, dS, dO = e.to_device(R), e.to_device(S), e.alloc(16 * (n + 256))
        canary = np.zeros(n + 256, dtype=PAIR)
        canary["keyR"], canary["keyS"] = CANARY, ~CANARY
        for cap in (1, n // 2, n - 1):
            fill(e, dO, canary)
            rc, cnt = join_dev_status(e, dR, len(R), dS, len(S), f.plan, dO, cap)
            assert (rc, cnt) == (RHJ_E_OVERFLOW, n), (cap, rc, cnt)
            f.assert_ran(R, S)
            out = dO.to_numpy(PAIR, n + 256)
            guard = out[cap:]
            assert np.all(guard["keyR"] == CANARY) and np.all(guard["keyS"] == ~CANARY), f"a pair past capacity {cap}"
            got = pair_codes(out[:cap])
            assert len(np.unique(got)) == cap, f"holes or repeated pairs below capacity {cap}"
            assert np.isin(got, codes, assume_unique=True).all(), f"a slot below capacity {cap} is not a pair of the result"
        rc, cnt = join_dev_status(e, dR, len(R), dS, len(S), f.plan, None, 0)  # count only
        assert (rc, cnt) == (RHJ_OK, n)
        f.assert_ran(R, S)
        fill(e, dO, canary)
        rc, cnt = join_dev_status(e, dR, len(R), dS, len(S), f.plan, dO, n)
        assert (rc, cnt) == (RHJ_OK, n)
        f.assert_ran(R, S)
        out = dO.to_numpy(PAIR, n + 256)
        assert np.array_equal(np.sort(pair_codes(out[:n])), codes)
        assert np.all(out[n:]["keyR"] == CANARY) and np.all(out[n:]["keyS"] == ~CANARY)
        for b in (dR, dS, dO):
            b.free()


# ---------------------------------------------------------------------------------------------------------------------------
# 4: rhj_join_batch at its boundaries
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch_pool():
    """joins of families a-d at the batch path's boundaries: as raw payloads for the joins of the one-launch path (it compares them as
    they are), in mixed space under the automatic plan's radix bits for the joins beyond its limits (rhj_join partitions them)"""
    from radixhashjoin_amd.binding import plan
    rng = np.random.default_rng(2024)
    pool = []

    def mk(fam, nb, npb, wide=False):
        direct = nb <= DIRECT_MAX_BUILD and npb <= DIRECT_MAX_PROBE
        rb = 0 if direct else radix_bits(plan(nb, npb))
        b, p = family(fam, rb, max(nb, 4000), 1, 3)
        pay = (lambda h: h) if direct else unmix64
        if fam == "extreme":
            b, p = np.concatenate([pay(b[0]), b[1]]), np.concatenate([pay(p[0]), p[1]])
        else:
            b, p = pay(b), pay(p)
        bv = np.resize(b, nb)
        pv = np.resize(np.concatenate([p, b]), npb)
        R, S = rel(rng, bv), rel(rng, pv, key0=1 << 31)
        if wide:
            R["key"][: len(EXTREME_ROWIDS)] = EXTREME_ROWIDS[::-1]
            S["key"][-len(EXTREME_ROWIDS):] = EXTREME_ROWIDS
        return R, S

    pool.append(mk("near_miss", DIRECT_MAX_BUILD, DIRECT_MAX_PROBE))          # the direct path's limits, exactly
    pool.append(mk("fold", DIRECT_MAX_BUILD + 1, 90_000))                     # one build tuple beyond: rhj_join's own path
    pool.append(mk("near_miss", 30_000, DIRECT_MAX_PROBE + 1))                # one probe tuple beyond
    R, S = mk("extreme", 2_000, 5_000, wide=True)
    pool.append((S, R))                                                       # build side S, 64-bit rowIDs on both sides
    pool.append(mk("fold", 5_000, 9_000))
    pool.append((R[:0], S[:1000]))                                            # R empty
    pool.append((R[:1000], S[:0]))                                            # S empty
    pool.append((R[:0], S[:0]))                                               # both empty
    one = rel(rng, np.array([(1 << 63) | 12345], dtype=U64))
    pool.append((one, one.copy()))                                            # one tuple against one tuple: a pair
    miss = one.copy()
    miss["payload"] ^= U64(1 << 40)
    pool.append((one, miss))                                                  # ... and a near miss: none
    pool.append((rel(rng, np.full(250, 77, U64)), rel(rng, np.full(260, 77, U64))))   # 65000 pairs > 32 x the size guess (1284)
    pool.append(mk("near_miss", 3_000, 4_500, wide=True))
    return pool


@pytest.mark.parametrize("njoins", [1, 15, 16, 17, 32, 33, 48])
def test_join_batch_boundaries(engine, oracle, njoins):
    pool = batch_pool()
    joins = [pool[(i * 5 + njoins) % len(pool)] for i in range(njoins)]
    exp = {}
    for R, S in joins:
        k = id(R), id(S)
        if k not in exp:
            e = sorted_pairs(oracle.join(R, S))
            single = engine.join(R, S)
            assert np.array_equal(sorted_pairs(single), e)
            exp[k] = e
    for _ in range(2):                                                        # the same call again on the same context
        got = engine.join_batch(joins)
        assert len(got) == njoins
        for (R, S), g in zip(joins, got):
            assert np.array_equal(sorted_pairs(g), exp[id(R), id(S)]), (len(R), len(S), len(g))


def test_empty_input_reports_no_kernel(engines, oracle):
    """include/rhj.h: "last.join_kernel" is -1 after a join with an empty input, and "last.narrow" 0, whatever ran before"""
    with Forced(engines("ct"), "ct", 2) as f:
        rng = np.random.default_rng(1)
        R, S = relations(f, rng, "near_miss", nbuild=5_000)
        for A, B in ((R[:0], S), (R, S[:0])):
            check(f, oracle, R, S)
            assert len(f.eng.join(A, B, opts=f.plan)) == 0
            assert (f.eng.info("last.join_kernel"), f.eng.info("last.narrow")) == (-1, 0)
            check(f, oracle, R, S)
            dA, dB = f.eng.to_device(A), f.eng.to_device(B)
            assert f.eng.join_dev(dA, len(A), dB, len(B), opts=f.plan) == 0
            assert (f.eng.info("last.join_kernel"), f.eng.info("last.narrow")) == (-1, 0)
