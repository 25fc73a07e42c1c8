"""Inputs for the two count-free partition passes, built in the mixed space: a builder chooses h = mix64(payload)
and hands over unmix64(h), so the digits the passes see are set, not drawn.  numpy only; tests/test_cf_cases.py checks on the CPU that
every builder is what it says, tests/test_gpu_cf_walk.py runs them through the kernels.

The geometry, restated from cf_geometry / cf2_geometry / make_geom (rhj_api.hip):
    unit_len(n)      L = max(4096, round_up_4096(ceil(n / 1024)))          a pass-1 unit
    units(n)         U = ceil(n / L)
    cap(L, b1)       round_up_32(int(m + 10 sqrt(m)) + 1),  m  = L / 2^b1        slots of one (unit, digit) region of pass 1
    cap2(n, b1, b2)  likewise with                          m2 = n / 2^(b1 + b2)  slots of one final partition's region
A "piece" is the run of one pass-1 digit inside one pass-1 unit; pass-1 bucket d is the U pieces of digit d, read by pass 2 as one
dense sequence of slots ("slot t": the t-th tuple of the bucket in unit order).  Final partition p = d1 * 2^b2 + d2 with d1 the low
b1 bits of h and d2 the next b2.

predict() gives the state words a side of a forced join must report; set_lengths() sets every piece length of an 8+8 join, all_full()
fills every live region of both passes to the last slot, plain() is the random input the older count-free files use."""
import math

import numpy as np

from radixhashjoin_amd import mix64, unmix64

U64 = np.uint64
TUPLE = np.dtype([("key", "<u8"), ("payload", "<u8")])
TILE, TARGET_UNITS = 4096, 1024                               # pass-1 unit length: n / 1024 rounded up to whole tiles
# piece lengths every unit carries, by unit length (0 ... cap and both sides of every 32-slot line in between)
SPECIAL = {4096: [0, 1, 31, 32, 33, 63, 64], 8192: [0, 1, 31, 32, 33, 63, 64, 65, 95, 96]}
# the marked buckets of set_lengths (pass-1 digits)
MARK_FRONT, MARK_BACK, MARK_SEVENTH, MARK_EDGE = 0x40, 0x80, 0xC0, 0x20
EDGE_SLOTS = (1024, 4096)                                     # one slot per thread of the workgroup; one tile


def unit_len(n):
    per = -(-n // TARGET_UNITS)
    return max(TILE, -(-per // TILE) * TILE)


def units(n):
    return -(-n // unit_len(n))


def _region(m):
    return (int(m + 10.0 * math.sqrt(m)) + 1 + 31) // 32 * 32


def cap(L, b1):
    return _region(L / (1 << b1))


def cap2(n, b1, b2):
    return _region(n / (1 << (b1 + b2)))


def bits_of(plan):
    """(b1, b2) of an Opts or of a pair"""
    return (plan.bits1, plan.bits2) if hasattr(plan, "bits1") else tuple(plan)


def piece_lengths(t, b1=8):
    """[U, 2^b1] run lengths per (pass-1 unit, digit), from the relation as the library sees it"""
    n, L = len(t), unit_len(len(t))
    d1 = (mix64(t["payload"]) & U64((1 << b1) - 1)).astype(np.int64)
    return np.bincount((np.arange(n) // L << b1) + d1, minlength=units(n) << b1).reshape(units(n), 1 << b1)


def partition_sizes(t, b1=8, b2=8):
    """[2^b1, 2^b2] tuples per final partition (d1, d2)"""
    h = mix64(t["payload"])
    d1, d2 = (h & U64((1 << b1) - 1)).astype(np.int64), ((h >> U64(b1)) & U64((1 << b2) - 1)).astype(np.int64)
    return np.bincount((d1 << b2) + d2, minlength=1 << (b1 + b2)).reshape(1 << b1, 1 << b2)


def predict(rel, plan, cus):
    """("last.countfree_X", "last.countfree2_X") of relation `rel` as one side of a pair join under a fused narrow plan with
    "partition.narrow" 2, "partition.countfree" 1 and "partition.countfree2" 1 freshly set (no back-off pending), every rowID
    below 2^32, on a device of `cus` compute units -- from the data alone:
      * pass 1 is 1 if the largest piece fits cap, else 2 (tried, repeated with exact cursors);
      * pass 2 is tried iff 2^b1 >= cus (cf2_applies; its other conditions hold for every relation of fewer than 2^32 rows whose pass
        1 applied), and is then 1 if the largest final partition fits cap2, else 2;
      * a side whose pass 1 fell back reports 0 for pass 2, whatever its partitions: the repeat runs with cf_off_once set, so
        cf_side_for answers -1, cf2_end_for returns before it sets anything, and partition_phase has reset the word to 0 (the
        kernels of a join whose skip word is raised return at once, so the first attempt never got as far as a pass-2 overflow)."""
    b1, b2 = bits_of(plan)
    if int(piece_lengths(rel, b1).max()) > cap(unit_len(len(rel)), b1):
        return (2, 0)
    if (1 << b1) < cus:
        return (1, 0)
    return (1, 1 if int(partition_sizes(rel, b1, b2).max()) <= cap2(len(rel), b1, b2) else 2)


def rel(rng, h):
    """the relation of mixed values h, rowIDs a permutation of 0 .. n - 1"""
    t = np.empty(len(h), dtype=TUPLE)
    t["key"] = rng.permutation(len(h)).astype(U64)
    t["payload"] = unmix64(h)
    return t


# ---- set piece lengths -------------------------------------------------------------------------------------------------------

def forced_lengths(n):
    """-> ([256, U] piece lengths that set_lengths forces, -1 = left to digit_plan; {slot: unit} of the edge bucket).
    MARK_FRONT: 0 in its first 5 units; MARK_BACK: 0 in its last 5 units (with U <= 5 both buckets are wholly empty: no tile is
    loaded, 256 ends are written); MARK_SEVENTH: 0 everywhere except cap in every 7th whole unit; MARK_EDGE: whole regions (and
    one shorter piece where cap does not divide the distance) from unit 0 on until the prefix of the bucket is exactly 1024, then
    exactly 4096 -- edge[s] is the unit whose piece starts at slot s, None where the relation has too few whole units."""
    L, U, whole = unit_len(n), units(n), n // unit_len(n)
    c = cap(L, 8)
    f = np.full((256, U), -1, dtype=np.int64)
    f[MARK_FRONT, :5] = 0
    f[MARK_BACK, max(U - 5, 0):] = 0
    f[MARK_SEVENTH, :] = 0
    f[MARK_SEVENTH, 0:whole:7] = c
    edge, at, u = {}, 0, 0
    for target in EDGE_SLOTS:
        while at < target and u < whole:
            f[MARK_EDGE, u] = min(c, target - at)
            at += int(f[MARK_EDGE, u])
            u += 1
        edge[target] = u if at == target and u < U else None
    return f, edge


def digit_plan(rng, n, forced=None):
    """-> the pass-1 digit (low 8 bits of h) of every input position: inside unit u the digits (u + j) % 256, j < len(SPECIAL),
    get exactly SPECIAL[j] tuples, the other digits share the rest evenly; shuffled inside the unit.  With `forced` ([256, U]) a
    digit with forced[d, u] >= 0 gets exactly that many, and the special lengths rotate over the digits that are forced in no unit."""
    L = unit_len(n)
    special = SPECIAL[L]
    d1 = np.empty(n, dtype=np.int64)
    free = np.arange(256) if forced is None else np.flatnonzero((forced < 0).all(axis=1))
    for u in range(-(-n // L)):
        lens = np.full(256, -1, dtype=np.int64)
        for j, s in enumerate(special):
            lens[free[(u + j) % len(free)]] = s
        if forced is not None:
            lens = np.where(forced[:, u] >= 0, forced[:, u], lens)
        rest = np.flatnonzero(lens < 0)
        left = L - int(lens[lens >= 0].sum())
        lens[rest] = left // len(rest)
        lens[rest[: left % len(rest)]] += 1
        assert lens.sum() == L and lens.max() <= cap(L, 8)
        unit = np.repeat(np.arange(256), lens)
        rng.shuffle(unit)
        d1[u * L: (u + 1) * L] = unit[: min(L, n - u * L)]    # (the last unit may be cut short)
    return d1


def d2_plan(rng, d1, limit):
    """-> the pass-2 digit of every position, no final partition above `limit` (= cap2): a bucket of at least limit + 254 tuples
    fills partition d2 = d1 to exactly `limit`, leaves d2 = d1 + 1 empty and spreads the rest evenly; a smaller bucket is spread
    evenly over all 256.  Which tuple of the bucket takes which digit is shuffled."""
    d2 = np.empty(len(d1), dtype=np.int64)
    order = np.argsort(d1, kind="stable")
    start = np.searchsorted(d1[order], np.arange(257))
    for d in range(256):
        T = int(start[d + 1] - start[d])
        if T == 0:
            continue
        cnt = np.zeros(256, dtype=np.int64)
        if T >= limit + 254:
            others = np.array([x for x in range(256) if x not in (d, (d + 1) % 256)])
            cnt[d] = limit
            cnt[others] = (T - limit) // 254
            cnt[others[: (T - limit) % 254]] += 1
        else:
            cnt[:] = T // 256
            cnt[(np.arange(T % 256) + d) % 256] += 1
        assert cnt.sum() == T and cnt.max() <= limit
        v = np.repeat(np.arange(256), cnt)
        rng.shuffle(v)
        d2[order[start[d]: start[d + 1]]] = v
    return d2


def build_side(rng, n, kind, d1=None, d2=None):
    """R: n distinct mixed values whose low 8 bits follow d1 (default: digit_plan) and the next 8 d2 (default: drawn)"""
    i = np.arange(n, dtype=U64)
    d1 = (digit_plan(rng, n) if d1 is None else d1).astype(U64)
    d2 = (rng.integers(0, 256, n) if d2 is None else d2).astype(U64)
    if kind == "lowdup":      # low word: 4 values of its upper half -> at most 2^18 low words in all; high word: distinct
        lo = (U64(0x5A5A) + (i & U64(3))) << U64(16) | d2 << U64(8) | d1
        hi = ((i + U64(1)) * U64(0x9E3779B1)) & U64(0xFFFFFFFF)
    else:                     # high word: one per 65,536 rows; low word: its upper half distinct inside a high word
        assert n <= 1 << 24
        lo = (i & U64(0xFFFF)) << U64(16) | d2 << U64(8) | d1
        hi = U64(0xC0FFEE00) | ((i >> U64(16)) & U64(0xFF))
    h = hi << U64(32) | lo
    assert len(np.unique(h)) == n
    return h


def probe_side(rng, hR, n, d1=None, d2=None):
    """S: position p takes a build value of the digit d1 gives p (default: digit_plan; so S's piece lengths are set too) and, with
    d2 given, of that final partition -- where R has no value there, a value of the partition that R does not hold; a fifth of
    the rows then change the high word, another fifth the upper half of the low word: same partition, no match (unless the changed
    value happens to be another build value, which the oracle knows as well)"""
    d1 = digit_plan(rng, n) if d1 is None else d1
    if d2 is None:
        bits, p = 8, d1
    else:
        bits, p = 16, d2 << 8 | d1
    pR = (hR & U64((1 << bits) - 1)).astype(np.int64)
    order = np.argsort(pR, kind="stable")
    start = np.searchsorted(pR[order], np.arange((1 << bits) + 1))
    cnt = np.diff(start)
    have = cnt[p] > 0
    assert d2 is not None or have.all()
    r = rng.integers(0, 1 << 62, n)
    pick = order[np.where(have, start[p] + r % np.maximum(cnt[p], 1), 0)]
    h = hR[pick].copy()
    h[~have] = (r[~have].astype(U64) & U64((1 << 48) - 1)) << U64(16) | p[~have].astype(U64)
    r = rng.random(n)
    flip_hi = r < 0.2
    flip_lo = (r >= 0.2) & (r < 0.4)
    h[flip_hi] ^= rng.integers(1, 1 << 32, int(flip_hi.sum())).astype(U64) << U64(32)
    h[flip_lo] ^= rng.integers(1, 1 << 16, int(flip_lo.sum())).astype(U64) << U64(16)
    return h


def set_lengths(n, seed, nS=None):
    """-> (R of n rows, S of nS rows (default n), info) for Opts(2, 8, 8).  On BOTH sides every piece length is set: SPECIAL[L] in
    every unit (digit_plan), the four marked buckets of forced_lengths, the rest even -- none above cap; and every final partition
    is set by d2_plan with limit cap2: none above it, in every bucket of a tile or so one partition exactly AT cap2 and one empty.
    The last unit, where it is cut short, keeps a random part of its plan (a forced 0 stays 0).  R's values are distinct ("lowdup"
    for an even seed, "highdup" for an odd one: see build_side); S draws them partition by partition, two fifths altered so that
    they stay in the partition and match nothing.  info[side]: L, U, cap, cap2 and "edge" = {slot: unit} of bucket MARK_EDGE."""
    rng = np.random.default_rng(seed * 1_000_003 + n)
    nS = n if nS is None else nS
    info, d = {}, {}
    for side, m in (("R", n), ("S", nS)):
        forced, edge = forced_lengths(m)
        d1 = digit_plan(rng, m, forced)
        d[side] = (d1, d2_plan(rng, d1, cap2(m, 8, 8)))
        info[side] = {"L": unit_len(m), "U": units(m), "cap": cap(unit_len(m), 8), "cap2": cap2(m, 8, 8), "edge": edge}
    hR = build_side(rng, n, "lowdup" if seed % 2 == 0 else "highdup", *d["R"])
    hS = probe_side(rng, hR, nS, *d["S"])
    return rel(rng, hR), rel(rng, hS), info


# ---- every live region full ---------------------------------------------------------------------------------------------------

FULL_N, FULL_CAP = 1 << 20, 64                                # 256 units of 4096; cap = cap2 = 64 (m = m2 = 16)
FULL_DIGITS = np.arange(64) * 4 + 1                           # the pass-1 digits that occur


def _full_layout(rng):
    """(d1, d2) per row: in every unit each of the 64 digits of FULL_DIGITS has exactly 64 rows, and row r of digit d in unit u
    takes d2 = 64 * (u % 4) + r -- the 64 units with the same u % 4 put one tuple each into final partition (d, d2)"""
    d1, d2 = np.empty(FULL_N, dtype=np.int64), np.empty(FULL_N, dtype=np.int64)
    dd, rr = np.repeat(FULL_DIGITS, 64), np.tile(np.arange(64), 64)
    for u in range(FULL_N // TILE):
        perm = rng.permutation(TILE)
        d1[u * TILE: (u + 1) * TILE] = dd[perm]
        d2[u * TILE: (u + 1) * TILE] = (64 * (u % 4) + rr)[perm]
    return d1, d2


def all_full(variant=None, side="R"):
    """-> (R, S, info), 2^20 rows each, for Opts(2, 8, 8): 64 of the 256 pass-1 digits occur, each with exactly cap = 64 rows in every
    one of the 256 units, and every live final partition holds exactly cap2 = 64 tuples (16,384 of them; 192 buckets = 49,152
    partitions are empty).  The high 48 bits of R's values are distinct; S has the same layout (shuffled on its own) and takes its
    values from R partition by partition, a fifth of them changed above bit 16 so that they match nothing.
    variant "over2": the LAST row of relation `side` moves to the neighbouring final partition (d2 ^ 1) of its own bucket: 65 there,
      63 where it was, pass 1 untouched.  The row lies in the last unit, so among the last 64 slots of the bucket's 16,384: the
      one-writer pass 2 gives up on the bucket's fourth tile, after three were stored.
    variant "over1": one row of unit 100 of `side` changes its pass-1 digit from FULL_DIGITS[0] to FULL_DIGITS[1]: a run of 65."""
    assert variant in (None, "over2", "over1") and side in ("R", "S")
    assert cap(TILE, 8) == FULL_CAP and cap2(FULL_N, 8, 8) == FULL_CAP and unit_len(FULL_N) == TILE
    rng = np.random.default_rng(20)
    i = np.arange(FULL_N, dtype=U64)
    d1, d2 = _full_layout(rng)
    hR = ((i + U64(1)) * U64(0x9E3779B97F4B) & U64((1 << 48) - 1)) << U64(16) | (d2 << 8 | d1).astype(U64)
    assert len(np.unique(hR >> U64(16))) == FULL_N
    e1, e2 = _full_layout(rng)
    order = np.argsort(d1 << 8 | d2, kind="stable").reshape(-1, 64)          # R's rows by final partition, 64 each
    part = np.full(1 << 16, -1, dtype=np.int64)
    part[(d1 << 8 | d2)[order[:, 0]]] = np.arange(len(order))
    hS = hR[order[part[e1 << 8 | e2], rng.integers(0, 64, FULL_N)]]
    changed = rng.random(FULL_N) < 0.2
    hS[changed] ^= rng.integers(1, 1 << 40, int(changed.sum())).astype(U64) << U64(16)
    assert not np.isin(hS[changed], hR).any()
    info = {"variant": variant, "side": side, "row": None}
    h = hR if side == "R" else hS
    if variant == "over2":
        info["row"] = FULL_N - 1
        h[-1] ^= U64(0x100)
    elif variant == "over1":
        u = 100
        row = u * TILE + int(np.flatnonzero((h[u * TILE: (u + 1) * TILE] & U64(255)) == U64(FULL_DIGITS[0]))[0])
        info["row"] = row
        h[row] = (h[row] & ~U64(255)) | U64(FULL_DIGITS[1])
    return rel(rng, hR), rel(rng, hS), info


# ---- random inputs ------------------------------------------------------------------------------------------------------------

def plain(n, dist, seed, nS=None):
    """-> (R of n rows, S of nS rows): "uniform" -- distinct random join values in R, foreign keys in S; "dups" -- values drawn with
    repetition from a pool of n / 2 on the build side, S drawn from R's rows; every 97th row of S matches nothing"""
    nS = n if nS is None else nS
    rng = np.random.default_rng(n * 31 + nS + seed)
    if dist == "uniform":
        rv = rng.integers(1, 1 << 62, n, dtype=np.uint64)
    else:
        pool = rng.integers(1, 1 << 62, max(n // 2, 1), dtype=np.uint64)
        rv = pool[rng.integers(0, len(pool), n)]
    sv = rv[rng.integers(0, n, nS)]
    sv[::97] ^= np.uint64(1 << 62)
    R, S = np.empty(n, dtype=TUPLE), np.empty(nS, dtype=TUPLE)
    R["key"], S["key"] = rng.permutation(n).astype(U64), rng.permutation(nS).astype(U64)
    R["payload"], S["payload"] = rv, sv
    return R, S
