"""Adversarial inputs and the oracle of the keyed-table kernels (k_semi_bkt in its three forms, k_agg_bkt, k_mult_bkt, k_group_bkt,
k_gjoin_bkt), shared by test_keyed_table_cases.py (CPU: the builders are what they claim) and test_gpu_keyed_table_adversarial.py.
numpy only.

The five kernels share one LDS table: 8192 slots of 8-byte keys, open addressing from the start slot 2 * bj_bucket<12>(key,
radix_bits), a linear walk that wraps at slot 8192 (the probe reads 16-byte pairs and wraps at pair 4096), insert-if-absent by a
64-bit compare-and-swap, the all-ones word as the empty marker -- a key that IS all ones lives in a word beside the table --, and a
close rule that counts distinct keys tile by tile.  A kernel under a plan of rb radix bits sees h = rhj_mix64(payload), or the
payload itself where nothing mixes (an unpartitioned plan, any plan under "partition.mix" 0); inside a partition all h share their
low rb bits and the table hashes x = h >> rb.  Everything below is built in that space: h = (x << rb) | pattern, and the payload
handed to the engine is unmix64(h) where the path mixes, h where it does not.

Builders -- each returns a Case (valR, idR, valS, idS, colsR, colsS, info); ids are a permutation, the columns are indexed by id:
  markers            the values a kernel can mistake for its empty marker, on R only, S only or both, once or three times
  marker_and_tables  unpartitioned: ~9,000 distinct keys on the table side (three tables per task) with the marker key first, in the
                     middle, last or absent, and 0, 1 or 5 probes of it
  chain              3,000 distinct keys of ONE start slot in one partition: the chain starts at slot 0, wraps from slot 8191 to 0, or
                     ends exactly at slot 8191; probes of every third key, of absent keys of the same start slot, and of absent keys
                     whose start slot lies inside the chain
  fill_edge          unpartitioned: 4095 ... 8193 distinct keys on the table side, where a table closes
Oracle: one stable sort per side gives, per distinct value, cntR, cntS and the per-column aggregates; every entry's answer is derived
from those.  tables_closed / group_rounds restate the two close rules, so "last.semi_tables" / "last.group_rounds" are exact."""
import collections

import numpy as np

from radixhashjoin_amd import AGG_MAX_I64, AGG_MAX_U64, AGG_MIN_I64, AGG_MIN_U64, AGG_SUM, mix64, unmix64

U64 = np.uint64
ONES = U64(0xFFFFFFFFFFFFFFFF)
M32 = U64(0xFFFFFFFF)
FOLD = U64(0x100000001)                    # d * FOLD has equal 32-bit halves: x ^ (d * FOLD) folds like x
GOLD = 0x9E3779B1                          # bj_bucket's multiplier (rhj_kernels.hip); odd, so invertible mod 2^32
GOLD_INV = pow(GOLD, -1, 1 << 32)
BBITS = 12                                 # bj_bucket<SLOT_BITS - 1>: 4096 start pairs
NBUCKETS, SLOTS = 1 << BBITS, 2 << BBITS
# rhj_internal.h: SEMI_BUILD_TILE == AGG_BUILD_TILE == 1024 tuples per build tile, SEMI_FILL == AGG_FILL == 4608 distinct keys
BUILD_TILE, FILL = 1024, 4608
GROUP_CLASS_SALT = U64(0xA0761D6478BD642F)  # rhj_kernels.hip: the class of a key is mix64(key ^ salt) & (2^d - 1)
I64_MIN, I64_MAX = 1 << 63, (1 << 63) - 1
IDENTITY = {AGG_SUM: 0, AGG_MIN_U64: (1 << 64) - 1, AGG_MAX_U64: 0, AGG_MIN_I64: I64_MAX, AGG_MAX_I64: I64_MIN}
NCOLS = 3                                  # weight columns per side

Case = collections.namedtuple("Case", "valR idR valS idS colsR colsS info")


# ---- the start slot ------------------------------------------------------------------------------------------------------------
def start_bucket(h, rb):
    """numpy copy of bj_bucket<12>(h, rb): x = h >> rb; (((u32)x ^ (u32)(x >> 32)) * 0x9E3779B1 mod 2^32) >> 20.  The start slot is
    twice this."""
    x = np.asarray(h, dtype=U64) >> U64(rb)
    f = (x & M32) ^ (x >> U64(32))
    return (((f * U64(GOLD)) & M32) >> U64(32 - BBITS)).astype(np.int64)


def fold_for_bucket(bucket, low=0):
    """a fold f = (u32)x ^ (u32)(x >> 32) that bj_bucket<12> sends to `bucket` (low: the 20 bits of the product below the bucket)"""
    assert 0 <= bucket < NBUCKETS and 0 <= low < 1 << (32 - BBITS)
    return (((bucket << (32 - BBITS)) | low) * GOLD_INV) & 0xFFFFFFFF


def keys_of_fold(rng, f, n, rb):
    """n distinct x < 2^(64 - rb) with fold f: a random upper half below 2^(32 - rb) and the lower half that completes the fold.
    (Any two of them differ by d * FOLD in the sense of x ^ (d * FOLD): the trick of test_gpu_adversarial.py.)"""
    hi = rng.choice(1 << min(32 - rb, 24), n, replace=False).astype(U64)
    x = (hi << U64(32)) | (hi ^ U64(f))
    assert rb == 0 or int(x.max()) < 1 << (64 - rb)
    return x


def place(x, rb, pattern):
    """h = (x << rb) | pattern"""
    x = np.asarray(x, dtype=U64)
    return x if rb == 0 else (x << U64(rb)) | U64(pattern)


def payload_of(h, mixes):
    """the payload whose kernel-side value is h"""
    h = np.asarray(h, dtype=U64)
    return unmix64(h) if mixes else h


def seen(payload, mixes):
    """the value a kernel compares and hashes for this payload"""
    payload = np.asarray(payload, dtype=U64)
    return mix64(payload) if mixes else payload


def radix_bits(plan):
    return plan.bits1 + plan.bits2 if plan.passes == 2 else plan.bits1 if plan.passes == 1 else 0


# ---- the two close rules -------------------------------------------------------------------------------------------------------
def tables_closed(keys_in_order):
    """LDS tables that k_semi_bkt / k_agg_bkt / k_mult_bkt build over one task's table side, read in this order: whole tiles of
    BUILD_TILE tuples while filled + BUILD_TILE <= FILL, `filled` the distinct keys in the table (the all-ones key sits beside it
    and is not counted).  The kernels read the count between two barriers after every tile, so this is exact."""
    keys = np.asarray(keys_in_order, dtype=U64)
    done, tables = 0, 0
    while True:
        tables += 1
        inside, filled = set(), 0
        while done < len(keys) and filled + BUILD_TILE <= FILL:
            tile = keys[done: done + BUILD_TILE]
            inside.update(tile[tile != ONES].tolist())
            filled = len(inside)
            done += len(tile)
        if done >= len(keys):
            return tables


def group_rounds(keys_seen):
    """table builds of k_group_bkt / k_gjoin_bkt over one partition of R: a class (d, p) holds the keys with mix64(key ^ salt) &
    (2^d - 1) == p and fails -- its two children are built instead -- when it holds more than FILL distinct keys (the all-ones key
    not counted); every class visited is one build, an empty one too.  The count depends on the keys' hashes, not on their order."""
    k = np.unique(np.asarray(keys_seen, dtype=U64))
    hashed = mix64(k[k != ONES] ^ GROUP_CLASS_SALT)

    def walk(d, p):
        n = int(((hashed & U64((1 << d) - 1)) == U64(p)).sum())
        return 1 if n <= FILL else 1 + walk(d + 1, p) + walk(d + 1, p | (1 << d))
    return walk(0, 0)


# ---- shared pieces of the builders -----------------------------------------------------------------------------------------------
def ordinary(rng, nR, nS, rb, mixes, avoid=None):
    """ordinary random rows under both sides: R random, S half sampled from R and half fresh; with avoid (a partition pattern, rb > 0)
    no row falls into that partition.  Returned as payloads."""
    def draw(n):
        h = rng.integers(0, 1 << 63, n, dtype=U64) * U64(2) + rng.integers(0, 2, n, dtype=U64)
        if avoid is not None and rb > 0:
            clash = (h & U64((1 << rb) - 1)) == U64(avoid)
            h[clash] ^= U64(1)
        return h
    hR = draw(nR)
    hS = np.concatenate([hR[rng.integers(0, nR, nS // 2)], draw(nS - nS // 2)]) if nR else draw(nS)
    return payload_of(hR, mixes), payload_of(hS, mixes)


def finish(rng, vR, vS, info, table_side="S"):
    """shuffle both sides (unless info says the order matters), give ids and columns; table_side "R" exchanges the sides"""
    if not info.get("keep_order"):
        vR, vS = rng.permutation(vR), rng.permutation(vS)
    if table_side == "R":
        vR, vS = vS, vR
    vR, vS = np.ascontiguousarray(vR, dtype=U64), np.ascontiguousarray(vS, dtype=U64)
    idR, idS = rng.permutation(len(vR)).astype(U64), rng.permutation(len(vS)).astype(U64)
    colsR = [rng.integers(0, 1 << 64, len(vR), dtype=U64) for _ in range(NCOLS)]
    colsS = [rng.integers(0, 1 << 64, len(vS), dtype=U64) for _ in range(NCOLS)]
    info = dict(info, table_side=table_side)
    return Case(vR, idR, vS, idS, colsR, colsS, info)


def null_ids(case):
    """the case as a call with NULL id columns sees it: the rowID of a tuple is its index"""
    return case._replace(idR=np.arange(len(case.valR), dtype=U64), idS=np.arange(len(case.valS), dtype=U64))


# ---- markers ---------------------------------------------------------------------------------------------------------------------
MARKER_SEEN = [ONES, ONES - U64(1), U64(0), U64(1), U64(1 << 63)]          # in the space the kernel sees
MARKER_RAW = [U64(0), ONES, unmix64(U64(0))]                               # raw payloads, whatever they map to
PLACEMENTS = ("R", "S", "both")
MARKER_VARIANTS = (0, 1, 2)


def marker_payloads(mixes):
    """the distinct payloads of the family, in a fixed order (under a path that does not mix the two lists overlap)"""
    out = []
    for p in [payload_of(h, mixes) for h in MARKER_SEEN] + MARKER_RAW:
        if int(p) not in [int(q) for q in out]:
            out.append(U64(p))
    return out


def markers(rb, pattern, mixes, variant=0, n_ordinary=(3000, 2500)):
    """Every marker value on R only, S only or both -- value i takes PLACEMENTS[(i + variant) % 3], so over the three variants every
    value meets every placement --, once on one side and three times on the other (which, alternates with i + variant).  Beside them
    20 ordinary keys in the partition of the all-ones h and 20 in the partition `pattern`, half of each on both sides: the tables
    that hold a marker hold other keys too.  info["markers"]: [(payload, rows on R, rows on S)]."""
    rng = np.random.default_rng(1000 * rb + 10 * variant + int(mixes) + 7)
    vR, vS = ordinary(rng, *n_ordinary, rb, mixes)
    placed = []
    for i, p in enumerate(marker_payloads(mixes)):
        where = PLACEMENTS[(i + variant) % 3]
        mR, mS = (1, 3) if (i + variant) % 2 == 0 else (3, 1)
        nR, nS = (mR if where in ("R", "both") else 0), (mS if where in ("S", "both") else 0)
        placed.append((p, nR, nS))
        vR = np.concatenate([vR, np.full(nR, p, dtype=U64)])
        vS = np.concatenate([vS, np.full(nS, p, dtype=U64)])
    for pat in dict.fromkeys([(1 << rb) - 1 if rb else 0, pattern]):
        x = rng.integers(1, 1 << 40, 20, dtype=U64)
        comp = payload_of(place(x, rb, pat), mixes)
        vR = np.concatenate([vR, comp[:15]])
        vS = np.concatenate([vS, comp[5:]])
    return finish(rng, vR, vS, {"markers": placed, "rb": rb, "mixes": mixes})


# ---- marker_and_tables -------------------------------------------------------------------------------------------------------------
MARKER_POSITIONS = ("first", "middle", "last", "absent")
MARKER_PROBES = (0, 1, 5)
N_TABLE_KEYS = 9000


def marker_and_tables(position, probes, table_side="S"):
    """Unpartitioned (the kernel sees the payloads, the marker key is the all-ones payload, the table side is read in input order):
    N_TABLE_KEYS distinct keys on the table side -- three tables per task -- with the marker key as its first row, in the middle (the
    second table), as its last row (the third table) or absent; the probe side holds 3,000 hits, 2,000 misses and the marker key
    `probes` times, shuffled.  info["table_keys"]: the table side in input order."""
    rng = np.random.default_rng(100 * MARKER_POSITIONS.index(position) + probes)
    keys = np.unique(rng.integers(1, 1 << 62, N_TABLE_KEYS + 64, dtype=U64))
    table = rng.permutation(keys)[:N_TABLE_KEYS]
    at = {"first": 0, "middle": N_TABLE_KEYS // 2, "last": N_TABLE_KEYS}.get(position)
    if at is not None:
        table = np.concatenate([table[:at], [ONES], table[at:]])
    probe = np.concatenate([table[table != ONES][rng.integers(0, N_TABLE_KEYS, 3000)],
                            rng.integers(1, 1 << 62, 2000, dtype=U64) | U64(1 << 62), np.full(probes, ONES, dtype=U64)])
    probe = rng.permutation(probe)
    return finish(rng, probe, table, {"keep_order": True, "table_keys": table, "position": position, "probes": probes}, table_side)


# ---- chain ---------------------------------------------------------------------------------------------------------------------------
CHAIN_KEYS, CHAIN_ABSENT = 3000, 500
CHAIN_START = {"start0": 0, "wrap": NBUCKETS - 1, "end8191": (SLOTS - CHAIN_KEYS) // 2}   # start buckets: slots 0, 8190, 5192
CHAIN_VARIANTS = tuple(CHAIN_START)
assert 2 * CHAIN_START["end8191"] + CHAIN_KEYS - 1 == SLOTS - 1            # 3,000 keys from slot 5192 on end at slot 8191
assert 2 * CHAIN_START["wrap"] + CHAIN_KEYS > SLOTS                        # ... from slot 8190 on run over the table's end
CHAIN_INSIDE = 500                                                         # start pairs into the chain where the second fold begins


def chain(rb, pattern, mixes, variant="start0", table_side="S", n_ordinary=(2000, 2000)):
    """The table side: CHAIN_KEYS distinct keys of one fold whose start bucket is CHAIN_START[variant], in the partition `pattern`,
    every 7th three times; with nothing else in that partition they fill slots 2 * bucket ... 2 * bucket + 2999 (mod 8192).
    The probe side: every 3rd chain key, CHAIN_ABSENT absent keys of the same fold (a probe walks the whole chain to the empty slot
    behind it) and CHAIN_ABSENT absent keys of a fold that starts CHAIN_INSIDE pairs into the chain (it walks the rest of it), every
    7th of all of them three times.  Ordinary rows go to the other partitions only (rb == 0 has none: no ordinary rows).
    info: chain / absent_same / absent_inside as payloads, bucket, inside_bucket."""
    rng = np.random.default_rng(1000 * rb + 10 * CHAIN_VARIANTS.index(variant) + int(mixes) + 3)
    bucket = CHAIN_START[variant]
    inside = (bucket + CHAIN_INSIDE) % NBUCKETS
    x = keys_of_fold(rng, fold_for_bucket(bucket, int(rng.integers(0, 1 << 20))), CHAIN_KEYS + CHAIN_ABSENT, rb)
    y = keys_of_fold(rng, fold_for_bucket(inside, int(rng.integers(0, 1 << 20))), CHAIN_ABSENT, rb)
    keys, same, other = (payload_of(place(k, rb, pattern), mixes) for k in (x[:CHAIN_KEYS], x[CHAIN_KEYS:], y))
    table = np.concatenate([keys, np.repeat(keys[::7], 2)])
    asked = np.concatenate([keys[::3], same, other])
    probe = np.concatenate([asked, np.repeat(asked[::7], 2)])
    oP, oT = ordinary(rng, *n_ordinary, rb, mixes, avoid=pattern) if rb else (np.zeros(0, dtype=U64),) * 2
    info = {"chain": keys, "absent_same": same, "absent_inside": other, "bucket": bucket, "inside_bucket": inside, "rb": rb,
            "pattern": pattern, "mixes": mixes}
    return finish(rng, np.concatenate([probe, oP]), np.concatenate([table, oT]), info, table_side)


# ---- fill_edge -----------------------------------------------------------------------------------------------------------------------
FILL_EDGES = (4095, 4096, 4097, 8192, 8193, "4096+repeats")
FILL_REPEATS = 10_000


def fill_edge(edge, table_side="S"):
    """Unpartitioned: `edge` distinct keys on the table side, in input order -- a k_semi_bkt table takes whole 1024-tuple tiles while
    filled + 1024 <= 4608, so 4096 distinct keys are one table and 4097 two --; "4096+repeats": 4096 distinct keys, then FILL_REPEATS
    repeats of the first of them (a second table of one key that the first table holds too: its tuples of S are counted in two
    tables).  The probe side: 2,000 hits and 1,000 misses.  info["table_keys"]: the table side in input order."""
    n = 4096 if edge == "4096+repeats" else edge
    rng = np.random.default_rng(n + (100_000 if edge == "4096+repeats" else 0))
    keys = np.unique(rng.integers(1, 1 << 62, n + 64, dtype=U64))
    table = rng.permutation(keys)[:n]
    if edge == "4096+repeats":
        table = np.concatenate([table, np.full(FILL_REPEATS, table[0], dtype=U64)])
    # hits drawn from the distinct keys behind the first, which is probed exactly twice (it is the one that may be repeated)
    probe = rng.permutation(np.concatenate([table[rng.integers(1, n, 1998)], table[:1], table[:1],
                                            rng.integers(1, 1 << 62, 1000, dtype=U64) | U64(1 << 62)]))
    return finish(rng, probe, table, {"keep_order": True, "table_keys": table, "edge": edge, "distinct": n}, table_side)


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
_REDUCE = {AGG_SUM: (np.add, U64), AGG_MIN_U64: (np.minimum, U64), AGG_MAX_U64: (np.maximum, U64),
           AGG_MIN_I64: (np.minimum, np.int64), AGG_MAX_I64: (np.maximum, np.int64)}


class Side:
    """one relation after ONE stable sort by value: .keys ascending, .cnt per key, .row_key the key index of every row"""

    def __init__(self, val, ids, cols):
        self.val, self.ids, self.cols = np.asarray(val, dtype=U64), np.asarray(ids, dtype=U64).astype(np.int64), cols
        self.order = np.argsort(self.val, kind="stable")
        s = self.val[self.order]
        first = np.concatenate([[True], s[1:] != s[:-1]]) if len(s) else np.zeros(0, dtype=bool)
        self.starts = np.flatnonzero(first)
        self.keys = s[self.starts]
        self.cnt = np.diff(np.concatenate([self.starts, [len(s)]])).astype(U64)
        self.row_key = np.empty(len(s), dtype=np.int64)
        self.row_key[self.order] = np.cumsum(first) - 1

    def agg(self, j, op):
        """per key, the aggregate `op` of column j over the key's rows, as uint64 words"""
        if len(self.keys) == 0:
            return np.zeros(0, dtype=U64)
        fn, view = _REDUCE[op]
        with np.errstate(over="ignore"):
            return fn.reduceat(self.cols[j][self.ids][self.order].view(view), self.starts).view(U64)


class Oracle:
    """cntR / cntS and the aggregates per distinct value; every entry's expected answer derived from them"""

    def __init__(self, case):
        self.R, self.S = Side(case.valR, case.idR, case.colsR), Side(case.valS, case.idS, case.colsS)
        R, S = self.R, self.S
        # per key of R its count in S, and the other way round
        self.R_in_S = self._lookup(R.keys, S.keys, S.cnt)
        self.S_in_R = self._lookup(S.keys, R.keys, R.cnt)
        self.partners_R = self.R_in_S[R.row_key] if len(R.val) else np.zeros(0, dtype=U64)     # per row of R: tuples of S with its value
        self.partners_S = self.S_in_R[S.row_key] if len(S.val) else np.zeros(0, dtype=U64)

    @staticmethod
    def _lookup(keys, other_keys, other_words, missing=0):
        out = np.full(len(keys), missing, dtype=U64)
        if len(other_keys):
            at = np.minimum(np.searchsorted(other_keys, keys), len(other_keys) - 1)
            hit = other_keys[at] == keys
            out[hit] = other_words[at[hit]]
        return out

    def pair_count(self):
        return int((self.R.cnt.astype(object) * self.R_in_S.astype(object)).sum()) if len(self.R.keys) else 0

    def semi_ids(self, anti):
        return np.sort(self.R.ids[(self.partners_R == 0) == bool(anti)]).astype(U64)

    def r_only(self):
        return self.semi_ids(True)

    def s_only(self):
        return np.sort(self.S.ids[self.partners_S == 0]).astype(U64)

    def join_sums(self, ncols):
        """COUNT(*) and SUM(colsR[j][rowR]) over the pairs, mod 2^64"""
        with np.errstate(over="ignore"):
            return self.pair_count(), [int((self.partners_R * self.R.cols[j][self.R.ids]).sum(dtype=U64)) for j in range(ncols)]

    def mult(self, out_rows, weight_col=None):
        """(per rowID of R its multiplicity in S -- with weight_col the sum of colsS[weight_col][rowS] over its partners --, the total)"""
        per_key = self.R_in_S if weight_col is None else self._lookup(self.R.keys, self.S.keys, self.S.agg(weight_col, AGG_SUM))
        out = np.zeros(out_rows, dtype=U64)
        if len(self.R.val):
            out[self.R.ids] = per_key[self.R.row_key]
        with np.errstate(over="ignore"):
            return out, int(out.sum(dtype=U64))

    def groups(self, ops):
        """GROUP BY on R: (keys ascending, counts, [aggregate of colsR[j] under ops[j]])"""
        return self.R.keys, self.R.cnt, [self.R.agg(j, op) for j, op in enumerate(ops)]

    def group_join(self, left, opsR, opsS):
        """(keys ascending, cntR, cntS, [aggsR], [aggsS]) of the values both sides have (left: every value of R; a group without a
        tuple of S holds 0 in S's sums and the op's identity in its minima and maxima)"""
        keep = np.ones(len(self.R.keys), dtype=bool) if left else self.R_in_S != 0
        aggsS = [self._lookup(self.R.keys, self.S.keys, self.S.agg(j, op), missing=IDENTITY[op])[keep] for j, op in enumerate(opsS)]
        return self.R.keys[keep], self.R.cnt[keep], self.R_in_S[keep], [self.R.agg(j, op)[keep] for j, op in enumerate(opsR)], aggsS


# ---- a second, independent oracle for small inputs: dictionaries and Python integers -------------------------------------------------
def _py_agg(words, op):
    if op == AGG_SUM:
        return sum(words) & ((1 << 64) - 1)
    if op in (AGG_MIN_U64, AGG_MAX_U64):
        return (min if op == AGG_MIN_U64 else max)(words)
    signed = [w - (1 << 64) if w >> 63 else w for w in words]
    return (min if op == AGG_MIN_I64 else max)(signed) & ((1 << 64) - 1)


class BruteForce:
    """the same answers from {value: [rowIDs]} dictionaries"""

    def __init__(self, case):
        self.c = case
        self.R, self.S = collections.defaultdict(list), collections.defaultdict(list)
        for v, i in zip(case.valR.tolist(), case.idR.tolist()):
            self.R[v].append(i)
        for v, i in zip(case.valS.tolist(), case.idS.tolist()):
            self.S[v].append(i)

    def pair_count(self):
        return sum(len(r) * len(self.S[v]) for v, r in self.R.items() if v in self.S)

    def semi_ids(self, anti):
        return np.array(sorted(i for v, r in self.R.items() if (v not in self.S) == bool(anti) for i in r), dtype=U64)

    def s_only(self):
        return np.array(sorted(i for v, s in self.S.items() if v not in self.R for i in s), dtype=U64)

    def join_sums(self, ncols):
        cols = [c.tolist() for c in self.c.colsR[:ncols]]
        return self.pair_count(), [sum(len(self.S[v]) * col[i] for v, r in self.R.items() if v in self.S for i in r) & ((1 << 64) - 1)
                                   for col in cols]

    def mult(self, out_rows, weight_col=None):
        w = None if weight_col is None else self.c.colsS[weight_col].tolist()
        out = [0] * out_rows
        for v, r in self.R.items():
            if v in self.S:
                m = len(self.S[v]) if w is None else sum(w[i] for i in self.S[v]) & ((1 << 64) - 1)
                for i in r:
                    out[i] = m
        return np.array(out, dtype=U64), sum(out) & ((1 << 64) - 1)

    def groups(self, ops):
        keys = sorted(self.R)
        cols = [c.tolist() for c in self.c.colsR]
        return (np.array(keys, dtype=U64), np.array([len(self.R[k]) for k in keys], dtype=U64),
                [np.array([_py_agg([cols[j][i] for i in self.R[k]], op) for k in keys], dtype=U64) for j, op in enumerate(ops)])

    def group_join(self, left, opsR, opsS):
        keys = sorted(k for k in self.R if left or k in self.S)
        cR, cS = [c.tolist() for c in self.c.colsR], [c.tolist() for c in self.c.colsS]
        aggsR = [np.array([_py_agg([cR[j][i] for i in self.R[k]], op) for k in keys], dtype=U64) for j, op in enumerate(opsR)]
        aggsS = [np.array([_py_agg([cS[j][i] for i in self.S[k]], op) if k in self.S else IDENTITY[op] for k in keys], dtype=U64)
                 for j, op in enumerate(opsS)]
        return (np.array(keys, dtype=U64), np.array([len(self.R[k]) for k in keys], dtype=U64),
                np.array([len(self.S[k]) if k in self.S else 0 for k in keys], dtype=U64), aggsR, aggsS)


def subsample(case, n=200, seed=0):
    """n rows of each side of a case -- half of S's chosen among the rows whose value the rows kept of R have, where there are such --
    with ids and columns of their own"""
    rng = np.random.default_rng(seed)
    keepR = rng.permutation(len(case.valR))[:n]
    vR = case.valR[keepR]
    hit = np.flatnonzero(np.isin(case.valS, vR))
    rest = np.flatnonzero(~np.isin(case.valS, vR))
    keepS = np.concatenate([rng.permutation(hit)[: n // 2], rng.permutation(rest)])[:n]
    return finish(rng, vR, case.valS[keepS], {"keep_order": True})
