"""CPU suite: the builders and the oracle of keyed_table_cases.py are what they claim, so that a pass of
test_gpu_keyed_table_adversarial.py cannot be vacuous.  No GPU, no library call."""
import os
import re

import numpy as np
import pytest

import keyed_table_cases as K
from radixhashjoin_amd import AGG_MAX_I64, AGG_MAX_U64, AGG_MIN_I64, AGG_MIN_U64, AGG_SUM, mix64, unmix64

U64 = np.uint64
# (rb, pattern, mixes) of the paths of the GPU suite: unpartitioned; one pass of 4 bits and two of 8, mixed and on raw digits
SPACES = [(0, 0, False), (4, 9, True), (16, 0xBEEF, True), (4, 9, False), (16, 0xBEEF, False)]
SPACE_IDS = [f"rb{rb}-{'mixed' if m else 'raw'}" for rb, _, m in SPACES]


def test_start_bucket_and_its_inverse():
    buckets = np.arange(K.NBUCKETS)
    for low in (0, 1, (1 << 20) - 1):
        folds = np.array([K.fold_for_bucket(int(b), low) for b in buckets], dtype=U64)
        assert np.array_equal(K.start_bucket(folds, 0), buckets)
        for rb in (4, 16):                                                   # the fold as a key x of a plan of rb bits, any pattern
            assert np.array_equal(K.start_bucket(K.place(folds, rb, (1 << rb) - 1), rb), buckets)
    x = np.array([0x123456789ABCDEF0, 0xFFFFFFFFFFFFFFFF, 1 << 32], dtype=U64)
    by_hand = [((((int(v) & 0xFFFFFFFF) ^ (int(v) >> 32)) * 0x9E3779B1) & 0xFFFFFFFF) >> 20 for v in x]
    assert K.start_bucket(x, 0).tolist() == by_hand
    d = np.arange(1, 2000, dtype=U64)
    assert len(set(K.start_bucket(x[0] ^ (d * K.FOLD), 0).tolist())) == 1   # x ^ (d * FOLD) keeps the fold
    assert np.array_equal(unmix64(mix64(x)), x)


def test_bj_bucket_still_reads_as_the_numpy_copy_assumes():
    """a plain text check: if it fails, bj_bucket changed -- update keyed_table_cases.start_bucket / fold_for_bucket to the new hash
    (and this check), or the crafted chains no longer share a start slot"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "radixhashjoin_amd", "csrc", "rhj_kernels.hip")
    with open(path) as f:
        text = f.read()
    m = re.search(r"u32 bj_bucket\(u64 v, int radix_bits\)\s*\{(.*?)\n\}", text, re.S)
    assert m, "bj_bucket is gone from rhj_kernels.hip: update keyed_table_cases.start_bucket"
    body = m.group(1)
    assert "0x9E3779B1u" in body and ">> (32 - BBITS)" in body and "v >> radix_bits" in body, \
        "bj_bucket no longer multiplies the fold by 0x9E3779B1u and takes its top BBITS bits: update keyed_table_cases.start_bucket"


@pytest.mark.parametrize("variant", K.CHAIN_VARIANTS)
@pytest.mark.parametrize("rb,pattern,mixes", SPACES, ids=SPACE_IDS)
def test_chain_is_one_start_slot_in_one_partition(rb, pattern, mixes, variant):
    for side in ("S", "R"):
        c = K.chain(rb, pattern, mixes, variant, table_side=side)
        info = c.info
        table, probe = (c.valS, c.valR) if side == "S" else (c.valR, c.valS)
        h = K.seen(info["chain"], mixes)
        low = U64((1 << rb) - 1)
        assert len(np.unique(h)) == K.CHAIN_KEYS == 3000
        assert (K.start_bucket(h, rb) == K.CHAIN_START[variant]).all() and info["bucket"] == K.CHAIN_START[variant]
        assert ((h & low) == U64(pattern)).all()
        hs, hi = K.seen(info["absent_same"], mixes), K.seen(info["absent_inside"], mixes)
        assert len(np.unique(np.concatenate([h, hs, hi]))) == 3000 + 500 + 500
        assert (K.start_bucket(hs, rb) == info["bucket"]).all() and ((hs & low) == U64(pattern)).all()
        assert (K.start_bucket(hi, rb) == info["inside_bucket"]).all() and ((hi & low) == U64(pattern)).all()
        # the second fold starts inside the chain's 3,000 slots, in walk order from the chain's start slot
        assert 0 < (2 * info["inside_bucket"] - 2 * info["bucket"]) % K.SLOTS < K.CHAIN_KEYS
        # the table side's partition `pattern` holds the chain and nothing else: the chain's slots are exactly as stated
        ht = K.seen(table, mixes)
        mine = ht[(ht & low) == U64(pattern)] if rb else ht
        assert np.array_equal(np.unique(mine), np.sort(h)) and len(mine) == 3000 + 2 * len(h[::7])
        assert not np.isin(info["absent_same"], table).any() and not np.isin(info["absent_inside"], table).any()
        vals, counts = np.unique(mine, return_counts=True)
        assert sorted(set(counts.tolist())) == [1, 3] and int((counts == 3).sum()) == len(h[::7])
        # one table for every kernel: at most four build tiles, so no close rule can end it early
        assert len(mine) <= 4 * K.BUILD_TILE and K.tables_closed(mine) == 1 and K.group_rounds(mine) == 1
        # the probe side: every 3rd chain key, all absent keys, every 7th of them three times; its own partition fits a table too
        assert np.isin(info["chain"][::3], probe).all() and np.isin(info["absent_same"], probe).all() and np.isin(info["absent_inside"], probe).all()
        assert int(np.isin(info["chain"], probe).sum()) == 1000
        hp = K.seen(probe, mixes)
        theirs = hp[(hp & low) == U64(pattern)] if rb else hp
        assert len(np.unique(theirs)) == 2000 and len(theirs) == 2000 + 2 * len(np.arange(2000)[::7])
        assert K.tables_closed(theirs) == 1 and K.group_rounds(theirs) == 1
        assert len(c.valR) + len(c.valS) < 50_000 and min(len(c.valR), len(c.valS)) >= 1024
        if rb:                                                             # the other partitions are not empty
            assert len(np.unique(ht & low)) > min(1 << rb, 1000) // 2


@pytest.mark.parametrize("rb,pattern,mixes", SPACES, ids=SPACE_IDS)
def test_markers_meet_every_placement(rb, pattern, mixes):
    met = {}
    for variant in K.MARKER_VARIANTS:
        c = K.markers(rb, pattern, mixes, variant)
        for p, nR, nS in c.info["markers"]:
            assert int((c.valR == p).sum()) == nR and int((c.valS == p).sum()) == nS
            assert sorted({nR, nS} - {0}) in ([1], [3], [1, 3])
            met.setdefault(int(p), set()).add("both" if nR and nS else "R" if nR else "S")
        assert len(c.valR) + len(c.valS) < 50_000 and min(len(c.valR), len(c.valS)) >= 1024
        # one table and one round in every partition, on either side
        for v in (c.valR, c.valS):
            h = K.seen(v, mixes)
            part = (h & U64((1 << rb) - 1)).astype(np.int64) if rb else np.zeros(len(h), dtype=np.int64)
            assert np.bincount(part).max() <= 4 * K.BUILD_TILE
    assert all(m == {"R", "S", "both"} for m in met.values()), met
    # what the kernel sees includes its marker and the marker's neighbours; the raw payloads are there whatever they map to
    seen = K.seen(np.array(list(met), dtype=U64), mixes).tolist()
    for h in (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFE, 0, 1, 1 << 63):
        assert h in seen
    for p in (0, 0xFFFFFFFFFFFFFFFF, int(unmix64(U64(0)))):
        assert p in met
    assert len(met) == (7 if mixes else 6)                                 # (unmix64(0) is the kernel-side 0 where the path mixes)


def test_marker_and_tables_layout():
    for position in K.MARKER_POSITIONS:
        for probes in K.MARKER_PROBES:
            for side in ("S", "R"):
                c = K.marker_and_tables(position, probes, table_side=side)
                table, probe = (c.valS, c.valR) if side == "S" else (c.valR, c.valS)
                assert np.array_equal(table, c.info["table_keys"])
                real = table[table != K.ONES]
                assert len(np.unique(real)) == len(real) == K.N_TABLE_KEYS
                at = np.flatnonzero(table == K.ONES)
                # 4096 distinct keys per table: the marker key's row lies in the first, the second, the third table, or nowhere
                want = {"first": [0], "middle": [K.N_TABLE_KEYS // 2], "last": [len(table) - 1], "absent": []}[position]
                assert at.tolist() == want
                assert K.tables_closed(table) == 3 and [a // 4096 for a in want] == {"first": [0], "middle": [1], "last": [2], "absent": []}[position]
                assert int((probe == K.ONES).sum()) == probes
                hits = np.isin(probe[probe != K.ONES], table)
                assert int(hits.sum()) == 3000 and int((~hits).sum()) == 2000
                assert len(c.valR) + len(c.valS) < 50_000


def test_fill_edge_and_the_close_rule():
    expected = {4095: 1, 4096: 1, 4097: 2, 8192: 2, 8193: 3, "4096+repeats": 2}
    for edge in K.FILL_EDGES:
        c = K.fill_edge(edge)
        table = c.info["table_keys"]
        assert np.array_equal(table, c.valS) and len(np.unique(table)) == c.info["distinct"]
        assert K.tables_closed(table) == expected[edge]
        if edge != "4096+repeats":                                          # distinct keys: ceil(n / 4096)
            assert len(table) == edge and expected[edge] == -(-edge // 4096)
        else:
            assert len(table) == 4096 + K.FILL_REPEATS and int((table == table[0]).sum()) == K.FILL_REPEATS + 1
            assert int((c.valR == table[0]).sum()) == 2
        assert int(np.isin(c.valR, table).sum()) == 2000 and len(c.valR) == 3000
        assert len(c.valR) + len(c.valS) < 50_000
    # the rule itself: the all-ones key fills no slot, a repeated key fills one, the order of arrival matters only through the tiles
    keys = np.arange(1, 20_001, dtype=U64)
    assert [K.tables_closed(keys[:n]) for n in (1, 4096, 4097, 8192, 8193, 20_000)] == [1, 1, 2, 2, 3, 5]
    assert K.tables_closed(np.concatenate([[K.ONES], keys[:4096]])) == 2     # 4097 rows: the fifth tile does not fit behind 4095 keys
    assert K.tables_closed(np.concatenate([keys[:3584], np.full(50_000, 7, dtype=U64)])) == 1
    assert K.tables_closed(np.zeros(0, dtype=U64)) == 1
    # the class walk: at most FILL distinct keys are one build; beyond, the root fails and both halves are built
    assert K.group_rounds(keys[:K.FILL]) == 1 and K.group_rounds(keys[:K.FILL + 1]) == 3
    assert K.group_rounds(np.concatenate([keys[:K.FILL], [K.ONES]])) == 1
    assert K.group_rounds(np.repeat(keys[:100], 1000)) == 1


OPS = [AGG_SUM, AGG_MIN_I64, AGG_MAX_U64]
ALL_OPS = [AGG_SUM, AGG_MIN_U64, AGG_MAX_U64, AGG_MIN_I64, AGG_MAX_I64]


def small_cases():
    yield "markers", K.subsample(K.markers(16, 0xBEEF, True, 1))
    yield "markers-raw", K.subsample(K.markers(0, 0, False, 2), seed=1)
    yield "marker_and_tables", K.subsample(K.marker_and_tables("first", 5), seed=2)
    yield "chain", K.subsample(K.chain(4, 9, True, "wrap"), seed=3)
    yield "fill_edge", K.subsample(K.fill_edge("4096+repeats"), seed=4)
    c = K.subsample(K.chain(0, 0, False, "start0", table_side="R"), seed=5)
    yield "chain-null-ids", K.null_ids(c)
    yield "empty-S", c._replace(valS=c.valS[:0], idS=c.idS[:0])


@pytest.mark.parametrize("name,case", list(small_cases()), ids=[n for n, _ in small_cases()])
def test_oracle_equals_brute_force(name, case):
    assert len(case.valR) == 200 and len(case.valS) in (200, 0)
    fast, slow = K.Oracle(case), K.BruteForce(case)
    if len(case.valS):
        assert 0 < len(fast.semi_ids(False)) < 200, "the sample has hits and misses"
    assert fast.pair_count() == slow.pair_count()
    for anti in (False, True):
        assert np.array_equal(fast.semi_ids(anti), slow.semi_ids(anti))
    assert np.array_equal(fast.r_only(), slow.semi_ids(True)) and np.array_equal(fast.s_only(), slow.s_only())
    assert fast.join_sums(2) == slow.join_sums(2)
    for w in (None, 0, 2):
        a, b = fast.mult(200, w), slow.mult(200, w)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    for ops in (OPS, ALL_OPS[:3], ALL_OPS[2:]):
        for got, exp in ((fast.groups(ops), slow.groups(ops)), (fast.group_join(False, ops[:1], ops[1:2]), slow.group_join(False, ops[:1], ops[1:2])),
                         (fast.group_join(True, ops[1:], ops[:2]), slow.group_join(True, ops[1:], ops[:2]))):
            flat = lambda t: [a for x in t for a in (x if isinstance(x, list) else [x])]
            assert len(flat(got)) == len(flat(exp))
            for a, b in zip(flat(got), flat(exp)):
                assert a.dtype == b.dtype == U64 and np.array_equal(a, b)
