"""GPU suite: composite keys -- rhj_keys_pack_dev / rhj_keys_unpack_dev (include/rhj.h), Engine.pack_keys and the torch
entries on lists of key tensors.

The oracle is numpy alone: np.unique(np.stack(cols, 1), axis=0, return_inverse=True) over the concatenation of both sides gives every
row its composite id; everything expected is built from those ids.
  * the pack property: #distinct (packed, composite id) pairs == #distinct packed == #distinct composite, i.e. the partition of
    R u S by packed word is the partition by composite key; unpack returns the input columns bit for bit; every output has guard
    words behind it; every case runs twice;
  * every layout by the input that asks for it: RANGE (narrow, negative through the biased view, a constant column, one 64-bit
    column), DICT, mixed, one fold, two folds -- asserted on plan.layout --; one relation; an empty side; rows that differ in the
    first or the last column only; all ones and 0;
  * the operators on lists of key tensors against the oracle: join (unpartitioned, one pass, and a narrow two-pass plan on pack_keys
    output), semi / anti, full outer, join-sum, multiplicity, group-by, factorize, group-by join; a constant column beside the real key;
  * refusals before any launch; a plan without dictionaries; close twice; single tensors never pack."""
import numpy as np
import pytest
import torch

from radixhashjoin_amd import KEYS_DICT as DICT, KEYS_NO_UNPACK, KEYS_RANGE as RANGE, Engine, Opts, RhjError
from radixhashjoin_amd.binding import KEYS_FOLD0 as FOLD0, RHJ_E_INVALID

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 64, 0x5A5A5A5A5A5A5A5A
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
TOP = np.uint64(1) << np.uint64(63)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def dev(a):
    """an int64 tensor on the GPU with the bits of a numpy 64-bit integer array"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def host_u64(t):
    return t.cpu().numpy().view(np.uint64)


def composite_ids(R, S):
    """(ids of R's rows, ids of S's rows, number of distinct composite keys): the oracle"""
    rows = np.stack([np.concatenate([np.asarray(r).view(np.uint64), np.asarray(s).view(np.uint64)]) for r, s in zip(R, S)], 1)
    uniq, inv = np.unique(rows, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    return inv[:len(R[0])], inv[len(R[0]):], len(uniq)


class Guarded:
    """n words of output with GUARD sentinel words behind them"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")

    def words(self):
        return host_u64(self.buf[:self.n])

    def intact(self):
        return bool((self.buf[self.n:] == SENTINEL).all())


def check_pack(eng, R, S):
    """packs the columns R (and S: a list of as many columns, or None), twice; checks the pack property against the oracle, the
    guards, and the unpack of both outputs; returns the layout (as_dict) of the last plan"""
    R = [np.asarray(c).view(np.uint64) for c in R]
    S = [np.asarray(c).view(np.uint64) for c in S] if S is not None else [np.empty(0, dtype=np.uint64) for _ in R]
    nR, nS, k = len(R[0]), len(S[0]), len(R)
    idR, idS, distinct = composite_ids(R, S)
    cid = np.concatenate([idR, idS]).astype(np.uint64)
    tR, tS = [dev(c) for c in R], [dev(c) for c in S]
    lay = None
    for _ in range(2):
        outR, outS = Guarded(nR), Guarded(nS)
        torch.cuda.synchronize()
        plan = eng.keys_pack_dev(tR, nR, tS if nS else (), nS, outR.buf if nR else None, outS.buf if nS else None)
        try:
            assert outR.intact() and outS.intact(), "a pack output's guard words were written"
            packed = np.concatenate([outR.words(), outS.words()])
            if nR + nS:
                order = np.lexsort((cid, packed))                            # distinct (packed, composite id) pairs, and distinct packed
                p, c = packed[order], cid[order]
                both, words = 1 + int(((p[1:] != p[:-1]) | (c[1:] != c[:-1])).sum()), 1 + int((p[1:] != p[:-1]).sum())
                assert both == words == distinct, (both, words, distinct)
            for out, cols, n in ((outR, R, nR), (outS, S, nS)):
                back = [Guarded(n) for _ in range(k)]
                torch.cuda.synchronize()
                eng.keys_unpack_dev(plan, out.buf, n, [b.buf for b in back])
                for j in range(k):
                    assert back[j].intact(), "an unpack output's guard words were written"
                    assert np.array_equal(back[j].words(), cols[j]), f"column {j} did not come back bit for bit"
            lay = plan.layout.as_dict()
            assert lay["nkeys"] == k and lay["total_bits"] <= 64
            if nR + nS:
                assert int(packed.max()) >> lay["total_bits"] == 0
        finally:
            plan.close()
    print(f"nR {nR} nS {nS} layout {lay}")
    return lay


def full_range(rng, n, pool):
    """n full-range 64-bit words drawn from `pool` distinct ones, with 0, all ones and the two values around the sign among them:
    64 bits wide in the plain and in the biased view"""
    values = rng.integers(0, 1 << 64, pool, dtype=np.uint64)
    values[:4] = [0, ONES, TOP, TOP - np.uint64(1)]
    col = values[rng.integers(0, pool, n)]
    col[rng.permutation(n)[:4]] = values[:4]
    return col


def split(cols, nR):
    return [c[:nR] for c in cols], [c[nR:] for c in cols]


# ---- layouts by their natural inputs ----------------------------------------------------------------------------------------------
def test_two_narrow_columns_are_range(eng):
    rng = np.random.default_rng(1)
    a = rng.integers(1000, 1000 + (1 << 10), 6000).astype(np.uint64)
    b = rng.integers(5, 5 + 300, 6000).astype(np.uint64)
    a[:2], b[:2] = [1000, 1000 + 1023], [5, 304]
    R, S = split([a, b], 3000)
    lay = check_pack(eng, R, S)
    assert lay["kind"] == [RANGE, RANGE] and lay["range_bits"] == [10, 9] and lay["shifts"] == [0, 10] and lay["total_bits"] == 19
    assert lay["base"] == [1000, 5] and lay["folds"] == []


def test_negative_int64_columns_are_narrow_through_the_biased_view(eng):
    rng = np.random.default_rng(2)
    a = rng.integers(-3, 4, 6000)
    b = rng.integers(-(1 << 40), (1 << 40) + 1, 6000)
    a[:2], b[:2] = [-3, 3], [-(1 << 40), 1 << 40]
    R, S = split([a, b], 3000)
    lay = check_pack(eng, R, S)
    assert lay["kind"] == [RANGE, RANGE] and lay["range_bits"] == [3, 42] and lay["total_bits"] == 45
    assert lay["base"] == [(1 << 64) - 3, (1 << 64) - (1 << 40)]


def test_a_constant_column_has_width_0(eng):
    rng = np.random.default_rng(3)
    a = np.full(6000, 0xDEADBEEF12345678, dtype=np.uint64)
    b = rng.integers(0, 1 << 12, 6000).astype(np.uint64)
    b[:2] = [0, 4095]
    lay = check_pack(eng, *split([a, b], 3000))
    assert lay["range_bits"] == [0, 12] and lay["widths"] == [0, 12] and lay["total_bits"] == 12 and lay["base"][0] == 0xDEADBEEF12345678
    lay = check_pack(eng, *split([b, a, a], 3000))                           # ... also behind a field, and twice
    assert lay["widths"] == [12, 0, 0] and lay["total_bits"] == 12


def test_two_full_range_columns_are_both_dictionaries(eng):
    rng = np.random.default_rng(4)
    lay = check_pack(eng, *split([full_range(rng, 6000, 900), full_range(rng, 6000, 700)], 3000))
    assert lay["kind"] == [DICT, DICT] and lay["range_bits"] == [64, 64] and lay["wd"] == 13 and lay["total_bits"] == 26
    assert 890 <= lay["dict_size"][0] <= 900 and 690 <= lay["dict_size"][1] <= 700 and lay["folds"] == []


def test_full_range_beside_narrow_is_mixed(eng):
    rng = np.random.default_rng(5)
    narrow = rng.integers(-50, 50, 6000)
    narrow[:2] = [-50, 49]
    lay = check_pack(eng, *split([full_range(rng, 6000, 2000), narrow], 3000))
    assert lay["kind"] == [DICT, RANGE] and lay["widths"] == [13, 7] and lay["total_bits"] == 20
    lay = check_pack(eng, *split([narrow, full_range(rng, 6000, 2000)], 3000))
    assert lay["kind"] == [RANGE, DICT] and lay["widths"] == [7, 13] and lay["shifts"] == [0, 7]


def four_full_range(seed, n, pool_rows):
    """four full-range columns of n rows drawn from pool_rows composite rows, whose columns repeat values on their own too"""
    rng = np.random.default_rng(seed)
    pool = [full_range(rng, pool_rows, max(pool_rows // 3, 8)) for _ in range(4)]
    pick = rng.integers(0, pool_rows, n)
    return [p[pick] for p in pool]


def test_four_full_range_columns_fold_once(eng):
    cols = four_full_range(6, 140_000, 50_000)
    lay = check_pack(eng, *split(cols, 70_000))
    assert lay["kind"] == [DICT] * 4 and lay["wd"] == 18 and lay["folds"] == [(0, 1)] and lay["fields"] == [FOLD0, 2, 3]
    assert lay["total_bits"] == 54 and 0 < lay["fold_size"][0] <= 140_000


def test_four_full_range_columns_fold_twice(eng):
    cols = four_full_range(7, 2_200_000, 700_000)
    lay = check_pack(eng, *split(cols, 1_100_000))
    assert lay["kind"] == [DICT] * 4 and lay["wd"] == 22 and lay["folds"] == [(0, 1), (FOLD0, 2)] and lay["fields"] == [FOLD0 + 1, 3]
    assert lay["total_bits"] == 44 and lay["fold_size"][0] <= lay["fold_size"][1] <= 2_200_000


def test_a_fold_with_a_range_field_inside(eng):
    """[18 bits, full, full, full] over 140,001 rows: 4 x 18 bits do not fit, and the fold's first input is a RANGE field; an odd nR,
    so S's id arrays start off a 16-byte line"""
    rng = np.random.default_rng(8)
    n, pool = 140_001, 40_000
    pick = rng.integers(0, pool, n)
    pick[:2] = [0, 1]
    narrow = rng.integers(0, 1 << 18, pool).astype(np.uint64)
    narrow[:2] = [0, (1 << 18) - 1]
    cols = [narrow[pick]] + [full_range(rng, pool, 9000)[pick] for _ in range(3)]
    lay = check_pack(eng, *split(cols, 70_001))
    assert lay["kind"] == [RANGE, DICT, DICT, DICT] and lay["range_bits"][0] == 18 and lay["wd"] == 18
    assert lay["folds"] == [(0, 1)] and lay["fields"] == [FOLD0, 2, 3] and lay["total_bits"] == 54


def test_one_key_column(eng):
    rng = np.random.default_rng(9)
    lay = check_pack(eng, *split([full_range(rng, 6000, 1500)], 3000))
    assert lay["kind"] == [RANGE] and lay["total_bits"] == 64
    lay = check_pack(eng, *split([rng.integers(-5, 5, 6001)], 3000))
    assert lay["kind"] == [RANGE] and lay["total_bits"] <= 4


def test_one_relation_and_empty_sides(eng):
    rng = np.random.default_rng(10)
    cols = [full_range(rng, 3001, 500), rng.integers(0, 9, 3001).astype(np.uint64), full_range(rng, 3001, 800)]
    lay = check_pack(eng, cols, None)                                        # one relation: the dictionaries read R's column in place
    assert lay["kind"] == [DICT, RANGE, DICT] and lay["wd"] == 12
    empty = [np.empty(0, dtype=np.uint64) for _ in cols]
    assert check_pack(eng, cols, empty)["kind"] == [DICT, RANGE, DICT]       # nS == 0
    assert check_pack(eng, empty, cols)["kind"] == [DICT, RANGE, DICT]       # nR == 0
    lay = check_pack(eng, empty, empty)                                      # no rows: a plan, nothing launched
    assert lay["kind"] == [RANGE] * 3 and lay["total_bits"] == 0
    # ... and through the torch entry, keys_S=None
    e_cols = [dev(c) for c in cols]
    packed, none, plan = eng.pack_keys(e_cols)
    assert none is None and packed.dtype == torch.int64 and packed.numel() == 3001
    back = plan.unpack(packed)
    assert all(torch.equal(b, c) for b, c in zip(back, e_cols))
    plan.close()


@pytest.mark.parametrize("wide", [False, True], ids=["range", "dict"])
def test_rows_that_differ_in_one_column_only(eng, wide):
    """R: (i, c, c), S: (c, c, i) -- a pack that drops its first or its last field merges the rows of a side"""
    n = 3000
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        i = i * np.uint64(0x9E3779B97F4A7C15) if wide else i + np.uint64(17)
    c = np.full(n, i[5], dtype=np.uint64)
    R, S = [i, c, c], [c, c, i]
    assert composite_ids(R, S)[2] == 2 * n - 1
    lay = check_pack(eng, R, S)
    assert lay["kind"] == ([DICT, RANGE, DICT] if wide else [RANGE] * 3)


def test_all_ones_and_zero(eng):
    z = np.array([0, ONES] * 1500, dtype=np.uint64)
    w = np.array([0, 0, ONES, ONES] * 750, dtype=np.uint64)
    lay = check_pack(eng, [z, w], [w, z])
    assert lay["range_bits"] == [1, 1] and lay["total_bits"] == 2 and lay["base"] == [int(ONES), int(ONES)]     # the biased view: -1, 0
    rng = np.random.default_rng(11)
    lay = check_pack(eng, *split([full_range(rng, 6000, 50), z.repeat(2)], 3000))
    assert lay["kind"] == [DICT, RANGE] and lay["widths"] == [13, 1]


# ---- operators on composite keys --------------------------------------------------------------------------------------------------
class Case:
    """two key columns per side -- a narrow signed one and a full-range one, each heavily repeated on its own, the pair moderately --
    their composite ids, and a weight column per side; built once per size, never written"""

    def __init__(self, nR, nS, seed, narrow_only=False):
        rng = np.random.default_rng(seed)
        D = max((nR + nS) // 5, 4)
        ka = rng.integers(-40, 40, D)
        kb = rng.integers(0, 1 << 20, D).astype(np.uint64) if narrow_only else full_range(rng, D, max(D // 6, 8))
        pR, pS = rng.integers(0, D * 3 // 4, nR), rng.integers(D // 4, D, nS)      # a quarter of the keys on one side only, each way
        self.R = [ka[pR].view(np.uint64), kb[pR]]
        self.S = [ka[pS].view(np.uint64), kb[pS]]
        self.idR, self.idS, self.G = composite_ids(self.R, self.S)
        self.wR, self.wS = rng.integers(-1000, 1000, nR), rng.integers(-1000, 1000, nS)
        self.tR, self.tS = [dev(c) for c in self.R], [dev(c) for c in self.S]
        self.twR, self.twS = dev(self.wR), dev(self.wS)
        self.cntR, self.cntS = np.bincount(self.idR, minlength=self.G), np.bincount(self.idS, minlength=self.G)

    def pairs(self):
        """the join's (row of R, row of S) pairs, sorted"""
        order = np.argsort(self.idS, kind="stable")
        start = np.concatenate([[0], np.cumsum(self.cntS)])
        reps = self.cntS[self.idR]
        r = np.repeat(np.arange(len(self.idR)), reps)
        off = np.arange(reps.sum()) - np.repeat(np.cumsum(reps) - reps, reps)
        s = order[np.repeat(start[self.idR], reps) + off]
        return sorted_pairs(r, s)


def sorted_pairs(r, s):
    p = np.stack([np.asarray(r, dtype=np.int64), np.asarray(s, dtype=np.int64)], 1)
    return p[np.lexsort((p[:, 1], p[:, 0]))]


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = Case(n, n + n // 7, n)
        return cache[n]
    return get


@pytest.mark.parametrize("n", [3_000, 70_000], ids=["unpartitioned", "one-pass"])
def test_join_columns_on_two_key_columns(eng, cases, n):
    c = cases(n)
    exp = c.pairs()
    for _ in range(2):
        iR, iS = eng.join_columns(c.tR, c.tS)
        print(f"n {n} pairs {iR.numel()} passes {eng.timings()['passes']}")
        assert np.array_equal(sorted_pairs(iR.cpu().numpy(), iS.cpu().numpy()), exp)
    assert eng.timings()["passes"] == (0 if n == 3_000 else 1)


def test_a_narrow_two_pass_join_on_packed_keys(eng):
    """3,000,000 rows of R against 500,000 of S under Opts(2, 8, 8), narrow: join_cols_dev on what pack_keys returns"""
    nR, nS = 3_000_000, 500_000
    c = Case(nR, nS, 33, narrow_only=True)
    exp = c.pairs()
    pR, pS, plan = eng.pack_keys(c.tR, c.tS, keep_dictionaries=False)
    assert plan.layout.as_dict()["kind"] == [RANGE, RANGE]
    plan.close()
    out = torch.empty((len(exp) + 1, 2), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.set_option("partition.narrow", 2)
    try:
        got = eng.join_cols_dev(pR, None, nR, pS, None, nS, out, len(exp) + 1, opts=Opts(2, 8, 8))
        print(f"pairs {got} passes {eng.timings()['passes']} narrow {eng.info('last.narrow')}")
        assert got == len(exp) and eng.timings()["passes"] == 2 and eng.info("last.narrow") == 2
    finally:
        eng.set_option("partition.narrow", -1)
    pairs = out[:got].cpu().numpy()
    assert np.array_equal(sorted_pairs(pairs[:, 0], pairs[:, 1]), exp)


def test_semi_and_anti_join_columns(eng, cases):
    c = cases(3_000)
    hit = c.cntS[c.idR] > 0
    for anti in (False, True):
        idx = eng.semi_join_columns(c.tR, c.tS, anti=anti)
        assert np.array_equal(np.sort(idx.cpu().numpy()), np.flatnonzero(hit != anti))
    hit = c.cntR[c.idS] > 0                                                  # ... and the other way round
    for anti in (False, True):
        idx = eng.semi_join_columns(c.tS, c.tR, anti=anti)
        assert np.array_equal(np.sort(idx.cpu().numpy()), np.flatnonzero(hit != anti))


def test_full_outer_join_columns(eng, cases):
    c = cases(3_000)
    exp = c.pairs()
    iR, iS = (t.cpu().numpy() for t in eng.outer_join_columns(c.tR, c.tS, how="full"))
    m = len(exp)
    onlyR, onlyS = np.flatnonzero(c.cntS[c.idR] == 0), np.flatnonzero(c.cntR[c.idS] == 0)
    assert len(iR) == len(iS) == m + len(onlyR) + len(onlyS) and len(onlyR) and len(onlyS)
    assert np.array_equal(sorted_pairs(iR[:m], iS[:m]), exp)
    a, b = m + len(onlyR), m + len(onlyR) + len(onlyS)
    assert np.array_equal(np.sort(iR[m:a]), onlyR) and (iS[m:a] == -1).all()
    assert np.array_equal(np.sort(iS[a:b]), onlyS) and (iR[a:b] == -1).all()


def test_join_sum_and_multiplicity_columns(eng, cases):
    c = cases(3_000)
    mult = c.cntS[c.idR]
    count, sums = eng.join_sum_columns(c.tR, c.tS, [c.twR])
    assert count == int(mult.sum()) and sums == [int((c.wR * mult).sum()) % (1 << 64)]
    got, total = eng.join_multiplicity_columns(c.tR, c.tS)
    assert total == int(mult.sum()) and np.array_equal(got.cpu().numpy(), mult)
    got, total = eng.join_multiplicity_columns(c.tR, c.tS, weights_S=c.twS)
    wsum = np.zeros(c.G, dtype=np.int64)
    np.add.at(wsum, c.idS, c.wS)
    assert np.array_equal(got.cpu().numpy(), wsum[c.idR]) and total == int(wsum[c.idR].sum()) % (1 << 64)


def by_key(keys, *cols):
    """the columns (numpy), rows sorted by the int64 key columns, first key first"""
    keys = [k.cpu().numpy() if hasattr(k, "cpu") else np.asarray(k) for k in keys]
    order = np.lexsort(tuple(reversed(keys)))
    return [k[order] for k in keys] + [(x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x))[order] for x in cols]


def group_oracle(cols, weights):
    """np.unique over the rows of one relation: [key columns as int64, counts, sum of weights], in np.unique's order on int64"""
    rows = np.stack([np.asarray(c).view(np.int64) for c in cols], 1)
    uniq, inv, counts = np.unique(rows, axis=0, return_inverse=True, return_counts=True)
    sums = np.zeros(len(uniq), dtype=np.int64)
    np.add.at(sums, inv.reshape(-1), weights)
    return [uniq[:, j] for j in range(rows.shape[1])], inv.reshape(-1), counts, sums


@pytest.mark.parametrize("n", [3_000, 70_000])
def test_group_by_columns_on_two_key_columns(eng, cases, n):
    c = cases(n)
    ekeys, _, ecounts, esums = group_oracle(c.R, c.wR)
    for _ in range(2):
        keys, counts, sums = eng.group_by_columns(c.tR, [c.twR], ops=["sum"])
        assert isinstance(keys, list) and len(keys) == 2 and all(k.dtype == torch.int64 and k.numel() == len(ecounts) for k in keys)
        a, b, cnt, s = by_key(keys, counts, sums[0])
        assert np.array_equal(a, ekeys[0]) and np.array_equal(b, ekeys[1]) and np.array_equal(cnt, ecounts) and np.array_equal(s, esums)


def test_factorize_and_group_by_with_inverse(eng, cases):
    c = cases(3_000)
    ekeys, _, ecounts, _ = group_oracle(c.R, c.wR)
    codes, uniques = eng.factorize_columns(c.tR)
    assert len(uniques) == 2 and uniques[0].numel() == len(ecounts) and codes.numel() == 3_000
    for j in range(2):
        assert torch.equal(uniques[j][codes], c.tR[j])
    keys, counts, _, inverse = eng.group_by_columns_with_inverse(c.tR)
    assert all(torch.equal(keys[j][inverse], c.tR[j]) for j in range(2))
    assert np.array_equal(np.bincount(inverse.cpu().numpy(), minlength=len(ecounts)), counts.cpu().numpy())


def test_join_group_by_columns_left(eng, cases):
    c = cases(3_000)
    ekeys, inv, cntR, sumR = group_oracle(c.R, c.wR)
    gid_of = np.zeros(len(cntR), dtype=np.int64)                             # R's group -> composite id over both sides
    gid_of[inv] = c.idR
    cntS = c.cntS[gid_of]
    sumS = np.zeros(c.G, dtype=np.int64)
    np.add.at(sumS, c.idS, c.wS)
    keys, count, sums_R, sums_S = eng.join_group_by_columns(c.tR, c.tS, [c.twR], [c.twS], how="left")
    a, b, cnt, sR, sS = by_key(keys, count, sums_R[0], sums_S[0])
    assert np.array_equal(a, ekeys[0]) and np.array_equal(b, ekeys[1])
    assert np.array_equal(cnt, cntR * np.maximum(cntS, 1)) and np.array_equal(sR, sumR * np.maximum(cntS, 1))
    assert np.array_equal(sS, sumS[gid_of] * cntR) and (cntS == 0).any() and (cntS > 1).any()
    keys, count, _, _, (inv_R, inv_S) = eng.join_group_by_columns_with_inverse(c.tR, c.tS, how="inner")
    assert keys[0].numel() == int(((c.cntR > 0) & (c.cntS > 0)).sum())
    has = inv_S >= 0
    assert np.array_equal(has.cpu().numpy(), c.cntR[c.idS] > 0)
    assert all(torch.equal(keys[j][inv_S[has]], c.tS[j][has]) for j in range(2))


@pytest.mark.parametrize("const_first", [True, False], ids=["const-first", "const-last"])
def test_a_constant_column_beside_the_real_key(eng, const_first):
    """each column alone: one is constant (joins everything), the other is the key -- n pairs, not n^2"""
    n = 3_000
    rng = np.random.default_rng(12)
    key_R, key_S = rng.permutation(n).astype(np.int64) - 1500, rng.permutation(n).astype(np.int64) - 1500
    const = np.full(n, -7, dtype=np.int64)
    R, S = ([const, key_R], [const, key_S]) if const_first else ([key_R, const], [key_S, const])
    tR, tS = [dev(x) for x in R], [dev(x) for x in S]
    iR, iS = eng.join_columns(tR, tS)
    assert iR.numel() == n and np.array_equal(key_R[iR.cpu().numpy()], key_S[iS.cpu().numpy()])
    count, _ = eng.join_sum_columns(tR, tS)
    assert count == n
    keys, counts, _ = eng.group_by_columns(tR)
    assert keys[0].numel() == n and bool((counts == 1).all())


# ---- refusals, plans, single tensors ----------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(eng, monkeypatch):
    k = torch.arange(100, device="cuda", dtype=torch.int64)
    monkeypatch.setattr(Engine, "keys_pack_dev", lambda *a, **kw: pytest.fail("a refused call reached the pack"))
    for bad_R, bad_S in (([k] * 5, [k] * 5), ([k, k], [k]), ([k], [k, k]), ([k, k[:50]], [k, k]), ([k, k], [k, k[:7]]), ([], []),
                         ([k, k], k)):
        for call in (eng.join_columns, eng.semi_join_columns, eng.outer_join_columns, eng.join_sum_columns, eng.join_multiplicity_columns,
                     eng.join_group_by_columns, eng.pack_keys):
            with pytest.raises(ValueError):
                call(bad_R, bad_S)
    for bad in ([k] * 5, [k, k[:50]], []):
        for call in (eng.group_by_columns, eng.group_by_columns_with_inverse, eng.factorize_columns, eng.pack_keys):
            with pytest.raises(ValueError):
                call(bad)


def test_a_plan_without_dictionaries_and_close_twice(eng):
    rng = np.random.default_rng(13)
    cols = [dev(full_range(rng, 3000, 400)), dev(full_range(rng, 3000, 300))]
    packed, _, plan = eng.pack_keys(cols, keep_dictionaries=False)
    assert plan.layout.as_dict()["kind"] == [DICT, DICT]
    with pytest.raises(RhjError) as e:
        plan.unpack(packed)
    assert e.value.code == RHJ_E_INVALID
    plan.close()
    plan.close()
    packed2, _, plan2 = eng.pack_keys(cols)                                  # the context is as usable as before
    assert all(torch.equal(b, c) for b, c in zip(plan2.unpack(packed2), cols))
    # a word the plan did not produce is refused, not used as an index
    with pytest.raises(RhjError) as e:
        plan2.unpack(torch.full((10,), (1 << 26) - 1, dtype=torch.int64, device="cuda"))
    assert e.value.code == RHJ_E_INVALID
    assert all(torch.equal(b, c) for b, c in zip(plan2.unpack(packed2), cols))
    plan2.close()
    plan2.close()
    with pytest.raises(RhjError) as e:
        eng.keys_pack_dev(cols, 3000, (), 0, packed, None, flags=2)
    assert e.value.code == RHJ_E_INVALID
    assert KEYS_NO_UNPACK == 1


def test_single_tensors_never_pack(eng, monkeypatch):
    def refuse(*a, **kw):
        raise AssertionError("a single key tensor went through rhj_keys_pack_dev")
    monkeypatch.setattr(Engine, "keys_pack_dev", refuse)
    k_R = torch.arange(5_000, device="cuda", dtype=torch.int64) % 1000
    k_S = torch.arange(700, device="cuda", dtype=torch.int64)
    iR, iS = eng.join_columns(k_R, k_S)
    assert iR.numel() == 3_500 and torch.equal(k_R[iR], k_S[iS])
    keys, counts, _ = eng.group_by_columns(k_R)
    assert isinstance(keys, torch.Tensor) and keys.numel() == 1000 and bool((counts == 5).all())
    with pytest.raises(AssertionError):
        eng.join_columns([k_R], [k_S])
