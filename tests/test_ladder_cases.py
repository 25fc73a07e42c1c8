"""CPU suite: the builders of ladder_cases.py are what they claim, so that a pass of test_gpu_ladder.py cannot be vacuous -- a rung
that is meant to overflow does, by one row, in the unit it names, and nothing else comes near.  No GPU, no library call."""
import numpy as np
import pytest

import cf_cases
import keyed_table_cases as K
import ladder_cases as LC

U64 = np.uint64
PATTERN = 0xBEEF
BASES = {"one-unit": (3000, 2500), "partial-unit": (9000, 7000)}
RUNGS = [("both", 0), ("S", 1), ("R", 1), ("both", 1)]


def base_case(name, variant):
    return K.markers(16, PATTERN, True, variant, n_ordinary=BASES[name])


def relation(values):
    t = np.empty(len(values), dtype=cf_cases.TUPLE)
    t["key"], t["payload"] = 0, values
    return t


def test_the_geometry_is_the_one_the_module_states():
    assert LC.CAP == cf_cases.cap(4096, 8) == 64
    for n in (1024, 3040, 4096, 9105, 10_000):
        assert cf_cases.unit_len(n) == 4096
    assert LC.choose_digit(PATTERN) not in (0xFF, 0xEF) and LC.choose_digit(0x5A) == 0x5B


@pytest.mark.parametrize("variant", K.MARKER_VARIANTS)
@pytest.mark.parametrize("base", list(BASES))
def test_the_bases_stay_far_below_a_region(base, variant):
    c = base_case(base, variant)
    units = {"one-unit": (1, 1), "partial-unit": (3, 2)}[base]
    for v, u in zip((c.valR, c.valS), units):
        p = cf_cases.piece_lengths(relation(v), 8)
        assert p.shape == (u, 256) and int(p.max()) <= 40 and np.array_equal(p, LC.pieces(v))
    assert LC.expect(LC.plain_info(c)) == ((2, 1, 1, 1, 1), (0, 0))


@pytest.mark.parametrize("side,extra", RUNGS, ids=[f"{s}+{e}" for s, e in RUNGS])
@pytest.mark.parametrize("variant", K.MARKER_VARIANTS)
@pytest.mark.parametrize("base", list(BASES))
def test_rung_fills_one_piece_to_the_row(base, variant, side, extra):
    b = base_case(base, variant)
    c = LC.rung(b, side, extra, PATTERN)
    d, info = c.info["digit"], c.info
    assert d not in (0xFF, PATTERN & 0xFF)
    for s, val, old, ids, oids, cols, ocols in (("R", c.valR, b.valR, c.idR, b.idR, c.colsR, b.colsR),
                                                ("S", c.valS, b.valS, c.idS, b.idS, c.colsS, b.colsS)):
        n, chosen = len(val), side in (s, "both")
        p = cf_cases.piece_lengths(relation(val), 8)
        U, u = cf_cases.units(n), info["unit"][s]
        assert u == U - 1 and cf_cases.unit_len(n) == 4096 and (base == "one-unit") == (U == 1)
        if base == "partial-unit":
            assert n % 4096 != 0 and n - u * 4096 < 4096                    # the piece that fills lies in a unit shorter than L
        want = LC.CAP + extra if chosen else None
        print(f"{s}: n {n} units {U} piece [{u}, {d:#x}] = {p[u, d]} largest elsewhere {np.delete(p.ravel(), u * 256 + d).max()}")
        if chosen:
            assert p[u, d] == want
        else:
            assert LC.SHARED <= p[u, d] < LC.CAP
        assert int(np.delete(p.ravel(), u * 256 + d).max()) < LC.CAP        # every other piece of the side
        assert info["over"][s] == bool(chosen and extra) == bool(p.max() > LC.CAP)
        # the old rows stand where they were; the new ones are distinct, fresh, of digit d, and behind them
        k = len(old)
        assert np.array_equal(val[:k], old) and np.array_equal(ids[:k], oids)
        assert all(np.array_equal(a[:k], o) and len(a) == n for a, o in zip(cols, ocols))
        new = val[k:]
        assert np.array_equal(new, info["new"][s]) and len(np.unique(new)) == len(new)
        assert (LC.digit_of(new) == d).all() and not np.isin(new, b.valR).any() and not np.isin(new, b.valS).any()
        if not chosen:                                                     # the other side is unchanged but for the shared keys
            assert np.array_equal(np.sort(new), np.sort(info["shared"])) and len(new) == LC.SHARED
        assert np.array_equal(np.sort(ids), np.arange(n, dtype=U64))        # ids are a permutation
    both = np.intersect1d(c.info["new"]["R"], c.info["new"]["S"])
    assert np.array_equal(both, np.sort(info["shared"])) and len(both) == LC.SHARED
    if side == "both":                                                     # hits and misses of the block's own on both sides
        assert len(info["new"]["R"]) > LC.SHARED and len(info["new"]["S"]) > LC.SHARED
    state, skip = LC.expect(info)
    oR, oS = side in ("R", "both") and extra, side in ("S", "both") and extra
    assert state == (2, 2 if oR else 1, 2 if oS else 1, 1, 1) and skip == (2 if oR else 0, 2 if oS else 0)
    assert LC.phases(info) == 1 + bool(oR) + bool(oS)
    assert LC.expect(info, one_sided=True) == ((2, 2 if oR else 1, 0, 1, 0), (2 if oR else 0, 0))


@pytest.mark.parametrize("table_side", ["S", "R"])
@pytest.mark.parametrize("variant", K.CHAIN_VARIANTS)
def test_chain_overflows_on_both_sides(variant, table_side):
    c = K.chain(16, PATTERN, True, variant, table_side)
    for v in (c.valR, c.valS):
        p = cf_cases.piece_lengths(relation(v), 8)
        print(f"chain {variant} table side {table_side}: n {len(v)} units {p.shape[0]} largest piece {p.max()}")
        assert 2304 <= int(p.max()) <= 2717 and int(p.max()) > LC.CAP
    assert LC.expect(LC.chain_info(c)) == ((2, 2, 2, 1, 1), (2, 2)) and LC.phases(LC.chain_info(c)) == 3


def test_wide_gives_one_row_the_id_two_to_the_32():
    b = base_case("one-unit", 0)
    for side in ("R", "S"):
        c = LC.wide(b, side, 17)
        ids, oids = (c.idR, b.idR) if side == "R" else (c.idS, b.idS)
        assert int(ids[17]) == 1 << 32 and np.array_equal(np.delete(ids, 17), np.delete(oids, 17))
        assert np.array_equal(c.idS if side == "R" else c.idR, b.idS if side == "R" else b.idR)
        assert np.array_equal(c.valR, b.valR) and np.array_equal(c.valS, b.valS)
        assert LC.expect(c.info) == ((0, 0, 0, 2, 2), (0, 0)) and LC.phases(c.info) == 2
    # an overflow of S beside a wide id of R: bit 0 wins in the first attempt; an overflow of R BEFORE a wide id of S: three phases
    s1, r1 = LC.rung(b, "S", 1, PATTERN), LC.rung(b, "R", 1, PATTERN)
    assert LC.expect(LC.wide(s1, "R", 5).info) == ((0, 0, 0, 2, 2), (0, 0)) and LC.phases(LC.wide(s1, "R", 5).info) == 2
    assert LC.expect(LC.wide(r1, "S", 5).info) == ((0, 0, 0, 2, 2), (2, 0)) and LC.phases(LC.wide(r1, "S", 5).info) == 3
    assert LC.expect(LC.wide(r1, "R", 5).info, one_sided=True) == ((0, 0, 0, 2, 0), (0, 0))


def ladder_samples():
    b = base_case("one-unit", 1)
    big = base_case("partial-unit", 2)
    yield "full", LC.rung(b, "both", 0, PATTERN)
    yield "S+1", LC.rung(b, "S", 1, PATTERN)
    yield "R+1-partial-unit", LC.rung(big, "R", 1, PATTERN)
    yield "both+1-partial-unit", LC.rung(big, "both", 1, PATTERN)


@pytest.mark.parametrize("name,case", list(ladder_samples()), ids=[n for n, _ in ladder_samples()])
def test_oracle_equals_brute_force_on_the_rungs(name, case):
    """on a sample, and on the block itself with some rows around it (the sample rarely meets the block)"""
    block = np.concatenate([case.info["new"]["R"], case.info["new"]["S"]])
    keepR, keepS = np.flatnonzero(np.isin(case.valR, block)), np.flatnonzero(np.isin(case.valS, block))
    keepR, keepS = np.concatenate([np.arange(100), keepR]), np.concatenate([np.arange(100), keepS])
    rng = np.random.default_rng(3)
    around = K.finish(rng, case.valR[keepR], case.valS[keepS], {"keep_order": True})
    for small in (K.subsample(case), around):
        fast, slow = K.Oracle(small), K.BruteForce(small)
        assert fast.pair_count() == slow.pair_count() > 0
        for anti in (False, True):
            assert np.array_equal(fast.semi_ids(anti), slow.semi_ids(anti))
        assert np.array_equal(fast.s_only(), slow.s_only()) and fast.join_sums(2) == slow.join_sums(2)
        for w in (None, 0):
            a, b = fast.mult(len(small.valR), w), slow.mult(len(small.valR), w)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1]
        ops = [K.AGG_SUM, K.AGG_MIN_I64, K.AGG_MAX_U64]
        for got, exp in ((fast.groups(ops), slow.groups(ops)), (fast.group_join(False, ops[:1], ops[1:2]), slow.group_join(False, ops[:1], ops[1:2])),
                         (fast.group_join(True, ops[:1], ops[1:2]), slow.group_join(True, ops[:1], ops[1:2]))):
            flat = lambda t: [a for x in t for a in (x if isinstance(x, list) else [x])]
            for a, b in zip(flat(got), flat(exp)):
                assert np.array_equal(a, b)
    assert 0 < len(K.Oracle(around).semi_ids(False)) and 0 < len(K.Oracle(around).semi_ids(True))
