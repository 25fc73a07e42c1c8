"""CPU checks of tests/cf_cases.py: the builders are what they claim, seen through mix64 as the library sees them, and predict()
says what the GPU tests then demand.  No GPU, no library call beyond the numpy mix64 / unmix64."""
import numpy as np
import pytest

import cf_cases as CF
from radixhashjoin_amd import mix64, unmix64

CUS = 256                                                     # the MI355X; a device with more than 2^b1 units tries no pass 2


def test_geometry_restated():
    assert [CF.unit_len(n) for n in (1, 4096, 4097, 1 << 22, (1 << 22) + 1, 5_000_000, 10**9)] == \
        [4096, 4096, 4096, 4096, 8192, 8192, 978_944]
    assert [CF.units(n) for n in (3 * 4096 + 33, 70_000, (1 << 20) + 17, 4_194_299, 4_500_031, 5_000_000)] == [4, 18, 257, 1024, 550, 611]
    assert (CF.cap(4096, 8), CF.cap(8192, 8), CF.cap(978_944, 8)) == (64, 96, 4448)          # DESIGN 4.10's figures
    assert (CF.cap(4096, 1), CF.cap(4096, 3), CF.cap(4096, 4), CF.cap(4096, 5)) == (2528, 768, 448, 256)
    assert (CF.cap2(1 << 20, 8, 8), CF.cap2(10**9, 8, 8), CF.cap2(300_000, 8, 8)) == (64, 16_512, 32)      # DESIGN 4.20's
    assert CF.cap2(5_000_000, 8, 8) == 192 and CF.cap2(4 * 512, 8, 1) == 32
    x = np.random.default_rng(0).integers(0, 1 << 63, 1000, dtype=np.uint64)
    assert np.array_equal(mix64(unmix64(x)), x)


@pytest.mark.parametrize("n,nS", [(3 * 4096 + 33, 5 * 4096 + 1), (70_000, 100_031), ((1 << 20) + 17, (1 << 20) + 17), (4_500_031, 70_000)])
def test_set_lengths(n, nS):
    R, S, info = CF.set_lengths(n, n % 7, nS)
    assert len(np.unique(R["payload"])) == n and len(R) == n and len(S) == nS
    for side, t in (("R", R), ("S", S)):
        m, i = len(t), info[side]
        L, U, cap, cap2 = i["L"], i["U"], i["cap"], i["cap2"]
        assert (L, U, cap, cap2) == (CF.unit_len(m), CF.units(m), CF.cap(L, 8), CF.cap2(m, 8, 8))
        lens, whole = CF.piece_lengths(t), m // L
        assert lens.shape == (U, 256) and lens.max() <= cap
        for u in range(whole):                                 # every whole unit carries every special length
            assert set(CF.SPECIAL[L]) <= set(lens[u].tolist()), (u, sorted(set(CF.SPECIAL[L]) - set(lens[u].tolist())))
        # the marked buckets: empty pieces in front, at the end, and all but every 7th, which is full
        front, back, seventh = lens[:, CF.MARK_FRONT], lens[:, CF.MARK_BACK], lens[:, CF.MARK_SEVENTH]
        assert not front[:5].any() and not back[max(U - 5, 0):].any()
        if U > 5:
            assert (whole <= 5 or front[5] > 0) and back[U - 6] > 0
        else:
            assert front.sum() == 0 and back.sum() == 0       # wholly empty buckets
        assert np.array_equal(seventh[:whole], np.where(np.arange(whole) % 7 == 0, cap, 0)) and not seventh[whole:].any()
        # the edge bucket: a piece starts exactly at slot 1024 and another at slot 4096 of the bucket's dense sequence
        pre = np.concatenate([[0], np.cumsum(lens[:, CF.MARK_EDGE])])
        for slot, u in i["edge"].items():
            feasible = -(-slot // cap) < whole
            assert (u is not None) == feasible, (slot, u)
            if u is not None:
                assert pre[u] == slot and lens[u, CF.MARK_EDGE] > 0 and lens[u - 1, CF.MARK_EDGE] > 0
        # pass 2: nothing above cap2; a bucket of a tile or so has one partition AT cap2 and one empty
        parts = CF.partition_sizes(t)
        assert parts.max() <= cap2
        big = np.flatnonzero(parts.sum(axis=1) >= cap2 + 254)
        assert len(big) > 200 or m <= 1 << 20
        for d in big:
            assert parts[d, d] == cap2 and parts[d, (d + 1) % 256] == 0
        assert CF.predict(t, (8, 8), CUS) == (1, 1)
        assert CF.predict(t, (8, 8), CUS + 1) == (1, 0)
    assert set(info["R" if n > nS else "S"]["edge"].values()) != {None} or max(n, nS) < 17 * 4096
    # S stays in R's partitions or in partitions R does not have, and some of it matches
    hR, hS = mix64(R["payload"]), mix64(S["payload"])
    match = np.isin(hS, hR)
    pR = CF.partition_sizes(R).ravel()
    d1, d2 = (hS & np.uint64(255)).astype(np.int64), ((hS >> np.uint64(8)) & np.uint64(255)).astype(np.int64)
    inR = pR[(d1 << 8) + d2] > 0
    assert 0.55 < match[inR].mean() < 0.65 and not match[~inR].any() and inR.mean() > 0.15


def test_set_lengths_covers_the_last_piece_of_a_full_prefix_table():
    """1024 units: every entry of the one-writer pass 2's prefix table is a piece, the walk of the last one ends on the sentinel"""
    assert CF.units(4_194_299) == 1024 and CF.unit_len(4_194_299) == 4096
    f, edge = CF.forced_lengths(4_194_299)
    assert f.shape == (256, 1024) and edge == {1024: 16, 4096: 64}


@pytest.mark.parametrize("side", ["R", "S"])
def test_all_full(side):
    other = "S" if side == "R" else "R"
    for variant in (None, "over2", "over1"):
        R, S, info = CF.all_full(variant, side)
        rels = {"R": R, "S": S}
        assert len(R) == len(S) == CF.FULL_N == 64 * 256 * 64
        assert len(np.unique(mix64(R["payload"]) >> np.uint64(16))) == CF.FULL_N
        live = np.zeros(256, dtype=bool)
        live[CF.FULL_DIGITS] = True
        for name in ((other,) if variant else ("R", "S")):     # the untouched relation(s): every live region exactly full
            lens, parts = CF.piece_lengths(rels[name]), CF.partition_sizes(rels[name])
            assert lens.shape == (256, 256) and (lens[:, live] == 64).all() and not lens[:, ~live].any()
            assert (parts[live] == 64).all() and not parts[~live].any()
            assert int((parts == 0).sum()) == 49_152 and int((parts.sum(axis=1) == 0).sum()) == 192
            assert CF.predict(rels[name], (8, 8), CUS) == (1, 1)
        match = np.isin(mix64(S["payload"]), mix64(R["payload"]))
        assert 0.79 < match.mean() < 0.81
        if variant is None:
            continue
        lens, parts = CF.piece_lengths(rels[side]), CF.partition_sizes(rels[side])
        h = mix64(rels[side]["payload"])
        if variant == "over2":
            assert info["row"] == CF.FULL_N - 1
            assert (lens[:, live] == 64).all() and not lens[:, ~live].any()          # pass 1 as before
            d1, d2 = int(h[-1] & np.uint64(255)), int((h[-1] >> np.uint64(8)) & np.uint64(255))
            assert parts[d1, d2] == 65 and parts[d1, d2 ^ 1] == 63 and d2 >= 192
            assert sorted(np.bincount(parts.ravel())[[0, 63, 64, 65]].tolist()) == [1, 1, 16_382, 49_152]
            # its bucket is 16,384 slots = 4 tiles, the row lies in the last piece: pass 2 sees partition (d1, d2) pass 64 in tile 4
            assert lens[:, d1].sum() == 4 * 4096 and info["row"] // 4096 == 255
            assert CF.predict(rels[side], (8, 8), CUS) == (1, 2)
        else:
            u, a, b = info["row"] // 4096, int(CF.FULL_DIGITS[0]), int(CF.FULL_DIGITS[1])
            assert u == 100 and lens[u, a] == 63 and lens[u, b] == 65 and int(h[info["row"]] & np.uint64(255)) == b
            assert sorted(np.bincount(lens.ravel())[[0, 63, 64, 65]].tolist()) == [1, 1, 64 * 256 - 2, 192 * 256]
            assert CF.predict(rels[side], (8, 8), CUS) == (2, 0)


@pytest.mark.parametrize("dist", ["uniform", "dups"])
def test_plain_and_predict_against_a_plain_count(dist):
    n = 50_000
    R, S = CF.plain(n, dist, 1, n + 999)
    assert len(R) == n and len(S) == n + 999
    assert np.array_equal(np.sort(R["key"]), np.arange(n)) and np.array_equal(np.sort(S["key"]), np.arange(n + 999))
    assert 0.98 < np.isin(S["payload"], R["payload"]).mean() < 1.0
    assert (len(np.unique(R["payload"])) == n) == (dist == "uniform")
    for b1, b2 in ((8, 8), (8, 1), (5, 5), (3, 8), (1, 8)):
        h = mix64(R["payload"]).tolist()
        runs, parts = {}, {}
        for i, x in enumerate(h):                              # predict() restated with dictionaries
            k = (i // 4096, x & ((1 << b1) - 1))
            runs[k] = runs.get(k, 0) + 1
            k = x & ((1 << (b1 + b2)) - 1)
            parts[k] = parts.get(k, 0) + 1
        one = 1 if max(runs.values()) <= CF.cap(4096, b1) else 2
        two = 0 if one == 2 or (1 << b1) < CUS else (1 if max(parts.values()) <= CF.cap2(n, b1, b2) else 2)
        assert CF.predict(R, (b1, b2), CUS) == (one, two)
        assert CF.piece_lengths(R, b1).sum() == n and CF.partition_sizes(R, b1, b2).sum() == n

