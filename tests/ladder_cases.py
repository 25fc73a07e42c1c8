"""Inputs for the repeat ladder of partition_and_join (rhj_api.hip), shared by test_ladder_cases.py (CPU: the builders
are what they claim) and test_gpu_ladder.py.  numpy only.

Under "partition.narrow" 2, "partition.countfree" 1 and Opts(2, 8, 8) a relation of at most 4096 * 1024 rows is cut into pass-1
units of L = 4096 tuples (cf_cases.unit_len), and the run of one pass-1 digit -- the low 8 bits of mix64(value) -- inside one unit, a
"piece", has a region of cap = cf_cases.cap(4096, 8) = 64 slots.  64 rows of one digit in one unit fit; the 65th raises the side's
overflow bit and the call partitions that side again with exact cursors.

rung(base, side, extra)   a keyed_table_cases.Case with a block of distinct fresh keys of ONE pass-1 digit d appended to `side` ("R",
                          "S" or "both"), so that the piece of d in the side's LAST unit -- the partial one, where the relation has
                          more than one -- holds exactly cap + extra rows: extra 0 is a full region, extra 1 is one too many.  SHARED
                          of the new keys go to the other side too (on "both": to both), so the block has hits, misses and groups of
                          its own.  ids stay a permutation, the columns stay indexed by id.
wide(case, side, row)     the rowID of one row becomes 2^32: the narrow format cannot hold it, the call runs again at 16 bytes.  The
                          id indexes nothing any more, so this is for the calls whose contract reads no column and no array by it.
expect(info)              the state words the call must report and the back-off words the context is left with."""
import numpy as np

import cf_cases
import keyed_table_cases as K
from radixhashjoin_amd import mix64, unmix64

U64 = np.uint64
B1 = 8                                                                     # pass-1 bits of Opts(2, 8, 8)
CAP = cf_cases.cap(cf_cases.TILE, B1)                                      # 64
SHARED = 10
WIDE_ID = U64(1 << 32)
STATE = ("last.narrow", "last.countfree_R", "last.countfree_S", "last.cols_R", "last.cols_S")


def digit_of(values):
    return (mix64(np.asarray(values, dtype=U64)) & U64((1 << B1) - 1)).astype(np.int64)


def pieces(values):
    """[U, 256] piece lengths of a bare value column (cf_cases.piece_lengths reads the same from a relation)"""
    t = np.empty(len(values), dtype=cf_cases.TUPLE)
    t["key"], t["payload"] = 0, values
    return cf_cases.piece_lengths(t, B1)


def choose_digit(pattern):
    """a pass-1 digit that is neither the all-ones digit (the partition of the empty marker) nor the low byte of the case's pattern"""
    for d in (0x5A, 0x5B, 0x5C):
        if d not in ((1 << B1) - 1, pattern & ((1 << B1) - 1)):
            return d
    raise AssertionError("no digit left")


def _extend(rng, val, ids, cols, new):
    """`new` appended to a side: fresh ids behind the old ones (shuffled), fresh column words at those ids"""
    n, k = len(val), len(new)
    ids = np.concatenate([ids, U64(n) + rng.permutation(k).astype(U64)])
    cols = [np.concatenate([c, rng.integers(0, 1 << 64, k, dtype=U64)]) for c in cols]
    return np.concatenate([val, new]).astype(U64), ids, cols


def rung(base, side, extra, pattern=0xBEEF, seed=0):
    """-> the Case with info = {"side", "extra", "digit", "unit": {"R", "S"} (the unit that holds the block), "over": {"R", "S"},
    "new": {"R", "S"} (the keys appended), "shared", "wide": None}"""
    assert side in ("R", "S", "both") and extra in (0, 1)
    rng = np.random.default_rng(977 * seed + 31 * extra + ("R", "S", "both").index(side))
    d = choose_digit(pattern)
    chosen = {"R": side in ("R", "both"), "S": side in ("S", "both")}
    old = {"R": base.valR, "S": base.valS}
    need = {}
    for s in ("R", "S"):
        n = len(old[s])
        L = cf_cases.unit_len(n + CAP + 1)
        assert L == cf_cases.TILE == cf_cases.unit_len(n) and n % L != 0
        here = int((digit_of(old[s][n // L * L:]) == d).sum())              # rows of digit d that the last unit holds already
        need[s] = CAP + extra - here if chosen[s] else SHARED
        assert need[s] >= SHARED and n % L + need[s] <= L                   # the block stays inside the last unit
    total = need["R"] + need["S"] - SHARED
    x = rng.choice(1 << 40, total, replace=False).astype(U64) + U64(1 << 41)
    fresh = unmix64((x << U64(B1)) | U64(d))
    assert not np.isin(fresh, base.valR).any() and not np.isin(fresh, base.valS).any()
    new = {"R": rng.permutation(fresh[:need["R"]]), "S": rng.permutation(fresh[need["R"] - SHARED:])}
    vR, iR, cR = _extend(rng, base.valR, base.idR, base.colsR, new["R"])
    vS, iS, cS = _extend(rng, base.valS, base.idS, base.colsS, new["S"])
    info = dict(base.info, side=side, extra=extra, digit=d, wide=None, shared=fresh[need["R"] - SHARED: need["R"]], new=new,
                unit={"R": (len(vR) - 1) // cf_cases.TILE, "S": (len(vS) - 1) // cf_cases.TILE},
                over={s: bool(chosen[s] and extra) for s in ("R", "S")})
    return K.Case(vR, iR, vS, iS, cR, cS, info)


def chain_info(case):
    """a K.chain case as a rung: both sides overflow (their partition's rows share one pass-1 digit)"""
    return dict(case.info, over={"R": True, "S": True}, wide=None)


def plain_info(case):
    return dict(case.info, over={"R": False, "S": False}, wide=None)


def wide(case, side, row):
    """the rowID of row `row` of `side` becomes 2^32 (info["wide"] = side, info["wide_row"] = row); needs explicit ids"""
    assert side in ("R", "S")
    ids = (case.idR if side == "R" else case.idS).copy()
    ids[row] = WIDE_ID
    info = dict(case.info, wide=side, wide_row=row)
    if "over" not in info:
        info["over"] = {"R": False, "S": False}
    return case._replace(info=info, **{"idR" if side == "R" else "idS": ids})


def expect(info, one_sided=False):
    """-> (the STATE words of the call, (cf_skip[R], cf_skip[S]) the context is left with), for a call armed with "partition.narrow"
    2 and "partition.countfree" 1 freshly set (no back-off pending), from partition_and_join:
      * a side that overflowed reports 2 and arms its back-off at 1 << 1 = 2 eligible calls; a side that fitted reports 1;
      * a wide rowID ends the call at 16 bytes: narrow 0, both count-free words 0, the columns converted (2).  The flag's bit 0 is
        read before the overflow bits, so an overflow that the same attempt saw arms nothing -- but R is partitioned first and the
        kernels of S return at once while a bit is up, so an overflow of R is seen, and armed, one attempt BEFORE a wide id of S;
      * a one-sided call (a group-by) partitions R alone under R's words and reports 0 in S's."""
    over, w = info["over"], info.get("wide")
    if one_sided:
        over = {"R": over["R"], "S": False}
        assert w != "S"
    if w is None:
        state = (2, 2 if over["R"] else 1, 2 if over["S"] else 1, 1, 1)
        skip = (2 if over["R"] else 0, 2 if over["S"] else 0)
    else:
        state = (0, 0, 0, 2, 2)
        skip = (2 if (w == "S" and over["R"]) else 0, 0)
    if one_sided:
        state = (state[0], state[1], 0, state[3], 0)
    return state, skip


def phases(info, one_sided=False):
    """partition phases of the call (documentation of the rung table; nothing reports it)"""
    over, w = info["over"], info.get("wide")
    oR, oS = over["R"], over["S"] and not one_sided
    if w is None:
        return 1 + int(oR) + int(oS)
    return 2 + int(w == "S" and oR)
