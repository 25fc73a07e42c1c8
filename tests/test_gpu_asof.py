"""GPU suite: the as-of join entry (rhj_asof_cols_dev, Engine.asof_join_columns) against the numpy oracle of tests/asof_cases.py.
Every comparison is exact and aligned with R.  Every output lies between guard words, the inputs are compared before and after, and
"last.asof_*" are asserted after each call.

Under the automatic "sort.max_units" every input below 2048 tiles is cut into units of one tile; the carry across the tiles of a unit
runs under "sort.max_units" 1 and 3, and the large case has more units than the device has CUs."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import asof_cases as AC
from radixhashjoin_amd import Engine, RhjError
from radixhashjoin_amd.binding import RHJ_E_INVALID

pytestmark = pytest.mark.gpu

GUARD, NGUARD = AC.GUARD, AC.NGUARD
NO = int(AC.NO_ROW)
ONES, TOP = (1 << 64) - 1, 1 << 63
I64, FWD, STRICT, TOL = AC.ASOF_I64, AC.ASOF_FORWARD, AC.ASOF_STRICT, AC.ASOF_TOLERANCE
BIG = 3_000_000


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def T(eng):
    t = eng.info("asof.tile_rows")
    assert t >= 128 and t % 64 == 0
    return t


class Array:
    """n words in HBM at an offset of `off` words into a buffer of off + n + NGUARD words, guard words before and behind (and in the
    n words themselves until something is written there)"""
    def __init__(self, eng, n, off=0, data=None):
        self.n, self.off = n, off
        host = np.full(off + n + NGUARD, GUARD, dtype=np.uint64)
        if data is not None:
            host[off:off + n] = data
        self.buf = eng.to_device(host)
        self.ptr = self.buf.ptr + 8 * off

    def read(self):
        host = self.buf.to_numpy(np.uint64, self.off + self.n + NGUARD)
        assert (host[:self.off] == GUARD).all() and (host[self.off + self.n:] == GUARD).all(), "a word outside the array was written"
        return host[self.off:self.off + self.n]

    def free(self):
        self.buf.free()


@contextlib.contextmanager
def option(eng, name, value):
    eng.set_option(name, value)
    try:
        yield
    finally:
        eng.set_option(name, -1)


def units_of(n, T, max_units=2048):
    tiles = -(-n // T)
    per = -(-tiles // max_units)
    return -(-n // (per * T)) if n else 0


def check_info(eng, nR, nS, T, by, matched, max_units=2048):
    got = {name: eng.info("last." + name) for name in ("asof_units", "asof_sorts", "asof_matched", "join_kernel", "sort_bits", "sort_passes",
                                                       "sort_units", "topk_bits", "topk_passes", "topk_candidates", "topk_sorted_rows",
                                                       "window_units", "window_sorts", "window_partitions")}
    ran = nR > 0 and nS > 0
    assert got["join_kernel"] == -1
    assert got["sort_bits"] == got["sort_passes"] == got["sort_units"] == 0, got
    assert got["topk_bits"] == got["topk_passes"] == got["topk_candidates"] == got["topk_sorted_rows"] == 0, got
    assert got["window_units"] == got["window_sorts"] == got["window_partitions"] == 0, got
    assert got["asof_units"] == (units_of(nR + nS, T, max_units) if ran else 0), got
    assert got["asof_sorts"] == ((2 if by else 1) if ran else 0) and got["asof_matched"] == matched, got


class Tables:
    """the four input columns of a case in HBM, between guard words; read back and compared before and after every call"""
    def __init__(self, eng, byR, onR, byS, onS):
        self.eng = eng
        self.host = {"byR": byR, "onR": onR, "byS": byS, "onS": onS}
        self.nR, self.nS = len(onR), len(onS)
        self.dev = {k: Array(eng, len(a), off=1 + i, data=a) for i, (k, a) in enumerate(self.host.items()) if a is not None}

    def ptr(self, name):
        return self.dev[name].ptr if name in self.dev else None

    def check(self):
        for k, a in self.dev.items():
            assert np.array_equal(a.read(), self.host[k]), f"the input column {k} was modified"

    def close(self):
        self.check()
        for a in self.dev.values():
            a.free()


def call(eng, T, tab, flags, tol=0, max_units=2048, twice=False, expect=None):
    """one rhj_asof_cols_dev call on the tables' columns against the oracle (expect: its answer, where a test has it already);
    returns the rows"""
    h = tab.host
    want, matched = expect if expect is not None else AC.oracle(h["byR"], h["onR"], h["byS"], h["onS"], flags, tol)
    out = Array(eng, tab.nR, off=3)
    runs = []
    for _ in range(2 if twice else 1):
        tab.check()                                                          # the inputs before and after every call
        got = eng.asof_cols_dev(tab.ptr("byR"), tab.ptr("onR"), tab.nR, tab.ptr("byS"), tab.ptr("onS"), tab.nS, flags, tol, out.ptr)
        tab.check()
        assert got == matched, (got, matched, flags, tol)
        check_info(eng, tab.nR, tab.nS, T, h["byR"] is not None, matched, max_units)
        runs.append(out.read().copy())
    bad = np.nonzero(runs[0] != want)[0]
    assert len(bad) == 0, (f"flags {flags}, tolerance {tol}, nR {tab.nR}, nS {tab.nS}: {len(bad)} rows differ, first at row {bad[:5].tolist()}: "
                           f"{runs[0][bad[:5]].tolist()} for {want[bad[:5]].tolist()}")
    if twice:
        assert np.array_equal(runs[0], runs[1]), "two runs differ"
    out.free()
    return runs[0]


def small_sizes(T):
    return {"0": 0, "1": 1, "63": 63, "64": 64, "65": 65, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1}


@pytest.mark.parametrize("shape", AC.SHAPES + ("none",))
def test_every_small_size_split_and_partition_shape(eng, T, shape):
    """nR + nS at the wave and tile edges, split roughly in half, with one row of S, one row of R, no S and no R; the `on` kinds and
    the 8 flag combinations rotate over the grid (shape "none": no `by` columns)"""
    turn = 0
    for n in small_sizes(T).values():
        for nR, nS in AC.splits(n):
            kind, flags = AC.ONS[turn % 4], AC.FLAGS8[(turn // 4 + turn) % 8]
            turn += 1
            tab = Tables(eng, *AC.make_tables(shape if shape != "none" else "one", kind, nR, nS, T, seed=turn, by=shape != "none"))
            call(eng, T, tab, flags)
            call(eng, T, tab, flags ^ (FWD | STRICT))
            tab.close()
    assert turn >= 8 * 4


def restart_tables(T, forward):
    """Partitions laid out by their sorted positions.  In sorted order a partition is [a rows of R, b of S, c of R, d of S]: its first
    a rows of R have no candidate, and the partition before it ends in rows of S.  Partition boundaries fall at position 64 (a wave
    boundary), T (a tile boundary; a unit boundary under the automatic units), 2T and 4T (the unit boundaries under "sort.max_units" 3:
    6T positions are 6 tiles, cut into 3 units of 2T; tile boundaries inside the one unit of "sort.max_units" 1).  At 2T a partition
    that ends in rows of S meets one that holds only rows of R, at 4T one that holds only rows of S meets one that starts with rows
    of R.  The `on` words of a partition are distinct and ascend along that order (forward: descend, the sort is descending there).
    Returns the four columns, which rows of R head their partition, and the sorted positions at which partitions start."""
    parts = [(10, 20, 14, 20), (30, T - 64 - 90, 40, 20), (7, T - 100, 3, 90), (100, 0, 0, 0), (0, 0, 0, 2 * T - 100), (50, T, 5, T - 55)]
    starts = np.cumsum([sum(p) for p in parts]).tolist()
    assert starts == [64, T, 2 * T, 2 * T + 100, 4 * T, 6 * T]
    by, on, side, first = [], [], [], []
    for k, (a, b, c, d) in enumerate(parts):
        size = a + b + c + d
        pos = np.arange(size, dtype=np.uint64)
        by.append(np.full(size, ONES if k == len(parts) - 1 else 3 * k + 1, dtype=np.uint64))       # ascending words, the last all ones
        on.append(np.uint64(1000) * np.uint64(k) + (np.uint64(size) - pos if forward else pos))
        side.append(np.repeat([0, 1, 0, 1], [a, b, c, d]))                                           # 0: R
        first.append(np.repeat([1, 0, 0, 0], [a, b, c, d]))                                          # the R rows at the partition's head
    by, on, side, first = (np.concatenate(x) for x in (by, on, side, first))
    order = np.random.default_rng(17).permutation(len(by))                                           # the tables are not sorted
    by, on, side, first = by[order], on[order], side[order], first[order]
    r, s = side == 0, side == 1
    return (by[r], on[r], by[s], on[s]), first[r] == 1, starts[:-1]


@pytest.mark.parametrize("forward", [False, True])
def test_the_scan_restarts_at_partition_heads(eng, T, forward):
    """rows of R at the head of a partition read RHJ_NO_ROW, not the last row of S of the partition before -- at a wave boundary, a
    tile boundary and a unit boundary; partitions with only rows of R and only rows of S"""
    cols, heads, starts = restart_tables(T, forward)
    tab = Tables(eng, *cols)
    n = tab.nR + tab.nS
    assert heads.sum() == 10 + 30 + 7 + 100 + 50 and n == 6 * T
    for max_units in (2048, 1, 3):
        with option(eng, "sort.max_units", max_units):
            for flags in (0, I64, STRICT, STRICT | I64):
                rows = call(eng, T, tab, flags | (FWD if forward else 0), max_units=max_units)
                U = eng.info("last.asof_units")                              # the cut the call used: U units of L positions
                L = -(-(n // T) // U) * T
                assert U == {2048: 6, 1: 1, 3: 3}[max_units] and U * L == n
                cuts = [k * L for k in range(1, U)]
                if max_units == 3:                                           # a partition starts on every boundary between the multi-tile units
                    assert cuts == [2 * T, 4 * T] and all(c in starts for c in cuts)
                else:                                                        # one-tile units: T, 2T and 4T are unit boundaries; one unit: none is
                    assert set(cuts) >= ({T, 2 * T, 4 * T} if max_units == 2048 else set()) and (max_units != 1 or cuts == [])
                assert (rows[heads] == AC.NO_ROW).all() and (rows[~heads] != AC.NO_ROW).all()
                other = call(eng, T, tab, flags | (0 if forward else FWD), max_units=max_units)      # the mirrored direction on the same layout
                assert (other == AC.NO_ROW).sum() == 100                                             # there only the partition without S has none
    tab.close()


@pytest.mark.parametrize("by", [False, True])
def test_ties_in_S(eng, T, by):
    """S holds runs of equal (by, on) of length 2, 64, 65 and T + 1 that cross tiles: backward returns the largest index of the run,
    forward the smallest, and under STRICT a row of R whose `on` equals the run's skips the whole run"""
    runs = {0: T - 40, 10: 2, 20: 64, 30: 65, 40: T + 1}
    onS = np.repeat(np.array(list(runs), dtype=np.uint64), list(runs.values()))
    onR = np.repeat(np.arange(0, 50, 5, dtype=np.uint64), 3)
    rng = np.random.default_rng(23)
    onS, onR = onS[rng.permutation(len(onS))], onR[rng.permutation(len(onR))]
    byR = byS = None
    if by:                                                                   # two partitions with the same rows, interleaved
        onS, onR = np.concatenate([onS, onS]), np.concatenate([onR, onR])
        byS, byR = np.repeat(np.array([TOP, 5], dtype=np.uint64), len(onS) // 2), np.repeat(np.array([TOP, 5], dtype=np.uint64), len(onR) // 2)
        pS, pR = rng.permutation(len(onS)), rng.permutation(len(onR))
        onS, byS, onR, byR = onS[pS], byS[pS], onR[pR], byR[pR]
    tab = Tables(eng, byR, onR, byS, onS)

    def run_of(word, i):
        return np.nonzero((onS == np.uint64(word)) & ((byS == byR[i]) if by else True))[0]

    for max_units in (2048, 1):
        with option(eng, "sort.max_units", max_units):
            for view in (0, I64):
                got = {f: call(eng, T, tab, f | view, max_units=max_units) for f in (0, FWD, STRICT, FWD | STRICT)}
                for i, x in enumerate(onR.tolist()):
                    at, below, above = x - x % 10, x - x % 10 - (10 if x % 10 == 0 else 0), x - x % 10 + 10
                    assert int(got[0][i]) == run_of(at, i).max()
                    assert int(got[STRICT][i]) == (run_of(below, i).max() if below >= 0 else NO)
                    assert int(got[FWD][i]) == (run_of(at if x % 10 == 0 else above, i).min() if x <= 40 else NO)
                    assert int(got[FWD | STRICT][i]) == (run_of(above, i).min() if above <= 40 else NO)
    tab.close()


@pytest.mark.parametrize("shape", ["none", "runs64"])
def test_the_extreme_words_in_both_views_and_directions(eng, T, shape):
    n = 2 * T + 1
    tab = Tables(eng, *AC.make_tables("runs64", "extremes", n - n // 3, n // 3, T, by=shape != "none"))
    for flags in AC.FLAGS8:
        call(eng, T, tab, flags)
    tab.close()


def test_tolerance(eng, T):
    u = lambda *x: np.array(x, dtype=np.uint64)
    # S holds one row at 1000: distances 0, tol, tol + 1 on both sides of it
    tol = 37
    tab = Tables(eng, None, u(1000, 1000 + tol, 1000 + tol + 1, 1000 - tol, 1000 - tol - 1), None, u(1000))
    assert call(eng, T, tab, TOL, tol).tolist() == [0, 0, NO, NO, NO]
    assert call(eng, T, tab, TOL | FWD, tol).tolist() == [0, NO, NO, 0, NO]
    assert call(eng, T, tab, TOL | STRICT, tol).tolist() == [NO, 0, NO, NO, NO]
    assert call(eng, T, tab, TOL, 0).tolist() == [0, NO, NO, NO, NO]                      # equal words only
    assert call(eng, T, tab, TOL | STRICT, 0).tolist() == [NO] * 5                        # legal, and matches nothing
    assert call(eng, T, tab, TOL | FWD | STRICT, 0).tolist() == [NO] * 5
    assert call(eng, T, tab, TOL, ONES).tolist() == [0, 0, 0, NO, NO]
    assert call(eng, T, tab, 0, 0).tolist() == [0, 0, 0, NO, NO]                          # ignored without the flag
    assert call(eng, T, tab, FWD, 1).tolist() == [0, NO, NO, 0, 0]
    tab.close()
    # INT64_MIN and INT64_MAX are 2^64 - 1 apart; unsigned, 0 and all ones are
    for flags, lo, hi in ((I64, TOP, TOP - 1), (0, 0, ONES)):
        tab = Tables(eng, None, u(hi), None, u(lo))
        assert call(eng, T, tab, flags | TOL, ONES - 1).tolist() == [NO] and call(eng, T, tab, flags | TOL, ONES).tolist() == [0]
        assert call(eng, T, tab, flags, 0).tolist() == [0]
        tab.close()
        tab = Tables(eng, None, u(lo), None, u(hi))
        assert call(eng, T, tab, flags | TOL | FWD, ONES - 1).tolist() == [NO] and call(eng, T, tab, flags | TOL | FWD, ONES).tolist() == [0]
        assert call(eng, T, tab, flags | TOL, ONES).tolist() == [NO]
        tab.close()
    # many rows with near `on` words around 0 and around 1 << 63, so that both views have pairs across their wrap
    rng = np.random.default_rng(29)
    n = 2 * T + 1
    base = u(0, TOP)[rng.integers(0, 2, n)]
    on = base + rng.integers(-200, 200, n).astype(np.int64).view(np.uint64)
    part = AC.WC.make_part("runs64", n, T)
    tab = Tables(eng, part[:n // 2], on[:n // 2], part[n // 2:], on[n // 2:])
    for flags in AC.FLAGS8:
        for tol in (0, 1, 7, 150, TOP - 1, TOP, ONES):
            call(eng, T, tab, flags | TOL, tol)
    tab.close()


@pytest.mark.parametrize("max_units", [1, 3])
def test_several_tiles_per_unit(eng, T, max_units):
    n = 70_000
    tab = Tables(eng, *AC.make_tables("zipf", "sixteen", n // 2, n - n // 2, T))
    with option(eng, "sort.max_units", max_units):
        for flags in (I64, FWD, STRICT | I64, FWD | STRICT):
            call(eng, T, tab, flags, max_units=max_units)
    tab.close()


@pytest.mark.parametrize("shape", ["one", "zipf"])
def test_three_million_rows(eng, T, shape):
    """more units than CUs; one partition -- the carry crosses every unit -- and a few thousand Zipf partitions"""
    n = BIG
    assert units_of(n, T) > 512
    tab = Tables(eng, *AC.make_tables(shape, "sixteen" if shape == "zipf" else "distinct", n // 2, n - n // 2, T, groups=3000))
    if shape == "zipf":
        assert len(np.unique(np.concatenate([tab.host["byR"], tab.host["byS"]]))) == 3000
    call(eng, T, tab, I64 if shape == "one" else FWD | STRICT)
    tab.close()


def test_two_runs_are_bit_identical(eng, T):
    n = 2 * T + 1
    tab = Tables(eng, *AC.make_tables("zipf", "sixteen", n // 2, n - n // 2, T))
    call(eng, T, tab, 0, twice=True)
    call(eng, T, tab, FWD | I64, twice=True)
    tab.close()


def test_release_workspace_and_call_again(eng, T):
    n = T + 1
    tab = Tables(eng, *AC.make_tables("geometric", "sixteen", n // 2, n - n // 2, T))
    call(eng, T, tab, 0)
    eng.release_workspace()
    call(eng, T, tab, FWD)
    eng.release_workspace()
    call(eng, T, tab, STRICT | I64)
    tab.close()


def test_other_calls_reset_the_asof_names_and_an_asof_call_the_window_names(eng, T):
    tab = Tables(eng, *AC.make_tables("runs64", "sixteen", 40, 25, T))
    call(eng, T, tab, 0)
    assert eng.info("last.asof_units") == 1 and eng.info("last.asof_sorts") == 2 and eng.info("last.asof_matched") > 0
    out = Array(eng, 40)
    eng.sort_cols_dev(tab.ptr("onR"), None, 40, 0, None, out.ptr)
    assert eng.info("last.asof_units") == eng.info("last.asof_sorts") == eng.info("last.asof_matched") == 0
    eng.window_cols_dev(tab.ptr("byR"), None, 40, 0, [0], None, None, [out.ptr])
    assert eng.info("last.window_units") == 1 and eng.info("last.window_sorts") == 1
    assert eng.info("last.asof_units") == eng.info("last.asof_sorts") == eng.info("last.asof_matched") == 0
    call(eng, T, tab, FWD)                                                   # (check_info: the window names are 0 again)
    out.free()
    tab.close()


def test_invalid_arguments_are_refused_before_any_launch(eng, T):
    tab = Tables(eng, *AC.make_tables("runs64", "sixteen", 40, 25, T))
    out = Array(eng, 40, off=2)
    bR, oR, bS, oS, o = tab.ptr("byR"), tab.ptr("onR"), tab.ptr("byS"), tab.ptr("onS"), out.ptr
    matched = C.c_uint64(77)
    # (d_byR, d_onR, nR, d_byS, d_onS, nS, flags, tolerance, d_out_rowS): the word the message must hold
    bad = [((bR, oR, 40, bS, oS, 25, 16, 0, o), "flags"),
           ((bR, oR, 40, bS, oS, 25, 0x80000000, 0, o), "flags"),
           ((None, None, 0, None, None, 0, 32, 0, None), "flags"),                    # ... also with both tables empty
           ((bR, None, 40, bS, oS, 25, 0, 0, o), "d_onR"),
           ((bR, None, 40, bS, None, 0, 0, 0, o), "d_onR"),
           ((bR, oR, 40, bS, None, 25, 0, 0, o), "d_onS"),
           ((None, None, 0, bS, None, 25, 0, 0, None), "d_onS"),
           ((bR, oR, 40, bS, oS, 25, 0, 0, None), "d_out_rowS"),
           ((bR, oR, 40, None, None, 0, 0, 0, None), "d_out_rowS"),
           ((None, oR, 40, bS, oS, 25, 0, 0, o), "d_byR"),
           ((bR, oR, 40, None, oS, 25, TOL, 5, o), "d_byS")]
    for args, word in bad:
        rc = eng.lib.rhj_asof_cols_dev(eng.ctx, *args, C.byref(matched))
        assert rc == RHJ_E_INVALID, (rc, word)
        with pytest.raises(RhjError, match=r"rhj_asof_cols_dev: .*" + word) as err:
            eng._chk(rc)
        assert err.value.code == RHJ_E_INVALID
        assert matched.value == 77                                           # out_matched is untouched
    assert (out.read() == GUARD).all()                                       # nothing was launched
    # no rows of R: no launch, whatever else is NULL; a one-sided `by` is fine while a table is empty
    assert eng.lib.rhj_asof_cols_dev(eng.ctx, None, None, 0, bS, oS, 25, 0, 0, None, C.byref(matched)) == 0 and matched.value == 0
    check_info(eng, 0, 25, T, True, 0)
    matched.value = 77
    assert eng.lib.rhj_asof_cols_dev(eng.ctx, bR, oR, 40, None, None, 0, FWD, 0, o, C.byref(matched)) == 0 and matched.value == 0
    check_info(eng, 40, 0, T, True, 0)
    assert (out.read() == AC.NO_ROW).all()                                   # the fill launch
    assert eng.lib.rhj_asof_cols_dev(eng.ctx, bR, oR, 40, bS, oS, 25, I64, 0, o, None) == 0                    # out_matched NULL
    want, m = AC.oracle(*[tab.host[k] for k in ("byR", "onR", "byS", "onS")], I64)
    assert np.array_equal(out.read(), want) and eng.info("last.asof_matched") == m
    out.free()
    tab.close()


def as_i64(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def test_asof_join_columns(eng, T):
    """a two-tensor `by` on each side against a hand-packed single word, two value tensors with a fill, unsigned=True, empty tensors;
    the inputs are left unmodified"""
    nR, nS = T + 7, T - 3
    rng = np.random.default_rng(31)
    aR, aS = rng.integers(-3, 4, nR).astype(np.int64), rng.integers(-3, 3, nS).astype(np.int64)
    bR, bS = rng.integers(0, 5, nR).astype(np.int64) * (1 << 40), rng.integers(0, 5, nS).astype(np.int64) * (1 << 40)
    pack = lambda a, b: (a.view(np.uint64) << np.uint64(3)) ^ (b.view(np.uint64) >> np.uint64(40))      # one word per distinct (a, b)
    on = AC.make_on("extremes", nR + nS)
    onR, onS = on[:nR], on[nR:]
    v0, v1 = rng.integers(-1 << 62, 1 << 62, nS).astype(np.int64), np.arange(nS, dtype=np.int64)
    tens = [torch.from_numpy(x).cuda() for x in (aR, bR, aS, bS, v0, v1)] + [as_i64(onR), as_i64(onS)]
    taR, tbR, taS, tbS, tv0, tv1, tonR, tonS = tens
    keep = [t.clone() for t in tens]
    fill = [-12345, 7]
    for kw, flags, tol in (({}, I64, 0), ({"direction": "forward", "allow_exact_matches": False}, I64 | FWD | STRICT, 0),
                           ({"unsigned": True, "tolerance": 1}, TOL, 1), ({"unsigned": True, "direction": "forward"}, FWD, 0)):
        idx, matched, values = eng.asof_join_columns(tonR, tonS, [taR, tbR], [taS, tbS], [tv0, tv1], fill=fill, **kw)
        want, m = AC.oracle(pack(aR, bR), onR, pack(aS, bS), onS, flags, tol)
        assert idx.dtype == torch.int64 and len(idx) == nR and matched == m and 0 < m < nR
        assert np.array_equal(idx.cpu().numpy().view(np.uint64), want)
        there = want != AC.NO_ROW
        for g, v, f in zip(values, (v0, v1), fill):
            exp = np.full(nR, f, dtype=np.int64)
            exp[there] = v[want[there].astype(np.int64)]
            assert g.dtype == torch.int64 and np.array_equal(g.cpu().numpy(), exp)
    # a single tensor per side, and none; no value tensors
    idx, matched, values = eng.asof_join_columns(tonR, tonS, taR, taS)
    want, m = AC.oracle(aR.view(np.uint64), onR, aS.view(np.uint64), onS, I64)
    assert np.array_equal(idx.cpu().numpy().view(np.uint64), want) and matched == m and values == []
    idx, matched, _ = eng.asof_join_columns(tonR, tonS, direction="forward")
    want, m = AC.oracle(None, onR, None, onS, I64 | FWD)
    assert np.array_equal(idx.cpu().numpy().view(np.uint64), want) and matched == m
    for t, k in zip(tens, keep):
        assert torch.equal(t, k)
    empty = torch.empty(0, dtype=torch.int64, device="cuda")
    idx, matched, values = eng.asof_join_columns(empty, tonS, empty, taS, [tv0])
    assert len(idx) == 0 and matched == 0 and [len(v) for v in values] == [0]
    idx, matched, values = eng.asof_join_columns(tonR, empty, taR, empty, [empty], fill=9)
    assert (idx == -1).all() and len(idx) == nR and matched == 0 and (values[0] == 9).all()
    idx, matched, values = eng.asof_join_columns(empty, empty)
    assert len(idx) == 0 and matched == 0 and values == []
