"""GPU suite: the range join entries (rhj_range_join_cols_dev, rhj_range_expand_dev, Engine.range_join_csr_columns / range_join_columns /
band_join_columns) against the numpy oracle of tests/range_join_cases.py.  Every comparison is exact: the pairs in order, not as a
set, the offsets, rowsS, and first wherever a row has partners.  Every output lies between guard words, the inputs are compared before
and after, and "last.range_join_*" are asserted after each call.

Under the automatic "sort.max_units" every input below 2048 tiles is cut into units of one tile; the carry across the tiles of a unit
runs under "sort.max_units" 1 and 3, and the large case has more units than the device has CUs.

Every test of this file fails without the feature: each calls one of the two entries."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import range_join_cases as RC
from radixhashjoin_amd import Engine, RhjError
from radixhashjoin_amd.binding import RHJ_E_INVALID, RHJ_E_OVERFLOW, RHJ_OK

pytestmark = pytest.mark.gpu

GUARD, NGUARD = RC.GUARD, RC.NGUARD
ONES, TOP = (1 << 64) - 1, 1 << 63
I64, LO_OPEN, HI_OPEN, BAND = RC.RANGE_I64, RC.RANGE_LO_OPEN, RC.RANGE_HI_OPEN, RC.RANGE_BAND
CLOSED4 = (0, LO_OPEN, HI_OPEN, LO_OPEN | HI_OPEN)
BIG = 1_500_000
ZERO_NAMES = ("sort_bits", "sort_passes", "sort_units", "topk_bits", "topk_passes", "topk_candidates", "topk_sorted_rows", "window_units",
              "window_sorts", "window_partitions", "asof_units", "asof_sorts", "asof_matched", "frame_units", "frame_sorts", "frame_scans",
              "frame_partitions", "frame_range_units", "frame_range_sorts", "frame_range_scans", "frame_range_levels", "frame_range_partitions")
RANGE_NAMES = ("range_join_units", "range_join_sorts", "range_join_pairs", "range_join_expand_tiles")


def u(*x):
    return np.array(x, dtype=np.uint64)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def T(eng):
    t = eng.info("range_join.tile_rows")
    assert t >= 128 and t % 64 == 0
    return t


@pytest.fixture(scope="module")
def E(eng):
    e = eng.info("range_join.expand_tile")
    assert e >= 64
    return e


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


def check_info(eng, units, sorts, pairs, tiles):
    got = {name: eng.info("last." + name) for name in ZERO_NAMES + RANGE_NAMES + ("join_kernel",)}
    assert got["join_kernel"] == -1
    assert all(got[name] == 0 for name in ZERO_NAMES), got
    assert [got[name] for name in RANGE_NAMES] == [units, sorts, pairs, tiles], got


class Tables:
    """the five input columns of a case in HBM, between guard words; read back and compared before and after every call"""
    NAMES = ("byR", "loR", "hiR", "byS", "onS")

    def __init__(self, eng, byR, loR, hiR, byS, onS):
        self.eng = eng
        self.host = dict(zip(self.NAMES, (byR, loR, hiR, byS, onS)))
        self.nR, self.nS = len(loR), len(onS)
        self.dev = {k: Array(eng, len(a), off=1 + i, data=a) for i, (k, a) in enumerate(self.host.items()) if a is not None}
        self.by = byR is not None

    def ptr(self, name):
        return self.dev[name].ptr if name in self.dev else None

    def check(self):
        for k, a in self.dev.items():
            assert np.array_equal(a.read(), self.host[k]), f"the input column {k} was modified"

    def oracle(self, flags, below=0, above=0):
        h = self.host
        return RC.oracle(h["byR"], h["loR"], None if flags & BAND else h["hiR"], h["byS"], h["onS"], flags, below, above)

    def close(self):
        self.check()
        for a in self.dev.values():
            a.free()


class Outputs:
    """the four outputs of a call between guard words; cap None: no pair buffer (count only).  The pair buffer starts at an even
    word: 16-byte aligned."""
    def __init__(self, eng, nR, nS, cap, offsets=True, first=True, rowsS=True):
        self.cap = cap
        self.offsets = Array(eng, nR + 1, off=1) if offsets else None
        self.first = Array(eng, nR, off=2) if first else None
        self.rowsS = Array(eng, nS, off=3) if rowsS else None
        self.pairs = Array(eng, 2 * cap, off=2) if cap is not None else None

    def ptrs(self):
        return [a.ptr if a is not None else None for a in (self.offsets, self.first, self.rowsS, self.pairs)]

    def untouched(self):
        return all((a.read() == GUARD).all() for a in (self.offsets, self.first, self.rowsS, self.pairs) if a is not None)

    def free(self):
        for a in (self.offsets, self.first, self.rowsS, self.pairs):
            if a is not None:
                a.free()


def compare(out, want, nR, nS, what):
    """the outputs of a call (or an expansion: only pairs) against the oracle's answer"""
    offsets, first, defined, rowsS, pairs = want
    total = len(pairs)
    if out.offsets is not None:
        got = out.offsets.read()
        assert np.array_equal(got, offsets) if nR else got[0] == 0, (what, "offsets")
    if out.first is not None and nR:
        got = out.first.read()
        assert np.array_equal(got[defined], first[defined]) and (got <= nS).all(), (what, "first")
        if nS == 0:
            assert (got == 0).all(), (what, "first with no row of S")
    if out.rowsS is not None:
        got = out.rowsS.read()
        assert np.array_equal(got, rowsS) if nR else (got == GUARD).all(), (what, "rowsS")
    if out.pairs is not None:
        got = out.pairs.read().reshape(-1, 2)                                 # (the guard directly behind slot cap - 1 was compared in read())
        k = min(total, out.cap)
        bad = np.nonzero((got[:k] != pairs[:k]).any(axis=1))[0]
        assert len(bad) == 0, f"{what}: {len(bad)} of {k} pairs differ, first at slot {bad[:3].tolist()}: {got[bad[:3]].tolist()} for {pairs[bad[:3]].tolist()}"
        assert (got[k:] == GUARD).all(), (what, "a slot past the result was written")


def call(eng, T, E, tab, flags, below=0, above=0, cap="total", max_units=2048, twice=False, expect=None, offsets=True, first=True, rowsS=True):
    """one rhj_range_join_cols_dev call on the tables' columns against the oracle (expect: its answer, where a test has it already);
    cap: "total", a number of pairs, or None (d_out NULL, capacity 0).  Returns (oracle's answer, total)"""
    want = expect if expect is not None else tab.oracle(flags, below, above)
    total = len(want[4])
    what = f"flags {flags}, below {below}, above {above}, nR {tab.nR}, nS {tab.nS}, cap {cap}"
    if cap == "total":
        cap = total
    runs = []
    for _ in range(2 if twice else 1):
        out = Outputs(eng, tab.nR, tab.nS, cap, offsets, first, rowsS)
        tab.check()                                                          # the inputs before and after every call
        count = C.c_uint64(12345)
        rc = eng.lib.rhj_range_join_cols_dev(eng.ctx, tab.ptr("byR"), tab.ptr("loR"), None if flags & BAND else tab.ptr("hiR"), tab.nR,
                                             tab.ptr("byS"), tab.ptr("onS"), tab.nS, flags, below, above, *out.ptrs(), cap or 0, C.byref(count))
        tab.check()
        assert rc == (RHJ_E_OVERFLOW if cap is not None and total > cap else RHJ_OK), (rc, what, eng.lib.rhj_last_error(eng.ctx))
        assert count.value == total, (count.value, total, what)
        ran = tab.nR > 0 and tab.nS > 0
        check_info(eng, units_of(tab.nR + tab.nS, T, max_units) if ran else 0, (2 if tab.by else 1) if ran else 0, total,
                   -(-min(total, cap or 0) // E))
        compare(out, want, tab.nR, tab.nS, what)
        runs.append([a.read().copy() if a is not None else None for a in (out.offsets, out.rowsS, out.pairs)])
        out.free()
    if twice:
        assert all(np.array_equal(a, b) for a, b in zip(*runs)), "two runs differ"
    return want, total


def small_sizes(T):
    return {"0": 0, "1": 1, "63": 63, "64": 64, "65": 65, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1}


BIG_PARTS = ("one", "edges", "geometric", "zipf", "runsT", "runsT-1", "runsT+1", "none")


@pytest.mark.parametrize("shape", RC.SHAPES + ("none",))
def test_every_small_size_split_and_partition_shape(eng, T, E, shape):
    """nR + nS at the wave and tile edges, split roughly in half, with one row of S, one row of R, no S and no R; the order kinds and
    the 16 flag combinations rotate over the grid (shape "none": no `by` columns).  Where partitions are large and the tables are not
    tiny, the two kinds with few distinct words are left to the interval tests: every row would pair with a large share of S."""
    turn = 0
    for n in small_sizes(T).values():
        for nR, nS in RC.splits(n):
            kinds = RC.ONS[:2] if n > 65 and shape in BIG_PARTS else RC.ONS
            kind, flags = kinds[turn % len(kinds)], RC.FLAGS16[(turn + turn // 16) % 16]
            below, above = ((1 << 52, 1 << 51), (0, 1), (3, 0))[turn % 3]
            turn += 1
            tab = Tables(eng, *RC.make_tables(shape if shape != "none" else "one", kind, nR, nS, T, seed=turn, by=shape != "none", flags=flags))
            call(eng, T, E, tab, flags, below, above)
            call(eng, T, E, tab, flags ^ (LO_OPEN | HI_OPEN), below, above)
            tab.close()
    assert turn >= 8 * 4


def cut_tables(T):
    """6T sorted positions laid out by hand: the word at sorted position p is 10 p, so the words ascend ACROSS partitions and a test
    that forgot `by` would see the next partition's rows qualify.  Partitions start at positions 0, 64, T, 2T and 4T: on a wave
    boundary, and on every boundary between the units of "sort.max_units" 3 (2T and 4T) and on tile boundaries.  Rows of R stand at
    positions 63 / 64 / 65, T - 1 / T / T + 1, 2T and 4T and at every 97th position; the intervals of the named ones reach 200
    positions on, across the cut behind them -- those at 63 and T - 1 are the last row of their partition and have no partner at all.
    Returns the five columns and, per named position, the row of R that stands there."""
    n = 6 * T
    starts = [0, 64, T, 2 * T, 4 * T, n]
    named = [63, 64, 65, T - 1, T, T + 1, 2 * T, 4 * T]
    pos = np.arange(n, dtype=np.uint64)
    by = np.zeros(n, dtype=np.uint64)
    for k in range(5):
        by[starts[k]:starts[k + 1]] = ONES if k == 4 else 3 * k + 1
    isR = (pos % np.uint64(97) == 5)
    isR[named] = True
    word = pos * np.uint64(10)
    reach = np.where(np.isin(pos, named), 200, 30).astype(np.uint64)
    hi = (pos + reach) * np.uint64(10)
    order = np.random.default_rng(17).permutation(n)                          # the tables are not sorted
    r, s = order[isR[order]], order[~isR[order]]
    where = {p: int(np.nonzero(r == p)[0][0]) for p in named}
    return (by[r], word[r], hi[r], by[s], word[s]), where, isR


def test_the_rank_scan_across_waves_tiles_and_units(eng, T, E):
    cols, where, isR = cut_tables(T)
    tab = Tables(eng, *cols)
    n = tab.nR + tab.nS
    assert n == 6 * T
    for max_units in (2048, 1, 3):
        with option(eng, "sort.max_units", max_units):
            for flags in (0, I64, LO_OPEN, HI_OPEN | I64):
                want, _ = call(eng, T, E, tab, flags, max_units=max_units)
                assert eng.info("last.range_join_units") == {2048: 6, 1: 1, 3: 3}[max_units]
                cnt = np.diff(want[0].astype(np.int64))
                assert cnt[where[63]] == 0 and cnt[where[T - 1]] == 0             # nothing leaks out of the partition that ends there
                for p in (64, 65, T, T + 1, 2 * T, 4 * T):                       # 200 positions on, minus the rows of R among them
                    inside = int((~isR[p + 1:p + 201]).sum()) - (1 if flags & HI_OPEN and not isR[p + 200] else 0)
                    assert cnt[where[p]] == inside, (p, flags)
    tab.close()


def interval_tables():
    """Partition 1: rows of R only.  Partition 2: rows of S only.  Partition 3: S holds 100 once, 200 twice, 300 sixty-five times
    and 400, 500; partition 4 (the next `by` word) holds 350 .. 600, words that would qualify for partition 3's intervals.
    R in partition 3: empty (lo > hi), lo == hi on a word of S and between two, covering nothing, covering the whole partition, hi
    beyond the partition's last word, and ends equal to the words S repeats 1, 2 and 65 times."""
    onS3 = np.concatenate([u(100), u(200, 200), np.full(65, 300, dtype=np.uint64), u(400, 500)])
    onS4 = np.arange(350, 601, 10, dtype=np.uint64)
    onS2 = u(1, 2, 3)
    byS = np.concatenate([np.full(len(onS2), 2, dtype=np.uint64), np.full(len(onS3), 3, dtype=np.uint64), np.full(len(onS4), 4, dtype=np.uint64)])
    onS = np.concatenate([onS2, onS3, onS4])
    iv3 = [(300, 200), (200, 200), (250, 250), (201, 299), (0, ONES >> 1), (450, 10_000), (100, 200), (200, 300), (100, 300), (300, 300),
           (100, 100), (99, 101), (300, 400), (501, 502), (0, 99)]
    iv1 = [(0, ONES >> 1), (5, 5)]
    byR = u(*([3] * len(iv3) + [1] * len(iv1)))
    loR = u(*[a for a, _ in iv3 + iv1])
    hiR = u(*[b for _, b in iv3 + iv1])
    rng = np.random.default_rng(19)
    pS, pR = rng.permutation(len(onS)), rng.permutation(len(loR))
    back = np.argsort(pR)                                                      # back[k]: where interval k went
    return (byR[pR], loR[pR], hiR[pR], byS[pS], onS[pS]), back


def test_intervals(eng, T, E):
    cols, back = interval_tables()
    tab = Tables(eng, *cols)
    closed_counts = [0, 2, 0, 0, 70, 1, 3, 67, 68, 65, 1, 1, 66, 0, 0, 0, 0]
    for view in (0, I64):
        for flags in CLOSED4:
            want, _ = call(eng, T, E, tab, flags | view)
            cnt = np.diff(want[0].astype(np.int64))[back]
            if flags == 0:
                assert cnt.tolist() == closed_counts
            assert cnt[0] == 0 and cnt[2] == 0 and cnt[3] == 0                     # empty, between two words, covering nothing
            assert cnt[1] == (2 if flags == 0 else 0)                              # lo == hi: only the closed form has partners
            assert cnt[5] == 1                                                     # 500 only: partition 4's 460 .. 600 do not leak in
            assert cnt[15] == 0 and cnt[16] == 0                                   # a partition without rows of S
    tab.close()


@pytest.mark.parametrize("view", [0, I64])
def test_the_band_at_the_ends_of_the_view(eng, T, E, view):
    """x at the view's minimum, minimum + 1, maximum - 1 and maximum; below / above in {0, 1, 2^63, all ones}; all four closed forms,
    the open ends at the saturated bound included; S holds the four extreme words, two of them twice, and three words in between"""
    vmin = TOP if view else 0
    word = lambda v: (v + vmin) & ONES                                         # the word whose view value is v
    xs = u(word(0), word(1), word(ONES - 1), word(ONES), word(TOP))
    onS = u(word(0), word(0), word(1), word(ONES - 1), word(ONES), word(ONES), word(TOP - 1), word(TOP), word(5))
    tab = Tables(eng, None, xs, xs, None, onS)
    for below in RC.DISTANCES:
        for above in RC.DISTANCES:
            for flags in CLOSED4:
                want, total = call(eng, T, E, tab, flags | view | BAND, below, above)
                assert np.array_equal(want[4], RC.brute(None, xs, None, None, onS, flags | view | BAND, below, above))
    want, total = call(eng, T, E, tab, view | BAND, ONES, ONES)
    assert total == len(xs) * len(onS)                                         # to both ends of the view: every pair
    want, total = call(eng, T, E, tab, view | BAND | LO_OPEN | HI_OPEN, ONES, ONES)
    assert total == len(xs) * 5                                                # ... minus the rows that sit on the saturated ends
    call(eng, T, E, tab, view, 7, 7)                                           # without the bit: [x, x], below and above ignored
    tab.close()


@pytest.mark.parametrize("shape", ["none", "runs64"])
def test_the_extreme_words_in_both_views(eng, T, E, shape):
    n = 2 * T + 1
    for flags in RC.FLAGS16:
        if shape == "none":                                                    # one partition of 192 rows: the extremes tie heavily
            tab = Tables(eng, *RC.make_tables("one", "extremes", 128, 64, T, by=False, flags=flags))
        else:
            tab = Tables(eng, *RC.make_tables("runs64", "extremes", n - n // 3, n // 3, T, flags=flags))
        call(eng, T, E, tab, flags, 1, TOP)
        tab.close()


def expansion_tables(E):
    """One partition.  Row 0 of R has 5E + 3 partners; then a row with one, 3E rows with none, a row with one; then 2E rows whose
    counts alternate 0, 1; then E - 6 rows with one partner each, which brings the running total to 7E - 1, and a row with E + 5: its
    run starts on slot E - 1 of a tile.  R is in this order -- the pairs are ordered by row --, S is shuffled."""
    onS = np.concatenate([np.full(5 * E + 3, 1000, dtype=np.uint64), np.full(E + 5, 3000, dtype=np.uint64), u(2000, 2002, 2004)])
    none, one = (1, 0), (2002, 2002)
    iv = [(1000, 1000), (2000, 2000)] + [none] * (3 * E) + [(2004, 2004)] + [none, one] * E + [one] * (E - 6) + [(3000, 3000)]
    loR, hiR = u(*[a for a, _ in iv]), u(*[b for _, b in iv])
    onS = onS[np.random.default_rng(23).permutation(len(onS))]
    return None, loR, hiR, None, onS


def test_the_expansion_and_every_capacity(eng, T, E):
    tab = Tables(eng, *expansion_tables(E))
    want = tab.oracle(0)
    offsets, total = want[0], len(want[4])
    assert total == 8 * E + 4 and int(offsets[1]) == 5 * E + 3 and int(offsets[-2]) == 7 * E - 1
    assert int(offsets[3 * E + 2]) == int(offsets[2]) == 5 * E + 4                 # 3E rows without partners share one offset
    call(eng, T, E, tab, 0, expect=want, twice=True)
    middle = 2 * E + E // 2 + 1                                                # inside row 0's run, and inside a tile
    assert 0 < middle < int(offsets[1]) and middle % E not in (0, E - 1)
    for cap in (None, 0, 1, total - 1, total, total + 1, middle, 7 * E - 1, 7 * E):
        call(eng, T, E, tab, 0, expect=want, cap=cap)                          # (overflow: the return, the exact count, the prefix, the guard behind it, the CSR)
    tab.close()


def expand(eng, E, arrays, nR, nS, cap, want_pairs=None):
    """rhj_range_expand_dev on three host arrays; returns (rc, count, the pair buffer's words) -- the guards are compared in read()"""
    dev = [Array(eng, len(a), off=1 + i, data=a) for i, a in enumerate(arrays)]
    out = Array(eng, 2 * cap, off=2)
    count = C.c_uint64(777)
    rc = eng.lib.rhj_range_expand_dev(eng.ctx, dev[0].ptr, dev[1].ptr, nR, dev[2].ptr, nS, out.ptr if cap else None, cap, C.byref(count))
    for d, a in zip(dev, arrays):
        assert np.array_equal(d.read(), a), "an input array was modified"
        d.free()
    got = out.read().copy()
    out.free()
    return rc, count.value, got


def test_the_expand_entry(eng, T, E):
    tab = Tables(eng, *RC.make_tables("zipf", "sixteen", 3 * E, 2 * E + 7, T, seed=3))
    want, total = call(eng, T, E, tab, I64)
    offsets, first, defined, rowsS, pairs = want
    nR, nS = tab.nR, tab.nS
    assert total > 3 * E
    first = np.where(defined, first, np.uint64(nS))                            # where cnt == 0, first is any value <= nS
    for cap in (total, total + 5, total - 1, E + 1, 0):
        rc, count, got = expand(eng, E, (offsets, first, rowsS), nR, nS, cap)
        assert rc == (RHJ_E_OVERFLOW if cap and cap < total else RHJ_OK) and count == total
        k = min(cap, total)
        assert np.array_equal(got.reshape(-1, 2)[:k], pairs[:k]) and (got.reshape(-1, 2)[k:] == GUARD).all()
        check_info(eng, units_of(nR + nS, T), 2, total, -(-k // E))        # no sort ran: units and sorts still speak of the call above
    i = int(np.nonzero(defined)[0][len(defined.nonzero()[0]) // 2])            # a row with partners, in the middle
    bad = {}
    bad["offsets[0] != 0"] = (np.concatenate([u(1), offsets[1:]]), first)
    dec = offsets.copy()
    dec[i + 1] = dec[i] - np.uint64(1) if dec[i] else dec[i + 2] + np.uint64(1)
    bad["a decreasing pair of offsets"] = (dec, first)
    past = first.copy()
    past[i] = np.uint64(nS + 1) - (offsets[i + 1] - offsets[i])
    bad["first[i] + cnt[i] == nS + 1"] = (offsets, past)
    for what, (o, f) in bad.items():
        rc, count, got = expand(eng, E, (o, f, rowsS), nR, nS, total)
        assert rc == RHJ_E_INVALID and count == 777 and (got == GUARD).all(), what
        with pytest.raises(RhjError, match="rhj_range_expand_dev: .*CSR"):
            eng._chk(rc)
    rc, count, got = expand(eng, E, (offsets, past, rowsS), nR, nS, 0)            # also refused when only the count is asked for
    assert rc == RHJ_E_INVALID and count == 777
    rc, count, got = expand(eng, E, (u(0), u(), rowsS), 0, nS, 4)              # no row of R
    assert rc == RHJ_OK and count == 0 and (got == GUARD).all()
    tab.close()


def test_each_csr_output_may_be_null(eng, T, E):
    tab = Tables(eng, *RC.make_tables("runs64", "sixteen", T + 9, T - 5, T, seed=5))
    want = tab.oracle(HI_OPEN)
    for keep in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        call(eng, T, E, tab, HI_OPEN, expect=want, offsets=keep[0], first=keep[1], rowsS=keep[2])
        call(eng, T, E, tab, HI_OPEN, expect=want, offsets=keep[0], first=keep[1], rowsS=keep[2], cap=None)
    tab.close()


def test_two_runs_are_bit_identical(eng, T, E):
    n = 2 * T + 1
    tab = Tables(eng, *RC.make_tables("zipf", "sixteen", n // 2, n - n // 2, T))
    call(eng, T, E, tab, 0, twice=True)
    call(eng, T, E, tab, LO_OPEN | I64, twice=True)
    tab.close()


def test_release_workspace_and_call_again(eng, T, E):
    n = T + 1
    tab = Tables(eng, *RC.make_tables("geometric", "distinct", n // 2, n - n // 2, T))
    want, _ = call(eng, T, E, tab, 0)
    eng.release_workspace()
    call(eng, T, E, tab, 0, expect=want)
    eng.release_workspace()
    call(eng, T, E, tab, BAND | I64, 1 << 60, 1 << 60)
    tab.close()


def test_other_calls_reset_the_range_names(eng, T, E):
    tab = Tables(eng, *RC.make_tables("runs64", "sixteen", 40, 25, T))
    _, total = call(eng, T, E, tab, 0)
    assert total > 0 and eng.info("last.range_join_units") == 1 and eng.info("last.range_join_sorts") == 2
    out = Array(eng, 40)

    def all_zero():
        return all(eng.info("last." + name) == 0 for name in RANGE_NAMES)
    eng.asof_cols_dev(tab.ptr("byR"), tab.ptr("loR"), 40, tab.ptr("byS"), tab.ptr("onS"), 25, 0, 0, out.ptr)
    assert eng.info("last.asof_units") == 1 and all_zero()
    call(eng, T, E, tab, 0)                                                    # (check_info: the as-of names are 0 again)
    eng.sort_cols_dev(tab.ptr("loR"), None, 40, 0, None, out.ptr)
    assert eng.info("last.sort_passes") >= 0 and all_zero()
    call(eng, T, E, tab, I64)
    assert eng.join_cols_dev(tab.ptr("byR"), None, 40, tab.ptr("byS"), None, 25) > 0
    assert all_zero()
    call(eng, T, E, tab, I64 | BAND, 5, 5)
    out.free()
    tab.close()


def test_invalid_arguments_are_refused_before_any_launch(eng, T, E):
    tab = Tables(eng, *RC.make_tables("runs64", "sixteen", 40, 25, T))
    out = Outputs(eng, 40, 25, 40 * 25)
    bR, lR, hR, bS, oS = (tab.ptr(k) for k in Tables.NAMES)
    o = out.ptrs()
    count = C.c_uint64(77)
    # (d_byR, d_loR, d_hiR, nR, d_byS, d_onS, nS, flags, below, above, offsets, first, rowsS, d_out, capacity): the word the message must hold
    bad = [((bR, lR, hR, 40, bS, oS, 25, 16, 0, 0, *o, 64), "flags"),
           ((bR, lR, hR, 40, bS, oS, 25, 0x80000000, 0, 0, *o, 64), "flags"),
           ((None, None, None, 0, None, None, 0, 32, 0, 0, None, None, None, None, 0), "flags"),      # ... also with both tables empty
           ((bR, None, hR, 40, bS, oS, 25, 0, 0, 0, *o, 64), "d_loR"),
           ((bR, None, None, 40, bS, oS, 25, BAND, 1, 1, *o, 64), "d_loR"),
           ((bR, lR, hR, 40, bS, None, 25, 0, 0, 0, *o, 64), "d_onS"),
           ((bR, lR, None, 40, bS, oS, 25, I64, 0, 0, *o, 64), "d_hiR"),
           ((bR, lR, hR, 40, bS, oS, 25, BAND, 1, 1, *o, 64), "d_hiR"),
           ((None, lR, hR, 40, bS, oS, 25, 0, 0, 0, *o, 64), "d_byR"),
           ((bR, lR, hR, 40, None, oS, 25, LO_OPEN, 0, 0, *o, 64), "d_byS"),
           ((bR, lR, hR, 40, bS, oS, 25, 0, 0, 0, o[0], o[1], o[2], None, 64), "d_out")]
    for args, word in bad:
        rc = eng.lib.rhj_range_join_cols_dev(eng.ctx, *args, C.byref(count))
        assert rc == RHJ_E_INVALID, (rc, word)
        with pytest.raises(RhjError, match=r"rhj_range_join_cols_dev: .*" + word) as err:
            eng._chk(rc)
        assert err.value.code == RHJ_E_INVALID
        assert count.value == 77                                             # out_count is untouched
    assert out.untouched()                                                   # nothing was launched
    for args, word in (((None, o[1], 40, o[2], 25, o[3], 64), "d_offsets"), ((o[0], None, 40, o[2], 25, o[3], 64), "d_first"),
                       ((o[0], o[1], 40, None, 25, o[3], 64), "d_rowsS"), ((o[0], o[1], 40, o[2], 25, None, 64), "d_out")):
        rc = eng.lib.rhj_range_expand_dev(eng.ctx, *args, C.byref(count))
        assert rc == RHJ_E_INVALID and count.value == 77, word
        with pytest.raises(RhjError, match=r"rhj_range_expand_dev: .*" + word):
            eng._chk(rc)
    assert out.untouched()
    # no rows of R: offsets[0] = 0 and nothing else, whatever else is NULL; a one-sided `by` is fine while a table is empty
    assert eng.lib.rhj_range_join_cols_dev(eng.ctx, None, None, None, 0, bS, oS, 25, 0, 0, 0, *o, 64, C.byref(count)) == 0 and count.value == 0
    check_info(eng, 0, 0, 0, 0)
    assert out.offsets.read()[0] == 0 and (out.offsets.read()[1:] == GUARD).all() and (out.first.read() == GUARD).all()
    assert (out.rowsS.read() == GUARD).all() and (out.pairs.read() == GUARD).all()
    count.value = 77
    assert eng.lib.rhj_range_join_cols_dev(eng.ctx, bR, lR, hR, 40, None, None, 0, 0, 0, 0, *o, 64, C.byref(count)) == 0 and count.value == 0
    check_info(eng, 0, 0, 0, 0)
    assert (out.offsets.read() == 0).all() and (out.first.read() == 0).all() and (out.pairs.read() == GUARD).all()   # the fill launch
    assert eng.lib.rhj_range_join_cols_dev(eng.ctx, bR, lR, hR, 40, bS, oS, 25, I64, 0, 0, *o, 40 * 25, None) == 0          # out_count NULL
    want = tab.oracle(I64)
    compare(out, want, 40, 25, "out_count NULL")
    assert eng.info("last.range_join_pairs") == len(want[4])
    out.free()
    tab.close()


@pytest.mark.parametrize("shape", ["one", "zipf"])
def test_one_and_a_half_million_rows_per_side(eng, T, E, shape):
    """more units than CUs; one partition -- the carry crosses every unit -- and a few thousand Zipf partitions.  The reach of the
    intervals is fixed so that the oracle's total lies in [2^20, 2^24]: 2 626 103 pairs with one partition, 3 750 332 with Zipf's."""
    n = BIG
    assert units_of(2 * n, T) > 512
    tab = Tables(eng, *RC.make_tables(shape, "distinct", n, n, T, groups=3000, reach=8 if shape == "one" else 1000, flags=I64))
    if shape == "zipf":
        assert len(np.unique(np.concatenate([tab.host["byR"], tab.host["byS"]]))) == 3000
    want = tab.oracle(I64)
    assert 1 << 20 <= len(want[4]) <= 1 << 24
    call(eng, T, E, tab, I64, expect=want)
    tab.close()


def as_i64(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def test_the_torch_methods(eng, T, E):
    """a two-tensor `by` on each side against a hand-packed single word, unsigned=True, all four closed forms, the band, empty tensors;
    the inputs are left unmodified, and range_join_columns runs the inner sorts once"""
    nR, nS = T + 7, T - 3
    rng = np.random.default_rng(31)
    aR, aS = rng.integers(-3, 4, nR).astype(np.int64), rng.integers(-3, 3, nS).astype(np.int64)
    bR, bS = rng.integers(0, 5, nR).astype(np.int64) * (1 << 40), rng.integers(0, 5, nS).astype(np.int64) * (1 << 40)
    pack = lambda a, b: (a.view(np.uint64) << np.uint64(3)) ^ (b.view(np.uint64) >> np.uint64(40))      # one word per distinct (a, b)
    _, loR, hiR, _, onS = RC.make_tables("one", "extremes", nR, nS, T, by=False, flags=I64)
    tens = [torch.from_numpy(x).cuda() for x in (aR, bR, aS, bS)] + [as_i64(loR), as_i64(hiR), as_i64(onS)]
    taR, tbR, taS, tbS, tlo, thi, ton = tens
    keep = [t.clone() for t in tens]
    flags_of = {"both": 0, "left": HI_OPEN, "right": LO_OPEN, "neither": LO_OPEN | HI_OPEN}
    for closed, fl in flags_of.items():
        for unsigned in (False, True):
            flags = fl | (0 if unsigned else I64)
            offsets, first, defined, rowsS, pairs = RC.oracle(pack(aR, bR), loR, hiR, pack(aS, bS), onS, flags)
            o, f, r, total = eng.range_join_csr_columns(tlo, thi, ton, [taR, tbR], [taS, tbS], closed=closed, unsigned=unsigned)
            sorts = eng.info("last.range_join_sorts")
            assert total == len(pairs) and sorts == 2 and all(t.dtype == torch.int64 for t in (o, f, r))
            # (rows_S is ordered by the PACKED `by` word first, which is pack_keys' and not the hand-packed one: the runs are compared)
            o, f, r = (t.cpu().numpy() for t in (o, f, r))
            assert np.array_equal(o.view(np.uint64), offsets) and np.array_equal(np.sort(r), np.arange(nS))
            rows = np.repeat(np.arange(nR), np.diff(o))
            assert np.array_equal(np.stack([rows, r[np.arange(total) - o[rows] + f[rows]]], 1).view(np.uint64), pairs)
            iR, iS = eng.range_join_columns(tlo, thi, ton, [taR, tbR], [taS, tbS], closed=closed, unsigned=unsigned)
            assert eng.info("last.range_join_sorts") == sorts and eng.info("last.range_join_pairs") == total      # the sorts of ONE csr call
            assert iR.dtype == iS.dtype == torch.int64
            assert np.array_equal(torch.stack([iR, iS], 1).cpu().numpy().view(np.uint64), pairs)
    # a single tensor per side: rows_S and first word for word
    offsets, first, defined, rowsS, pairs = RC.oracle(aR.view(np.uint64), loR, hiR, aS.view(np.uint64), onS, HI_OPEN)
    o, f, r, total = eng.range_join_csr_columns(tlo, thi, ton, taR, taS, closed="left", unsigned=True)
    assert total == len(pairs) and np.array_equal(o.cpu().numpy().view(np.uint64), offsets) and np.array_equal(r.cpu().numpy().view(np.uint64), rowsS)
    assert np.array_equal(f.cpu().numpy().view(np.uint64)[defined], first[defined])
    # ... as pairs, and no `by`; the band
    iR, iS = eng.range_join_columns(tlo, thi, ton, taR, taS)
    pairs = RC.oracle(aR.view(np.uint64), loR, hiR, aS.view(np.uint64), onS, I64)[4]
    assert np.array_equal(torch.stack([iR, iS], 1).cpu().numpy().view(np.uint64), pairs) and eng.info("last.range_join_sorts") == 2
    for kw, flags, below, above in (({}, I64, 1, 2), ({"unsigned": True, "closed": "left"}, HI_OPEN, 0, TOP), ({"closed": "neither"}, I64 | LO_OPEN | HI_OPEN, ONES, 1)):
        iR, iS = eng.band_join_columns(tlo[:300], ton[:200], below, above, **kw)                         # (no `by`: the extremes tie heavily)
        pairs = RC.oracle(None, loR[:300], None, None, onS[:200], flags | BAND, below, above)[4]
        assert np.array_equal(torch.stack([iR, iS], 1).cpu().numpy().view(np.uint64), pairs), kw
        assert eng.info("last.range_join_sorts") == 1
    iR, iS = eng.band_join_columns(tlo, ton, 1, 1, [taR, tbR], [taS, tbS])
    pairs = RC.oracle(pack(aR, bR), loR, None, pack(aS, bS), onS, I64 | BAND, 1, 1)[4]
    assert np.array_equal(torch.stack([iR, iS], 1).cpu().numpy().view(np.uint64), pairs)
    for t, k in zip(tens, keep):
        assert torch.equal(t, k)
    empty = torch.empty(0, dtype=torch.int64, device="cuda")
    o, f, r, total = eng.range_join_csr_columns(empty, empty, ton, empty, taS)
    assert o.tolist() == [0] and len(f) == 0 and len(r) == 0 and total == 0
    o, f, r, total = eng.range_join_csr_columns(tlo, thi, empty)
    assert (o == 0).all() and len(o) == nR + 1 and (f == 0).all() and len(r) == 0 and total == 0
    for iR, iS in (eng.range_join_columns(empty, empty, empty), eng.range_join_columns(tlo, thi, empty), eng.band_join_columns(empty, ton, 1, 1)):
        assert len(iR) == len(iS) == 0 and iR.dtype == torch.int64
