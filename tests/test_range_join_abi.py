"""CPU suite: the range join entries are part of the C-ABI -- declared in include/rhj.h with their argument names and flag bits between
the RANGE frame entry and the composite-key block, exported by librhj_hip.so, bound in binding.SYMBOLS with their argument types -- and
the addition left RHJ_ABI_VERSION at 3.  Engine.range_join_csr_columns, range_join_columns and band_join_columns refuse wrong arguments
before they touch a device.  The two oracles of the GPU tests (tests/range_join_cases.py) agree on a grid of tiny tables, are checked by
hand on one table of eight rows of S, and agree with a filtered cross merge where pandas is installed.

Without the feature the header, export, constant, signature and ValueError tests fail; the oracle-against-brute tests, the hand check,
the pandas test and the generator test pass with or without it: they do not touch the product."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import radixhashjoin_amd as rhj
from radixhashjoin_amd import binding

import asof_cases as AC
import range_join_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _u64, _u32, _P = C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER
ENTRIES = {
    "rhj_range_join_cols_dev": (["ctx", "d_byR", "d_loR", "d_hiR", "nR", "d_byS", "d_onS", "nS", "flags", "below", "above", "d_out_offsets",
                                 "d_out_first", "d_out_rowsS", "d_out", "out_capacity", "out_count"],
                                [_vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _u32, _u64, _u64, _vp, _vp, _vp, _vp, _u64, _P(_u64)]),
    "rhj_range_expand_dev": (["ctx", "d_offsets", "d_first", "nR", "d_rowsS", "nS", "d_out", "out_capacity", "out_count"],
                             [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _u64, _P(_u64)]),
}
CONSTANTS = {"RANGE_I64": 1, "RANGE_LO_OPEN": 2, "RANGE_HI_OPEN": 4, "RANGE_BAND": 8}


def header(strip_comments=True):
    with open(os.path.join(ROOT, "include", "rhj.h")) as f:
        h = f.read()
    return re.sub(r"/\*.*?\*/", " ", h, flags=re.S) if strip_comments else h


def test_header_declares_the_entries_with_their_argument_names_and_constants():
    h = header()
    for name, (names, _) in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", h)
        assert m, f"include/rhj.h does not declare {name}"
        args = [a.strip() for a in m.group(1).split(",")]
        assert [a.split()[-1].lstrip("*") for a in args] == names
    for name, value in CONSTANTS.items():
        assert re.search(r"#define\s+RHJ_" + name + r"\s+" + str(value) + r"u(?!\w)", h), name
    assert re.search(r"#define\s+RHJ_ABI_VERSION\s+3\b", h)


def test_the_block_stands_between_the_range_frames_and_the_composite_keys():
    h = header()
    at = {name: h.index(name + "(") for name in ("rhj_frame_range_cols_dev", "rhj_range_join_cols_dev", "rhj_range_expand_dev")}
    keys = h.index("#define RHJ_KEYS_MAX_COLS")
    assert at["rhj_frame_range_cols_dev"] < at["rhj_range_join_cols_dev"] < at["rhj_range_expand_dev"] < keys
    assert h[at["rhj_frame_range_cols_dev"]:at["rhj_range_join_cols_dev"]].count("(") == 1, "a declaration stands between the RANGE frames and the range join"
    assert h[at["rhj_range_join_cols_dev"]:at["rhj_range_expand_dev"]].count("(") == 1
    assert h[at["rhj_range_expand_dev"]:keys].count("(") == 1, "a declaration stands between rhj_range_expand_dev and the composite keys"
    assert at["rhj_frame_range_cols_dev"] < h.index("RHJ_RANGE_I64") < h.index("RHJ_RANGE_BAND") < at["rhj_range_join_cols_dev"]


def test_library_exports_them_and_binding_knows_their_types():
    lib = rhj.load_library()
    for name, (_, types) in ENTRIES.items():
        assert isinstance(getattr(lib, name), C._CFuncPtr)
        res, args = binding.SYMBOLS[name]
        assert res is C.c_int and list(args) == types
    for method in ("range_join_cols_dev", "range_expand_dev", "range_join_csr_columns", "range_join_columns", "band_join_columns"):
        assert callable(getattr(rhj.Engine, method))


def test_constants_are_exported():
    for name, value in CONSTANTS.items():
        assert getattr(rhj, name) == getattr(binding, name) == value and name in rhj.__all__
    assert (RC.RANGE_I64, RC.RANGE_LO_OPEN, RC.RANGE_HI_OPEN, RC.RANGE_BAND) == tuple(CONSTANTS.values())


def test_abi_version_is_still_3():
    assert rhj.load_library().rhj_abi_version() == 3


def test_signatures_and_defaults_of_the_torch_entries():
    for name in ("range_join_csr_columns", "range_join_columns"):
        p = inspect.signature(getattr(rhj.Engine, name)).parameters
        assert list(p) == ["self", "lo_R", "hi_R", "on_S", "by_R", "by_S", "closed", "unsigned"]
        assert p["by_R"].default is None and p["by_S"].default is None and p["closed"].default == "both" and p["unsigned"].default is False
    p = inspect.signature(rhj.Engine.band_join_columns).parameters
    assert list(p) == ["self", "on_R", "on_S", "below", "above", "by_R", "by_S", "closed", "unsigned"]
    assert p["below"].default is inspect.Parameter.empty and p["above"].default is inspect.Parameter.empty
    assert p["by_R"].default is None and p["by_S"].default is None and p["closed"].default == "both" and p["unsigned"].default is False
    p = inspect.signature(rhj.Engine.range_join_cols_dev).parameters
    assert list(p)[:11] == ["self", "d_byR", "d_loR", "d_hiR", "nR", "d_byS", "d_onS", "nS", "flags", "below", "above"]
    p = inspect.signature(rhj.Engine.range_expand_dev).parameters
    assert list(p)[:6] == ["self", "d_offsets", "d_first", "nR", "d_rowsS", "nS"]


def test_value_errors_come_before_any_device_use():
    """an Engine that was never constructed reaches every one of them"""
    import torch
    e = rhj.Engine.__new__(rhj.Engine)
    e.ctx = None
    calls = {"csr": lambda **kw: e.range_join_csr_columns(None, None, None, **kw),
             "pairs": lambda **kw: e.range_join_columns(None, None, None, **kw),
             "band": lambda **kw: e.band_join_columns(None, None, kw.pop("below", 0), kw.pop("above", 0), **kw)}
    for a in calls.values():
        for bad in ("all", "BOTH", None, 1, True):
            with pytest.raises(ValueError, match="^closed: 'both', 'left', 'right' or 'neither' is needed"):
                a(closed=bad)
        for bad in (1, None, [True]):
            with pytest.raises(ValueError, match="^unsigned: a bool"):
                a(unsigned=bad)
        with pytest.raises(ValueError, match="^by_S: None"):
            a(by_R=0)
        with pytest.raises(ValueError, match="^by_R: None"):
            a(by_S=[0, 0])
        with pytest.raises(ValueError, match="^by_S: 1 tensors, by_R has 2"):
            a(by_R=[0, 0], by_S=[0])
        with pytest.raises(ValueError, match="^by_S: 2 tensors, by_R has 1"):
            a(by_R=0, by_S=[0, 0])
        with pytest.raises(ValueError, match="^by_R: 1 to 4 tensors are needed, not 5"):
            a(by_R=[0] * 5, by_S=[0] * 5)
    for name in ("below", "above"):
        for bad in (-1, True, False, 1.0, "3", 1 << 64):
            with pytest.raises(ValueError, match=f"^{name}: an int >= 0"):
                calls["band"](**{name: bad})
    lo, hi = torch.zeros(3, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)
    for a in (e.range_join_csr_columns, e.range_join_columns):
        with pytest.raises(ValueError, match="^hi_R: 4 elements, lo_R has 3"):
            a(lo, hi, lo)


def test_header_states_the_contract():
    h = re.sub(r"\s*\n \* ", " ", header(strip_comments=False))       # (comment lines joined: a phrase may wrap)
    for phrase in ("Rows are the indices 0 .. n - 1 of their table",
                   "Neither table needs to be sorted",
                   "`by` is compared for bit-equality only",
                   "d_byR == NULL && d_byS == NULL: one partition",
                   "lo[i] <= on[j] <= hi[i] in the view",
                   "An interval with lo > hi in the view has no partner and is legal",
                   "d_loR holds R's own order word x and d_hiR must be NULL",
                   "saturate at the view's ends",
                   "Open flags apply to the saturated bound like to any other",
                   "Without the bit `below` and `above` are ignored and d_hiR is required",
                   "rowsS[first[i] .. first[i] + cnt[i])",
                   "offsets[0] = 0 and offsets[nR] the total",
                   "where cnt[i] == 0, first[i] is any value <= nS",
                   "Each of the three may be NULL",
                   "16 nR + 8 nS bytes however many pairs there are",
                   "d_out[offsets[i] + q] = {i, rowsS[first[i] + q]}",
                   "d_out == NULL with out_capacity == 0 writes no pairs",
                   "it always receives the exact total",
                   "slots [0, capacity) hold the first `capacity` pairs of the defined order",
                   "nothing at or past capacity is written",
                   "the three CSR outputs are complete",
                   "bit-identical from run to run",
                   "nR == 0: RHJ_OK, total 0, offsets[0] = 0 if given",
                   "offsets all 0 and first all 0 (one fill launch)",
                   "before any launch, with a message naming the argument",
                   "non-NULL d_hiR under RHJ_RANGE_BAND", "the one-sided `by`",
                   "Inputs are neither modified nor retained", "outputs must not overlap inputs",
                   "The call synchronises", "rhj_set_stream and rhj_set_profiling",
                   "No workgroup waits on another inside a kernel", "no position, count or value comes from an atomic",
                   '"last.range_join_units"', '"last.range_join_sorts"', '"last.range_join_pairs"', '"last.range_join_expand_tiles"',
                   '"range_join.tile_rows"', '"range_join.expand_tile"',
                   "all four are 0 after every other call", '"last.join_kernel" is -1',
                   "kept until rhj_release_workspace",
                   "offsets[0] == 0, offsets[i] <= offsets[i + 1], and first[i] + cnt[i] <= nS wherever cnt[i] > 0",
                   "an error code, never an address",
                   "interval-overlap joins with intervals on both sides", "There is no 16-byte tuple form"):
        assert phrase in h, phrase


def words_of(kind, rng, n):
    if kind == "extremes":
        w = np.array([0, 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 2, (1 << 64) - 1], dtype=np.uint64)
    elif kind == "constant":
        w = np.array([0xFEDCBA9876543210], dtype=np.uint64)
    elif kind == "sixteen":
        w = np.array([0, 1, 2, 3, 5, 8, 13, 21, (1 << 63) - 2, (1 << 63) + 2, 1 << 62, 3 << 62, 100, 101, 102, (1 << 64) - 3], dtype=np.uint64)
    else:
        return rng.permutation(4 * n + 1)[:n].astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    return w[rng.integers(0, len(w), n)]


def test_the_two_oracles_agree_on_a_grid_of_tiny_tables():
    """all 16 flag combinations, every split of asof_cases.splits of totals up to 40 rows, the four order kinds (extremes: 0, all ones,
    INT64_MIN / MAX and their neighbours), with and without `by`, below / above in {0, 1, 2^63, all ones} under BAND.  (Passes with or
    without the feature.)"""
    rng = np.random.default_rng(5)
    cases = 0
    for n in (0, 1, 2, 9, 40):
        for nR, nS in AC.splits(n):
            for kind in RC.ONS:
                for parts in (None, 3):
                    lo, hi, on = words_of(kind, rng, nR), words_of(kind, rng, nR), words_of(kind, rng, nS)
                    byR = byS = None
                    if parts:
                        w = np.array([(1 << 64) - 1, 1 << 63, 7], dtype=np.uint64)
                        byR, byS = w[rng.integers(0, 3, nR)], w[rng.integers(0, 2, nS)]
                    for flags in RC.FLAGS16:
                        dists = [(b, a) for b in RC.DISTANCES for a in RC.DISTANCES] if flags & RC.RANGE_BAND else [(0, 0)]
                        for below, above in dists:
                            h = None if flags & RC.RANGE_BAND else hi
                            want = RC.brute(byR, lo, h, byS, on, flags, below, above)
                            offsets, first, defined, rowsS, pairs = RC.oracle(byR, lo, h, byS, on, flags, below, above)
                            assert np.array_equal(pairs, want), (nR, nS, kind, parts, flags, below, above)
                            assert offsets[0] == 0 and int(offsets[-1]) == len(want) and len(rowsS) == nS
                            assert np.array_equal(defined, np.diff(offsets.astype(np.int64)) > 0)
                            cases += 1
    assert cases >= 5 * 2 * 4 * 2 * (8 + 8 * 16)


ONES, TOP = (1 << 64) - 1, 1 << 63
A, B = ONES, 7
BY_S = np.array([A, A, A, A, B, B, A, B], dtype=np.uint64)
ON_S = np.array([10, 20, 20, 30, 5, ONES, TOP, 20], dtype=np.uint64)
BY_R = np.array([A, A, B, 9, A], dtype=np.uint64)
LO_R = np.array([20, 10, 0, 0, 30], dtype=np.uint64)
HI_R = np.array([20, 30, ONES, ONES, 10], dtype=np.uint64)


def test_the_oracles_by_hand_on_eight_rows_of_S():
    """Partitions A = all ones and B = 7; R's partition 9 has no row of S; rows 1 and 2 of S are a duplicate (by, on).
    rowsS, unsigned: B sorts first -- 5 (row 4), 20 (row 7), all ones (row 5) --, then A -- 10, 20, 20, 30, 1 << 63 (rows 0, 1, 2, 3, 6).
    rowsS, int64: B is -1 (row 5), 5, 20; A is the minimum (row 6), then 10, 20, 20, 30.
    Row 0 of R [20, 20]: the duplicate run, in index order.  Row 1 [10, 30]: rows 0, 1, 2, 3.  Row 2 (B) [0, all ones]: all of B
    unsigned, and empty as int64, where it is [0, -1].  Row 3: no partition.  Row 4 [30, 10]: empty."""
    def one(flags, below=0, above=0):
        h = None if flags & RC.RANGE_BAND else HI_R
        offsets, first, defined, rowsS, pairs = RC.oracle(BY_R, LO_R, h, BY_S, ON_S, flags, below, above)
        assert np.array_equal(pairs, RC.brute(BY_R, LO_R, h, BY_S, ON_S, flags, below, above))
        return offsets.tolist(), [int(f) if d else None for f, d in zip(first, defined)], rowsS.tolist(), [tuple(p) for p in pairs.tolist()]

    I64, LO, HI, BAND = RC.RANGE_I64, RC.RANGE_LO_OPEN, RC.RANGE_HI_OPEN, RC.RANGE_BAND
    offsets, first, rowsS, pairs = one(0)
    assert rowsS == [4, 7, 5, 0, 1, 2, 3, 6]
    assert offsets == [0, 2, 6, 9, 9, 9] and first == [4, 3, 0, None, None]
    assert pairs == [(0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (1, 3), (2, 4), (2, 7), (2, 5)]
    offsets, first, _, pairs = one(LO)                                     # 20 < on <= 20: nothing; 10 < on: the run onwards; 0 < on: all of B
    assert offsets == [0, 0, 3, 6, 6, 6] and first == [None, 4, 0, None, None] and pairs[:3] == [(1, 1), (1, 2), (1, 3)]
    offsets, first, _, pairs = one(HI)                                     # on < 30: rows 0, 1, 2; on < all ones: rows 4 and 7
    assert offsets == [0, 0, 3, 5, 5, 5] and first == [None, 3, 0, None, None] and pairs[3:] == [(2, 4), (2, 7)]
    offsets, first, _, pairs = one(LO | HI)
    assert offsets == [0, 0, 2, 4, 4, 4] and pairs == [(1, 1), (1, 2), (2, 4), (2, 7)]
    offsets, first, rowsS, pairs = one(I64)
    assert rowsS == [5, 4, 7, 6, 0, 1, 2, 3]
    assert offsets == [0, 2, 6, 6, 6, 6] and first == [5, 4, None, None, None]
    # the band [x - 10, x + 10] around x = 20, 10, 0, 0, 30: row 2's lower end saturates at 0
    offsets, first, _, pairs = one(BAND, 10, 10)
    assert offsets == [0, 4, 7, 8, 8, 11] and pairs[7:] == [(2, 4), (4, 1), (4, 2), (4, 3)]
    offsets, _, _, pairs = one(BAND, 0, ONES)                              # to the end of the view: 1 << 63 is above every x in A
    assert offsets == [0, 4, 9, 12, 12, 14] and pairs[-2:] == [(4, 3), (4, 6)]
    offsets, _, _, pairs = one(BAND | I64, ONES, 0)                        # from the minimum up to x: row 6 (the minimum) comes first
    assert pairs[:3] == [(0, 6), (0, 0), (0, 1)] and offsets == [0, 4, 6, 7, 7, 12]
    offsets, _, _, pairs = one(BAND | HI, 0, 0)                            # [x, x): legal, and empty
    assert offsets == [0] * 6 and pairs == []
    # one partition: B's rows join A's
    offsets, _, defined, rowsS, pairs = RC.oracle(None, LO_R, HI_R, None, ON_S, 0)
    assert rowsS.tolist() == [4, 0, 1, 2, 7, 3, 6, 5] and offsets.tolist() == [0, 3, 8, 16, 24, 24]
    offsets, first, defined, rowsS, pairs = RC.oracle(BY_R[:0], LO_R[:0], HI_R[:0], BY_S, ON_S, 0)
    assert offsets.tolist() == [0] and len(pairs) == 0 and len(rowsS) == 8
    offsets, first, defined, rowsS, pairs = RC.oracle(BY_R, LO_R, HI_R, BY_S[:0], ON_S[:0], 0)
    assert offsets.tolist() == [0] * 6 and first.tolist() == [0] * 5 and len(rowsS) == 0 and len(pairs) == 0


def test_the_pair_set_is_a_filtered_cross_merge():
    """pandas: R x S, filtered by the predicate in int64 -- the set of pairs, with and without `by`, in all four closed forms.  (Passes
    with or without the feature.)"""
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(11)
    for nR, nS, span in ((30, 40, 20), (120, 90, 60)):
        lo = rng.integers(-span, span, nR).astype(np.int64)
        hi = lo + rng.integers(-3, 12, nR)
        on = rng.integers(-span, span, nS).astype(np.int64)
        byR, byS = rng.integers(0, 3, nR).astype(np.int64), rng.integers(0, 4, nS).astype(np.int64)
        left = pd.DataFrame({"i": np.arange(nR), "lo": lo, "hi": hi, "byR": byR})
        right = pd.DataFrame({"j": np.arange(nS), "on": on, "byS": byS})
        x = left.merge(right, how="cross")
        for with_by in (False, True):
            for flags in (0, RC.RANGE_LO_OPEN, RC.RANGE_HI_OPEN, RC.RANGE_LO_OPEN | RC.RANGE_HI_OPEN):
                keep = (x.on > x.lo if flags & RC.RANGE_LO_OPEN else x.on >= x.lo) & (x.on < x.hi if flags & RC.RANGE_HI_OPEN else x.on <= x.hi)
                if with_by:
                    keep &= x.byR == x.byS
                want = set(zip(x.i[keep].tolist(), x.j[keep].tolist()))
                pairs = RC.oracle(byR.view(np.uint64) if with_by else None, lo.view(np.uint64), hi.view(np.uint64),
                                  byS.view(np.uint64) if with_by else None, on.view(np.uint64), flags | RC.RANGE_I64)[4]
                assert len(pairs) == len(want) and set(map(tuple, pairs.tolist())) == want


def test_case_generators_split_the_window_shapes_between_the_tables():
    T = 4096
    for shape in RC.SHAPES:
        for kind in RC.ONS:
            byR, loR, hiR, byS, onS = RC.make_tables(shape, kind, 300, 200, T, flags=RC.RANGE_I64)
            assert [a.dtype for a in (byR, loR, hiR, byS, onS)] == [np.uint64] * 5 and len(byR) == len(loR) == len(hiR) == 300 and len(onS) == 200
    byR, loR, hiR, byS, onS = RC.make_tables("one", "distinct", 3000, 2000, T)
    offsets, _, defined, _, pairs = RC.oracle(byR, loR, hiR, byS, onS, 0)
    assert 2000 < len(pairs) < 12000 and 100 < (~defined).sum() < 2000             # a handful of partners per row, and empty intervals
    assert (RC.view(loR, 0) > RC.view(hiR, 0)).sum() > 100
    assert RC.make_tables("one", "extremes", 5, 5, T, by=False)[0] is None
    assert RC.splits(9) == AC.splits(9)
