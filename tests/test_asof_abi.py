"""CPU suite: the as-of join entry is part of the C-ABI -- declared in include/rhj.h with its argument names and flag bits between the
composite-key entries and the sort block, exported by librhj_hip.so, bound in binding.SYMBOLS with its argument types -- and the
addition left RHJ_ABI_VERSION at 3.  Engine.asof_join_columns refuses wrong arguments before it touches a device.  The two oracles of
the GPU tests (tests/asof_cases.py) agree on a grid of tiny tables, are checked by hand on eight rows, and agree with
pandas.merge_asof where pandas is installed."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import radixhashjoin_amd as rhj
from radixhashjoin_amd import binding

import asof_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _u64, _u32, _P = C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER
ENTRIES = {
    "rhj_asof_cols_dev": (["ctx", "d_byR", "d_onR", "nR", "d_byS", "d_onS", "nS", "flags", "tolerance", "d_out_rowS", "out_matched"],
                          [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _u32, _u64, _vp, _P(_u64)]),
}
CONSTANTS = {"ASOF_I64": 1, "ASOF_FORWARD": 2, "ASOF_STRICT": 4, "ASOF_TOLERANCE": 8}


def header(strip_comments=True):
    with open(os.path.join(ROOT, "include", "rhj.h")) as f:
        h = f.read()
    return re.sub(r"/\*.*?\*/", " ", h, flags=re.S) if strip_comments else h


def test_header_declares_the_entry_with_its_argument_names_and_constants():
    h = header()
    for name, (names, _) in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", h)
        assert m, f"include/rhj.h does not declare {name}"
        args = [a.strip() for a in m.group(1).split(",")]
        assert [a.split()[-1].lstrip("*") for a in args] == names
    for name, value in CONSTANTS.items():
        assert re.search(r"#define\s+RHJ_" + name + r"\s+" + str(value) + r"u(?!\w)", h), name
    assert re.search(r"#define\s+RHJ_ABI_VERSION\s+3\b", h)


def test_the_block_stands_between_the_composite_keys_and_the_sort_block():
    h = header()
    at = {name: h.index(name + "(") for name in ("rhj_keys_plan_free", "rhj_asof_cols_dev", "rhj_sort_cols_dev", "rhj_sort_dev", "rhj_histogram")}
    assert at["rhj_keys_plan_free"] < at["rhj_asof_cols_dev"] < at["rhj_sort_cols_dev"]
    assert h[at["rhj_keys_plan_free"]:at["rhj_asof_cols_dev"]].count("(") == 1, "a declaration stands between rhj_keys_plan_free and rhj_asof_cols_dev"
    assert h[at["rhj_asof_cols_dev"]:at["rhj_sort_cols_dev"]].count("(") == 1, "a declaration stands between rhj_asof_cols_dev and rhj_sort_cols_dev"
    assert at["rhj_keys_plan_free"] < h.index("RHJ_ASOF_I64") < h.index("RHJ_ASOF_TOLERANCE") < at["rhj_asof_cols_dev"]
    assert "asof" not in h[at["rhj_sort_dev"]:at["rhj_histogram"]].lower()      # nothing of it among the sort, top-k and window blocks


def test_library_exports_it_and_binding_knows_its_types():
    lib = rhj.load_library()
    for name, (_, types) in ENTRIES.items():
        assert isinstance(getattr(lib, name), C._CFuncPtr)
        res, args = binding.SYMBOLS[name]
        assert res is C.c_int and list(args) == types
    for method in ("asof_cols_dev", "asof_join_columns"):
        assert callable(getattr(rhj.Engine, method))


def test_constants_are_exported():
    for name, value in CONSTANTS.items():
        assert getattr(rhj, name) == getattr(binding, name) == value and name in rhj.__all__
    assert (AC.ASOF_I64, AC.ASOF_FORWARD, AC.ASOF_STRICT, AC.ASOF_TOLERANCE) == tuple(CONSTANTS.values())
    assert int(AC.NO_ROW) == rhj.NO_ROW


def test_abi_version_is_still_3():
    assert rhj.load_library().rhj_abi_version() == 3


def test_signatures_and_defaults_of_the_torch_entries():
    p = inspect.signature(rhj.Engine.asof_join_columns).parameters
    assert list(p) == ["self", "on_R", "on_S", "by_R", "by_S", "values_S", "direction", "allow_exact_matches", "tolerance", "unsigned", "fill"]
    assert p["by_R"].default is None and p["by_S"].default is None and p["values_S"].default == () and p["direction"].default == "backward"
    assert p["allow_exact_matches"].default is True and p["tolerance"].default is None and p["unsigned"].default is False
    assert p["fill"].default == 0
    p = inspect.signature(rhj.Engine.asof_cols_dev).parameters
    assert list(p) == ["self", "d_byR", "d_onR", "nR", "d_byS", "d_onS", "nS", "flags", "tolerance", "d_out_rowS"]
    assert p["flags"].default == 0 and p["tolerance"].default == 0 and p["d_out_rowS"].default is None


def test_value_errors_come_before_any_device_use():
    """an Engine that was never constructed reaches every one of them"""
    e = rhj.Engine.__new__(rhj.Engine)
    e.ctx = None
    a = e.asof_join_columns
    with pytest.raises(ValueError, match="^direction: 'nearest' is not supported"):
        a(None, None, direction="nearest")
    for bad in ("sideways", None, 1):
        with pytest.raises(ValueError, match=r"^direction: 'backward' or 'forward' is needed \('nearest' is not supported\)"):
            a(None, None, direction=bad)
    for bad in (1, None, [True]):
        with pytest.raises(ValueError, match="^allow_exact_matches: a bool"):
            a(None, None, allow_exact_matches=bad)
        with pytest.raises(ValueError, match="^unsigned: a bool"):
            a(None, None, unsigned=bad)
    for bad in (-1, True, False, 1.0, "3", 1 << 64):
        with pytest.raises(ValueError, match="^tolerance: an int >= 0"):
            a(None, None, tolerance=bad)
    with pytest.raises(ValueError, match="^by_S: None"):
        a(None, None, by_R=0)
    with pytest.raises(ValueError, match="^by_R: None"):
        a(None, None, by_S=[0, 0])
    with pytest.raises(ValueError, match="^by_S: 1 tensors, by_R has 2"):
        a(None, None, by_R=[0, 0], by_S=[0])
    with pytest.raises(ValueError, match="^by_S: 2 tensors, by_R has 1"):
        a(None, None, by_R=0, by_S=[0, 0])
    with pytest.raises(ValueError, match="^by_R: 1 to 4 tensors are needed, not 5"):
        a(None, None, by_R=[0] * 5, by_S=[0] * 5)
    with pytest.raises(ValueError, match="^by_S: 1 to 4 tensors are needed, not 0"):
        a(None, None, by_R=[0], by_S=[])
    with pytest.raises(ValueError, match="^values_S: at most 4 value tensors"):
        a(None, None, values_S=[0] * 5)
    for bad in (1.5, True, [True], [1, 2], None):
        with pytest.raises(ValueError, match="^fill: an int"):
            a(None, None, values_S=[0], fill=bad)


def test_header_states_the_contract():
    h = re.sub(r"\s*\n \* ", " ", header(strip_comments=False))       # (comment lines joined: a phrase may wrap)
    for phrase in ("Rows are the indices 0 .. n - 1 of their table",
                   "out_matched is a HOST pointer and may be NULL",
                   "Neither table needs to be sorted: pandas requires sorted inputs, this entry does not",
                   "the word is compared for equality only",
                   "d_byR == NULL && d_byS == NULL: one partition",
                   "Exactly one of the two NULL with both tables non-empty is RHJ_E_INVALID",
                   "onS[j] <= onR[i]", "onS[j] <  onR[i]", "onS[j] >= onR[i]", "onS[j] >  onR[i]",
                   "|onR[i] - onS[j]| <= tolerance", "a comparison of exact integers, not mod 2^64",
                   "the distance between INT64_MIN and INT64_MAX is 2^64 - 1 and still fits the word",
                   "a difference of the order-transformed words",
                   "tolerance 0 means equal words only", "that matches nothing, and it is legal",
                   "Without the bit `tolerance` is ignored",
                   "the largest `on` for backward, the smallest for forward",
                   "backward takes the LARGEST row index and forward takes the SMALLEST",
                   "With no candidate the output is RHJ_NO_ROW",
                   "aligned with R, 8 bytes per row, no pair set is written",
                   "the number of rows of R with a partner",
                   "bit-identical from run to run",
                   "rhj_gather_cols_fill(ctx, &bid, 1, nS, rowS, nR, &fill, &bid_R)",
                   "nR == 0: RHJ_OK, no launch, *out_matched = 0",
                   "nS == 0 with nR > 0: every output is RHJ_NO_ROW (one fill launch)",
                   "before any launch, with a message naming the argument",
                   "unknown flag bits (also when both tables are empty)",
                   "NULL d_onR with nR > 0", "NULL d_onS with nS > 0", "NULL d_out_rowS with nR > 0", "the one-sided `by`",
                   "*out_matched is then untouched",
                   "Inputs are neither modified nor retained", "outputs must not overlap inputs", "pointers need 8-byte alignment",
                   "The call synchronises", "rhj_set_stream and rhj_set_profiling",
                   "No workgroup waits on another inside a kernel", "no position, value or count comes from an atomic",
                   '"last.asof_units"', '"last.asof_sorts"', '"last.asof_matched"', '"asof.tile_rows"',
                   "all three are 0 after every other call",
                   '"last.join_kernel" is -1', '"last.sort_*" / "last.topk_*" / "last.window_*" are 0',
                   '"sort.max_units" caps them here too', "the result never depends on it",
                   "kept until rhj_release_workspace", "2 x 8 + 1 bytes per row of nR + nS, 5 x 8 + 1 with `by`",
                   'direction "nearest" is not part of this entry',
                   "There is no 16-byte tuple form"):
        assert phrase in h, phrase


def test_the_two_oracles_agree_on_a_grid_of_tiny_tables():
    """all 8 combinations of direction, strictness and view, with and without a tolerance, with and without `by`, empty sides too"""
    rng = np.random.default_rng(5)
    words = np.array([0, 1, 2, 3, 5, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 2, (1 << 64) - 1], dtype=np.uint64)
    cases = 0
    for nR, nS in ((0, 0), (0, 3), (3, 0), (1, 1), (5, 7), (40, 30), (64, 65)):
        for parts in (None, 1, 3):
            for wide in (False, True):
                onR = words[rng.integers(0, 5 if not wide else len(words), nR)]
                onS = words[rng.integers(0, 5 if not wide else len(words), nS)]
                byR = byS = None
                if parts:
                    byR, byS = words[-parts:][rng.integers(0, parts, nR)], words[-parts:][rng.integers(0, max(parts - 1, 1), nS)]
                for flags in AC.FLAGS8:
                    for tol in (None, 0, 1, 2, (1 << 63) - 1, (1 << 64) - 2, (1 << 64) - 1):
                        f = flags | (AC.ASOF_TOLERANCE if tol is not None else 0)
                        want, m = AC.brute(byR, onR, byS, onS, f, tol or 0)
                        got, k = AC.oracle(byR, onR, byS, onS, f, tol or 0)
                        assert np.array_equal(got, want) and m == k, (nR, nS, parts, wide, flags, tol)
                        cases += 1
                    got, _ = AC.oracle(byR, onR, byS, onS, flags, 1)             # without the bit the tolerance is ignored
                    assert np.array_equal(got, AC.oracle(byR, onR, byS, onS, flags, 0)[0])
    assert cases == 7 * 3 * 2 * 8 * 7


ONES, TOP = (1 << 64) - 1, 1 << 63
NO = ONES
# partitions A = all ones, B = 1 << 63, C = 7 (no row of S).  S: rows 1 and 2 are a duplicate (by, on); partition B holds the all-ones
# word (the unsigned maximum, the signed -1) and 1 << 63 (the signed minimum); row 1 of R lies before every row of S of its partition
BY_S = np.array([ONES, ONES, ONES, TOP, TOP, ONES], dtype=np.uint64)
ON_S = np.array([10, 20, 20, ONES, TOP, 5], dtype=np.uint64)
BY_R = np.array([ONES, ONES, 7, TOP, TOP, ONES, ONES, TOP], dtype=np.uint64)
ON_R = np.array([20, 4, 20, 0, ONES, 15, 25, TOP], dtype=np.uint64)


def test_the_oracles_by_hand_on_eight_rows():
    def one(flags, tol=0):
        rows, matched = AC.oracle(BY_R, ON_R, BY_S, ON_S, flags, tol)
        assert np.array_equal(rows, AC.brute(BY_R, ON_R, BY_S, ON_S, flags, tol)[0])
        assert matched == sum(int(r) != NO for r in rows)
        return [int(r) for r in rows]

    I64, FWD, STRICT, TOL = AC.ASOF_I64, AC.ASOF_FORWARD, AC.ASOF_STRICT, AC.ASOF_TOLERANCE
    # backward, unsigned.  row 0 (A, 20): the run 20 20 -> its LARGEST index 2; row 1 (A, 4): 5 is A's smallest -> none; row 2: C has
    # no S; row 3 (B, 0): nothing <= 0; row 4 (B, ones): the maximum itself, row 3; row 5 (A, 15): 10; row 6 (A, 25): the run again;
    # row 7 (B, 1 << 63): itself, row 4
    assert one(0) == [2, NO, NO, NO, 3, 0, 2, 4]
    # int64: B's words are -1 (row 3) and the minimum (row 4); row 3 of R (0) now has both before it and takes -1
    assert one(I64) == [2, NO, NO, 3, 3, 0, 2, 4]
    # forward: row 0 takes the run's SMALLEST index 1; row 1 takes 5 (row 5); row 3 (B, 0) the smallest word >= 0, 1 << 63; row 6 none
    assert one(FWD) == [1, 5, NO, 4, 3, 1, NO, 4]
    assert one(FWD | I64) == [1, 5, NO, NO, 3, 1, NO, 4]                   # nothing of B is >= 0 as int64
    # strict: row 0 skips the whole run of 20s -> 10; row 4 (ones) takes 1 << 63; row 7 has nothing below 1 << 63
    assert one(STRICT) == [0, NO, NO, NO, 4, 0, 2, NO]
    assert one(STRICT | I64) == [0, NO, NO, 3, 4, 0, 2, NO]                # -1 < 0; the minimum < -1; nothing below the minimum
    assert one(STRICT | FWD) == [NO, 5, NO, 4, NO, 1, NO, 3]               # nothing of A above 20; above 1 << 63: all ones
    assert one(STRICT | FWD | I64) == [NO, 5, NO, NO, NO, 1, NO, 3]        # above the minimum: -1
    # tolerance: rows 5 and 6 are 5 away from their partners
    assert one(TOL, 5) == [2, NO, NO, NO, 3, 0, 2, 4]
    assert one(TOL, 4) == [2, NO, NO, NO, 3, NO, NO, 4]
    assert one(TOL | I64, 0) == [2, NO, NO, NO, 3, NO, NO, 4]              # equal words only: 0 and -1 are 1 apart
    assert one(TOL | I64, 1) == [2, NO, NO, 3, 3, NO, NO, 4]
    assert one(TOL | STRICT, 0) == [NO] * 8                                # legal, and matches nothing
    assert one(0, 4) == one(0)                                             # ignored without the bit
    # one partition: rows 3 and 4 of S (all ones, 1 << 63) join A's
    rows, matched = AC.oracle(None, ON_R, None, ON_S, 0)
    assert [int(r) for r in rows] == [2, NO, 2, NO, 3, 0, 2, 4] and matched == 6
    # INT64_MIN against INT64_MAX: the distance is 2^64 - 1
    lo, hi = np.array([TOP], dtype=np.uint64), np.array([TOP - 1], dtype=np.uint64)
    assert int(AC.oracle(None, hi, None, lo, I64 | TOL, ONES - 1)[0][0]) == NO and int(AC.oracle(None, hi, None, lo, I64 | TOL, ONES)[0][0]) == 0
    assert int(AC.brute(None, hi, None, lo, I64 | TOL, ONES - 1)[0][0]) == NO and int(AC.brute(None, hi, None, lo, I64 | TOL, ONES)[0][0]) == 0
    rows, matched = AC.oracle(BY_R[:0], ON_R[:0], BY_S, ON_S, 0)
    assert len(rows) == 0 and matched == 0
    rows, matched = AC.oracle(BY_R, ON_R, BY_S[:0], ON_S[:0], 0)
    assert [int(r) for r in rows] == [NO] * 8 and matched == 0


def test_the_oracle_is_pandas_merge_asof():
    """on sorted int64 inputs, both directions, both allow_exact_matches settings, with and without tolerance, with and without by;
    S holds duplicate (by, on): the contract's tie rule -- backward the last of the duplicates, forward the first -- is pandas'"""
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(11)
    for nR, nS, span in ((50, 40, 30), (200, 300, 60), (300, 100, 2000)):
        onR = np.sort(rng.integers(-span, span, nR)).astype(np.int64)
        onS = np.sort(rng.integers(-span, span, nS)).astype(np.int64)
        byR, byS = rng.integers(0, 4, nR).astype(np.int64), rng.integers(0, 3, nS).astype(np.int64)
        assert len(set(zip(byS.tolist(), onS.tolist()))) < nS or span > 1000              # duplicates of (by, on) in S
        for with_by in (False, True):
            left = pd.DataFrame({"on": onR, "by": byR})
            right = pd.DataFrame({"on": onS, "by": byS, "j": np.arange(nS)})
            for direction in ("backward", "forward"):
                for exact in (True, False):
                    for tol in (None, 0, 3, 25):
                        got = pd.merge_asof(left, right, on="on", by="by" if with_by else None, direction=direction,
                                            allow_exact_matches=exact, tolerance=tol)["j"]
                        want = np.where(got.isna(), -1, got.fillna(0)).astype(np.int64).view(np.uint64)
                        flags = (AC.ASOF_I64 | (AC.ASOF_FORWARD if direction == "forward" else 0) | (0 if exact else AC.ASOF_STRICT) |
                                 (AC.ASOF_TOLERANCE if tol is not None else 0))
                        rows, _ = AC.oracle(byR.view(np.uint64) if with_by else None, onR.view(np.uint64),
                                            byS.view(np.uint64) if with_by else None, onS.view(np.uint64), flags, tol or 0)
                        assert np.array_equal(rows, want), (nR, nS, with_by, direction, exact, tol)


def test_case_generators_split_the_window_shapes_between_the_tables():
    T = 4096
    for shape in AC.SHAPES:
        for kind in AC.ONS:
            byR, onR, byS, onS = AC.make_tables(shape, kind, 3000, 2000, T)
            assert [a.dtype for a in (byR, onR, byS, onS)] == [np.uint64] * 4 and len(byR) == len(onR) == 3000 and len(byS) == len(onS) == 2000
    byR, onR, byS, onS = AC.make_tables("runs64", "sixteen", 3000, 2000, T)
    assert len(np.intersect1d(byR, byS)) > 50 and len(np.intersect1d(onR, onS)) > 8     # shared partitions, exact matches
    byR, onR, byS, onS = AC.make_tables("each", "distinct", 30, 20, T)
    assert len(np.intersect1d(byR, byS)) == 0 and len(np.intersect1d(onR, onS)) == 0
    assert AC.make_tables("one", "extremes", 5, 5, T, by=False)[0] is None
    x = np.concatenate(AC.make_tables("one", "extremes", 500, 500, T)[1::2])
    for w in (0, (1 << 63) - 1, 1 << 63, (1 << 64) - 1):
        assert (x == np.uint64(w)).any()
    assert AC.splits(9) == [(5, 4), (8, 1), (1, 8), (9, 0), (0, 9)] and AC.splits(1) == [(1, 0), (0, 1)] and AC.splits(0) == [(0, 0)]
