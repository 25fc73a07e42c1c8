"""CPU suite: the RANGE frame entry is part of the C-ABI -- declared in include/rhj.h with its argument names directly behind
rhj_frame_cols_dev and in front of the composite-key block, exported by librhj_hip.so, bound in binding.SYMBOLS with its argument
types -- and the addition left RHJ_ABI_VERSION at 3.  Engine.frame_range_columns refuses wrong arguments before it touches a device.
The two oracles of the GPU tests (tests/frame_range_cases.py) agree on a grid of tiny tables and are checked by hand on eight rows."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import radixhashjoin_amd as rhj
from radixhashjoin_amd import binding

import frame_cases as FC
import frame_range_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _u64, _u32, _P = C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER
NAME = "rhj_frame_range_cols_dev"
ARGS = ["ctx", "d_part", "d_order", "n", "flags", "ops", "preceding", "following", "d_cols", "nops", "d_outs", "out_partitions"]
TYPES = [_vp, _vp, _vp, _u64, _u32, _P(_u32), _P(_u64), _P(_u64), _P(_vp), _u32, _P(_vp), _P(_u64)]


def header(strip_comments=True):
    with open(os.path.join(ROOT, "include", "rhj.h")) as f:
        h = f.read()
    return re.sub(r"/\*.*?\*/", " ", h, flags=re.S) if strip_comments else h


def test_header_declares_the_entry_with_its_argument_names():
    h = header()
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", h)
    assert m, f"include/rhj.h does not declare {NAME}"
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    frame = re.search(r"\bint\s+rhj_frame_cols_dev\s*\(([^)]*)\)\s*;", h)
    assert re.sub(r"\s+", " ", frame.group(1)) == re.sub(r"\s+", " ", m.group(1)), "the argument list is the frame entry's"
    assert re.search(r"#define\s+RHJ_ABI_VERSION\s+3\b", h)


def test_the_declaration_stands_behind_the_frame_entry_and_before_the_composite_keys():
    h = header()
    at = {name: h.index(name + "(") for name in ("rhj_group_arg_dev", "rhj_frame_cols_dev", NAME, "rhj_keys_layout")}
    assert at["rhj_group_arg_dev"] < at["rhj_frame_cols_dev"] < at[NAME] < h.index("RHJ_KEYS_MAX_COLS") < at["rhj_keys_layout"]
    assert h[at["rhj_frame_cols_dev"]:at[NAME]].count("(") == 1, "a declaration stands between rhj_frame_cols_dev and " + NAME
    assert h.count(NAME + "(") == 1


def test_library_exports_it_and_binding_knows_its_types():
    lib = rhj.load_library()
    assert isinstance(getattr(lib, NAME), C._CFuncPtr)
    res, args = binding.SYMBOLS[NAME]
    assert res is C.c_int and list(args) == TYPES
    assert list(args) == list(binding.SYMBOLS["rhj_frame_cols_dev"][1])
    for method in ("frame_range_cols_dev", "frame_range_columns"):
        assert callable(getattr(rhj.Engine, method))
    assert (RC.COUNT, RC.SUM, RC.MIN_U64, RC.MAX_U64, RC.MIN_I64, RC.MAX_I64, RC.FIRST_ROW, RC.LAST_ROW) == (
        rhj.FRAME_COUNT, rhj.FRAME_SUM, rhj.FRAME_MIN_U64, rhj.FRAME_MAX_U64, rhj.FRAME_MIN_I64, rhj.FRAME_MAX_I64, rhj.FRAME_FIRST_ROW,
        rhj.FRAME_LAST_ROW)
    assert RC.UNBOUNDED == rhj.FRAME_UNBOUNDED
    assert "rhj_frame_range_cols_dev" in rhj.__doc__ and "frame_range_columns" in rhj.__doc__


def test_abi_version_is_still_3():
    assert rhj.load_library().rhj_abi_version() == 3


def test_signatures_and_defaults_of_the_python_entries():
    p = inspect.signature(rhj.Engine.frame_range_columns).parameters
    assert list(p) == ["self", "part", "order", "cols", "ops", "preceding", "following", "descending", "unsigned"]
    assert p["preceding"].default is None and p["following"].default == 0
    assert p["descending"].default is False and p["unsigned"].default is False
    assert all(p[k].default is inspect.Parameter.empty for k in ("part", "order", "cols", "ops"))
    p = inspect.signature(rhj.Engine.frame_range_cols_dev).parameters
    assert list(p) == list(inspect.signature(rhj.Engine.frame_cols_dev).parameters)
    assert p["flags"].default == 0 and p["preceding"].default is None and p["following"].default is None


def test_value_errors_come_before_any_device_use():
    """an Engine that was never constructed reaches every one of them; `order` only has to be there for most"""
    e = rhj.Engine.__new__(rhj.Engine)
    e.ctx = None
    f = e.frame_range_columns
    for bad in (None, [0, 0], (0,)):
        with pytest.raises(ValueError, match="^order: one tensor is needed -- a value distance needs a value"):
            f(None, bad, (), ["count"])
    with pytest.raises(ValueError, match="^ops: a sequence of op names is needed, not the string 'sum'"):
        f(None, 0, [0], "sum")
    with pytest.raises(ValueError, match="^ops: at least one op is needed"):
        f(None, 0, [], [])
    with pytest.raises(ValueError, match="^ops: at most 4 ops per call, not 5"):
        f(None, 0, [None] * 5, ["count"] * 5)
    for bad in ("cumsum", "MIN", 1, None):
        with pytest.raises(ValueError, match=r"^ops\[1\]: one of 'count', 'sum', 'min', 'max', 'first_row', 'last_row', not "):
            f(None, 0, [None, None], ["count", bad])
    with pytest.raises(ValueError, match="^cols: 1 entries for 2 ops"):
        f(None, 0, [None], ["count", "count"])
    with pytest.raises(ValueError, match=r"^cols\[0\]: 'count' takes no column"):
        f(None, 0, [0], ["count"])
    for op in ("sum", "min", "max"):
        with pytest.raises(ValueError, match=r"^cols\[1\]: '" + op + "' needs a tensor"):
            f(None, 0, [None, None], ["count", op])
    for name in ("preceding", "following"):
        for bad in (-1, True, 1.0, "3", 1 << 64):
            with pytest.raises(ValueError, match="^" + name + r": an int >= 0 \(below 2\^64\) or None \(unbounded\) is needed"):
                f(None, 0, (), ["count"], **{name: bad})
            with pytest.raises(ValueError, match="^" + name + r"\[1\]: an int >= 0"):
                f(None, 0, (), ["count", "count"], **{name: [0, bad]})
        with pytest.raises(ValueError, match="^" + name + ": 3 entries for 2 ops"):
            f(None, 0, (), ["count", "count"], **{name: [0, 1, 2]})
    for bad in (1, None, [True]):
        with pytest.raises(ValueError, match="^descending: a bool"):
            f(None, 0, (), ["count"], descending=bad)
        with pytest.raises(ValueError, match="^unsigned: a bool"):
            f(None, 0, (), ["count"], unsigned=bad)
    with pytest.raises(ValueError, match="^order: a 1-D torch tensor of 64-bit integers is needed"):
        f(None, 0, (), ["count"])
    with pytest.raises(ValueError, match="^order: a 1-D torch tensor of 64-bit integers is needed"):
        f(None, np.zeros(3, dtype=np.int64), (), ["count"], 2**64 - 2, None)


def test_header_states_the_contract():
    h = re.sub(r"\s*\n \* ", " ", header(strip_comments=False))       # (comment lines joined: a phrase may wrap)
    block = h[h.index("/* ---- RANGE frames"):h.index("int " + NAME)]
    for phrase in ("The argument list, the RHJ_FRAME_* ops and RHJ_FRAME_UNBOUNDED are rhj_frame_cols_dev's",
                   "are the frame entry's, word for word",
                   "a bit-equal d_part word", "d_part == NULL: one partition",
                   "ties keep their input order in both directions", "aligned with the input rows", "bit-identical from run to run",
                   "d_order == NULL is RHJ_E_INVALID: a value distance needs a value",
                   "lies in [t - preceding[j], t + following[j]]",
                   "under RHJ_SORT_DESC the interval is [t - following[j], t + preceding[j]]",
                   'PRECEDING still means "earlier in the order"',
                   "Distances are exact integers", "both ends saturate at the view's minimum and maximum, nothing wraps",
                   "a distance of 2^64 - 2 between INT64_MIN and INT64_MAX is honoured",
                   "RHJ_FRAME_UNBOUNDED (all ones) on a side is the partition's edge, which is also what a distance of 2^64 - 1 means",
                   "preceding == NULL: unbounded for every op; following == NULL: 0 for every op",
                   "SQL's default frame, RANGE UNBOUNDED PRECEDING to CURRENT ROW",
                   "a contiguous run of sorted positions",
                   "always contains the current row and all its peers, also at distance 0: this is the difference from ROWS",
                   "pandas' time-based rolling stops at the current row among peers, so the results agree with pandas exactly when the "
                   "order keys are distinct within a partition",
                   "Frames that exclude the current row are not part of this entry", "there is never RHJ_NO_ROW",
                   "Each op has its own frame",
                   "the sum mod 2^64", "bit for bit a column word", "which the tie rule defines",
                   "n == 0: RHJ_OK, no launch, 0 partitions",
                   "before any launch, with a message naming the argument",
                   "unknown flag bits", "d_order == NULL with n > 0 or with flags",
                   "an op above RHJ_FRAME_LAST_ROW", "a NULL d_cols[j] for a column op with n > 0",
                   "Inputs are neither modified nor retained",
                   "it honours rhj_set_stream and rhj_set_profiling",
                   "max(0, v - preceding) <= v_r <= min(2^64 - 1, v + following)",
                   "S[hi] - (lo above the start ? S[lo - 1] : 0)",
                   "at the FIXED block length 64", "op(T_l[bl + 1], T_l[bh - 2^l])", "at most 62 words",
                   "table words that span a partition boundary are never read",
                   "No workgroup waits on another inside a kernel, and no position, value or count comes from an atomic",
                   '"last.frame_range_units"', '"last.frame_range_sorts"', '"last.frame_range_partitions"', '"last.frame_range_scans"',
                   '"last.frame_range_levels"', "0 when no op needed them",
                   "All five are 0 after every other call",
                   '"last.join_kernel" is -1', "every other entry's \"last.*\" (the frame entry's included) is 0",
                   "kept until rhj_release_workspace",
                   "There is no 16-byte tuple form"):
        assert phrase in block, phrase


DISTANCES = (0, 1, 5, 1 << 63, (1 << 64) - 2, RC.UNBOUNDED)
ALL_OPS = (RC.COUNT, RC.SUM, RC.MIN_U64, RC.MAX_U64, RC.MIN_I64, RC.MAX_I64, RC.FIRST_ROW, RC.LAST_ROW)


def test_the_two_oracles_agree_on_a_grid_of_tiny_tables():
    """every op under every pair of distances, in all four views, with tie-heavy, distinct and extreme-word order columns"""
    rng = np.random.default_rng(6)
    cases = 0
    for n in (1, 2, 7, 33, 70):
        for parts in (None, 3):
            for kind in ("sixteen", "distinct", "extremes", "near"):
                part = rng.integers(0, parts, n).astype(np.uint64) * np.uint64(1 << 62) if parts else None
                order = RC.make_order(kind, n, seed=cases)
                col = FC.make_values("extremes" if cases % 2 else "mixed", n, seed=cases)
                for flags in RC.FLAGS:
                    for pre in DISTANCES:
                        for fol in DISTANCES:
                            want, wp = RC.brute(part, order, flags, ALL_OPS, [pre] * 8, [fol] * 8, [col] * 8)
                            got, gp = RC.fast(part, order, flags, ALL_OPS, [pre] * 8, [fol] * 8, [col] * 8)
                            assert wp == gp
                            for j in range(8):
                                assert np.array_equal(got[j], want[j]), (n, parts, kind, flags, pre, fol, j)
                cases += 1
    assert cases == 5 * 2 * 4


ONES, TOP = (1 << 64) - 1, 1 << 63
# Partition A = 7: rows 0, 2, 3, 5, 7 with order words 10, 10 (a peer pair), 12, all ones, 0; partition B = 3: rows 1, 4, 6 with 5,
# 1 << 63, (1 << 63) - 1.  Unsigned A reads 7 (0), 0 (10), 2 (10), 3 (12), 5 (2^64 - 1) and B 1, 6, 4; signed A reads 5 (-1), 7, 0, 2, 3
# and B 4 (INT64_MIN), 1, 6 (INT64_MAX).
PART = np.array([7, 3, 7, 7, 3, 7, 3, 7], dtype=np.uint64)
ORDER = np.array([10, 5, 10, 12, TOP, ONES, TOP - 1, 0], dtype=np.uint64)
VALUE = np.array([1, 100, 2, 4, 200, 8, 400, 16], dtype=np.uint64)


def test_the_oracles_by_hand_on_eight_rows():
    U = RC.UNBOUNDED

    def one(flags, ops, pre, fol):
        pre, fol = [pre] * len(ops) if pre != "null" else None, [fol] * len(ops) if fol != "null" else None
        outs, parts = RC.brute(PART, ORDER, flags, ops, pre, fol, [VALUE] * len(ops))
        again, parts2 = RC.fast(PART, ORDER, flags, ops, pre, fol, [VALUE] * len(ops))
        assert parts == parts2 == 2
        for a, b in zip(outs, again):
            assert np.array_equal(a, b)
        return [[int(x) for x in o] for o in outs]

    # unsigned, two before: rows 0 and 2 are peers at distance 0 and share every value -- row 0's frame holds row 2, which stands
    # BEHIND it; row 3 reaches both; row 4 (2^63) reaches row 6 (2^63 - 1); row 7 (0) saturates at the view's minimum
    total, count, first, last = one(0, [RC.SUM, RC.COUNT, RC.FIRST_ROW, RC.LAST_ROW], 2, 0)
    assert total == [3, 100, 3, 7, 600, 8, 400, 16] and count == [2, 1, 2, 3, 2, 1, 1, 1]
    assert first == [0, 1, 0, 0, 6, 5, 6, 7] and last == [2, 1, 2, 3, 4, 5, 6, 7]
    assert one(0, [RC.COUNT], 0, 0) == [[2, 1, 2, 1, 1, 1, 1, 1]]                     # distance 0 on both sides: the peers
    # unsigned, 2^64 - 2 behind: from 0 it reaches everything but all ones (a saturating bound would be 2^64 - 1); from 10 and from 5
    # the upper end saturates at the view's maximum
    assert one(0, [RC.SUM], 0, ONES - 1) == [[15, 700, 15, 12, 200, 8, 600, 23]]
    # signed, 2^64 - 2 before: from INT64_MAX (row 6) it reaches 5 but NOT INT64_MIN (row 4), which is 2^64 - 1 away; everywhere else
    # the lower end saturates at INT64_MIN
    assert one(RC.SORT_I64, [RC.SUM, RC.COUNT], ONES - 1, 0) == [[27, 300, 27, 31, 200, 8, 500, 24], [4, 2, 4, 5, 1, 1, 2, 2]]
    assert one(RC.SORT_I64, [RC.COUNT], U, 0)[0][6] == 3                              # ... and all ones reaches it
    assert one(RC.SORT_I64, [RC.MAX_I64, RC.MIN_U64], 2, 0) == [[2, 100, 2, 4, 200, 8, 400, 16], [1, 100, 1, 1, 200, 8, 400, 8]]
    # descending, unsigned: PRECEDING is towards LARGER values -- [t, t + 2]; row 0's frame is rows 3, 0, 2 in order
    count, first, last = one(RC.SORT_DESC, [RC.COUNT, RC.FIRST_ROW, RC.LAST_ROW], 2, 0)
    assert count == [3, 1, 3, 1, 1, 1, 2, 1] and first == [3, 1, 3, 3, 4, 5, 4, 7] and last == [2, 1, 2, 3, 4, 5, 6, 7]
    assert one(RC.SORT_DESC, [RC.COUNT], ONES - 1, 0) == [[4, 3, 4, 2, 1, 1, 2, 4]]   # 0 reaches 2^64 - 2, not all ones
    # descending, signed: INT64_MIN (row 4, last in order) reaches 5 but not INT64_MAX
    assert one(RC.SORT_DESC | RC.SORT_I64, [RC.COUNT], ONES - 1, 0) == [[3, 2, 3, 1, 2, 5, 1, 4]]
    # the defaults are SQL's default frame: the running sum in which peers share a value
    assert one(0, [RC.SUM], "null", "null") == [[19, 100, 19, 23, 700, 31, 500, 16]]
    assert one(0, [RC.SUM], U, 0) == [[19, 100, 19, 23, 700, 31, 500, 16]]
    assert RC.value_scans([RC.COUNT, RC.SUM, RC.MIN_U64, RC.MAX_I64], [1, 1, 1, U], [1, 1, 1, 0]) == 0 + 1 + 2 + 1
    assert [RC.levels(n, [RC.MIN_U64], [1], [1]) for n in (1, 64, 128, 129, 192, 193, 256, 257, 320, 321)] == [0, 0, 0, 1, 1, 2, 2, 2, 2, 3]
    assert RC.levels(1000, [RC.MIN_U64, RC.SUM], [U, 1], [1, 1]) == 0


def test_the_path_counter_by_hand():
    """one partition of 300 positions and a second of 20: frames given by their two ends"""
    ps = np.array([0] * 6 + [300] * 2)
    pe = np.array([299] * 6 + [319] * 2)
    lo = np.array([0, 65, 70, 100, 60, 10, 300, 310])
    hi = np.array([10, 70, 127, 120, 130, 299, 305, 319])
    assert RC.paths(ps, pe, lo, hi) == {"start": 2, "end": 2, "walk": 2, "neighbours": 0, ("table", 1): 1, ("table", 3): 1}
    assert RC.paths(ps[:1], pe[:1], np.array([63]), np.array([64]))["neighbours"] == 1
    rank = RC.rank_order(np.array([5, 9, 5, 5, 9], dtype=np.uint64), 5)
    assert rank.tolist() == [0, 0, 1, 2, 1]
