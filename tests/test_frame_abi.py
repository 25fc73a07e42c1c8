"""CPU suite: the frame entry is part of the C-ABI -- declared in include/rhj.h with its argument names and constants directly behind
rhj_group_arg_dev and in front of the composite-key block, exported by librhj_hip.so, bound in binding.SYMBOLS with its argument
types -- and the addition left RHJ_ABI_VERSION at 3.  Engine.frame_columns and Engine.ntile_columns refuse wrong arguments before
they touch a device.  The two oracles of the GPU tests (tests/frame_cases.py) agree on a grid of tiny tables and are checked by hand
on eight rows."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import radixhashjoin_amd as rhj
from radixhashjoin_amd import binding

import frame_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _u64, _u32, _P = C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER
ENTRIES = {
    "rhj_frame_cols_dev": (["ctx", "d_part", "d_order", "n", "flags", "ops", "preceding", "following", "d_cols", "nops", "d_outs",
                            "out_partitions"],
                           [_vp, _vp, _vp, _u64, _u32, _P(_u32), _P(_u64), _P(_u64), _P(_vp), _u32, _P(_vp), _P(_u64)]),
}
CONSTANTS = {"FRAME_MAX_OPS": 4, "FRAME_COUNT": 0, "FRAME_SUM": 1, "FRAME_MIN_U64": 2, "FRAME_MAX_U64": 3, "FRAME_MIN_I64": 4,
             "FRAME_MAX_I64": 5, "FRAME_FIRST_ROW": 6, "FRAME_LAST_ROW": 7}


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
        assert re.search(r"#define\s+RHJ_" + name + r"\s+" + str(value) + r"(?!\w)", h), name
    assert re.search(r"#define\s+RHJ_FRAME_UNBOUNDED\s+0xFFFFFFFFFFFFFFFFull(?!\w)", h)
    assert re.search(r"#define\s+RHJ_ABI_VERSION\s+3\b", h)


def test_the_block_stands_behind_the_group_arg_entries_and_before_the_composite_keys():
    h = header()
    at = {name: h.index(name + "(") for name in ("rhj_group_arg_dev", "rhj_frame_cols_dev", "rhj_keys_layout", "rhj_keys_plan_free",
                                                 "rhj_histogram")}
    assert at["rhj_group_arg_dev"] < at["rhj_frame_cols_dev"] < h.index("RHJ_KEYS_MAX_COLS") < at["rhj_keys_layout"]
    assert h[at["rhj_group_arg_dev"]:at["rhj_frame_cols_dev"]].count("(") == 1, "a declaration stands between rhj_group_arg_dev and rhj_frame_cols_dev"
    assert at["rhj_group_arg_dev"] < h.index("RHJ_FRAME_MAX_OPS") < h.index("RHJ_FRAME_LAST_ROW") < at["rhj_frame_cols_dev"]
    assert "frame" not in h[at["rhj_keys_plan_free"]:at["rhj_histogram"]].lower()     # nothing of it among the as-of, sort, top-k and window blocks


def test_library_exports_it_and_binding_knows_its_types():
    lib = rhj.load_library()
    for name, (_, types) in ENTRIES.items():
        assert isinstance(getattr(lib, name), C._CFuncPtr)
        res, args = binding.SYMBOLS[name]
        assert res is C.c_int and list(args) == types
    for method in ("frame_cols_dev", "frame_columns", "ntile_columns"):
        assert callable(getattr(rhj.Engine, method))


def test_constants_are_exported():
    for name, value in dict(CONSTANTS, FRAME_UNBOUNDED=(1 << 64) - 1).items():
        assert getattr(rhj, name) == getattr(binding, name) == value and name in rhj.__all__
    assert (FC.COUNT, FC.SUM, FC.MIN_U64, FC.MAX_U64, FC.MIN_I64, FC.MAX_I64, FC.FIRST_ROW, FC.LAST_ROW) == tuple(CONSTANTS.values())[1:]
    assert FC.UNBOUNDED == rhj.FRAME_UNBOUNDED and FC.MAX_OPS == rhj.FRAME_MAX_OPS


def test_abi_version_is_still_3():
    assert rhj.load_library().rhj_abi_version() == 3


def test_signatures_and_defaults_of_the_torch_entries():
    p = inspect.signature(rhj.Engine.frame_columns).parameters
    assert list(p) == ["self", "part", "order", "cols", "ops", "preceding", "following", "descending", "unsigned"]
    assert p["preceding"].default is None and p["following"].default == 0
    assert p["descending"].default is False and p["unsigned"].default is False
    assert all(p[k].default is inspect.Parameter.empty for k in ("part", "order", "cols", "ops"))
    p = inspect.signature(rhj.Engine.frame_cols_dev).parameters
    assert list(p)[:10] == ["self", "d_part", "d_order", "n", "flags", "ops", "preceding", "following", "d_cols", "d_outs"]
    assert p["flags"].default == 0 and p["preceding"].default is None and p["following"].default is None
    p = inspect.signature(rhj.Engine.ntile_columns).parameters
    assert list(p)[:4] == ["self", "part", "order", "buckets"]
    assert all(p[k].default is inspect.Parameter.empty for k in ("part", "order", "buckets"))


def test_value_errors_come_before_any_device_use():
    """an Engine that was never constructed reaches every one of them"""
    e = rhj.Engine.__new__(rhj.Engine)
    e.ctx = None
    f = e.frame_columns
    with pytest.raises(ValueError, match="^ops: a sequence of op names is needed, not the string 'sum'"):
        f(None, None, [0], "sum")
    with pytest.raises(ValueError, match="^ops: at least one op is needed"):
        f(None, None, [], [])
    with pytest.raises(ValueError, match="^ops: at most 4 ops per call, not 5"):
        f(None, None, [None] * 5, ["count"] * 5)
    for bad in ("cumsum", "MIN", 1, None):
        with pytest.raises(ValueError, match=r"^ops\[1\]: one of 'count', 'sum', 'min', 'max', 'first_row', 'last_row', not "):
            f(None, None, [None, None], ["count", bad])
    with pytest.raises(ValueError, match="^cols: 1 entries for 2 ops"):
        f(None, None, [None], ["count", "count"])
    with pytest.raises(ValueError, match=r"^cols\[0\]: 'count' takes no column"):
        f(None, None, [0], ["count"])
    for op in ("sum", "min", "max"):
        with pytest.raises(ValueError, match=r"^cols\[1\]: '" + op + "' needs a tensor"):
            f(None, None, [None, None], ["count", op])
    for name in ("preceding", "following"):
        for bad in (-1, True, 1.0, "3", 1 << 64):
            with pytest.raises(ValueError, match="^" + name + r": an int >= 0 \(below 2\^64\) or None \(unbounded\) is needed"):
                f(None, None, (), ["count"], **{name: bad})
            with pytest.raises(ValueError, match="^" + name + r"\[1\]: an int >= 0"):
                f(None, None, (), ["count", "count"], **{name: [0, bad]})
        with pytest.raises(ValueError, match="^" + name + ": 3 entries for 2 ops"):
            f(None, None, (), ["count", "count"], **{name: [0, 1, 2]})
    for bad in (1, None, [True]):
        with pytest.raises(ValueError, match="^descending: a bool"):
            f(None, None, (), ["count"], descending=bad)
        with pytest.raises(ValueError, match="^unsigned: a bool"):
            f(None, None, (), ["count"], unsigned=bad)
    with pytest.raises(ValueError, match="^descending: True needs an order tensor"):
        f(None, None, (), ["count"], descending=True)
    with pytest.raises(ValueError, match="^order: one tensor or None"):
        f(None, [0, 0], (), ["count"])
    with pytest.raises(ValueError, match="^part, order and cols are all None"):
        f(None, None, (), ["count"])
    for bad in (0, -3, True, 2.0, None, "4"):
        with pytest.raises(ValueError, match="^buckets: an int >= 1"):
            e.ntile_columns(None, None, bad)


def test_header_states_the_contract():
    h = re.sub(r"\s*\n \* ", " ", header(strip_comments=False))       # (comment lines joined: a phrase may wrap)
    for phrase in ("[max(0, q - preceding[j]), min(m - 1, q + following[j])]",
                   "computed without wrap-around: q + following[j] saturates",
                   'RHJ_FRAME_UNBOUNDED (all ones) on either side means "to the partition\'s edge"',
                   "preceding == NULL: unbounded for every op; following == NULL: 0 for every op",
                   "The frame always contains the current row",
                   "value-based RANGE frames, are not part of this entry",
                   "Ties keep their input order in both directions", "bit-identical from run to run",
                   "a non-zero flags with d_order == NULL is RHJ_E_INVALID",
                   "the sum mod 2^64", "bit for bit a column word", "there is never RHJ_NO_ROW",
                   "rhj_gather_u64(ctx, x, first, n, x_first)",
                   "PERCENT_RANK is m > 1 ? (rk - 1) / (m - 1) : 0", "Two calls, so two sets of sorts",
                   "n == 0: RHJ_OK, no launch, 0 partitions",
                   "before any launch, with a message naming the argument",
                   "an op above RHJ_FRAME_LAST_ROW", "a NULL d_cols[j] for a column op with n > 0",
                   "Inputs are neither modified nor retained",
                   "stored BY SORTED POSITION", "S[hi] - (lo above the start ? S[lo - 1] : 0)",
                   "it is F[hi], B[lo] or op(B[lo], F[hi])",
                   "the mirrored position n - 1 - p",
                   "No workgroup waits on another inside a kernel, and no position, value or count comes from an atomic",
                   '"last.frame_units"', '"last.frame_sorts"', '"last.frame_partitions"', '"last.frame_scans"',
                   "all four are 0 after every other call",
                   '"last.join_kernel" is -1', '"last.sort_*" / "last.topk_*" / "last.window_*" / "last.asof_*" are 0',
                   '"sort.max_units" caps them here too', "the result never depends on it",
                   "kept until rhj_release_workspace",
                   "There is no 16-byte tuple form"):
        assert phrase in h, phrase


def test_the_two_oracles_agree_on_a_grid_of_tiny_tables():
    """minimum and maximum in both views under every pair of frame bounds, with and without partition and order columns; SUM against the
    cumulative sums"""
    rng = np.random.default_rng(5)
    bounds = (0, 1, 2, 5, 64, FC.UNBOUNDED)
    cases = 0
    for n in (1, 2, 7, 33, 70):
        for parts in (None, 1, 3, n):
            for kind in ("none", "sixteen", "extremes"):
                part = rng.integers(0, parts, n).astype(np.uint64) * np.uint64(1 << 62) if parts else None
                order = FC.make_order(kind, n, seed=cases)
                col = FC.make_values("extremes" if cases % 2 else "mixed", n, seed=cases)
                flags = FC.FLAGS[cases % 4] if order is not None else 0
                for pre in bounds:
                    for fol in bounds:
                        want, _ = FC.brute(part, order, flags, FC.EXTREMES + (FC.SUM,), [pre] * 5, [fol] * 5, [col] * 5)
                        got = FC.windows(part, order, flags, FC.EXTREMES, [pre] * 4, [fol] * 4, [col] * 4)
                        for j in range(4):
                            assert np.array_equal(got[j], want[j]), (n, parts, kind, flags, pre, fol, j)
                        assert np.array_equal(FC.sums(part, order, flags, col, pre, fol), want[4]), (n, parts, kind, flags, pre, fol)
                cases += 1
    assert cases == 5 * 4 * 3


ONES, TOP = (1 << 64) - 1, 1 << 63
# partitions B = 3 (rows 6, 1, 4 in order) and A = 7 (rows 2, 5 -- a tie, in input order --, 3, 0, 7).  B's values in order: 0, all
# ones, 2; A's: 1 << 63, (1 << 63) - 1, 5, 1, all ones
PART = np.array([7, 3, 7, 7, 3, 7, 3, 7], dtype=np.uint64)
ORDER = np.array([30, 10, 10, 20, 20, 10, 5, 40], dtype=np.uint64)
VALUE = np.array([1, ONES, TOP, 5, 2, TOP - 1, 0, ONES], dtype=np.uint64)


def test_the_oracles_by_hand_on_eight_rows():
    U = FC.UNBOUNDED

    def one(ops, pre, fol):
        outs, parts = FC.brute(PART, ORDER, 0, ops, [pre] * len(ops), [fol] * len(ops), [VALUE] * len(ops))
        assert parts == 2
        for j, o in enumerate(FC.windows(PART, ORDER, 0, ops, [pre] * len(ops), [fol] * len(ops), [VALUE] * len(ops))):
            assert o is None or np.array_equal(o, outs[j])
        return [[int(x) for x in o] for o in outs]

    # one row before and one behind.  COUNT: 2 at a partition's two ends, 3 inside
    count, total = one([FC.COUNT, FC.SUM], 1, 1)
    assert count == [3, 3, 2, 3, 2, 3, 2, 2]
    # SUM wraps: B 0 + ones = ones | 0 + ones + 2 = 1 | ones + 2 = 1; A 2^63 + (2^63 - 1) = ones | .. + 5 = 4 | (2^63 - 1) + 5 + 1 | 5 + 1 +
    # ones = 5 | 1 + ones = 0
    assert total == [5, 1, ONES, TOP + 5, 1, 4, ONES, 0]
    assert np.array_equal(FC.sums(PART, ORDER, 0, VALUE, 1, 1), np.array(total, dtype=np.uint64))
    # both views: unsigned the minimum of (2^63, 2^63 - 1) is 2^63 - 1; signed all ones is -1, 2^63 the minimum, 2^63 - 1 the maximum
    lo_u, hi_i = one([FC.MIN_U64, FC.MAX_I64], 1, 1)
    assert lo_u == [1, 0, TOP - 1, 1, 2, 5, 0, 1]
    assert hi_i == [5, 2, TOP - 1, TOP - 1, 2, TOP - 1, 0, 1]
    # the whole partition
    hi_u, lo_i, size = one([FC.MAX_U64, FC.MIN_I64, FC.COUNT], U, U)
    assert hi_u == [ONES] * 8 and lo_i == [TOP, ONES, TOP, TOP, ONES, TOP, ONES, TOP] and size == [5, 3, 5, 5, 3, 5, 3, 5]
    # the row before (the row itself at a partition's first position), and the partition's last row
    assert one([FC.FIRST_ROW], 1, 0) == [[3, 6, 2, 5, 1, 2, 6, 0]]
    assert one([FC.LAST_ROW], 0, U) == [[7, 4, 7, 7, 4, 7, 4, 7]]
    assert one([FC.FIRST_ROW, FC.LAST_ROW], 0, 0) == [list(range(8))] * 2
    # descending: the order inside a partition turns round, ties still in input order -- A: 7, 0, 3, 2, 5
    outs, _ = FC.brute(PART, ORDER, FC.SORT_DESC, [FC.FIRST_ROW, FC.SUM], [1, U], [0, 0], [None, VALUE])
    assert [int(x) for x in outs[0]] == [7, 4, 3, 0, 4, 2, 1, 7]
    assert [int(x) for x in outs[1]] == [0, 1, TOP + 5, 5, 2, 4, 1, ONES]      # running sums from the other end
    # the defaults are the running frame
    assert np.array_equal(FC.brute(PART, ORDER, 0, [FC.SUM], None, None, [VALUE])[0][0], FC.sums(PART, ORDER, 0, VALUE, U, 0))
    outs, parts = FC.brute(PART[:0], ORDER[:0], 0, [FC.COUNT], None, None, None, n=0)
    assert len(outs) == 1 and len(outs[0]) == 0 and parts == 0
    assert FC.ntile(PART, ORDER, 0, 2).tolist() == [2, 1, 1, 1, 2, 1, 1, 2] and FC.ntile(PART, ORDER, 0, 4).tolist() == [3, 2, 1, 2, 3, 1, 1, 4]
    assert FC.value_scans(8, [FC.COUNT, FC.SUM, FC.MIN_U64, FC.MAX_I64], [1, 1, 1, 7], [1, 1, 1, 0]) == 0 + 1 + 2 + 1
