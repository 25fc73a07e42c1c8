"""CPU suite: the window entry is part of the C-ABI -- declared in include/rhj.h with its argument names and constants directly behind
the top-k entries, exported by librhj_hip.so, bound in binding.SYMBOLS with its argument types -- and the addition left
RHJ_ABI_VERSION at 3.  Engine.window_columns / topk_per_group_columns refuse wrong arguments before they touch a device.  The oracle
of the GPU tests (tests/window_cases.py) is checked by hand on eight rows, and its generators have the shapes they are named for."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import radixhashjoin_amd as rhj
from radixhashjoin_amd import binding

import window_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _u64, _u32, _P = C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER
ENTRIES = {
    "rhj_window_cols_dev": (["ctx", "d_part", "d_order", "n", "flags", "ops", "args", "d_cols", "nops", "d_outs", "out_partitions"],
                            [_vp, _vp, _vp, _u64, _u32, _P(_u32), _P(_u64), _P(_vp), _u32, _P(_vp), _P(_u64)]),
}
CONSTANTS = {"WINDOW_MAX_OPS": 4, "WIN_ROW_NUMBER": 0, "WIN_RANK": 1, "WIN_DENSE_RANK": 2, "WIN_LAG_ROW": 3, "WIN_LEAD_ROW": 4,
             "WIN_CUMSUM": 5, "WIN_CUMMIN_U64": 6, "WIN_CUMMAX_U64": 7, "WIN_CUMMIN_I64": 8, "WIN_CUMMAX_I64": 9}


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
    assert re.search(r"#define\s+RHJ_ABI_VERSION\s+3\b", h)


def test_the_block_stands_directly_behind_the_topk_entries_and_before_the_stage_entries():
    h = header()
    at = {name: h.index(name + "(") for name in ("rhj_topk_cols_dev", "rhj_topk_dev", "rhj_window_cols_dev", "rhj_histogram")}
    assert at["rhj_topk_cols_dev"] < at["rhj_topk_dev"] < at["rhj_window_cols_dev"] < at["rhj_histogram"]
    assert h[at["rhj_topk_dev"]:at["rhj_window_cols_dev"]].count("(") == 1, "a declaration stands between rhj_topk_dev and rhj_window_cols_dev"
    assert h[at["rhj_window_cols_dev"]:at["rhj_histogram"]].count("(") == 1, "a declaration stands between rhj_window_cols_dev and rhj_histogram"
    assert at["rhj_topk_dev"] < h.index("RHJ_WINDOW_MAX_OPS") < h.index("RHJ_WIN_CUMMAX_I64") < at["rhj_window_cols_dev"]


def test_library_exports_it_and_binding_knows_its_types():
    lib = rhj.load_library()
    for name, (_, types) in ENTRIES.items():
        assert isinstance(getattr(lib, name), C._CFuncPtr)
        res, args = binding.SYMBOLS[name]
        assert res is C.c_int and list(args) == types
    for method in ("window_cols_dev", "window_columns", "topk_per_group_columns"):
        assert callable(getattr(rhj.Engine, method))


def test_constants_are_exported():
    for name, value in CONSTANTS.items():
        assert getattr(rhj, name) == getattr(binding, name) == value and name in rhj.__all__
    assert [WC.ROW_NUMBER, WC.RANK, WC.DENSE_RANK, WC.LAG_ROW, WC.LEAD_ROW, WC.CUMSUM, WC.CUMMIN_U64, WC.CUMMAX_U64, WC.CUMMIN_I64,
            WC.CUMMAX_I64] == [CONSTANTS[k] for k in list(CONSTANTS)[1:]] and WC.MAX_OPS == rhj.WINDOW_MAX_OPS
    assert int(WC.NO_ROW) == rhj.NO_ROW


def test_abi_version_is_still_3():
    assert rhj.load_library().rhj_abi_version() == 3


def test_signatures_and_defaults_of_the_torch_entries():
    p = inspect.signature(rhj.Engine.window_columns).parameters
    assert list(p) == ["self", "partition_by", "order_by", "values", "ops", "descending", "unsigned", "offsets", "fill"]
    assert p["order_by"].default is None and p["values"].default == () and p["ops"].default == ("row_number",)
    assert p["descending"].default is False and p["unsigned"].default is False and p["offsets"].default is None and p["fill"].default == 0
    p = inspect.signature(rhj.Engine.topk_per_group_columns).parameters
    assert list(p) == ["self", "partition_by", "order_by", "k", "descending", "unsigned"]
    assert p["descending"].default is False and p["unsigned"].default is False
    p = inspect.signature(rhj.Engine.window_cols_dev).parameters
    assert list(p)[:5] == ["self", "d_part", "d_order", "n", "flags"] and p["flags"].default == 0


def test_value_errors_come_before_any_device_use():
    """an Engine that was never constructed reaches every one of them"""
    e = rhj.Engine.__new__(rhj.Engine)
    e.ctx = None
    w = e.window_columns
    with pytest.raises(ValueError, match=r"^ops\[1\]: "):
        w(None, None, ops=["rank", "median"])
    with pytest.raises(ValueError, match=r"^ops\[0\]: "):
        w(None, None, ops=[3])
    with pytest.raises(ValueError, match="^ops: "):
        w(None, None, ops="rank")
    with pytest.raises(ValueError, match="^ops: at least one"):
        w(None, None, ops=[])
    with pytest.raises(ValueError, match="^ops: at most 4 ops"):
        w(None, None, ops=["row_number"] * 5)
    with pytest.raises(ValueError, match="^values: 1 entries for 2 ops"):
        w(None, None, values=[None], ops=["row_number", "rank"])
    with pytest.raises(ValueError, match="^offsets: 2 entries for 1 ops"):
        w(None, None, ops=["lag"], offsets=[1, 2])
    for bad in (1, None, [True]):
        with pytest.raises(ValueError, match="^descending: a bool"):
            w(None, 0, descending=bad)
        with pytest.raises(ValueError, match="^unsigned: a bool"):
            w(None, 0, unsigned=bad)
    for bad in (0, -1, 1.0, True, None):
        with pytest.raises(ValueError, match=r"^offsets\[1\]: an int >= 1"):
            w(None, None, ops=["rank", "lead"], offsets=[1, bad])
    with pytest.raises(ValueError, match="^descending: True needs an order_by"):
        w(None, None, descending=True)
    with pytest.raises(ValueError, match="^order_by: one tensor or None"):
        w(None, [None, None])
    with pytest.raises(ValueError, match=r"^values\[0\]: 'cumsum' needs a tensor"):
        w(None, None, ops=["cumsum"])
    with pytest.raises(ValueError, match=r"^values\[0\]: 'rank' takes no column"):
        w(None, None, values=[0], ops=["rank"])
    with pytest.raises(ValueError, match="^fill: an int"):
        w(None, None, ops=["lag"], fill=1.5)
    with pytest.raises(ValueError, match="all None"):
        w(None, None)
    t = e.topk_per_group_columns
    for bad in (2.0, "3", None, True):
        with pytest.raises(ValueError, match="^k: an int"):
            t(None, None, bad)
    with pytest.raises(ValueError, match="^k: a count"):
        t(None, None, -1)
    with pytest.raises(ValueError, match="^descending: True needs an order_by"):
        t(None, None, 3, descending=True)
    with pytest.raises(ValueError, match="^unsigned: a bool"):
        t(None, None, 3, unsigned=0)


def test_header_states_the_contract():
    h = re.sub(r"\s*\n \* ", " ", header(strip_comments=False))       # (comment lines joined: a phrase may wrap)
    for phrase in ("ROWS UNBOUNDED PRECEDING", "not SQL's default RANGE frame",
                   "Ties keep their input order in both directions",
                   "bit-identical from run to run",
                   "RHJ_NO_ROW where there is none",
                   "aligned with the input rows, not in sorted order",
                   "compared for equality only", "d_part == NULL: one partition",
                   "d_order == NULL: input order, and every row is its own peer",
                   "a non-zero flags with d_order == NULL is RHJ_E_INVALID",
                   "args == NULL: offset 1",
                   "the sum mod 2^64", "bit for bit a column word",
                   "two equal output pointers are undefined",
                   "rhj_gather_cols_fill(ctx, &x, 1, n, prev, n, &fill, &x_lag)",
                   "n == 0: RHJ_OK, no launch, 0 partitions",
                   "a lag or lead offset of 0",
                   "Inputs are neither modified nor retained",
                   "No workgroup waits on another inside a kernel", "no position or value comes from an atomic",
                   '"last.window_units"', '"last.window_sorts"', '"last.window_partitions"', '"window.tile_rows"',
                   "all three are 0 after every other call",
                   '"last.join_kernel" is -1',
                   "kept until rhj_release_workspace",
                   "There is no 16-byte tuple form"):
        assert phrase in h, phrase


ONES, TOP = (1 << 64) - 1, 1 << 63
NO = ONES
# eight rows: partition A = all ones (rows 0 2 3 5 7), partition B = 1 << 63 (rows 1 4 6), B before A as words; the order column
# holds ties, the all-ones word (the unsigned maximum, the signed -1) and 1 << 63 (the signed minimum)
PART = np.array([ONES, TOP, ONES, ONES, TOP, ONES, TOP, ONES], dtype=np.uint64)
ORDER = np.array([5, ONES, 5, 0, TOP, ONES, ONES, 0], dtype=np.uint64)
VALS = np.array([1, 2, ONES, 4, TOP, 6, 7, TOP], dtype=np.uint64)


def one(op, flags=0, off=1, part=PART, order=ORDER):
    outs, parts = WC.oracle(part, order, flags, [op], [off], [VALS])
    assert parts == (2 if part is not None else 1)
    return [int(x) for x in outs[0]]


def test_the_oracle_by_hand_on_eight_rows():
    # unsigned ascending: B = rows 4 1 6 (1 << 63, then the two all-ones words by position), A = rows 3 7 0 2 5 (0 0 5 5 ones)
    assert one(WC.ROW_NUMBER) == [3, 2, 4, 1, 1, 5, 3, 2]
    assert one(WC.RANK) == [3, 2, 3, 1, 1, 5, 2, 1]
    assert one(WC.DENSE_RANK) == [2, 2, 2, 1, 1, 3, 2, 1]
    assert one(WC.LAG_ROW) == [7, 4, 0, NO, NO, 2, 1, 3]
    assert one(WC.LEAD_ROW) == [2, 6, 5, 7, 1, NO, NO, 0]
    assert one(WC.LAG_ROW, off=2) == [3, NO, 7, NO, NO, 0, 4, NO]
    assert one(WC.LEAD_ROW, off=5) == [NO] * 8
    # A in order: 4, 4 + top, 5 + top, 5 + top + ones = 4 + top (the sum wraps), 10 + top; B: top, top + 2, top + 9
    assert one(WC.CUMSUM) == [TOP + 5, TOP + 2, TOP + 4, 4, TOP, TOP + 10, TOP + 9, TOP + 4]
    assert one(WC.CUMMIN_U64) == [1, 2, 1, 4, TOP, 1, 2, 4]
    assert one(WC.CUMMAX_U64) == [TOP, TOP, ONES, 4, TOP, ONES, TOP, TOP]
    assert one(WC.CUMMIN_I64) == [TOP, TOP, TOP, 4, TOP, TOP, TOP, TOP]           # 1 << 63 is the signed minimum
    assert one(WC.CUMMAX_I64) == [4, 2, 4, 4, TOP, 6, 7, 4]                         # all ones is -1
    # unsigned descending: B = rows 1 6 4, A = rows 5 0 2 3 7 -- ties STILL by position
    assert one(WC.ROW_NUMBER, WC.SORT_DESC) == [2, 1, 3, 4, 3, 1, 2, 5]
    assert one(WC.RANK, WC.SORT_DESC) == [2, 1, 2, 4, 3, 1, 1, 4]
    # int64 ascending: B = rows 4 1 6 (the minimum, then -1 -1), A = rows 5 3 7 0 2 (-1 0 0 5 5)
    assert one(WC.ROW_NUMBER, WC.SORT_I64) == [4, 2, 5, 2, 1, 1, 3, 3]
    # int64 descending: B = rows 1 6 4, A = rows 0 2 3 7 5
    assert one(WC.ROW_NUMBER, WC.SORT_I64 | WC.SORT_DESC) == [1, 1, 2, 3, 3, 5, 2, 4]
    assert one(WC.LAG_ROW, WC.SORT_I64 | WC.SORT_DESC) == [NO, NO, 0, 2, 6, 7, 1, 3]
    # no order column: input order, every row its own peer
    for op in (WC.ROW_NUMBER, WC.RANK, WC.DENSE_RANK):
        assert one(op, order=None) == [1, 1, 2, 3, 2, 4, 3, 5]
    # no partition column: one partition; neither: the plain running sum
    assert one(WC.RANK, part=None) == [3, 6, 3, 1, 5, 6, 6, 1]
    assert one(WC.CUMSUM, part=None, order=None) == [int(x) for x in np.cumsum(VALS, dtype=np.uint64)]
    outs, parts = WC.oracle(PART[:0], ORDER[:0], 0, [WC.RANK, WC.CUMSUM], None, [None, VALS[:0]])
    assert parts == 0 and [len(o) for o in outs] == [0, 0]


def test_case_generators_have_the_shapes_they_are_named_for():
    T = 4096

    def sizes_of(col):
        """partition sizes in sorted order of the words"""
        return np.unique(col, return_counts=True)[1].tolist()

    for n in (1, 65, 5000, 2 * T + 1):
        for shape in WC.SHAPES:
            col = WC.make_part(shape, n, T)
            assert col.dtype == np.uint64 and len(col) == n
            if shape != "zipf":
                assert sizes_of(col) == WC.part_sizes(shape, n, T), (shape, n)
        assert sizes_of(WC.make_part("one", n, T)) == [n] and sizes_of(WC.make_part("each", n, T)) == [1] * n
    n = 2 * T + 1
    assert sizes_of(WC.make_part("runs64", n, T)) == [64] * (n // 64) + [1]
    assert sizes_of(WC.make_part("runsT", n, T)) == [T, T, 1]
    assert sizes_of(WC.make_part("runsT-1", n, T)) == [T - 1, T - 1, 3]
    assert sizes_of(WC.make_part("runsT+1", n, T)) == [T + 1, T]
    e = sizes_of(WC.make_part("edges", n, T))
    assert e[0] == 1 and e[-1] == 1 and sum(e) == n
    g = sizes_of(WC.make_part("geometric", 5000, T))
    assert g[:12] == [1 << i for i in range(12)] and sum(g) == 5000
    z = np.sort(np.unique(WC.make_part("zipf", 70_000, T), return_counts=True)[1])[::-1]
    assert 300 < len(z) <= 700 and z[0] > 20 * z[len(z) // 2]                     # many partitions, a heavy head
    assert len(np.unique(WC.make_part("zipf", 100_000, T, groups=3000))) > 2000
    for shape in ("runs64", "edges", "geometric", "zipf"):                          # shuffled, and the special words are there
        col = WC.make_part(shape, 5000, T)
        assert (np.diff(col.astype(np.float64)) < 0).any()
        for w in WC.SPECIAL:
            assert (col == w).any(), (shape, int(w))
    n = 5000
    assert WC.make_order("none", n) is None
    assert len(np.unique(WC.make_order("constant", n))) == 1
    assert len(np.unique(WC.make_order("sixteen", n))) <= 16
    assert len(np.unique(WC.make_order("distinct", n))) == n
    x = WC.make_order("extremes", n)
    for w in (0, (1 << 63) - 1, 1 << 63, (1 << 64) - 1):
        assert (x == np.uint64(w)).any()
    assert len(np.unique(x)) <= 7
    v = WC.make_values("full64", n)
    assert int(v.astype(object).sum()) >= 1 << 64                                   # the sum wraps
    assert len(np.unique(WC.make_values("constant", n))) == 1
    x = WC.make_values("extremes", n)
    for w in (0, (1 << 63) - 1, 1 << 63, (1 << 64) - 1):
        assert (x == np.uint64(w)).any()
