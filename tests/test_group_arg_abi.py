"""CPU suite: the group-by argmin / argmax entries are part of the C-ABI -- rhj_group_arg_cols_dev / rhj_group_arg_dev declared in
include/rhj.h with their argument names, the eight RHJ_ARG_* / RHJ_GROUP_ARG_MAX_COLS macros with their values, exported by
librhj_hip.so, bound in binding.SYMBOLS with their argument types, the constants exported by the package; the addition left
RHJ_ABI_VERSION at 3 and the RHJ_AGG_* family alone; the header states the contract; the torch entries refuse wrong arguments before
any device use; and the numpy oracle of the GPU suite picks the rows a reader picks by hand."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import radixhashjoin_amd as rhj
from group_agg_cases import full_range_cols, side_oracle
from group_arg_cases import IDENTITY, VALUE_OPS, arg_oracle, tying_groups
from radixhashjoin_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _u64, _u32, _opts, _pvp, _pu32 = C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(binding.Opts), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)
_NAMES = ["d_cols", "ops", "ties", "ncols", "col_rows", "opts", "d_out_keys", "d_out_counts", "d_out_vals", "d_out_rows", "out_capacity",
          "out_groups"]
_TYPES = [_pvp, _pu32, _pu32, _u32, _u64, _opts, _vp, _vp, _pvp, _pvp, _u64, C.POINTER(_u64)]
ENTRIES = {
    "rhj_group_arg_cols_dev": (["ctx", "d_valR", "d_idR", "nR"] + _NAMES, [_vp, _vp, _vp, _u64] + _TYPES),
    "rhj_group_arg_dev": (["ctx", "d_R", "nR"] + _NAMES, [_vp, _vp, _u64] + _TYPES),
}
MACROS = {"RHJ_ARG_MIN_U64": 0, "RHJ_ARG_MAX_U64": 1, "RHJ_ARG_MIN_I64": 2, "RHJ_ARG_MAX_I64": 3, "RHJ_ARG_ROW": 4, "RHJ_ARG_TIE_FIRST": 0,
          "RHJ_ARG_TIE_LAST": 1, "RHJ_GROUP_ARG_MAX_COLS": 4}


def header(strip_comments=True):
    with open(os.path.join(ROOT, "include", "rhj.h")) as f:
        h = f.read()
    return re.sub(r"/\*.*?\*/", " ", h, flags=re.S) if strip_comments else h


def test_header_declares_both_entries_and_the_eight_macros():
    h = header()
    for name, (names, _) in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", h)
        assert m, f"include/rhj.h does not declare {name}"
        args = [a.strip() for a in m.group(1).split(",")]
        assert [a.split()[-1].lstrip("*") for a in args] == names
    for name, value in MACROS.items():
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", h), name
    assert re.search(r"#define\s+RHJ_ABI_VERSION\s+3\b", h)
    for name, value in {"SUM": 0, "MIN_U64": 1, "MAX_U64": 2, "MIN_I64": 3, "MAX_I64": 4}.items():       # the aggregates stand as they were
        assert re.search(r"#define\s+RHJ_AGG_" + name + r"\s+" + str(value) + r"\b", h), name


def test_they_are_declared_behind_the_ids_entries_and_before_the_keys():
    h = header()
    at = {name: h.index("int " + name) for name in list(ENTRIES) + ["rhj_group_agg_ids_dev", "rhj_group_join_agg_ids_dev"]}
    assert max(at["rhj_group_agg_ids_dev"], at["rhj_group_join_agg_ids_dev"]) < min(at[name] for name in ENTRIES)
    assert max(at[name] for name in ENTRIES) < h.index("RHJ_KEYS_MAX_COLS")
    assert h.index("RHJ_ARG_MIN_U64") < at["rhj_group_arg_cols_dev"]


def test_library_exports_them_and_binding_knows_their_types():
    lib = rhj.load_library()
    for name, (_, types) in ENTRIES.items():
        assert isinstance(getattr(lib, name), C._CFuncPtr)
        res, args = binding.SYMBOLS[name]
        assert res is C.c_int and list(args) == types
    for method in ("group_arg_cols_dev", "group_arg_dev", "group_by_columns_arg", "drop_duplicates_columns"):
        assert callable(getattr(rhj.Engine, method))
    for name, value in MACROS.items():
        short = name[len("RHJ_"):]
        assert getattr(rhj, short) == getattr(binding, short) == value
        assert short in rhj.__all__
    assert lib.rhj_abi_version() == 3


def test_the_torch_entries_and_their_defaults():
    g = inspect.signature(rhj.Engine.group_by_columns_arg).parameters
    assert list(g) == ["self", "keys", "by", "ops", "ties"] and g["ties"].default == "first"
    d = inspect.signature(rhj.Engine.drop_duplicates_columns).parameters
    assert list(d) == ["self", "keys", "keep"] and d["keep"].default == "first"


def test_header_states_the_contract():
    h = header(strip_comments=False)
    m = re.search(r"#define RHJ_GROUP_ARG_MAX_COLS 4(.*?)int rhj_group_arg_cols_dev", h, flags=re.S)
    assert m, "the contract stands in front of rhj_group_arg_cols_dev"
    for phrase in ("names a real row", "also when the extreme is the identity", "nothing at or past capacity written", "rows arrays included",
                   "the smallest rowID under RHJ_ARG_TIE_FIRST, the largest under RHJ_ARG_TIE_LAST", "ties == NULL: every column is RHJ_ARG_TIE_FIRST",
                   '"last.join_kernel" is 15', "bit for bit", "no row\n * guard for that column", "never dereferenced",
                   "above RHJ_ARG_ROW", "above RHJ_ARG_TIE_LAST", "above RHJ_GROUP_ARG_MAX_COLS", "names the column",
                   "before any launch, also in a count-only call", "same column pointer may appear several times",
                   "ncols == 0 returns keys and counts only", "one per tuple on one"):
        assert phrase in m.group(1), phrase


def test_torch_entries_refuse_wrong_arguments_before_any_device():
    """the checks come before anything that needs a context: an Engine that was never constructed reaches them"""
    e = rhj.Engine.__new__(rhj.Engine)
    e.ctx = None
    for ops in (["avg"], ["MIN"], [0], [None]):
        with pytest.raises(ValueError, match="ops"):
            e.group_by_columns_arg(None, [None], ops)
    for ties in ("any", ["any"], [0], [None]):
        with pytest.raises(ValueError, match="ties"):
            e.group_by_columns_arg(None, [None], ["row"], ties)
    with pytest.raises(ValueError, match="at most 4 columns"):
        e.group_by_columns_arg(None, [None] * 5, ["row"] * 5)
    with pytest.raises(ValueError, match="ops"):
        e.group_by_columns_arg(None, [None, None], ["row"])              # one op for two columns
    with pytest.raises(ValueError, match="ties"):
        e.group_by_columns_arg(None, [None, None], ["row", "row"], ["first"])
    with pytest.raises(ValueError, match="needs a tensor"):
        e.group_by_columns_arg(None, [None], ["min"])                    # None goes with "row" only
    for keep in ("any", False, None, 0):
        with pytest.raises(ValueError, match="keep"):
            e.drop_duplicates_columns(None, keep=keep)


def test_the_oracle_on_eight_rows_with_ties():
    """by hand.  key 5: rows 0 2 3 6 hold 7 7 9 9; key 8: rows 1 4 hold -1 (all ones) and 3; key 9: rows 5 7 hold 0 0"""
    F, L = rhj.ARG_TIE_FIRST, rhj.ARG_TIE_LAST
    values = np.array([5, 8, 5, 5, 8, 9, 5, 9], dtype=np.uint64)
    col = np.array([7, 0xFFFFFFFFFFFFFFFF, 7, 9, 3, 0, 9, 0], dtype=np.uint64)
    rows = np.arange(8)
    ops = [rhj.ARG_MIN_U64, rhj.ARG_MIN_U64, rhj.ARG_MAX_U64, rhj.ARG_MAX_U64]
    keys, counts, vals, out = arg_oracle(values, rows, [col] * 4, ops, [F, L, F, L])
    assert keys.tolist() == [5, 8, 9] and counts.tolist() == [4, 2, 2]
    assert vals[0].tolist() == vals[1].tolist() == [7, 3, 0] and vals[2].tolist() == vals[3].tolist() == [9, 0xFFFFFFFFFFFFFFFF, 0]
    assert [o.tolist() for o in out] == [[0, 4, 5], [2, 4, 7], [3, 1, 5], [6, 1, 7]]
    # signed: all ones is -1, the minimum of key 8 and no longer its maximum
    keys, counts, vals, out = arg_oracle(values, rows, [col] * 4, [rhj.ARG_MIN_I64, rhj.ARG_MAX_I64, rhj.ARG_ROW, rhj.ARG_ROW], [L, F, F, L])
    assert vals[0].tolist() == [7, 0xFFFFFFFFFFFFFFFF, 0] and vals[1].tolist() == [9, 3, 0] and vals[2] is None and vals[3] is None
    assert [o.tolist() for o in out] == [[2, 1, 7], [3, 4, 5], [0, 1, 5], [6, 4, 7]]
    assert tying_groups(values, rows, col, rhj.ARG_MAX_U64).tolist() == [2, 1, 2]
    # permuted rowIDs: position and rowID differ, the rowID decides.  Tuple i carries rowID perm[i]; the column is indexed by rowID.
    perm = np.array([7, 6, 5, 4, 3, 2, 1, 0])
    keys, counts, vals, out = arg_oracle(values, perm, [col[::-1].copy()] * 2, [rhj.ARG_MIN_U64] * 2, [F, L])
    assert vals[0].tolist() == [7, 3, 0] and out[0].tolist() == [5, 3, 0] and out[1].tolist() == [7, 3, 2]
    assert len(arg_oracle(values[:0], rows[:0], [col], [rhj.ARG_MIN_U64], [F])[0]) == 0


def test_the_oracle_agrees_with_the_aggregate_oracle_on_the_values():
    """the extremes, from a sort that shares nothing with side_oracle's reduceat; and every row it names holds its extreme"""
    n = 5_000
    rng = np.random.default_rng(11)
    values = rng.integers(0, 700, n, dtype=np.uint64)
    rows = rng.permutation(n)
    cols = full_range_cols(n, 4)
    cols[3] = rng.integers(0, 2, n, dtype=np.uint64)                       # ties
    agg = {rhj.ARG_MIN_U64: rhj.AGG_MIN_U64, rhj.ARG_MAX_U64: rhj.AGG_MAX_U64, rhj.ARG_MIN_I64: rhj.AGG_MIN_I64, rhj.ARG_MAX_I64: rhj.AGG_MAX_I64}
    for tie in (rhj.ARG_TIE_FIRST, rhj.ARG_TIE_LAST):
        for shift in range(4):
            ops = VALUE_OPS[shift:] + VALUE_OPS[:shift]
            keys, counts, vals, out = arg_oracle(values, rows, cols, ops, [tie] * 4)
            ek, ec, ea = side_oracle(values, rows, cols, [agg[o] for o in ops])
            assert np.array_equal(keys, ek) and np.array_equal(counts, ec)
            key_of_row = np.empty(n, dtype=np.uint64)
            key_of_row[rows] = values
            for j in range(4):
                assert np.array_equal(vals[j], ea[j]), (tie, ops[j])
                assert np.array_equal(cols[j][out[j].astype(np.int64)], vals[j]) and np.array_equal(key_of_row[out[j].astype(np.int64)], keys)
    assert sorted(IDENTITY) == sorted(VALUE_OPS)
