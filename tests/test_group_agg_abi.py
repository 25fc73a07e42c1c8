"""CPU suite: the per-column aggregate entries are part of the C-ABI -- rhj_group_agg_cols_dev / rhj_group_agg_dev and
rhj_group_join_agg_cols_dev / rhj_group_join_agg_dev declared in include/rhj.h with their argument names, the five RHJ_AGG_* values,
exported by librhj_hip.so, bound in binding.SYMBOLS with their argument types, the constants exported by the package -- the addition
left RHJ_ABI_VERSION at 3, and the header states what a minimum or maximum over no tuple of S holds."""
import ctypes as C
import inspect
import os
import re

import radixhashjoin_amd as rhj
from radixhashjoin_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _u64, _u32, _opts, _pvp, _pu32 = C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(binding.Opts), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)
_G_NAMES = ["d_cols", "ops", "ncols", "col_rows", "opts", "d_out_keys", "d_out_counts", "d_out_aggs", "out_capacity", "out_groups"]
_G_TYPES = [_pvp, _pu32, _u32, _u64, _opts, _vp, _vp, _pvp, _u64, C.POINTER(_u64)]
_J_NAMES = ["d_colsR", "opsR", "ncolsR", "colR_rows", "d_colsS", "opsS", "ncolsS", "colS_rows", "mode", "opts", "d_out_keys", "d_out_cntR",
            "d_out_cntS", "d_out_aggsR", "d_out_aggsS", "out_capacity", "out_groups"]
_J_TYPES = [_pvp, _pu32, _u32, _u64, _pvp, _pu32, _u32, _u64, C.c_int, _opts, _vp, _vp, _vp, _pvp, _pvp, _u64, C.POINTER(_u64)]
ENTRIES = {
    "rhj_group_agg_cols_dev": (["ctx", "d_valR", "d_idR", "nR"] + _G_NAMES, [_vp, _vp, _vp, _u64] + _G_TYPES),
    "rhj_group_agg_dev": (["ctx", "d_R", "nR"] + _G_NAMES, [_vp, _vp, _u64] + _G_TYPES),
    "rhj_group_join_agg_cols_dev": (["ctx", "d_valR", "d_idR", "nR", "d_valS", "d_idS", "nS"] + _J_NAMES,
                                    [_vp, _vp, _vp, _u64, _vp, _vp, _u64] + _J_TYPES),
    "rhj_group_join_agg_dev": (["ctx", "d_R", "nR", "d_S", "nS"] + _J_NAMES, [_vp, _vp, _u64, _vp, _u64] + _J_TYPES),
}
AGG = {"SUM": 0, "MIN_U64": 1, "MAX_U64": 2, "MIN_I64": 3, "MAX_I64": 4}


def header(strip_comments=True):
    with open(os.path.join(ROOT, "include", "rhj.h")) as f:
        h = f.read()
    return re.sub(r"/\*.*?\*/", " ", h, flags=re.S) if strip_comments else h


def test_header_declares_the_four_entries_with_their_argument_names():
    h = header()
    for name, (names, _) in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", h)
        assert m, f"include/rhj.h does not declare {name}"
        args = [a.strip() for a in m.group(1).split(",")]
        assert [a.split()[-1].lstrip("*") for a in args] == names
    for name, value in AGG.items():
        assert re.search(r"#define\s+RHJ_AGG_" + name + r"\s+" + str(value) + r"\b", h), name
    assert re.search(r"#define\s+RHJ_ABI_VERSION\s+3\b", h)


def test_they_are_declared_behind_the_group_entries():
    h = header()
    at = {name: h.index("int " + name) for name in list(ENTRIES) + ["rhj_group_sum_dev", "rhj_group_join_dev"]}
    assert max(at["rhj_group_sum_dev"], at["rhj_group_join_dev"]) < min(at[name] for name in ENTRIES)
    assert h.index("RHJ_GROUP_JOIN_MAX_COLS") < h.index("RHJ_AGG_SUM")


def test_library_exports_them_and_binding_knows_their_types():
    lib = rhj.load_library()
    for name, (_, types) in ENTRIES.items():
        assert isinstance(getattr(lib, name), C._CFuncPtr)
        res, args = binding.SYMBOLS[name]
        assert res is C.c_int and list(args) == types
    for method in ("group_agg_cols_dev", "group_agg_dev", "group_join_agg_cols_dev", "group_join_agg_dev"):
        assert callable(getattr(rhj.Engine, method))
    for name, value in AGG.items():
        assert getattr(rhj, "AGG_" + name) == getattr(binding, "AGG_" + name) == value
        assert "AGG_" + name in rhj.__all__


def test_the_torch_entries_gained_keyword_arguments_only():
    g = inspect.signature(rhj.Engine.group_by_columns).parameters
    assert list(g) == ["self", "keys", "weights", "ops"] and g["ops"].default is None
    j = inspect.signature(rhj.Engine.join_group_by_columns).parameters
    assert list(j) == ["self", "keys_R", "keys_S", "weights_R", "weights_S", "how", "ops_R", "ops_S"]
    assert j["ops_R"].default is None and j["ops_S"].default is None and j["how"].default == "inner"


def test_abi_version_is_still_3():
    assert rhj.load_library().rhj_abi_version() == 3


def test_header_states_the_identity_rule_and_the_contract():
    h = header(strip_comments=False)
    m = re.search(r"#define RHJ_AGG_MAX_I64 4(.*?)int rhj_group_agg_cols_dev", h, flags=re.S)
    assert m, "the contract stands in front of rhj_group_agg_cols_dev"
    for phrase in ("ops == NULL: every column is RHJ_AGG_SUM", "same column pointer may appear twice", "above RHJ_AGG_MAX_I64",
                   "before any launch, also in a count-only call", "names the column", "nothing at or past capacity written",
                   "never dereferenced", '"last.join_kernel" is 15', "bit for bit"):
        assert phrase in m.group(1), phrase
    m = re.search(r"int rhj_group_agg_dev(.*?)int rhj_group_join_agg_cols_dev", h, flags=re.S)
    assert m, "the contract stands in front of rhj_group_join_agg_cols_dev"
    for phrase in ("cntS == 0", "identity", "RHJ_AGG_MIN_U64: 0xFFFFFFFFFFFFFFFF", "RHJ_AGG_MAX_U64: 0", "RHJ_AGG_MIN_I64: INT64_MAX",
                   "RHJ_AGG_MAX_I64: INT64_MIN", "RHJ_AGG_SUM columns of S stay 0", "cntS tells", "RAW per-side value",
                   '"last.join_kernel" is 16', "names the side and the column", "bit for bit"):
        assert phrase in m.group(1), phrase
