"""CPU suite: the group-by join entry points are part of the C-ABI -- declared in include/rhj.h with their argument names,
RHJ_GJ_INNER, RHJ_GJ_LEFT and RHJ_GROUP_JOIN_MAX_COLS, exported by librhj_hip.so, bound in binding.SYMBOLS with their argument
types -- and the addition left RHJ_ABI_VERSION at 3."""
import ctypes as C
import os
import re

import radixhashjoin_amd as rhj
from radixhashjoin_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _u64, _u32, _opts, _pvp = C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(binding.Opts), C.POINTER(C.c_void_p)
_TAIL_NAMES = ["d_colsR", "ncolsR", "colR_rows", "d_colsS", "ncolsS", "colS_rows", "mode", "opts", "d_out_keys", "d_out_cntR",
               "d_out_cntS", "d_out_sumsR", "d_out_sumsS", "out_capacity", "out_groups"]
_TAIL_TYPES = [_pvp, _u32, _u64, _pvp, _u32, _u64, C.c_int, _opts, _vp, _vp, _vp, _pvp, _pvp, _u64, C.POINTER(_u64)]
ENTRIES = {
    "rhj_group_join_cols_dev": (["ctx", "d_valR", "d_idR", "nR", "d_valS", "d_idS", "nS"] + _TAIL_NAMES,
                                [_vp, _vp, _vp, _u64, _vp, _vp, _u64] + _TAIL_TYPES),
    "rhj_group_join_dev": (["ctx", "d_R", "nR", "d_S", "nS"] + _TAIL_NAMES, [_vp, _vp, _u64, _vp, _u64] + _TAIL_TYPES),
}


def header(strip_comments=True):
    with open(os.path.join(ROOT, "include", "rhj.h")) as f:
        h = f.read()
    return re.sub(r"/\*.*?\*/", " ", h, flags=re.S) if strip_comments else h


def test_header_declares_both_entries_with_their_argument_names():
    h = header()
    for name, (names, _) in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", h)
        assert m, f"include/rhj.h does not declare {name}"
        args = [a.strip() for a in m.group(1).split(",")]
        assert [a.split()[-1].lstrip("*") for a in args] == names
    assert re.search(r"#define\s+RHJ_GJ_INNER\s+0\b", h)
    assert re.search(r"#define\s+RHJ_GJ_LEFT\s+1\b", h)
    assert re.search(r"#define\s+RHJ_GROUP_JOIN_MAX_COLS\s+4\b", h)
    assert re.search(r"#define\s+RHJ_ABI_VERSION\s+3\b", h)


def test_library_exports_them_and_binding_knows_their_types():
    lib = rhj.load_library()
    for name, (_, types) in ENTRIES.items():
        assert isinstance(getattr(lib, name), C._CFuncPtr)
        res, args = binding.SYMBOLS[name]
        assert res is C.c_int and list(args) == types
    for method in ("group_join_cols_dev", "group_join_dev", "join_group_by_columns"):
        assert callable(getattr(rhj.Engine, method))
    assert rhj.GROUP_JOIN_MAX_COLS == binding.GROUP_JOIN_MAX_COLS == 4
    assert (rhj.GJ_INNER, rhj.GJ_LEFT) == (binding.GJ_INNER, binding.GJ_LEFT) == (0, 1)
    for name in ("GROUP_JOIN_MAX_COLS", "GJ_INNER", "GJ_LEFT"):
        assert name in rhj.__all__


def test_abi_version_is_still_3():
    assert rhj.load_library().rhj_abi_version() == 3


def test_header_documents_the_kernel_number_and_the_contract():
    h = header(strip_comments=False)
    assert re.search(r"16 the group-by join kernel", h)
    assert re.search(r"15 the group-by kernel", h)                         # (the wording before it stands)
    assert '"last.group_rounds"' in h
    m = re.search(r"RHJ_GROUP_JOIN_MAX_COLS 4(.*?)int rhj_group_join_cols_dev", h, flags=re.S)
    assert m, "the contract stands in front of rhj_group_join_cols_dev"
    for phrase in ("nothing at or past capacity is written", "never dereferenced", "probe_split is ignored", "last.group_rounds",
                   "COUNT(*) = cntR·cntS", "SUM(r.a) = sumsR·cntS", "SUM(s.b) = sumsS·cntR", "not rhj_mix64", "which side",
                   '"last.join_kernel" is 16', '"last.semi_tables" is 0', "use more radix bits"):
        assert phrase in m.group(1), phrase
