"""CPU suite: the group-id entries are part of the C-ABI -- rhj_group_agg_ids_cols_dev / rhj_group_agg_ids_dev and
rhj_group_join_agg_ids_cols_dev / rhj_group_join_agg_ids_dev declared in include/rhj.h as their _agg_ entries with the id arrays
appended, exported by librhj_hip.so, bound in binding.SYMBOLS with their argument types -- the _agg_ prototypes stand as they were,
the addition left RHJ_ABI_VERSION at 3, the torch entries that existed kept their signatures, and the header states the contract."""
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
_GID_NAMES, _GID_TYPES = ["d_out_gid", "gid_rows"], [_vp, _u64]
_JID_NAMES, _JID_TYPES = ["d_out_gidR", "gidR_rows", "d_out_gidS", "gidS_rows"], [_vp, _u64, _vp, _u64]
# the _agg_ entry every id entry extends, and what it appends
AGG_ENTRIES = {
    "rhj_group_agg_cols_dev": (["ctx", "d_valR", "d_idR", "nR"] + _G_NAMES, [_vp, _vp, _vp, _u64] + _G_TYPES),
    "rhj_group_agg_dev": (["ctx", "d_R", "nR"] + _G_NAMES, [_vp, _vp, _u64] + _G_TYPES),
    "rhj_group_join_agg_cols_dev": (["ctx", "d_valR", "d_idR", "nR", "d_valS", "d_idS", "nS"] + _J_NAMES,
                                    [_vp, _vp, _vp, _u64, _vp, _vp, _u64] + _J_TYPES),
    "rhj_group_join_agg_dev": (["ctx", "d_R", "nR", "d_S", "nS"] + _J_NAMES, [_vp, _vp, _u64, _vp, _u64] + _J_TYPES),
}
ID_ENTRIES = {
    "rhj_group_agg_ids_cols_dev": ("rhj_group_agg_cols_dev", _GID_NAMES, _GID_TYPES),
    "rhj_group_agg_ids_dev": ("rhj_group_agg_dev", _GID_NAMES, _GID_TYPES),
    "rhj_group_join_agg_ids_cols_dev": ("rhj_group_join_agg_cols_dev", _JID_NAMES, _JID_TYPES),
    "rhj_group_join_agg_ids_dev": ("rhj_group_join_agg_dev", _JID_NAMES, _JID_TYPES),
}


def header(strip_comments=True):
    with open(os.path.join(ROOT, "include", "rhj.h")) as f:
        h = f.read()
    return re.sub(r"/\*.*?\*/", " ", h, flags=re.S) if strip_comments else h


def declared(h, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", h)
    assert m, f"include/rhj.h does not declare {name}"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    return [a.split()[-1].lstrip("*") for a in args], [a[:a.rindex(a.split()[-1].lstrip("*"))].strip() for a in args]


def test_header_declares_each_id_entry_as_its_agg_entry_with_the_id_arrays_appended():
    h = header()
    for name, (base, more, _) in ID_ENTRIES.items():
        names, types = declared(h, name)
        base_names, base_types = declared(h, base)
        assert names == base_names + more, name
        assert types[:len(base_types)] == base_types, name                 # the same C types, argument for argument
        assert types[len(base_types):] == ["uint64_t *", "uint64_t"] * (len(more) // 2), name


def test_the_agg_prototypes_are_unchanged():
    h = header()
    for name, (names, _) in AGG_ENTRIES.items():
        assert declared(h, name)[0] == names, name
        res, args = binding.SYMBOLS[name]
        assert res is C.c_int and list(args) == AGG_ENTRIES[name][1], name
    assert re.search(r"#define\s+RHJ_ABI_VERSION\s+3\b", h)
    assert rhj.load_library().rhj_abi_version() == 3


def test_they_are_declared_behind_the_agg_entries():
    h = header()
    assert max(h.index("int " + name) for name in AGG_ENTRIES) < min(h.index("int " + name) for name in ID_ENTRIES)


def test_library_exports_them_and_binding_knows_their_types():
    lib = rhj.load_library()
    for name, (base, _, more) in ID_ENTRIES.items():
        assert isinstance(getattr(lib, name), C._CFuncPtr)
        res, args = binding.SYMBOLS[name]
        assert res is C.c_int and list(args) == AGG_ENTRIES[base][1] + more, name
        assert list(args)[:len(AGG_ENTRIES[base][1])] == list(binding.SYMBOLS[base][1]), name
    for method in ("group_agg_ids_cols_dev", "group_agg_ids_dev", "group_join_agg_ids_cols_dev", "group_join_agg_ids_dev",
                   "group_by_columns_with_inverse", "factorize_columns", "join_group_by_columns_with_inverse"):
        assert callable(getattr(rhj.Engine, method)), method


def test_the_torch_entries():
    """the entries that existed keep their signatures; the ones with the inverse take the same arguments"""
    g = inspect.signature(rhj.Engine.group_by_columns).parameters
    assert list(g) == ["self", "keys", "weights", "ops"]
    assert list(inspect.signature(rhj.Engine.group_by_columns_with_inverse).parameters) == list(g)
    j = inspect.signature(rhj.Engine.join_group_by_columns).parameters
    assert list(j) == ["self", "keys_R", "keys_S", "weights_R", "weights_S", "how", "ops_R", "ops_S"]
    ji = inspect.signature(rhj.Engine.join_group_by_columns_with_inverse).parameters
    assert list(ji) == list(j) and ji["how"].default == "inner" and ji["ops_R"].default is None and ji["ops_S"].default is None
    assert list(inspect.signature(rhj.Engine.factorize_columns).parameters) == ["self", "keys"]


def test_header_states_the_contract():
    h = header(strip_comments=False)
    m = re.search(r"int rhj_group_join_agg_dev\(.*?\);(.*?)int rhj_group_agg_ids_cols_dev", h, flags=re.S)
    assert m, "the contract stands in front of rhj_group_agg_ids_cols_dev"
    for phrase in ("d_out_gid[rowR] = g", "OF THIS CALL", "may differ", "left untouched", "same rowID", "d_out_gid == NULL",
                   "never compared with out_capacity", "[0, *out_groups)", "Count only", "never written", "names",
                   "nothing at or past gid_rows is touched", "context stays usable", '"last.join_kernel" is 15',
                   "one more sweep of the partition per class", "one scattered 8-byte store per tuple"):
        assert phrase in m.group(1), phrase
    m = re.search(r"int rhj_group_agg_ids_dev\(.*?\);(.*?)int rhj_group_join_agg_ids_cols_dev", h, flags=re.S)
    assert m, "the contract stands in front of rhj_group_join_agg_ids_cols_dev"
    for phrase in ("RHJ_GJ_LEFT", "RHJ_GJ_INNER", "all ones", "-1 as int64", "on every attempt", "partitions that get no task",
                   "classes that emit nothing", "nS == 0", "Either pointer may be NULL", "both NULL", "d_out_gidR or",
                   "d_out_gidS", '"last.join_kernel" is 16'):
        assert phrase in m.group(1), phrase
