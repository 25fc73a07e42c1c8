"""CPU suite: the outer-join entry points are part of the C-ABI -- declared in include/rhj.h with the RHJ_OUTER_* bits and RHJ_NO_ROW,
exported by librhj_hip.so, bound in binding.SYMBOLS with their argument types -- and the addition left RHJ_ABI_VERSION at 3."""
import ctypes as C
import os
import re

import radixhashjoin_amd as rhj
from radixhashjoin_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _u64, _opts = C.c_void_p, C.c_uint64, C.POINTER(binding.Opts)
ENTRIES = {
    "rhj_outer_join_cols_dev": (["ctx", "d_valR", "d_idR", "nR", "d_valS", "d_idS", "nS", "how", "opts", "d_out", "out_capacity", "out_count",
                                 "out_sections"],
                                [_vp, _vp, _vp, _u64, _vp, _vp, _u64, C.c_int, _opts, _vp, _u64, C.POINTER(_u64), C.POINTER(_u64)]),
    "rhj_outer_join_dev": (["ctx", "d_R", "nR", "d_S", "nS", "how", "opts", "d_out", "out_capacity", "out_count", "out_sections"],
                           [_vp, _vp, _u64, _vp, _u64, C.c_int, _opts, _vp, _u64, C.POINTER(_u64), C.POINTER(_u64)]),
}


def header(strip_comments=True):
    with open(os.path.join(ROOT, "include", "rhj.h")) as f:
        h = f.read()
    return re.sub(r"/\*.*?\*/", " ", h, flags=re.S) if strip_comments else h


def test_header_declares_both_entries_and_the_macros():
    h = header()
    for name, (names, _) in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", h)
        assert m, f"include/rhj.h does not declare {name}"
        args = [a.strip() for a in m.group(1).split(",")]
        assert [a.split()[-1].lstrip("*") for a in args] == names
    assert re.search(r"#define\s+RHJ_NO_ROW\s+0xFFFFFFFFFFFFFFFFull\b", h)
    for macro, value in (("RHJ_OUTER_LEFT", 1), ("RHJ_OUTER_RIGHT", 2), ("RHJ_OUTER_FULL", 3)):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(value) + r"\b", h), macro
    assert re.search(r"#define\s+RHJ_ABI_VERSION\s+3\b", h)


def test_library_exports_them_and_binding_knows_their_types():
    lib = rhj.load_library()
    for name, (_, types) in ENTRIES.items():
        assert isinstance(getattr(lib, name), C._CFuncPtr)
        res, args = binding.SYMBOLS[name]
        assert res is C.c_int and list(args) == types
    assert (binding.OUTER_LEFT, binding.OUTER_RIGHT, binding.OUTER_FULL) == (1, 2, 3) and binding.NO_ROW == (1 << 64) - 1
    assert (rhj.OUTER_LEFT, rhj.OUTER_RIGHT, rhj.OUTER_FULL, rhj.NO_ROW) == (1, 2, 3, (1 << 64) - 1)
    for method in ("outer_join_cols_dev", "outer_join_dev", "outer_join_columns"):
        assert callable(getattr(rhj.Engine, method))


def test_abi_version_is_still_3():
    lib = rhj.load_library()
    assert all(hasattr(lib, name) for name in ENTRIES) and lib.rhj_abi_version() == 3        # (added, and the version stayed)


def test_header_documents_the_reporting_names():
    h = header(strip_comments=False)
    assert '"last.outer_sweeps"' in h and '"last.semi_tables"' in h
    assert re.search(r"12 the semi / anti join kernel", h)
