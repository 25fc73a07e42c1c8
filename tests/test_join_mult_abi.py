"""CPU suite: the multiplicity-join entry points and the two query-layer calls beside them are part of the C-ABI -- declared in
include/rhj.h with their argument names, exported by librhj_hip.so, bound in binding.SYMBOLS with their argument types -- and the
addition left RHJ_ABI_VERSION at 3."""
import ctypes as C
import os
import re

import radixhashjoin_amd as rhj
from radixhashjoin_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _u64, _opts = C.c_void_p, C.c_uint64, C.POINTER(binding.Opts)
ENTRIES = {
    "rhj_join_mult_cols_dev": (["ctx", "d_valR", "d_idR", "nR", "d_valS", "d_idS", "nS", "d_wS", "wS_rows", "opts", "d_out", "out_rows", "out_total"],
                               [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _u64, _opts, _vp, _u64, C.POINTER(_u64)]),
    "rhj_join_mult_dev": (["ctx", "d_R", "nR", "d_S", "nS", "d_wS", "wS_rows", "opts", "d_out", "out_rows", "out_total"],
                          [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _opts, _vp, _u64, C.POINTER(_u64)]),
    "rhj_mul_u64": (["ctx", "d_a", "d_b", "n", "d_dst"], [_vp, _vp, _vp, _u64, _vp]),
    "rhj_sum_gather_weighted": (["ctx", "d_col", "d_rows", "d_w", "n", "sum"], [_vp, _vp, _vp, _vp, _u64, C.POINTER(_u64)]),
}


def header(strip_comments=True):
    with open(os.path.join(ROOT, "include", "rhj.h")) as f:
        h = f.read()
    return re.sub(r"/\*.*?\*/", " ", h, flags=re.S) if strip_comments else h


def test_header_declares_the_entries_with_their_argument_names():
    h = header()
    for name, (names, _) in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", h)
        assert m, f"include/rhj.h does not declare {name}"
        args = [a.strip() for a in m.group(1).split(",")]
        assert [a.split()[-1].lstrip("*") for a in args] == names
    assert re.search(r"#define\s+RHJ_ABI_VERSION\s+3\b", h)


def test_library_exports_them_and_binding_knows_their_types():
    lib = rhj.load_library()
    for name, (_, types) in ENTRIES.items():
        assert isinstance(getattr(lib, name), C._CFuncPtr)
        res, args = binding.SYMBOLS[name]
        assert res is C.c_int and list(args) == types
    for method in ("join_mult_cols_dev", "join_mult_dev", "join_multiplicity_columns"):
        assert callable(getattr(rhj.Engine, method))


def test_abi_version_is_still_3():
    assert rhj.load_library().rhj_abi_version() == 3


def test_header_documents_the_kernel_number_and_the_contract():
    h = header(strip_comments=False)
    assert re.search(r"14 the multiplicity join kernel", h)
    for phrase in ("zeroes all out_rows words", "never stored to", "never loaded from", "d_out must not overlap"):
        assert phrase in h, phrase
