"""CPU suite: the lookup-join entry points and the gather with a fill value are part of the C-ABI -- declared in include/rhj.h with
their argument names, exported by librhj_hip.so, bound in binding.SYMBOLS with their argument types, the constants exported by the
package -- and the addition left RHJ_ABI_VERSION at 3.  Engine.lookup_columns refuses a wrong `which` and too many value tensors
before it touches a device."""
import ctypes as C
import os
import re

import pytest

import radixhashjoin_amd as rhj
from radixhashjoin_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _u64, _opts = C.c_void_p, C.c_uint64, C.POINTER(binding.Opts)
ENTRIES = {
    "rhj_lookup_cols_dev": (["ctx", "d_valR", "d_idR", "nR", "d_valS", "d_idS", "nS", "which", "opts", "d_out", "out_rows", "out_matched"],
                            [_vp, _vp, _vp, _u64, _vp, _vp, _u64, C.c_int, _opts, _vp, _u64, C.POINTER(_u64)]),
    "rhj_lookup_dev": (["ctx", "d_R", "nR", "d_S", "nS", "which", "opts", "d_out", "out_rows", "out_matched"],
                       [_vp, _vp, _u64, _vp, _u64, C.c_int, _opts, _vp, _u64, C.POINTER(_u64)]),
    "rhj_gather_cols_fill": (["ctx", "d_srcs", "ncols", "src_rows", "d_idx", "n", "fills", "d_dsts"],
                             [_vp, C.POINTER(_vp), C.c_uint32, _u64, _vp, _u64, C.POINTER(_u64), C.POINTER(_vp)]),
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
    for name, value in (("RHJ_LOOKUP_FIRST", 0), ("RHJ_LOOKUP_LAST", 1), ("RHJ_LOOKUP_MAX_COLS", 4)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", h), name
    assert re.search(r"#define\s+RHJ_ABI_VERSION\s+3\b", h)


def test_library_exports_them_and_binding_knows_their_types():
    lib = rhj.load_library()
    for name, (_, types) in ENTRIES.items():
        assert isinstance(getattr(lib, name), C._CFuncPtr)
        res, args = binding.SYMBOLS[name]
        assert res is C.c_int and list(args) == types
    for method in ("lookup_cols_dev", "lookup_dev", "gather_cols_fill", "lookup_columns"):
        assert callable(getattr(rhj.Engine, method))


def test_constants_are_exported():
    assert rhj.LOOKUP_FIRST == binding.LOOKUP_FIRST == 0 and rhj.LOOKUP_LAST == binding.LOOKUP_LAST == 1
    assert rhj.LOOKUP_MAX_COLS == binding.LOOKUP_MAX_COLS == 4
    for name in ("LOOKUP_FIRST", "LOOKUP_LAST", "LOOKUP_MAX_COLS"):
        assert name in rhj.__all__


def test_abi_version_is_still_3():
    assert rhj.load_library().rhj_abi_version() == 3


def test_header_documents_the_kernel_number_and_the_contract():
    h = header(strip_comments=False)
    assert re.search(r"17 the lookup join kernel", h)
    for phrase in ("sets all out_rows words of d_out to RHJ_NO_ROW", "never stored to", "never inserted", "never dereferenced",
                   "cannot be\n * told from RHJ_NO_ROW", '"last.join_kernel" is 17', "d_out must not overlap", "bit-exact"):
        assert phrase in h, phrase


def test_lookup_columns_refuses_which_and_too_many_values_before_any_device():
    """the two checks come before anything that needs a context: an Engine that was never constructed reaches them"""
    e = rhj.Engine.__new__(rhj.Engine)
    e.ctx = None
    with pytest.raises(ValueError, match="which"):
        e.lookup_columns(None, None, which="any")
    with pytest.raises(ValueError, match="which"):
        e.lookup_columns(None, None, which=0)
    with pytest.raises(ValueError, match="at most 4 value tensors"):
        e.lookup_columns(None, None, values_S=[None] * 5)
    with pytest.raises(ValueError, match="fill"):
        e.lookup_columns(None, None, values_S=[None] * 2, fill=[0])
