"""CPU suite: the sort entry points are part of the C-ABI -- declared in include/rhj.h with their argument names behind the composite-key
block, exported by librhj_hip.so, bound in binding.SYMBOLS with their argument types, the flag constants exported by the package --
and the addition left RHJ_ABI_VERSION at 3.  Engine.sort_columns / argsort_columns refuse wrong arguments before they touch a device.
The oracle of the GPU tests (tests/sort_cases.py) is checked by hand on eight rows."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import radixhashjoin_amd as rhj
from radixhashjoin_amd import binding

import sort_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _u64 = C.c_void_p, C.c_uint64
ENTRIES = {
    "rhj_sort_cols_dev": (["ctx", "d_keys", "d_rows", "n", "flags", "d_out_keys", "d_out_rows"], [_vp, _vp, _vp, _u64, C.c_uint32, _vp, _vp]),
    "rhj_sort_dev": (["ctx", "d_R", "n", "flags", "d_out"], [_vp, _vp, _u64, C.c_uint32, _vp]),
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
    for name, value in (("RHJ_SORT_I64", "1u"), ("RHJ_SORT_DESC", "2u")):
        assert re.search(r"#define\s+" + name + r"\s+" + value + r"(?!\w)", h), name
    assert re.search(r"#define\s+RHJ_ABI_VERSION\s+3\b", h)


def test_the_block_stands_behind_the_composite_keys_and_before_the_stage_entries():
    h = header()
    at = {name: h.index(name + "(") for name in ("rhj_keys_plan_free", "rhj_sort_cols_dev", "rhj_sort_dev", "rhj_histogram")}
    assert at["rhj_keys_plan_free"] < at["rhj_sort_cols_dev"] < at["rhj_sort_dev"] < at["rhj_histogram"]


def test_library_exports_them_and_binding_knows_their_types():
    lib = rhj.load_library()
    for name, (_, types) in ENTRIES.items():
        assert isinstance(getattr(lib, name), C._CFuncPtr)
        res, args = binding.SYMBOLS[name]
        assert res is C.c_int and list(args) == types
    for method in ("sort_cols_dev", "sort_dev", "sort_columns", "argsort_columns"):
        assert callable(getattr(rhj.Engine, method))


def test_constants_are_exported():
    assert rhj.SORT_I64 == binding.SORT_I64 == SC.SORT_I64 == 1 and rhj.SORT_DESC == binding.SORT_DESC == SC.SORT_DESC == 2
    for name in ("SORT_I64", "SORT_DESC"):
        assert name in rhj.__all__


def test_abi_version_is_still_3():
    assert rhj.load_library().rhj_abi_version() == 3


def test_signatures_and_defaults_of_the_torch_entries():
    p = inspect.signature(rhj.Engine.sort_columns).parameters
    assert list(p) == ["self", "keys", "values", "descending", "unsigned"]
    assert p["values"].default == () and p["descending"].default is False and p["unsigned"].default is False
    p = inspect.signature(rhj.Engine.argsort_columns).parameters
    assert list(p) == ["self", "keys", "descending", "unsigned"]
    assert p["descending"].default is False and p["unsigned"].default is False


def test_value_errors_come_before_any_device_use():
    """an Engine that was never constructed reaches every one of them"""
    e = rhj.Engine.__new__(rhj.Engine)
    e.ctx = None
    for call in (e.sort_columns, e.argsort_columns):
        with pytest.raises(ValueError, match="descending"):
            call([None, None], descending=[False])
        with pytest.raises(ValueError, match="descending"):
            call([None, None], descending=[False, True, False])
        with pytest.raises(ValueError, match="descending"):
            call(None, descending=1)
        with pytest.raises(ValueError, match="descending"):
            call([None, None], descending=[False, 1])
        with pytest.raises(ValueError, match="at most 4 key tensors"):
            call([None] * 5)
        with pytest.raises(ValueError, match="empty"):
            call([])
        with pytest.raises(ValueError, match="unsigned"):
            call(None, unsigned=0)
    with pytest.raises(ValueError, match="at most 4 value tensors"):
        e.sort_columns(None, values=[None] * 5)


def test_header_states_the_contract():
    h = re.sub(r"\s*\n \* ", " ", header(strip_comments=False))       # (comment lines joined: a phrase may wrap)
    for phrase in ("Ties keep their input order in both directions",
                   "never compared and never used as indices",
                   "Both outputs NULL with n > 0 is RHJ_E_INVALID",
                   "ORDER BY a, b",
                   "rhj_gather_u64(ctx, a, perm1, n, a1)",
                   "last key first",
                   "Bytes per pass and tuple",
                   "8 + 8 + 8 = 24", "8 + 12 + 12 = 32", "8 + 16 + 16 = 40",
                   "the sort has no skew case",
                   "bit-identical from run to run",
                   "original word bit for bit",
                   '"last.sort_bits"', '"last.sort_passes"', '"sort.tile_rows"',
                   "kept until rhj_release_workspace",
                   '"last.sort_units"', '"sort.max_units": -1 automatic (2048), 1 .. 2048'):
        assert phrase in h, phrase


def test_the_oracle_by_hand_on_eight_rows():
    """keys with ties; the all-ones word is the signed -1 and the unsigned maximum"""
    ones, top = (1 << 64) - 1, 1 << 63
    keys = np.array([5, ones, 5, 0, top, 5, ones, 0], dtype=np.uint64)
    # unsigned ascending: 0 0 5 5 5 top ones ones, ties by position
    assert SC.oracle_perm(keys, 0).tolist() == [3, 7, 0, 2, 5, 4, 1, 6]
    # unsigned descending: ones ones top 5 5 5 0 0, ties STILL by position
    assert SC.oracle_perm(keys, SC.SORT_DESC).tolist() == [1, 6, 4, 0, 2, 5, 3, 7]
    # int64 ascending: top is INT64_MIN, ones is -1: top -1 -1 0 0 5 5 5
    assert SC.oracle_perm(keys, SC.SORT_I64).tolist() == [4, 1, 6, 3, 7, 0, 2, 5]
    # int64 descending: 5 5 5 0 0 -1 -1 top
    assert SC.oracle_perm(keys, SC.SORT_I64 | SC.SORT_DESC).tolist() == [0, 2, 5, 3, 7, 1, 6, 4]
    assert SC.oracle_bits(keys, 0) == 64 and SC.oracle_bits(keys, SC.SORT_I64) == 64
    small = np.array([-3, 3, 0], dtype=np.int64).view(np.uint64)
    assert SC.oracle_bits(small, SC.SORT_I64) == 3 and SC.oracle_bits(small, 0) == 64
    assert SC.oracle_bits(np.array([7, 7], dtype=np.uint64), 0) == 0


def test_case_generators_have_the_shapes_they_are_named_for():
    n = 5000
    assert len(np.unique(SC.make_keys("sixteen", n))) <= 16
    assert len(np.unique(SC.make_keys("constant", n))) == 1
    s = SC.make_keys("sorted", n)
    assert (np.diff(s.astype(np.int64)) >= 0).all() and (np.diff(SC.make_keys("reverse", n).astype(np.int64)) <= 0).all()
    v = SC.make_keys("small_signed", n).view(np.int64)
    assert v.min() == -3 and v.max() == 3
    x = SC.make_keys("extremes", n)
    for w in (0, (1 << 63) - 1, 1 << 63, (1 << 64) - 1):
        assert (x == np.uint64(w)).any()
    m = SC.make_keys("middle_digit", n)
    assert ((m >> np.uint64(8)) & np.uint64(255) == 0x55).all() and int(m.max()) < 1 << 24
    t = SC.make_keys("top_byte", n)
    assert len(np.unique(t & np.uint64((1 << 56) - 1))) == 1 and len(np.unique(t)) > 1
    r = SC.wide_rows(n)
    assert len(np.unique(r)) < n and int(r.max()) >= 1 << 32
