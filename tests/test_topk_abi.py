"""CPU suite: the top-k entry points are part of the C-ABI -- declared in include/rhj.h with their argument names directly behind the
sort entries, exported by librhj_hip.so, bound in binding.SYMBOLS with their argument types -- and the addition left RHJ_ABI_VERSION
at 3.  Engine.topk_columns / kth_value_columns refuse wrong arguments before they touch a device.  The oracle of the GPU tests
(tests/topk_cases.py) is checked by hand on test_sort_abi's eight rows."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import radixhashjoin_amd as rhj
from radixhashjoin_amd import binding

import sort_cases as SC
import topk_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _u64, _pu64 = C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)
ENTRIES = {
    "rhj_topk_cols_dev": (["ctx", "d_keys", "d_rows", "n", "k", "flags", "d_out_keys", "d_out_rows", "out_kth"],
                          [_vp, _vp, _vp, _u64, _u64, C.c_uint32, _vp, _vp, _pu64]),
    "rhj_topk_dev": (["ctx", "d_R", "n", "k", "flags", "d_out", "out_kth"], [_vp, _vp, _u64, _u64, C.c_uint32, _vp, _pu64]),
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


def test_the_block_stands_directly_behind_the_sort_entries_and_before_the_stage_entries():
    h = header()
    at = {name: h.index(name + "(") for name in ("rhj_sort_cols_dev", "rhj_sort_dev", "rhj_topk_cols_dev", "rhj_topk_dev", "rhj_histogram")}
    assert at["rhj_sort_cols_dev"] < at["rhj_sort_dev"] < at["rhj_topk_cols_dev"] < at["rhj_topk_dev"] < at["rhj_histogram"]
    between = h[at["rhj_sort_dev"]:at["rhj_topk_cols_dev"]]
    assert between.count("(") == 1, "a declaration stands between rhj_sort_dev and rhj_topk_cols_dev"


def test_library_exports_them_and_binding_knows_their_types():
    lib = rhj.load_library()
    for name, (_, types) in ENTRIES.items():
        assert isinstance(getattr(lib, name), C._CFuncPtr)
        res, args = binding.SYMBOLS[name]
        assert res is C.c_int and list(args) == types
    for method in ("topk_cols_dev", "topk_dev", "topk_columns", "kth_value_columns"):
        assert callable(getattr(rhj.Engine, method))


def test_abi_version_is_still_3():
    assert rhj.load_library().rhj_abi_version() == 3


def test_signatures_and_defaults_of_the_python_entries():
    p = inspect.signature(rhj.Engine.topk_columns).parameters
    assert list(p) == ["self", "keys", "k", "values", "descending", "unsigned"]
    assert p["values"].default == () and p["descending"].default is False and p["unsigned"].default is False
    p = inspect.signature(rhj.Engine.kth_value_columns).parameters
    assert list(p) == ["self", "keys", "k", "descending", "unsigned"]
    assert p["descending"].default is False and p["unsigned"].default is False
    p = inspect.signature(rhj.Engine.topk_cols_dev).parameters
    assert list(p)[:6] == ["self", "d_keys", "d_rows", "n", "k", "flags"] and p["flags"].default == 0
    p = inspect.signature(rhj.Engine.topk_dev).parameters
    assert list(p)[:5] == ["self", "d_R", "n", "k", "flags"] and p["flags"].default == 0


def test_value_errors_come_before_any_device_use():
    """an Engine that was never constructed reaches every one of them"""
    e = rhj.Engine.__new__(rhj.Engine)
    e.ctx = None
    for call in (e.topk_columns, e.kth_value_columns):
        with pytest.raises(ValueError, match="sort_columns"):
            call([None, None], 3)
        with pytest.raises(ValueError, match="sort_columns"):
            call((None,), 3)
        for bad in (2.0, "3", None, True):
            with pytest.raises(ValueError, match="^k: an int"):
                call(None, bad)
        with pytest.raises(ValueError, match="^k: "):
            call(None, -1)
        with pytest.raises(ValueError, match="descending"):
            call(None, 3, descending=1)
        with pytest.raises(ValueError, match="descending"):
            call(None, 3, descending=[False])
        with pytest.raises(ValueError, match="unsigned"):
            call(None, 3, unsigned=0)
        with pytest.raises(ValueError, match="^keys: a 1-D torch tensor of 64-bit integers"):
            call(None, 3)
    with pytest.raises(ValueError, match="at most 4 value tensors"):
        e.topk_columns(None, 3, values=[None] * 5)
    with pytest.raises(ValueError, match="^k: a rank from 1"):
        e.kth_value_columns(None, 0)


def test_header_states_the_contract():
    h = re.sub(r"\s*\n \* ", " ", header(strip_comments=False))       # (comment lines joined: a phrase may wrap)
    for phrase in ("the first m tuples of what rhj_sort_cols_dev / rhj_sort_dev would write",
                   "bit for bit, in the same positions",
                   "never compared and never used as indices",
                   "RHJ_SORT_DESC: the k largest",
                   "Ties keep their input order in both directions, also at the cut",
                   "the tuples earliest in the input are the ones taken",
                   "bit-identical from run to run",
                   "no word at or past m is written",
                   "out_kth is a HOST pointer to two words, or NULL",
                   "Both device outputs NULL is allowed if and only if out_kth is given",
                   "Both device outputs NULL with out_kth NULL and n, k > 0 is RHJ_E_INVALID",
                   "n == 0 or k == 0: RHJ_OK, no launch, nothing written, out_kth untouched",
                   "k >= n: the call is the sort",
                   "in INPUT ORDER", "never from atomics",
                   "a probe of 8, one to three select passes of 8 each", "a count of 8 and a compaction read of 8 = 32 .. 48",
                   "against 112 .. 272 for the sort",
                   '"last.topk_sorted_rows" <= m + "topk.max_candidates"', "or 1 when the digits ran out",
                   '"last.topk_bits"', '"last.topk_passes"', '"last.topk_candidates"', '"topk.auto_candidates"',
                   '"topk.max_candidates": -1 automatic, 1 .. 2^31 - 1',
                   '"sort.max_units" also caps the units of the histogram, count and compact launches',
                   "kept until rhj_release_workspace"):
        assert phrase in h, phrase


def test_the_oracle_by_hand_on_eight_rows():
    """test_sort_abi's rows: keys with ties; the all-ones word is the signed -1 and the unsigned maximum"""
    ones, top = (1 << 64) - 1, 1 << 63
    keys = np.array([5, ones, 5, 0, top, 5, ones, 0], dtype=np.uint64)
    assert TC.oracle_topk(keys, 3, 0).tolist() == [3, 7, 0]
    assert TC.oracle_topk(keys, 4, 0).tolist() == [3, 7, 0, 2]                  # the cut inside the run of 5s takes rows 0 and 2, never 5
    assert TC.oracle_topk(keys, 3, SC.SORT_DESC).tolist() == [1, 6, 4]
    assert TC.oracle_topk(keys, 3, SC.SORT_I64).tolist() == [4, 1, 6]
    assert TC.oracle_topk(keys, 3, SC.SORT_I64 | SC.SORT_DESC).tolist() == [0, 2, 5]
    assert TC.oracle_topk(keys, 9, 0).tolist() == SC.oracle_perm(keys, 0).tolist() and len(TC.oracle_topk(keys, 0, 0)) == 0
    assert TC.run_of(keys, 0, 3) == (2, 4) and TC.run_of(keys, SC.SORT_I64, 0) == (0, 0)


def test_case_generators_have_the_shapes_they_are_named_for():
    assert TC.DISTS[:len(SC.DISTS)] == SC.DISTS and TC.DISTS[len(SC.DISTS):] == ("outliers", "cut_run")
    for n in (1, 65, 70_000):
        o = TC.make_keys("outliers", n)
        assert len(o) == n and int((o >= np.uint64(1 << 8)).sum()) == min(n, 10)
        assert (o[o >= np.uint64(1 << 8)] >= np.uint64((1 << 40) - (1 << 8))).all() and int(o.max()) < 1 << 40
        c = TC.make_keys("cut_run", n)
        lo, hi = TC.cut_run_bounds(n)
        assert len(c) == n and lo <= (n - 1) // 2 < hi
        assert TC.run_of(c, 0, (n - 1) // 2) == (lo, hi - 1)
        assert np.array_equal(TC.make_keys("full64", n), SC.make_keys("full64", n))
    c = TC.make_keys("cut_run", 70_000)
    where = np.nonzero(c == TC.RUN_VALUE)[0]
    assert len(np.unique(where // 4096)) == -(-70_000 // 4096)                 # the run has rows in every tile
    assert (np.diff(c.astype(np.int64)) < 0).any()                              # shuffled, not sorted
