"""CPU suite: the composite-key entry points are part of the C-ABI -- declared in include/rhj.h with the RHJ_KEYS_* macros, exported by
librhj_hip.so, bound in binding.SYMBOLS with their argument types, the ABI version still 3 -- and rhj_keys_layout, which needs no
GPU, follows the layout rule of the header: checked on the cases that name every branch and against a replay of the rule in Python."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import radixhashjoin_amd as rhj
from radixhashjoin_amd import binding
from radixhashjoin_amd.binding import KEYS_DICT as DICT, KEYS_FOLD0 as FOLD0, KEYS_RANGE as RANGE, KeysLayout, keys_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _u64, _u32, _P = C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER
ENTRIES = {
    "rhj_keys_layout": (["nkeys", "range_bits", "n_total", "out"], [_u32, _P(C.c_uint8), _u64, _P(KeysLayout)]),
    "rhj_keys_pack_dev": (["ctx", "nkeys", "d_keysR", "nR", "d_keysS", "nS", "flags", "d_outR", "d_outS", "out_plan"],
                          [_vp, _u32, _P(_vp), _u64, _P(_vp), _u64, _u32, _vp, _vp, _P(_vp)]),
    "rhj_keys_unpack_dev": (["ctx", "plan", "d_packed", "n", "d_out_cols"], [_vp, _vp, _vp, _u64, _P(_vp)]),
    "rhj_keys_plan_info": (["plan", "out"], [_vp, _P(KeysLayout)]),
    "rhj_keys_plan_free": (["ctx", "plan"], [_vp, _vp]),
}


def header():
    with open(os.path.join(ROOT, "include", "rhj.h")) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def test_header_declares_the_five_entries_and_the_macros():
    h = header()
    for name, (names, _) in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", h)
        assert m, f"include/rhj.h does not declare {name}"
        assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == names
    assert re.search(r"#define\s+RHJ_KEYS_MAX_COLS\s+4\b", h) and re.search(r"#define\s+RHJ_KEYS_NO_UNPACK\s+1u\b", h)
    assert re.search(r"#define\s+RHJ_KEYS_RANGE\s+0\b", h) and re.search(r"#define\s+RHJ_KEYS_DICT\s+1\b", h)
    assert re.search(r"typedef\s+struct\s+rhj_keyplan\s+rhj_keyplan\s*;", h) and re.search(r"}\s*rhj_keys_layout_t\s*;", h)
    assert re.search(r"#define\s+RHJ_ABI_VERSION\s+3\b", h)


def test_library_exports_them_and_binding_knows_their_types():
    lib = rhj.load_library()
    for name, (_, types) in ENTRIES.items():
        assert isinstance(getattr(lib, name), C._CFuncPtr)
        res, args = binding.SYMBOLS[name]
        assert res is C.c_int and list(args) == types
    assert (binding.KEYS_MAX_COLS, binding.KEYS_NO_UNPACK, RANGE, DICT) == (4, 1, 0, 1)
    assert (rhj.KEYS_MAX_COLS, rhj.KEYS_NO_UNPACK, rhj.KEYS_RANGE, rhj.KEYS_DICT) == (4, 1, 0, 1)
    for method in ("keys_pack_dev", "keys_unpack_dev", "pack_keys"):
        assert callable(getattr(rhj.Engine, method))
    for method in ("unpack", "close", "__del__"):
        assert callable(getattr(rhj.KeyPlan, method))
    assert lib.rhj_abi_version() == 3                        # (added, and the version stayed)


def lay(widths, n_total):
    return keys_layout(widths, n_total).as_dict()


def test_layout_range_only():
    d = lay([20, 30], 1000)
    assert d["kind"] == [RANGE, RANGE] and d["fields"] == [0, 1] and d["shifts"] == [0, 20] and d["widths"] == [20, 30]
    assert d["total_bits"] == 50 and d["folds"] == []
    assert lay([0, 0], 1000)["total_bits"] == 0
    d = lay([64], 1000)
    assert d["kind"] == [RANGE] and d["total_bits"] == 64 and d["widths"] == [64]
    d = lay([32, 32], 1 << 33)                               # RANGE only: no limit on the rows
    assert d["kind"] == [RANGE, RANGE] and d["total_bits"] == 64


def test_layout_dictionaries():
    d = lay([64, 64], 6000)
    assert d["kind"] == [DICT, DICT] and d["wd"] == 13 and d["total_bits"] == 26 and d["widths"] == [13, 13] and d["folds"] == []
    d = lay([64, 10], 6000)
    assert d["kind"] == [DICT, RANGE] and d["widths"] == [13, 10] and d["total_bits"] == 23
    d = lay([40, 40], 1 << 20)                               # a tie: the lowest index, and one is enough
    assert d["kind"] == [DICT, RANGE] and d["wd"] == 20 and d["widths"] == [20, 40] and d["total_bits"] == 60


def test_layout_folds():
    d = lay([64] * 4, 140_000)
    assert d["kind"] == [DICT] * 4 and d["wd"] == 18 and d["folds"] == [(0, 1)] and d["fold_shift"] == [18]
    assert d["fields"] == [FOLD0, 2, 3] and d["widths"] == [18, 18, 18] and d["shifts"] == [0, 18, 36] and d["total_bits"] == 54
    d = lay([64] * 4, 2_200_000)
    assert d["wd"] == 22 and d["folds"] == [(0, 1), (FOLD0, 2)] and d["fields"] == [FOLD0 + 1, 3] and d["total_bits"] == 44


def test_layout_errors():
    for widths, n_total in (([64, 64], 1 << 32), ([], 10), ([1] * 5, 10), ([65], 10)):
        with pytest.raises(rhj.RhjError) as e:
            keys_layout(widths, n_total)
        assert e.value.code == binding.RHJ_E_INVALID
    lib = rhj.load_library()
    assert lib.rhj_keys_layout(1, None, 10, C.byref(KeysLayout())) == binding.RHJ_E_INVALID
    assert lib.rhj_keys_layout(1, (C.c_uint8 * 1)(3), 10, None) == binding.RHJ_E_INVALID
    assert lib.rhj_keys_plan_info(None, C.byref(KeysLayout())) == binding.RHJ_E_INVALID


def replay(widths, n_total):
    """the layout rule of include/rhj.h in Python: (kinds, wd, folds, [(field id, width, shift)], total bits), or None"""
    w, kind, ids, folds, wd = list(widths), [RANGE] * len(widths), list(range(len(widths))), [], 0
    if sum(w) > 64:
        if n_total >= 1 << 32:
            return None
        wd = max(n_total - 1, 0).bit_length()
        while sum(w) > 64:
            wide = [j for j in range(len(w)) if kind[j] == RANGE and w[j] > wd]
            if not wide:
                break
            j = max(wide, key=lambda j: (w[j], -j))
            kind[j], w[j] = DICT, wd
        while sum(w) > 64:
            folds.append((ids[0], ids[1], w[0]))
            ids[:2], w[:2] = [FOLD0 + len(folds) - 1], [wd]
    shifts = [sum(w[:i]) for i in range(len(w))]
    return kind, wd, folds, list(zip(ids, w, shifts)), sum(w)


def test_layout_is_the_rule_on_random_widths():
    rng = np.random.default_rng(21)
    seen_folds = set()
    for _ in range(600):
        k = int(rng.integers(1, 5))
        widths = [int(x) for x in rng.choice([0, 1, 7, 13, 20, 22, 31, 32, 33, 40, 47, 63, 64], k)]
        n_total = int(rng.choice([0, 1, 2, 6000, 140_000, 1 << 20, 2_200_000, (1 << 32) - 1, 1 << 32, 1 << 40]))
        exp = replay(widths, n_total)
        if exp is None:
            with pytest.raises(rhj.RhjError):
                keys_layout(widths, n_total)
            continue
        d = lay(widths, n_total)
        kind, wd, folds, fields, total = exp
        got = (d["kind"], d["wd"], [(a, b, s) for (a, b), s in zip(d["folds"], d["fold_shift"])],
               list(zip(d["fields"], d["widths"], d["shifts"])), d["total_bits"])
        assert got == (kind, wd, folds, fields, total), (widths, n_total)
        assert total <= 64 and d["range_bits"] == widths and lay(widths, n_total) == d          # fits, and says the same twice
        seen_folds.add(len(folds))
    assert seen_folds == {0, 1, 2}
