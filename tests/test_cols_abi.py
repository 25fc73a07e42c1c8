"""CPU suite: the columnar join entry point is part of the C-ABI -- declared in include/rhj.h, exported by librhj_hip.so, bound
in binding.SYMBOLS -- and the addition left RHJ_ABI_VERSION at 3."""
import ctypes as C
import os
import re

import radixhashjoin_amd as rhj
from radixhashjoin_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "rhj.h")) as f:
        return f.read()


def test_header_declares_rhj_join_cols_dev():
    h = re.sub(r"/\*.*?\*/", " ", header(), flags=re.S)
    m = re.search(r"\bint\s+rhj_join_cols_dev\s*\(([^)]*)\)\s*;", h)
    assert m, "include/rhj.h does not declare rhj_join_cols_dev"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 11
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "d_valR", "d_idR", "nR", "d_valS", "d_idS", "nS", "opts", "d_out",
                                                         "out_capacity", "out_count"]
    assert re.search(r"#define\s+RHJ_ABI_VERSION\s+3\b", h)


def test_library_exports_it_and_binding_knows_it():
    lib = rhj.load_library()
    assert isinstance(getattr(lib, "rhj_join_cols_dev"), C._CFuncPtr)
    res, args = binding.SYMBOLS["rhj_join_cols_dev"]
    assert res is C.c_int and len(args) == 11
    assert callable(rhj.Engine.join_cols_dev) and callable(rhj.Engine.join_columns)


def test_abi_version_is_still_3():
    assert rhj.load_library().rhj_abi_version() == 3


def test_header_documents_the_reporting_names():
    h = header()
    assert '"last.cols_R"' in h and '"last.cols_S"' in h
