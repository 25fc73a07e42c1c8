"""GPU suite: the top-k entries (rhj_topk_cols_dev / rhj_topk_dev, Engine.topk_columns / kth_value_columns) against the numpy oracle
of tests/topk_cases.py: the first min(k, n) tuples of the sort's oracle.  Every comparison is exact -- position p holds the tuple of
rank p, ties in input order in both directions and at the cut, the key words bit for bit.  Output arrays are exactly min(k, n) words
between guard words, and the inputs are compared before and after.

Under the automatic "topk.max_candidates" (max(k, info("topk.auto_candidates"))) an input of no more rows than that runs no select
pass -- it is sorted and cut --, so the edge sizes also run under "topk.max_candidates" 1, where selection walks down every digit
and the count, the scan over units and the compaction run at every size.  Under the automatic "sort.max_units" every input below
2048 tiles is cut into units of one tile; the cursors across the tiles of a unit run under "sort.max_units" 1 and 3."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import sort_cases as SC
import topk_cases as TC
from radixhashjoin_amd import SORT_DESC, SORT_I64, Engine, RhjError
from radixhashjoin_amd.binding import RHJ_E_INVALID

pytestmark = pytest.mark.gpu

GUARD, NGUARD = SC.GUARD, SC.NGUARD
BIG = 3_000_000


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def T(eng):
    t = eng.info("sort.tile_rows")
    assert t >= 64 and t % 64 == 0
    return t


@pytest.fixture(scope="module")
def AUTO(eng):
    a = eng.info("topk.auto_candidates")
    assert a >= 1
    return a


@pytest.fixture(scope="module")
def cases():
    """(dist, n) -> (keys, flags -> oracle permutation): built once, shared, never written"""
    cache = {}

    def get(dist, n):
        if (dist, n) not in cache:
            keys = TC.make_keys(dist, n)
            keys.setflags(write=False)
            cache[(dist, n)] = (keys, {})
        keys, perms = cache[(dist, n)]
        return keys, lambda flags: perms.setdefault(flags, SC.oracle_perm(keys, flags))
    return get


class Array:
    """n words in HBM at an offset of `off` words into a buffer of off + n + NGUARD words, guard words before and behind"""
    def __init__(self, eng, n, off=0, data=None):
        self.n, self.off = n, off
        host = np.full(off + n + NGUARD, GUARD, dtype=np.uint64)
        if data is not None:
            host[off:off + n] = data
        self.buf = eng.to_device(host)
        self.ptr = self.buf.ptr + 8 * off

    def read(self):
        host = self.buf.to_numpy(np.uint64, self.off + self.n + NGUARD)
        assert (host[:self.off] == GUARD).all() and (host[self.off + self.n:] == GUARD).all(), "a word outside the array was written"
        return host[self.off:self.off + self.n]

    def free(self):
        self.buf.free()


@contextlib.contextmanager
def option(eng, name, value):
    eng.set_option(name, value)
    try:
        yield
    finally:
        eng.set_option(name, -1)


def check_info(eng, keys, k, flags, cap, pure=False, to_sort=True):
    """what rhj_get_info says after a call: the sort's names when k >= n made the call the sort (to_sort), the top-k names and the cost
    bound otherwise; cap: the "topk.max_candidates" in force.  Returns (passes, candidates, sorted rows)."""
    n, bits = len(keys), SC.oracle_bits(keys, flags)
    m = min(k, n)
    got = {name: eng.info("last." + name) for name in ("topk_bits", "topk_passes", "topk_candidates", "topk_sorted_rows", "sort_bits",
                                                       "sort_passes", "sort_units", "join_kernel")}
    assert got["join_kernel"] == -1
    if k >= n and to_sort:
        assert got["sort_bits"] == bits and (got["sort_passes"] > 0) == (bits > 0)
        assert got["topk_bits"] == got["topk_passes"] == got["topk_candidates"] == got["topk_sorted_rows"] == 0
        return 0, 0, 0
    assert got["sort_bits"] == got["sort_passes"] == got["sort_units"] == 0, got
    assert got["topk_bits"] == bits
    passes, cand, srows = got["topk_passes"], got["topk_candidates"], got["topk_sorted_rows"]
    assert 0 <= passes <= (bits + 7) // 8
    if bits == 0:
        assert passes == 0 and srows == 0
    elif pure:
        assert srows <= cap or (srows == 1 and passes == (bits + 7) // 8), (got, cap)
    else:
        assert srows <= m + cap, (got, m, cap)
    if passes:
        assert cand <= cap or passes == (bits + 7) // 8, (got, cap)
        assert cand >= 1
    else:
        assert cand == n
    return passes, cand, srows


def topk_cols(eng, dk, keys, k, flags, dr=None, rows=None, want_keys=True, want_rows=True, want_kth=False, off=0):
    """one rhj_topk_cols_dev call into arrays of exactly min(k, n) words; returns (keys or None, rows or None, kth or None); checks the
    guards and that the inputs are unchanged"""
    n = len(keys)
    m = min(k, n)
    ok = Array(eng, m, off) if want_keys else None
    orr = Array(eng, m, off) if want_rows else None
    try:
        kth = eng.topk_cols_dev(dk.ptr if n else None, dr.ptr if dr is not None and n else None, n, k, flags, ok.ptr if ok else None,
                                orr.ptr if orr else None, want_kth=want_kth)
        assert np.array_equal(dk.read(), keys), "the key input was modified"
        if dr is not None:
            assert np.array_equal(dr.read(), rows), "the row input was modified"
        return (ok.read() if ok else None), (orr.read() if orr else None), kth
    finally:
        for a in (ok, orr):
            if a is not None:
                a.free()


def ks_of(n):
    return sorted(k for k in {1, 2, 64, 65, n // 2, n - 1, n, n + 1} if k >= 1)


def check_case(eng, keys, perm_of, ks, cap, AUTO, flagses=SC.FLAGS, off=0):
    """keys at every k of ks in every flag combination: rows and key words equal the oracle's, the info names hold"""
    n = len(keys)
    dk = Array(eng, n, off, keys)
    try:
        for flags in flagses:
            perm = perm_of(flags)
            for k in ks:
                m = min(k, n)
                got_keys, got_rows, _ = topk_cols(eng, dk, keys, k, flags, off=off)
                info = check_info(eng, keys, k, flags, cap if cap > 0 else max(m, AUTO))
                wrong = int((got_rows != perm[:m]).sum())
                print(f"n {n} k {k} flags {flags} cap {cap}: rows that differ {wrong}, (passes, candidates, sorted rows) {info}")
                assert np.array_equal(got_rows, perm[:m])
                assert np.array_equal(got_keys, keys[perm[:m].astype(np.int64)])
    finally:
        dk.free()


def small_sizes(T):
    return (1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 70_000)


@pytest.mark.parametrize("cap", (-1, 1))
@pytest.mark.parametrize("dist", TC.DISTS)
def test_every_distribution_at_every_edge_size_and_k_in_all_four_flag_combinations(eng, T, AUTO, cases, dist, cap):
    with option(eng, "topk.max_candidates", cap):
        for n in small_sizes(T):
            keys, perm_of = cases(dist, n)
            check_case(eng, keys, perm_of, ks_of(n), cap, AUTO)


def test_no_rows_or_k_zero_writes_nothing_and_leaves_out_kth_alone(eng, cases):
    keys, _ = cases("full64", 65)
    dk, ok, orr = Array(eng, 65, 0, keys), Array(eng, 0), Array(eng, 0)
    lib = eng.lib
    for flags in SC.FLAGS:
        for n, k, ptr in ((0, 5, None), (0, 5, dk.ptr), (65, 0, dk.ptr), (0, 0, None)):
            kth = (C.c_uint64 * 2)(111, 222)
            assert lib.rhj_topk_cols_dev(eng.ctx, ptr, None, n, k, flags, ok.ptr, orr.ptr, kth) == 0
            assert lib.rhj_topk_cols_dev(eng.ctx, ptr, None, n, k, flags, None, None, None) == 0       # nothing asked for, nothing to do
            assert lib.rhj_topk_dev(eng.ctx, ptr, n // 2, k, flags, ok.ptr, kth) == 0
            assert (kth[0], kth[1]) == (111, 222)
            assert eng.info("last.topk_passes") == 0 and eng.info("last.sort_passes") == 0
            assert eng.topk_cols_dev(ptr, None, n, k, flags, ok.ptr, orr.ptr, want_kth=True) is None
    assert len(ok.read()) == 0 and len(orr.read()) == 0                      # (the guards behind the empty arrays are whole)
    for a in (dk, ok, orr):
        a.free()


@pytest.mark.parametrize("dist", ("full64", "sixteen", "outliers", "cut_run", "small_signed", "top_byte"))
def test_the_descent_down_every_digit_and_the_cost_bound(eng, AUTO, cases, dist):
    """70,000 rows: under "topk.max_candidates" 1 selection goes on until one candidate is left or digit 0 is done; under the automatic
    cap it stops as soon as max(k, auto) rows are tied.  Either way the rows handed to the sort are within m + cap."""
    n = 70_000
    keys, perm_of = cases(dist, n)
    dk = Array(eng, n, 0, keys)
    try:
        for cap in (1, -1):
            with option(eng, "topk.max_candidates", cap):
                for flags in SC.FLAGS:
                    bits, perm = SC.oracle_bits(keys, flags), perm_of(flags)
                    for k in (1, 1000, n // 2, n - 1):
                        _, got_rows, _ = topk_cols(eng, dk, keys, k, flags, want_keys=False)
                        assert np.array_equal(got_rows, perm[:k])
                        in_force = cap if cap > 0 else max(k, AUTO)
                        passes, cand, srows = check_info(eng, keys, k, flags, in_force)
                        print(f"{dist} flags {flags} k {k} cap {cap}: bits {bits} passes {passes} candidates {cand} sorted rows {srows}")
                        assert 1 <= passes <= (bits + 7) // 8
                        assert cand <= in_force or passes == (bits + 7) // 8
                        assert srows <= k + in_force
                        if cap == 1 and dist == "full64":
                            assert cand == 1 and srows <= k                    # distinct keys: the threshold is found exactly
    finally:
        dk.free()


def test_max_candidates_refuses_values_outside_its_range(eng, AUTO):
    try:
        for bad in (0, -2, 1 << 31, -(1 << 40)):
            with pytest.raises(RhjError) as err:
                eng.set_option("topk.max_candidates", bad)
            assert err.value.code == RHJ_E_INVALID
        eng.set_option("topk.max_candidates", (1 << 31) - 1)
        eng.set_option("topk.max_candidates", 1)
    finally:
        eng.set_option("topk.max_candidates", -1)
    assert eng.info("topk.auto_candidates") == AUTO


@pytest.mark.parametrize("units", (1, 3))
@pytest.mark.parametrize("dist", ("sixteen", "full64", "cut_run"))
def test_units_of_several_tiles_the_cursors_across_tiles_and_the_scan_across_units(eng, T, AUTO, cases, dist, units):
    """"sort.max_units" 1: one workgroup walks every tile (3 and 18 of them); 3 at 70,000 rows: three units of six tiles.  Under
    "topk.max_candidates" 1 the count and the compaction run at both sizes; under the automatic cap at 70,000"""
    with option(eng, "sort.max_units", units):
        for cap in (1, -1):
            with option(eng, "topk.max_candidates", cap):
                for n in (2 * T + 1, 70_000):
                    keys, perm_of = cases(dist, n)
                    check_case(eng, keys, perm_of, (1, 65, n // 2, n - 1), cap, AUTO)


def test_a_constant_column_is_its_first_k_rows_and_no_pass(eng, T, cases):
    keys, _ = cases("constant", 2 * T + 1)
    dk = Array(eng, len(keys), 0, keys)
    for flags in SC.FLAGS:
        for k in (1, 65, T + 1, 2 * T):
            got_keys, got_rows, kth = topk_cols(eng, dk, keys, k, flags, want_kth=True)
            assert np.array_equal(got_rows, np.arange(k, dtype=np.uint64)) and np.array_equal(got_keys, keys[:k])
            assert kth == (int(keys[0]), k - 1)
            assert eng.info("last.topk_bits") == 0 and eng.info("last.topk_passes") == 0 and eng.info("last.topk_sorted_rows") == 0
            assert topk_cols(eng, dk, keys, k, flags, want_keys=False, want_rows=False, want_kth=True)[2] == kth
    dk.free()


@pytest.mark.parametrize("cap", (-1, 1))
@pytest.mark.parametrize("dist", ("sixteen", "cut_run", "outliers"))
def test_ties_at_the_cut_keep_input_order(eng, AUTO, cases, dist, cap):
    """k inside a tie run, at the run's first row and at its last: the rows taken from the run are its earliest in the input"""
    n = 70_000
    keys, perm_of = cases(dist, n)
    dk = Array(eng, n, 0, keys)
    try:
        with option(eng, "topk.max_candidates", cap):
            for flags in SC.FLAGS:
                perm = perm_of(flags)
                first, last = TC.run_of(keys, flags, n // 2)
                assert last - first >= 64, "the case has no run at its middle"
                for k in (first + 1, first + 2, (first + last) // 2 + 1, last, last + 1):
                    got_keys, got_rows, kth = topk_cols(eng, dk, keys, k, flags, want_kth=True)
                    assert np.array_equal(got_rows, perm[:k]) and np.array_equal(got_keys, keys[perm[:k].astype(np.int64)])
                    in_run = got_rows[first:].astype(np.int64)
                    assert (np.diff(in_run) > 0).all() and (keys[in_run] == keys[in_run[0]]).all()
                    assert kth == (int(got_keys[-1]), int(got_rows[-1]))
                    in_force = cap if cap > 0 else max(k, AUTO)
                    _, cand, srows = check_info(eng, keys, k, flags, in_force)
                    if cand > in_force:                                      # the digits ran out inside the run: only the rows the result needs went to the sort
                        assert srows == k
    finally:
        dk.free()


@pytest.mark.parametrize("cap", (-1, 1))
@pytest.mark.parametrize("n", (65, 8193, 70_000))
def test_the_forms_give_one_answer(eng, AUTO, cases, n, cap):
    """explicit wide rows (duplicates, values >= 2^32: carried, never compared), keys only, rows only, the 16-byte tuples, out_kth with
    and without device outputs"""
    with option(eng, "topk.max_candidates", cap):
        for dist in ("sixteen", "full64"):
            keys, perm_of = cases(dist, n)
            rows = SC.wide_rows(n)
            tuples = np.empty((n, 2), dtype=np.uint64)
            tuples[:, 0], tuples[:, 1] = rows, keys                          # .key = rowID, .payload = value
            dk, dr, dt = Array(eng, n, 0, keys), Array(eng, n, 0, rows), Array(eng, 2 * n, 0, tuples.reshape(-1))
            for flags in SC.FLAGS:
                for k in (1, 64, n // 2, n - 1, n, n + 7):
                    m = min(k, n)
                    perm = perm_of(flags)[:m].astype(np.int64)
                    exp_kth = (int(keys[perm[-1]]), int(rows[perm[-1]]))
                    wide_keys, wide_rows, kth = topk_cols(eng, dk, keys, k, flags, dr=dr, rows=rows, want_kth=True)
                    assert np.array_equal(wide_rows, rows[perm]) and np.array_equal(wide_keys, keys[perm]) and kth == exp_kth
                    only_keys, none, kth = topk_cols(eng, dk, keys, k, flags, want_rows=False, want_kth=True)
                    assert none is None and np.array_equal(only_keys, keys[perm]) and kth == (exp_kth[0], int(perm[-1]))
                    only_keys, _, kth = topk_cols(eng, dk, keys, k, flags, dr=dr, rows=rows, want_rows=False)
                    assert np.array_equal(only_keys, keys[perm]) and kth is None
                    none, arg, kth = topk_cols(eng, dk, keys, k, flags, want_keys=False)
                    assert none is None and np.array_equal(arg, perm.astype(np.uint64))
                    _, arg, kth = topk_cols(eng, dk, keys, k, flags, dr=dr, rows=rows, want_keys=False, want_kth=True)
                    assert np.array_equal(arg, rows[perm]) and kth == exp_kth
                    _, _, kth = topk_cols(eng, dk, keys, k, flags, dr=dr, rows=rows, want_keys=False, want_rows=False, want_kth=True)
                    assert kth == exp_kth
                    check_info(eng, keys, k, flags, cap if cap > 0 else max(m, AUTO), pure=True, to_sort=False)
                    d_out = Array(eng, 2 * m)
                    kth = eng.topk_dev(dt.ptr, n, k, flags, d_out.ptr, want_kth=True)
                    got = d_out.read().reshape(m, 2)
                    assert np.array_equal(got[:, 1], keys[perm]) and np.array_equal(got[:, 0], rows[perm]) and kth == exp_kth
                    assert eng.topk_dev(dt.ptr, n, k, flags, None, want_kth=True) == exp_kth
                    assert np.array_equal(dt.read(), tuples.reshape(-1))
                    d_out.free()
            for a in (dk, dr, dt):
                a.free()


@pytest.mark.parametrize("n", (65, 4097, 69_999))
def test_pointers_that_are_8_byte_but_not_16_byte_aligned(eng, AUTO, cases, n):
    assert n % 2 == 1
    for cap in (-1, 1):
        with option(eng, "topk.max_candidates", cap):
            for dist in ("full64", "sixteen"):
                keys, perm_of = cases(dist, n)
                check_case(eng, keys, perm_of, (1, 65, n // 2), cap, AUTO, off=1)


@pytest.mark.parametrize("n", (70_000, BIG))
def test_pure_selection_the_median(eng, AUTO, cases, n):
    """out_kth alone: nothing of size k is written, only the candidates go to the sort"""
    k = (n + 1) // 2
    for dist in ("full64", "sixteen", "outliers"):
        keys, perm_of = cases(dist, n)
        dk = Array(eng, n, 0, keys)
        for flags in SC.FLAGS:
            row = int(perm_of(flags)[k - 1])
            for cap in (-1, 1):
                with option(eng, "topk.max_candidates", cap):
                    kth = topk_cols(eng, dk, keys, k, flags, want_keys=False, want_rows=False, want_kth=True)[2]
                    assert kth == (int(keys[row]), row)
                    in_force = cap if cap > 0 else max(k, AUTO)
                    passes, cand, srows = check_info(eng, keys, k, flags, in_force, pure=True)
                    print(f"{dist} n {n} flags {flags} cap {cap}: passes {passes} candidates {cand} sorted rows {srows}")
                    assert passes >= 1 and srows <= in_force
        dk.free()


@pytest.mark.parametrize("dist", ("full64", "sixteen", "outliers"))
def test_three_million_rows_more_units_than_cus(eng, T, AUTO, cases, dist):
    keys, perm_of = cases(dist, BIG)
    assert -(-BIG // T) > 256
    check_case(eng, keys, perm_of, (1000, BIG // 2), -1, AUTO)


def test_two_runs_are_bit_identical_and_profiling_names_the_spans(eng, cases):
    n, k = 70_000, 35_001
    keys, _ = cases("sixteen", n)
    rows = SC.wide_rows(n)
    dk, dr = Array(eng, n, 0, keys), Array(eng, n, 0, rows)
    a = topk_cols(eng, dk, keys, k, SORT_I64 | SORT_DESC, dr=dr, rows=rows, want_kth=True)
    eng.set_profiling(True)
    b = topk_cols(eng, dk, keys, k, SORT_I64 | SORT_DESC, dr=dr, rows=rows, want_kth=True)
    t, passes = eng.timings(), eng.info("last.topk_passes")
    eng.set_profiling(False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert passes >= 1
    assert t["hist"]["launches"] >= passes + 1 and t["scan"]["launches"] >= passes + 1 and t["scatter"]["launches"] >= 1
    assert t["join"]["launches"] == 0 and t["tasks"]["launches"] == 0
    for x in (dk, dr):
        x.free()


def test_info_after_other_calls(eng, cases):
    n = 70_000
    keys, _ = cases("full64", n)
    dk = Array(eng, n, 0, keys)
    topk_cols(eng, dk, keys, 100, 0)
    assert eng.info("last.topk_passes") >= 1 and eng.info("last.topk_bits") == 64 and eng.info("last.topk_sorted_rows") >= 100
    assert eng.info("last.sort_passes") == 0 and eng.info("last.sort_bits") == 0 and eng.info("last.join_kernel") == -1
    assert eng.join_cols_dev(dk.ptr, None, 8193, dk.ptr, None, 8193) >= 8193
    for name in ("topk_bits", "topk_passes", "topk_candidates", "topk_sorted_rows"):
        assert eng.info("last." + name) == 0
    topk_cols(eng, dk, keys, 100, 0)
    assert eng.info("last.topk_passes") >= 1
    out = Array(eng, n)
    eng.sort_cols_dev(dk.ptr, None, n, 0, out.ptr, None)
    assert eng.info("last.sort_passes") == 8
    for name in ("topk_bits", "topk_passes", "topk_candidates", "topk_sorted_rows"):
        assert eng.info("last." + name) == 0
    for a in (dk, out):
        a.free()


def test_invalid_arguments_are_refused_and_the_context_stays_usable(eng, cases):
    keys, perm_of = cases("sixteen", 65)
    dk, ok, orr = Array(eng, 65, 0, keys), Array(eng, 10), Array(eng, 10)
    for args in ((dk.ptr, None, 65, 10, 0, None, None),                      # both outputs NULL and no out_kth
                 (dk.ptr, None, 65, 10, 4, ok.ptr, orr.ptr),                 # unknown flags
                 (dk.ptr, None, 65, 10, 0x80000000, ok.ptr, orr.ptr),
                 (dk.ptr, None, 0, 10, 8, None, None),                       # ... also with no rows
                 (None, None, 65, 10, 0, ok.ptr, orr.ptr)):                  # NULL keys with n > 0
        with pytest.raises(RhjError, match="rhj_topk_cols_dev") as err:
            eng.topk_cols_dev(*args)
        assert err.value.code == RHJ_E_INVALID
    with pytest.raises(RhjError, match="rhj_topk_dev") as err:
        eng.topk_dev(dk.ptr, 32, 10, 0, None)
    assert err.value.code == RHJ_E_INVALID
    with pytest.raises(RhjError, match="rhj_topk_dev") as err:
        eng.topk_dev(dk.ptr, 32, 10, 16, ok.ptr)
    assert err.value.code == RHJ_E_INVALID
    assert (ok.read() == GUARD).all() and (orr.read() == GUARD).all()        # nothing was launched
    eng.topk_cols_dev(dk.ptr, None, 65, 10, SORT_DESC, ok.ptr, orr.ptr)
    assert np.array_equal(orr.read(), perm_of(SORT_DESC)[:10])
    for a in (dk, ok, orr):
        a.free()


# ---- the torch entries -------------------------------------------------------------------------------------------------------------
def torch_keys(dist, n):
    return torch.from_numpy(TC.make_keys(dist, n).view(np.int64).copy()).cuda()


@pytest.mark.parametrize("descending", (False, True))
def test_topk_columns_equals_the_head_of_torch_sort_stable(eng, descending):
    for dist, n, k in (("sixteen", 70_000, 1000), ("full64", 70_000, 10), ("cut_run", 70_000, 35_000), ("full64", 8193, 8193),
                       ("small_signed", 65, 100), ("constant", 100, 7), ("full64", 100, 0), ("full64", 0, 5)):
        keys = torch_keys(dist, n)
        values = [torch.arange(n, device="cuda", dtype=torch.int64) * 3, torch_keys("full64", n)]
        before = keys.clone()
        top, idx, gathered = eng.topk_columns(keys, k, values, descending=descending)
        exp = torch.sort(keys, stable=True, descending=descending)
        m = min(k, n)
        assert idx.dtype == torch.int64 and top.dtype == torch.int64 and len(top) == len(idx) == m
        assert torch.equal(top, exp.values[:m]) and torch.equal(idx, exp.indices[:m])
        assert len(gathered) == 2 and all(torch.equal(g, v[idx]) for g, v in zip(gathered, values))
        assert torch.equal(keys, before)


def test_topk_columns_unsigned_orders_the_words_as_uint64(eng):
    host = SC.make_keys("extremes", 70_000)
    keys = torch.from_numpy(host.view(np.int64).copy()).cuda()
    for descending, flags in ((False, 0), (True, SC.SORT_DESC)):
        top, idx, _ = eng.topk_columns(keys, 500, descending=descending, unsigned=True)
        exp = TC.oracle_topk(host, 500, flags).astype(np.int64)
        assert np.array_equal(idx.cpu().numpy(), exp) and np.array_equal(top.cpu().numpy().view(np.uint64), host[exp])


def test_kth_value_columns_equals_the_sorted_tensor(eng):
    for dist, n in (("full64", 70_000), ("sixteen", 70_000), ("small_signed", 65), ("extremes", 8193)):
        keys = torch_keys(dist, n)
        for descending in (False, True):
            exp = torch.sort(keys, stable=True, descending=descending)
            for k in (1, (n + 1) // 2, n):
                value, row = eng.kth_value_columns(keys, k, descending=descending)
                assert isinstance(value, int) and isinstance(row, int)
                assert (value, row) == (int(exp.values[k - 1]), int(exp.indices[k - 1]))
        assert eng.kth_value_columns(keys, 3)[0] == int(torch.kthvalue(keys, 3).values)
        host = keys.cpu().numpy().view(np.uint64)
        value, row = eng.kth_value_columns(keys, n, unsigned=True)
        assert value == int(host.max()) and row == int(TC.oracle_topk(host, n, 0)[-1])
    with pytest.raises(ValueError, match=r"^k: 1 \.\. 65"):
        eng.kth_value_columns(torch_keys("full64", 65), 66)
    with pytest.raises(ValueError, match=r"^keys: .*engine's device"):
        eng.topk_columns(torch_keys("full64", 65).cpu(), 3)
    with pytest.raises(ValueError, match=r"^values\[0\]: 50 elements, keys has 65"):
        eng.topk_columns(torch_keys("full64", 65), 3, [torch_keys("full64", 50)])
