"""GPU suite: the sort entries (rhj_sort_cols_dev / rhj_sort_dev, Engine.sort_columns / argsort_columns) against the numpy oracle of
tests/sort_cases.py.  Every comparison is exact: output position p holds the tuple of rank p, ties in input order in both directions,
the key words bit for bit.  Guard words stand before and behind every output array, and the inputs are compared before and after.

Sizes, with T = info("sort.tile_rows"): 0, 1, 63, 64, 65 (a wave boundary); T-1, T, T+1, 2T+1 (tile tails, the running cursors);
70,000 (several units: the scan across units); 3,000,000 (more units than CUs, every pass with full tiles).  Under the automatic unit
cap every input below 2048 tiles is cut into units of ONE tile, so the running cursors across the tiles of a unit are run under
"sort.max_units" 1 (one workgroup walks every tile) and 3 (several units of several tiles); "last.sort_units" says which geometry ran."""
import contextlib

import numpy as np
import pytest
import torch

import sort_cases as SC
from radixhashjoin_amd import LOOKUP_MAX_COLS, SORT_DESC, SORT_I64, Engine, RhjError
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
def cases():
    """(dist, n) -> (keys, {flags: oracle permutation}): built once, shared, never written"""
    cache = {}

    def get(dist, n):
        if (dist, n) not in cache:
            keys = SC.make_keys(dist, n)
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


def check_info(eng, keys, flags):
    bits, passes = eng.info("last.sort_bits"), eng.info("last.sort_passes")
    exp_bits = SC.oracle_bits(keys, flags)
    print(f"n {len(keys)} flags {flags} bits {bits} (expected {exp_bits}) passes {passes}")
    assert bits == exp_bits
    if bits == 0:
        assert passes == 0
    else:
        assert 0 < passes <= (bits + 7) // 8
    assert eng.info("last.join_kernel") == -1
    return passes


def sort_cols(eng, keys, flags, rows=None, want_keys=True, want_rows=True, off=0, d_keys=None):
    """one rhj_sort_cols_dev call; returns (sorted keys or None, sorted rows or None); checks guards and that the inputs are unchanged"""
    n = len(keys)
    dk = d_keys if d_keys is not None else Array(eng, n, off, keys)
    dr = Array(eng, n, off, rows) if rows is not None else None
    ok = Array(eng, n, off) if want_keys else None
    orr = Array(eng, n, off) if want_rows else None
    try:
        eng.sort_cols_dev(dk.ptr if n else None, dr.ptr if dr is not None and n else None, n, flags, ok.ptr if ok else None, orr.ptr if orr else None)
        if n:
            check_info(eng, keys, flags)
        assert np.array_equal(dk.read(), keys), "the key input was modified"
        if dr is not None:
            assert np.array_equal(dr.read(), rows), "the row input was modified"
        return (ok.read() if ok else None), (orr.read() if orr else None)
    finally:
        for a in (dr, ok, orr) + ((dk,) if d_keys is None else ()):
            if a is not None:
                a.free()


def check_case(eng, keys, perm_of, flagses=SC.FLAGS, off=0):
    n = len(keys)
    dk = Array(eng, n, off, keys)
    try:
        for flags in flagses:
            got_keys, got_rows = sort_cols(eng, keys, flags, off=off, d_keys=dk)
            perm = perm_of(flags)
            wrong = int((got_rows != perm).sum())
            print(f"n {n} flags {flags}: rows that differ from the oracle's {wrong}")
            assert np.array_equal(got_rows, perm)
            assert np.array_equal(got_keys, keys[perm.astype(np.int64)])
    finally:
        dk.free()


def small_sizes(T):
    return (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 70_000)


@pytest.mark.parametrize("dist", SC.DISTS)
def test_every_distribution_at_every_edge_size_in_all_four_flag_combinations(eng, T, cases, dist):
    for n in small_sizes(T):
        keys, perm_of = cases(dist, n)
        check_case(eng, keys, perm_of)


@pytest.mark.parametrize("dist", SC.DISTS)
def test_three_million_rows_more_units_than_cus(eng, T, cases, dist):
    keys, perm_of = cases(dist, BIG)
    check_case(eng, keys, perm_of)
    if dist != "constant":
        assert eng.info("last.sort_units") == -(-BIG // T) > 256          # one tile per unit, more units than CUs


@contextlib.contextmanager
def max_units(eng, units):
    eng.set_option("sort.max_units", units)
    try:
        yield
    finally:
        eng.set_option("sort.max_units", -1)


def expected_units(n, T, cap):
    tiles = -(-n // T)
    per_unit = -(-tiles // cap)
    return -(-tiles // per_unit), per_unit


@pytest.mark.parametrize("cap", (1, 3))
@pytest.mark.parametrize("dist", ("sixteen", "full64"))
def test_several_tiles_per_unit_the_running_cursors(eng, T, cases, dist, cap):
    """cap 1: one unit spans every tile (2, 3 and 18 of them); cap 3 at 70,000 rows: three units of six tiles.  All four flag
    combinations in the narrow, wide, keys-only and argsort forms, and the 16-byte tuples"""
    with max_units(eng, cap):
        for n in (T + 1, 2 * T + 1, 70_000):
            units, per_unit = expected_units(n, T, cap)
            assert per_unit > 1 or cap == 3
            keys, perm_of = cases(dist, n)
            check_case(eng, keys, perm_of)
            assert eng.info("last.sort_units") == units
            rows = SC.wide_rows(n)
            tuples = np.empty((n, 2), dtype=np.uint64)
            tuples[:, 0], tuples[:, 1] = rows, keys
            d_in = Array(eng, 2 * n, 0, tuples.reshape(-1))
            for flags in SC.FLAGS:
                perm = perm_of(flags).astype(np.int64)
                wide_keys, wide_rows = sort_cols(eng, keys, flags, rows=rows)
                assert np.array_equal(wide_rows, rows[perm]) and np.array_equal(wide_keys, keys[perm])
                only_keys, _ = sort_cols(eng, keys, flags, want_rows=False)
                assert np.array_equal(only_keys, keys[perm])
                _, arg = sort_cols(eng, keys, flags, want_keys=False)
                assert np.array_equal(arg, perm.astype(np.uint64))
                assert eng.info("last.sort_units") == units
                d_out = Array(eng, 2 * n)
                eng.sort_dev(d_in.ptr, n, flags, d_out.ptr)
                got = d_out.read().reshape(n, 2)
                assert np.array_equal(got[:, 1], keys[perm]) and np.array_equal(got[:, 0], rows[perm])
                d_out.free()
            d_in.free()
    keys, _ = cases(dist, 70_000)
    sort_cols(eng, keys, 0)
    assert eng.info("last.sort_units") == -(-70_000 // T)                    # the automatic cap is back: one tile per unit


def test_three_million_rows_in_units_of_many_tiles(eng, T, cases):
    """a cap of 64: 62 units of 12 tiles each -- several multi-tile units, the scan across them"""
    keys, perm_of = cases("full64", BIG)
    with max_units(eng, 64):
        check_case(eng, keys, perm_of, flagses=(SORT_I64, SORT_DESC))
        assert eng.info("last.sort_units") == expected_units(BIG, T, 64)[0] and expected_units(BIG, T, 64)[1] > 1


def test_max_units_refuses_values_outside_its_range(eng):
    for bad in (0, -2, 2049):
        with pytest.raises(RhjError) as err:
            eng.set_option("sort.max_units", bad)
        assert err.value.code == RHJ_E_INVALID
    eng.set_option("sort.max_units", 2048)
    eng.set_option("sort.max_units", -1)


def test_full_range_keys_take_eight_passes_and_a_constant_column_none(eng, T, cases):
    keys, perm_of = cases("full64", 70_000)
    sort_cols(eng, keys, 0)
    assert eng.info("last.sort_bits") == 64 and eng.info("last.sort_passes") == 8
    keys, _ = cases("constant", 2 * T + 1)
    for flags in SC.FLAGS:
        got_keys, got_rows = sort_cols(eng, keys, flags)
        assert eng.info("last.sort_bits") == 0 and eng.info("last.sort_passes") == 0
        assert np.array_equal(got_rows, np.arange(len(keys), dtype=np.uint64)) and np.array_equal(got_keys, keys)
    keys, _ = cases("small_signed", 70_000)
    sort_cols(eng, keys, SORT_I64)
    assert eng.info("last.sort_bits") == 3 and eng.info("last.sort_passes") == 1
    sort_cols(eng, keys, 0)
    assert eng.info("last.sort_bits") == 64


def test_a_skipped_and_an_unskipped_middle_pass_agree(eng, cases):
    """r1 << 16 | 0x55 << 8 | r2, 24 bits wide.  Ascending the sort key is v - min: with the minimum's low digit 0 nothing borrows and
    the middle digit is one bin for every row -- the pass is skipped, 2 passes --, with 200 the rows below it borrow and it is two
    bins -- 3 passes.  Descending the key is max - v and the borrow comes from the MAXIMUM's low digit: 255 none, 50 some.  Both
    orders are the oracle's."""
    keys, _ = cases("middle_digit", 70_000)
    for low, high, passes in ((0, 255, 2), (200, 50, 3)):
        k = keys.copy()
        k[k < np.uint64(1 << 16)] |= np.uint64(200)                  # r1 == 0: no row below the planted minimum
        top = k >= np.uint64(255 << 16)                              # r1 == 255: no row above the planted maximum
        k[top] = (k[top] & ~np.uint64(255)) | ((k[top] & np.uint64(255)) % np.uint64(high + 1))
        k[12345] = np.uint64(0x55 << 8 | low)                        # the minimum: r1 = 0, r2 = low
        k[54321] = np.uint64(255 << 16 | 0x55 << 8 | high)           # the maximum: r1 = 255, r2 = high
        assert int(k.min()) == int(k[12345]) and int(k.max()) == int(k[54321])
        assert (k & np.uint64(255) < np.uint64(200)).any() and (k & np.uint64(255) > np.uint64(50)).any()
        for flags in SC.FLAGS:
            got_keys, got_rows = sort_cols(eng, k, flags)
            perm = SC.oracle_perm(k, flags)
            assert np.array_equal(got_rows, perm) and np.array_equal(got_keys, k[perm.astype(np.int64)])
            assert eng.info("last.sort_bits") == 24 and eng.info("last.sort_passes") == passes, (low, high, flags)


def test_keys_that_differ_only_in_their_top_byte_skip_the_passes_below(eng, cases):
    keys, perm_of = cases("top_byte", 70_000)
    _, got_rows = sort_cols(eng, keys, 0)
    assert np.array_equal(got_rows, perm_of(0))
    assert eng.info("last.sort_bits") == 64 and eng.info("last.sort_passes") == 1


@pytest.mark.parametrize("n", (65, 8193, 70_000))
def test_the_payload_forms_give_one_order(eng, cases, n):
    """wide (explicit rows with duplicates and values >= 2^32: ties go by position, not by row value), narrow (implicit rows),
    keys-only, argsort-only"""
    for dist in ("sixteen", "full64"):
        keys, perm_of = cases(dist, n)
        rows = SC.wide_rows(n)
        for flags in SC.FLAGS:
            perm = perm_of(flags).astype(np.int64)
            wide_keys, wide_rows = sort_cols(eng, keys, flags, rows=rows)
            assert np.array_equal(wide_rows, rows[perm]) and np.array_equal(wide_keys, keys[perm])
            narrow_keys, narrow_rows = sort_cols(eng, keys, flags)
            assert np.array_equal(narrow_rows, perm.astype(np.uint64)) and np.array_equal(narrow_keys, keys[perm])
            only_keys, none = sort_cols(eng, keys, flags, want_rows=False)
            assert none is None and np.array_equal(only_keys, keys[perm])
            only_keys, none = sort_cols(eng, keys, flags, rows=rows, want_rows=False)       # rows given, not wanted: never read
            assert np.array_equal(only_keys, keys[perm])
            none, arg = sort_cols(eng, keys, flags, want_keys=False)
            assert none is None and np.array_equal(arg, perm.astype(np.uint64))
            none, arg = sort_cols(eng, keys, flags, rows=rows, want_keys=False)
            assert np.array_equal(arg, rows[perm])


@pytest.mark.parametrize("n", (1, 65, 4097, 69_999))
def test_pointers_that_are_8_byte_but_not_16_byte_aligned(eng, cases, n):
    assert n % 2 == 1
    for dist in ("full64", "sixteen"):
        keys, perm_of = cases(dist, n)
        check_case(eng, keys, perm_of, off=1)
        rows = SC.wide_rows(n)
        perm = perm_of(SORT_DESC).astype(np.int64)
        got_keys, got_rows = sort_cols(eng, keys, SORT_DESC, rows=rows, off=1)
        assert np.array_equal(got_rows, rows[perm]) and np.array_equal(got_keys, keys[perm])


@pytest.mark.parametrize("n", (0, 1, 65, 8193, 70_000))
def test_sixteen_byte_tuples(eng, cases, n):
    for dist in ("sixteen", "extremes"):
        keys, perm_of = cases(dist, n)
        rows = SC.wide_rows(n)
        tuples = np.empty((n, 2), dtype=np.uint64)
        tuples[:, 0], tuples[:, 1] = rows, keys                              # .key = rowID, .payload = value
        d_in = Array(eng, 2 * n, 0, tuples.reshape(-1))
        for flags in SC.FLAGS:
            d_out = Array(eng, 2 * n)
            eng.sort_dev(d_in.ptr if n else None, n, flags, d_out.ptr if n else None)
            if n:
                check_info(eng, keys, flags)
            got = d_out.read().reshape(n, 2)
            perm = perm_of(flags).astype(np.int64)
            assert np.array_equal(got[:, 1], keys[perm]) and np.array_equal(got[:, 0], rows[perm])
            assert np.array_equal(d_in.read(), tuples.reshape(-1))
            d_out.free()
        d_in.free()


def test_invalid_arguments_are_refused_and_the_context_stays_usable(eng, cases):
    keys, perm_of = cases("sixteen", 65)
    dk, ok, orr = Array(eng, 65, 0, keys), Array(eng, 65), Array(eng, 65)
    for args in ((dk.ptr, None, 65, 0, None, None),                          # both outputs NULL
                 (dk.ptr, None, 65, 4, ok.ptr, orr.ptr),                     # unknown flags
                 (dk.ptr, None, 65, 0x80000000, ok.ptr, orr.ptr),
                 (dk.ptr, None, 0, 8, None, None),                           # ... also with no rows
                 (None, None, 65, 0, ok.ptr, orr.ptr)):                      # NULL keys with n > 0
        with pytest.raises(RhjError) as err:
            eng.sort_cols_dev(*args)
        assert err.value.code == RHJ_E_INVALID
    with pytest.raises(RhjError) as err:
        eng.sort_dev(dk.ptr, 32, 0, None)
    assert err.value.code == RHJ_E_INVALID
    with pytest.raises(RhjError) as err:
        eng.sort_dev(dk.ptr, 32, 16, ok.ptr)
    assert err.value.code == RHJ_E_INVALID
    assert (ok.read() == GUARD).all() and (orr.read() == GUARD).all()        # nothing was launched
    eng.sort_cols_dev(None, None, 0, 0, None, None)                          # n == 0: RHJ_OK
    eng.sort_cols_dev(dk.ptr, None, 65, SORT_DESC, ok.ptr, orr.ptr)
    assert np.array_equal(orr.read(), perm_of(SORT_DESC))
    for a in (dk, ok, orr):
        a.free()


def test_info_after_a_join_and_after_a_sort(eng, cases):
    keys, _ = cases("full64", 8193)
    sort_cols(eng, keys, 0)
    assert eng.info("last.sort_passes") == 8 and eng.info("last.join_kernel") == -1
    dk = eng.to_device(keys)
    assert eng.join_cols_dev(dk, None, len(keys), dk, None, len(keys)) >= len(keys)
    assert eng.info("last.sort_passes") == 0 and eng.info("last.sort_bits") == 0
    sort_cols(eng, keys, 0)
    assert eng.info("last.sort_passes") == 8 and eng.info("last.join_kernel") == -1
    dk.free()


def test_two_runs_are_bit_identical_and_profiling_names_the_spans(eng, cases):
    keys, _ = cases("sixteen", 70_000)
    rows = SC.wide_rows(70_000)
    a = sort_cols(eng, keys, SORT_I64 | SORT_DESC, rows=rows)
    eng.set_profiling(True)
    b = sort_cols(eng, keys, SORT_I64 | SORT_DESC, rows=rows)
    t, passes = eng.timings(), eng.info("last.sort_passes")
    eng.set_profiling(False)                                                 # (starts a new series: the "last.*" values go back to 0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert 0 < passes <= 8
    assert t["hist"]["launches"] == t["scan"]["launches"] == t["scatter"]["launches"] == passes      # three launches per pass
    assert t["aux"]["launches"] == 2 and t["join"]["launches"] == 0 and t["tasks"]["launches"] == 0   # the two probes


# ---- the torch entries -------------------------------------------------------------------------------------------------------------
def torch_keys(dist, n):
    return torch.from_numpy(SC.make_keys(dist, n).view(np.int64).copy()).cuda()


@pytest.mark.parametrize("descending", (False, True))
def test_sort_columns_equals_torch_sort_stable(eng, descending):
    for dist, n in (("sixteen", 70_000), ("full64", 8193), ("small_signed", 65), ("constant", 100), ("full64", 0)):
        keys = torch_keys(dist, n)
        values = [torch.arange(n, device="cuda", dtype=torch.int64) * 3, torch_keys("full64", n)]
        before = keys.clone()
        sorted_keys, perm, gathered = eng.sort_columns(keys, values, descending=descending)
        exp = torch.sort(keys, stable=True, descending=descending)
        assert perm.dtype == torch.int64 and sorted_keys.dtype == torch.int64
        assert torch.equal(sorted_keys, exp.values) and torch.equal(perm, exp.indices)
        assert len(gathered) == 2 and all(torch.equal(g, v[perm]) for g, v in zip(gathered, values))
        assert torch.equal(eng.argsort_columns(keys, descending=descending), perm)
        assert torch.equal(keys, before)


def test_sort_columns_unsigned_orders_the_words_as_uint64(eng):
    host = SC.make_keys("extremes", 8193)
    keys = torch.from_numpy(host.view(np.int64).copy()).cuda()
    for descending, flags in ((False, 0), (True, SC.SORT_DESC)):
        sorted_keys, perm, _ = eng.sort_columns(keys, descending=descending, unsigned=True)
        exp = SC.oracle_perm(host, flags).astype(np.int64)
        assert np.array_equal(perm.cpu().numpy(), exp) and np.array_equal(sorted_keys.cpu().numpy().view(np.uint64), host[exp])


def test_order_by_two_columns_equals_lexsort(eng):
    """a from 8 values, b from 5: both levels tie; ORDER BY a ASC, b DESC"""
    n = 70_000
    rng = np.random.default_rng(5)
    a = rng.integers(-4, 4, n, dtype=np.int64)
    b = rng.integers(-2, 3, n, dtype=np.int64)
    ta, tb = SC.transform(a.view(np.uint64), SC.SORT_I64), SC.transform(b.view(np.uint64), SC.SORT_I64 | SC.SORT_DESC)
    exp = np.lexsort((tb, ta))                                               # (stable; the last key is the primary one)
    v = torch.arange(n, device="cuda", dtype=torch.int64) * 7
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    sorted_keys, perm, gathered = eng.sort_columns([da, db], [v], descending=[False, True])
    assert isinstance(sorted_keys, list) and len(sorted_keys) == 2
    assert np.array_equal(perm.cpu().numpy(), exp)
    assert np.array_equal(sorted_keys[0].cpu().numpy(), a[exp]) and np.array_equal(sorted_keys[1].cpu().numpy(), b[exp])
    assert torch.equal(gathered[0], v[perm])
    assert torch.equal(eng.argsort_columns([da, db], descending=[False, True]), perm)
    # one bool for all, and a list of one tensor
    _, perm_all, _ = eng.sort_columns([da, db], descending=True)
    exp_all = np.lexsort((SC.transform(b.view(np.uint64), 3), SC.transform(a.view(np.uint64), 3)))
    assert np.array_equal(perm_all.cpu().numpy(), exp_all)
    one, perm_one, _ = eng.sort_columns([da])
    assert isinstance(one, list) and torch.equal(perm_one, torch.sort(da, stable=True).indices)


def test_wrong_tensors_are_value_errors_that_name_the_argument(eng):
    keys = torch_keys("sixteen", 100)
    with pytest.raises(ValueError, match=r"^keys: .*engine's device"):
        eng.sort_columns(keys.cpu())
    with pytest.raises(ValueError, match=r"^keys: a 1-D torch tensor of 64-bit integers"):
        eng.sort_columns(keys.to(torch.int32))
    with pytest.raises(ValueError, match=r"^values\[0\]: 50 elements, keys has 100"):
        eng.sort_columns(keys, [keys[:50]])
    with pytest.raises(ValueError, match=r"^values\[1\]: .*contiguous"):
        eng.sort_columns(keys, [keys, torch.cat([keys, keys])[::2]])
    with pytest.raises(ValueError, match="at most 4 value tensors"):
        eng.sort_columns(keys, [keys] * (LOOKUP_MAX_COLS + 1))
    with pytest.raises(ValueError, match=r"^keys\[1\]: 50 elements, keys\[0\] has 100"):
        eng.sort_columns([keys, keys[:50].clone()])
    with pytest.raises(ValueError, match=r"^keys\[1\]: a 1-D torch tensor"):
        eng.argsort_columns([keys, None])
    with pytest.raises(ValueError, match=r"^values\[0\]: .*engine's device"):
        eng.sort_columns([keys, keys], [keys.cpu()])


def test_a_run_on_a_non_default_torch_stream(eng):
    n = 70_000
    stream = torch.cuda.Stream()
    filler = torch.arange(1 << 20, device="cuda", dtype=torch.int64)
    torch.cuda.synchronize()
    stream.wait_stream(torch.cuda.default_stream())
    with torch.cuda.stream(stream):
        assert torch.cuda.current_stream().cuda_stream != 0
        for _ in range(20):
            filler.mul_(3).add_(1)                                           # queued work the sort must stay behind
        keys = (filler[:n] % 1000).clone()
        sorted_keys, perm, gathered = eng.sort_columns(keys, [filler[:n]])
        exp = torch.sort(keys, stable=True)
    stream.synchronize()
    assert torch.equal(perm, exp.indices) and torch.equal(sorted_keys, exp.values) and torch.equal(gathered[0], filler[:n][perm])
    assert eng.bound_stream in (0, None) or eng.bound_stream != stream.cuda_stream
