"""GPU suite: the frame entry (rhj_frame_cols_dev, Engine.frame_columns / ntile_columns) against the oracles of tests/frame_cases.py.
Every comparison is exact, aligned with the input rows.  Every output lies between guard words, the inputs are compared before and
after, and "last.frame_*" and the zeroed "last.*" of the other entries are asserted after each call.

Under the automatic "sort.max_units" every input below 2048 tiles is cut into units of one tile; the carry across the tiles of a unit
runs under "sort.max_units" 1 and 3, and the large case has more units than the device has CUs.  The naive oracle answers every case
but the large one, which goes against the gathered-window oracle and cumulative sums."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import frame_cases as FC
from radixhashjoin_amd import Engine, RhjError
from radixhashjoin_amd.binding import RHJ_E_INVALID

pytestmark = pytest.mark.gpu

GUARD, NGUARD = FC.GUARD, FC.NGUARD
U = FC.UNBOUNDED
BIG = 3_000_000
ZEROED = ("sort_bits", "sort_passes", "sort_units", "topk_bits", "topk_passes", "topk_candidates", "topk_sorted_rows", "window_units",
          "window_sorts", "window_partitions", "asof_units", "asof_sorts", "asof_matched")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def T(eng):
    t = eng.info("window.tile_rows")
    assert t >= 128 and t % 64 == 0
    return t


class Array:
    """n words in HBM at an offset of `off` words into a buffer of off + n + NGUARD words, guard words before and behind (and in the
    n words themselves until something is written there)"""
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


def units_of(n, T, max_units=2048):
    tiles = -(-n // T)
    per = -(-tiles // max_units)
    return -(-n // (per * T)) if n else 0


def check_info(eng, n, T, sorts, partitions, scans, max_units=2048):
    got = {name: eng.info("last." + name) for name in ("frame_units", "frame_sorts", "frame_partitions", "frame_scans", "join_kernel") + ZEROED}
    assert got["join_kernel"] == -1
    assert all(got[name] == 0 for name in ZEROED), got
    assert got["frame_units"] == units_of(n, T, max_units), got
    assert got["frame_sorts"] == (sorts if n else 0) and got["frame_partitions"] == partitions, got
    assert got["frame_scans"] == (scans if n else 0), got


class Table:
    """the input columns of a case in HBM, between guard words; read back and compared when the case is closed"""
    def __init__(self, eng, part, order, cols):
        self.eng = eng
        self.host = {"part": part, "order": order, **{f"col{j}": c for j, c in enumerate(cols)}}
        self.n = len(next(a for a in self.host.values() if a is not None))
        self.dev = {k: Array(eng, self.n, off=1 + i, data=a) for i, (k, a) in enumerate(self.host.items()) if a is not None}

    def ptr(self, name):
        return self.dev[name].ptr if name in self.dev else None

    def close(self):
        for k, a in self.dev.items():
            assert np.array_equal(a.read(), self.host[k]), f"the input column {k} was modified"
            a.free()


def call(eng, T, tab, flags, ops, pre, fol, which, max_units=2048, twice=False, expect=None):
    """one rhj_frame_cols_dev call on the table's columns (which[j]: the value column of op j, or None; pre / fol: one bound per op,
    or None for the entry's default) against the naive oracle (expect: the answer, where a test has it from elsewhere)"""
    n = tab.n
    part, order = tab.host["part"], tab.host["order"]
    cols = [tab.host[w] if w else None for w in which]
    want, partitions = expect if expect is not None else FC.brute(part, order, flags, ops, pre, fol, cols, n)
    outs = [Array(eng, n, off=3 + j) for j in range(len(ops))]
    runs = []
    for _ in range(2 if twice else 1):
        got = eng.frame_cols_dev(tab.ptr("part"), tab.ptr("order"), n, flags, ops, pre, fol, [tab.ptr(w) if w else None for w in which],
                                 [o.ptr for o in outs])
        assert got == partitions
        check_info(eng, n, T, (part is not None) + (order is not None), partitions, FC.value_scans(n, ops, pre, fol), max_units)
        runs.append([o.read().copy() for o in outs])
    for j, op in enumerate(ops):
        bad = np.nonzero(runs[0][j] != want[j])[0]
        assert len(bad) == 0, (f"op {op} (#{j}), frame ({pre[j] if pre else None}, {fol[j] if fol else None}), flags {flags}, n {n}: "
                               f"{len(bad)} rows differ, first at row {bad[:5].tolist()}: {runs[0][j][bad[:5]].tolist()} for "
                               f"{want[j][bad[:5]].tolist()}")
        if twice:
            assert np.array_equal(runs[0][j], runs[1][j]), "two runs differ"
    for o in outs:
        o.free()


ROWS4 = (FC.COUNT, FC.SUM, FC.FIRST_ROW, FC.LAST_ROW)
MIXED4 = (FC.MIN_I64, FC.MAX_U64, FC.SUM, FC.COUNT)


def small_sizes(T):
    return {"1": 1, "2": 2, "63": 63, "64": 64, "65": 65, "T-1": T - 1, "T": T, "T+1": T + 1, "3T+5": 3 * T + 5}


def make_part(shape, n, T, rng):
    if shape == "none":
        return None
    if shape == "one":
        return np.full(n, 1 << 63, dtype=np.uint64)
    if shape == "each":
        return FC.dense_part([1] * n, rng)
    if shape == "1..130":
        return FC.dense_part(FC.sizes_1_to(130, n), rng)
    raise ValueError(shape)


@pytest.mark.parametrize("shape", ["none", "one", "each", "1..130"])
@pytest.mark.parametrize("size", ["1", "2", "63", "64", "65", "T-1", "T", "T+1", "3T+5"])
def test_every_op_at_every_small_size_and_partition_shape(eng, T, size, shape):
    """four ops with four different frames in one call, then the same column under the four extremes"""
    n = small_sizes(T)[size]
    i = list(small_sizes(T)).index(size) + ["none", "one", "each", "1..130"].index(shape)
    rng = np.random.default_rng(100 + i)
    kind = ("none", "sixteen", "distinct", "extremes")[i % 4]
    flags = FC.FLAGS[i % 4] if kind != "none" else 0
    tab = Table(eng, make_part(shape, n, T, rng), FC.make_order(kind, n), [FC.make_values(("full64", "extremes", "mixed")[i % 3], n)])
    call(eng, T, tab, flags, ROWS4, [2, 10, 1, U], [3, 0, 0, 7], [None, "col0", None, None])
    widths = FC.frame_widths(T, n)
    pre, fol = zip(*[widths[(i + 5 * j) % len(widths)] for j in range(4)])
    call(eng, T, tab, flags, FC.EXTREMES, list(pre), list(fol), ["col0"] * 4)
    tab.close()


@pytest.mark.parametrize("big", [False, True], ids=["T+1", "3T+5"])
@pytest.mark.parametrize("width", range(17))
def test_every_frame_width(eng, T, width, big):
    """block boundaries on lane, wave, round, tile and unit cuts; partitions shorter than, equal to and longer than w; w >= n; w
    overflowing; each unbounded side.  Dense partition ids in input order, so the heads stand where the sizes put them"""
    n = 3 * T + 5 if big else T + 1
    pre, fol = FC.frame_widths(T, n)[width]
    w = min(pre + fol + 1, n)
    sizes = [s for s in (w - 1, w, w + 1, 1, 2 * w + 3) if 0 < s < n // 4]
    sizes += FC.sizes_1_to(130, n // 4)
    sizes = sizes + [n - sum(sizes)] if sum(sizes) < n else [n]
    part = FC.dense_part(sizes)
    tab = Table(eng, part, None, [FC.make_values("mixed", n, seed=width)])
    call(eng, T, tab, 0, MIXED4, [pre] * 4, [fol] * 4, ["col0", "col0", "col0", None])
    call(eng, T, tab, 0, (FC.MAX_I64, FC.MIN_U64, FC.FIRST_ROW, FC.LAST_ROW), [pre] * 4, [fol] * 4, ["col0", "col0", None, None])
    tab.close()
    one = Table(eng, None, None, [FC.make_values("mixed", n, seed=width + 50)])          # one partition: only block heads restart the scans
    call(eng, T, one, 0, (FC.MIN_U64, FC.MAX_U64, FC.SUM, FC.COUNT), [pre] * 4, [fol] * 4, ["col0", "col0", "col0", None])
    one.close()


@pytest.mark.parametrize("max_units", [1, 3])
def test_the_carry_crosses_tiles_inside_a_unit_and_units(eng, T, max_units):
    n = 7 * T - 3
    unit = -(-7 // max_units) * T
    rng = np.random.default_rng(31 + max_units)
    heads = FC.heads_around(n, (T, unit)) | FC.heads_around(min(n, 8 * 64), (64,))
    part = FC.dense_part(FC.sizes_with_heads_at(n, heads), rng)
    order = FC.make_order("distinct", n)
    tab = Table(eng, part, order, [FC.make_values("mixed", n, seed=max_units)])
    one = Table(eng, None, None, [FC.make_values("full64", n, seed=max_units)])
    with option(eng, "sort.max_units", max_units):
        assert units_of(n, T, max_units) == max_units
        call(eng, T, tab, FC.SORT_I64, (FC.MIN_I64, FC.MAX_U64, FC.SUM, FC.LAST_ROW), [2, T, U, 5], [3, 0, 5, U], ["col0", "col0", "col0", None],
             max_units)
        call(eng, T, tab, FC.SORT_DESC, (FC.MAX_I64, FC.MIN_U64, FC.SUM, FC.COUNT), [T // 2, 5, 63, U], [T // 2, U, 0, U],
             ["col0", "col0", "col0", None], max_units)
        call(eng, T, one, 0, (FC.MIN_U64, FC.MAX_I64, FC.SUM, FC.MIN_I64), [2 * T + 1, 63, T - 1, U], [T, 0, 1, 5], ["col0"] * 4, max_units)
    tab.close()
    one.close()


@pytest.mark.parametrize("marks", ["64", "T"])
def test_partition_heads_exactly_on_one_before_and_one_after_the_cuts(eng, T, marks):
    n = 3 * T + 5
    heads = FC.heads_around(n, (T,)) if marks == "T" else FC.heads_around(n, (64,))
    part = FC.dense_part(FC.sizes_with_heads_at(n, heads))
    tab = Table(eng, part, None, [FC.make_values("mixed", n, seed=3)])
    call(eng, T, tab, 0, (FC.MIN_U64, FC.MAX_I64, FC.SUM, FC.COUNT), [32, T - 1, 1, 0], [31, 0, 1, 1], ["col0", "col0", "col0", None])
    call(eng, T, tab, 0, (FC.MAX_U64, FC.MIN_I64, FC.FIRST_ROW, FC.LAST_ROW), [0, 1, 64, 2], [1, 0, 0, 3], ["col0", "col0", None, None])
    tab.close()


@pytest.mark.parametrize("kind", ["none", "sixteen", "distinct", "extremes"])
@pytest.mark.parametrize("parted", [True, False])
def test_directions_views_and_missing_columns(eng, T, parted, kind):
    """ascending, DESC, I64; no order column, no partition column, neither"""
    n = 2 * T + 1
    rng = np.random.default_rng(77)
    part = FC.dense_part(FC.sizes_1_to(130, n), rng) * np.uint64(0x8000000000000001) if parted else None
    order = FC.make_order(kind, n)
    tab = Table(eng, part, order, [FC.make_values("mixed", n, seed=9)])
    for flags in (FC.FLAGS if order is not None else (0,)):
        call(eng, T, tab, flags, (FC.SUM, FC.MIN_I64, FC.FIRST_ROW, FC.COUNT), [3, U, 1, 0], [2, 0, 1, U], ["col0", "col0", None, None])
    call(eng, T, tab, 0, (FC.SUM, FC.MAX_U64), None, None, ["col0", "col0"])              # NULL bounds: the running frame
    tab.close()


def test_the_identities_appear_as_data(eng, T):
    """0, all ones, 1 << 63 and (1 << 63) - 1 only: the four extremes differ between the views; one case twice for bit-identity"""
    n = 2 * T + 77
    rng = np.random.default_rng(5)
    col = FC.make_values("extremes", n)
    tab = Table(eng, FC.dense_part(FC.sizes_1_to(40, n), rng), FC.make_order("sixteen", n), [col])
    for pre, fol in ((0, 0), (2, 3), (U, U), (1, 0), (40, 40)):
        call(eng, T, tab, FC.SORT_I64, FC.EXTREMES, [pre] * 4, [fol] * 4, ["col0"] * 4, twice=(pre, fol) == (2, 3))
    outs, _ = FC.brute(tab.host["part"], tab.host["order"], 0, FC.EXTREMES, [U] * 4, [U] * 4, [col] * 4)
    assert len({int(o[0]) for o in outs}) == 4
    tab.close()


def test_value_scans_of_the_one_scan_and_two_scan_cases(eng, T):
    n = T + 9
    tab = Table(eng, None, None, [FC.make_values("full64", n)])
    out = Array(eng, n)

    def scans(op, pre, fol):
        eng.frame_cols_dev(None, None, n, 0, [op], [pre], [fol], [tab.ptr("col0")], [out.ptr])
        return eng.info("last.frame_scans")

    assert [scans(FC.COUNT, 1, 1), scans(FC.FIRST_ROW, U, 0), scans(FC.SUM, 1, 1), scans(FC.SUM, U, U)] == [0, 0, 1, 1]
    assert [scans(FC.MIN_U64, U, 0), scans(FC.MAX_I64, 0, U), scans(FC.MAX_U64, U, U), scans(FC.MIN_I64, U, 5), scans(FC.MIN_I64, 5, U)] == [1] * 5
    assert [scans(FC.MIN_U64, n - 1, 0), scans(FC.MIN_U64, 3, n - 1), scans(FC.MAX_U64, n, n), scans(FC.MAX_U64, 1 << 63, 1 << 63)] == [1] * 4
    # both sides short of n - 1: the rows near either end of a partition clip on different sides, whatever w is
    assert [scans(FC.MIN_U64, 0, 0), scans(FC.MAX_I64, 2, 3), scans(FC.MIN_I64, T, 0), scans(FC.MAX_U64, n - 2, n - 2)] == [2] * 4
    out.free()
    tab.close()


def test_invalid_arguments_and_no_rows(eng, T):
    n = 100
    tab = Table(eng, np.zeros(n, dtype=np.uint64), np.arange(n, dtype=np.uint64), [np.arange(n, dtype=np.uint64)])
    out = Array(eng, n)
    P, O, X = tab.ptr("part"), tab.ptr("order"), tab.ptr("col0")

    def refused(message, *args):
        with pytest.raises(RhjError) as err:
            eng.frame_cols_dev(*args)
        assert err.value.code == RHJ_E_INVALID and message in str(err.value), str(err.value)

    refused("rhj_frame_cols_dev: unknown flags", P, O, n, 4, [FC.COUNT], None, None, None, [out.ptr])
    refused("rhj_frame_cols_dev: unknown flags", P, O, 0, 1 << 31, [FC.COUNT], None, None, None, [out.ptr])
    refused("rhj_frame_cols_dev: flags without d_order", P, None, n, FC.SORT_DESC, [FC.COUNT], None, None, None, [out.ptr])
    refused("rhj_frame_cols_dev: nops must be 1 .. RHJ_FRAME_MAX_OPS", P, O, n, 0, [], None, None, None, [])
    refused("rhj_frame_cols_dev: nops must be 1 .. RHJ_FRAME_MAX_OPS", P, O, n, 0, [FC.COUNT] * 5, None, None, None, [out.ptr] * 5)
    parts = C.c_uint64(77)
    for message, ops, outs in (("ops is null", None, (C.c_void_p * 1)(out.ptr)), ("d_outs is null", (C.c_uint32 * 1)(FC.COUNT), None)):
        rc = eng.lib.rhj_frame_cols_dev(eng.ctx, P, O, n, 0, ops, None, None, None, 1, outs, C.byref(parts))     # (the binding would say nops 0)
        assert rc == RHJ_E_INVALID
        with pytest.raises(RhjError, match="rhj_frame_cols_dev: " + message):
            eng._chk(rc)
    refused("rhj_frame_cols_dev: d_outs[1] is null", P, O, n, 0, [FC.COUNT, FC.COUNT], None, None, None, [out.ptr, None])
    refused("rhj_frame_cols_dev: ops[1] is not an RHJ_FRAME_* op", P, O, n, 0, [FC.COUNT, FC.LAST_ROW + 1], None, None, None, [out.ptr] * 2)
    for op in (FC.SUM,) + FC.EXTREMES:
        refused("rhj_frame_cols_dev: d_cols[1] is null for a column op", P, O, n, 0, [FC.COUNT, op], None, None, [None, None], [out.ptr] * 2)
        refused("rhj_frame_cols_dev: d_cols[0] is null for a column op", P, O, n, 0, [op], None, None, None, [out.ptr])
    assert (out.read() == GUARD).all()                                   # nothing was launched
    # no rows: RHJ_OK, no launch, 0 partitions -- also for a column op without a column
    assert eng.frame_cols_dev(None, None, 0, 0, [FC.SUM], None, None, None, [out.ptr]) == 0
    check_info(eng, 0, T, 0, 0, 0)
    assert (out.read() == GUARD).all()
    x = tab.host["col0"]
    col, one = (C.c_void_p * 1)(X), (C.c_void_p * 1)(out.ptr)
    assert eng.lib.rhj_frame_cols_dev(eng.ctx, P, O, n, 0, (C.c_uint32 * 1)(FC.SUM), None, None, col, 1, one, None) == 0          # out_partitions NULL
    assert np.array_equal(out.read(), np.cumsum(x, dtype=np.uint64))
    out.free()
    tab.close()


def test_torch_entries(eng, T):
    n = T + 300
    rng = np.random.default_rng(23)
    a, b = rng.integers(0, 7, n), rng.integers(-3, 4, n)
    order = rng.integers(-50, 50, n)
    x = FC.make_values("mixed", n).view(np.int64)
    dev = lambda h: torch.from_numpy(np.ascontiguousarray(h)).to("cuda")
    pair = (a * 16 + (b + 3)).astype(np.uint64)                             # equal exactly where both columns are
    ops = [FC.SUM, FC.MIN_I64, FC.MAX_I64, FC.LAST_ROW]
    want, _ = FC.brute(pair, order.view(np.uint64), FC.SORT_I64 | FC.SORT_DESC, ops, [4, 2, U, 0], [0, 2, 0, 1], [x.view(np.uint64)] * 3 + [None])
    got = eng.frame_columns([dev(a), dev(b)], dev(order), [dev(x)] * 3 + [None], ["sum", "min", "max", "last_row"], [4, 2, None, 0], [0, 2, 0, 1],
                            descending=True)
    assert [g.dtype for g in got] == [torch.int64] * 4
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy().view(np.uint64), w)
    want, _ = FC.brute(a.astype(np.uint64), None, 0, [FC.MIN_U64, FC.COUNT, FC.FIRST_ROW], [U, U, 3], [0, U, 0], [x.view(np.uint64), None, None])
    got = eng.frame_columns(dev(a), None, [dev(x), None, None], ["min", "count", "first_row"], [None, None, 3], [0, None, 0], unsigned=True)
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy().view(np.uint64), w)
    got = eng.frame_columns(dev(a), None, [dev(x)], ["sum"])                # the defaults: the running sum
    assert np.array_equal(got[0].cpu().numpy().view(np.uint64), FC.sums(a.astype(np.uint64), None, 0, x.view(np.uint64), U, 0))
    for buckets in (1, 3, 4, 1000):
        tile = eng.ntile_columns(dev(a), dev(order), buckets)
        assert np.array_equal(tile.cpu().numpy(), FC.ntile(a.astype(np.uint64), order.view(np.uint64), FC.SORT_I64, buckets)), buckets
    tile = eng.ntile_columns([dev(a), dev(b)], dev(order), 5, descending=True)
    assert np.array_equal(tile.cpu().numpy(), FC.ntile(pair, order.view(np.uint64), FC.SORT_I64 | FC.SORT_DESC, 5))
    empty = torch.empty(0, dtype=torch.int64, device="cuda")
    assert [t.numel() for t in eng.frame_columns(empty, None, [empty], ["sum"])] == [0]


def test_more_units_than_cus(eng, T):
    """3 x 10^6 rows: minimum and maximum against the gathered windows, the sums against cumulative sums, the rows by arithmetic"""
    n = BIG
    assert units_of(n, T) > 512
    rng = np.random.default_rng(41)
    part = rng.integers(0, n // 100, n).astype(np.uint64)
    order = rng.integers(0, 1 << 20, n).astype(np.uint64)
    col = FC.make_values("mixed", n)
    ops, pre, fol = [FC.MIN_I64, FC.MAX_U64, FC.SUM, FC.COUNT], [17, U, 10, U], [6, 9, 0, U]
    want = FC.windows(part, order, 0, ops, pre, fol, [col] * 4)
    want[2] = FC.sums(part, order, 0, col, 10, 0)
    sizes = np.bincount(part.astype(np.int64), minlength=n // 100)
    want[3] = sizes[part.astype(np.int64)].astype(np.uint64)
    tab = Table(eng, part, order, [col])
    call(eng, T, tab, 0, ops, pre, fol, ["col0", "col0", "col0", None], expect=(want, int((sizes > 0).sum())))
    tab.close()
