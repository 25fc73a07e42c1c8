"""GPU suite: the window entry (rhj_window_cols_dev, Engine.window_columns / topk_per_group_columns) against the numpy oracle of
tests/window_cases.py.  Every comparison is exact: ranks, rows and running aggregates bit for bit, aligned with the input rows.
Every output lies between guard words, the inputs are compared before and after, and "last.window_*" are asserted after each call.

Under the automatic "sort.max_units" every input below 2048 tiles is cut into units of one tile; the carry across the tiles of a unit
runs under "sort.max_units" 1 and 3, and the large case has more units than the device has CUs."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import window_cases as WC
from radixhashjoin_amd import Engine, RhjError
from radixhashjoin_amd.binding import RHJ_E_INVALID

pytestmark = pytest.mark.gpu

GUARD, NGUARD = WC.GUARD, WC.NGUARD
BIG = 3_000_000
RANKS = (WC.ROW_NUMBER, WC.RANK, WC.DENSE_RANK, WC.CUMSUM)
EXTREMES = (WC.CUMMIN_U64, WC.CUMMAX_U64, WC.CUMMIN_I64, WC.CUMMAX_I64)      # the same column under four ops in one call
SHIFTS = (WC.LAG_ROW, WC.LEAD_ROW, WC.LAG_ROW, WC.LEAD_ROW)


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


def check_info(eng, n, T, sorts, partitions, max_units=2048):
    got = {name: eng.info("last." + name) for name in ("window_units", "window_sorts", "window_partitions", "join_kernel", "sort_bits",
                                                       "sort_passes", "sort_units", "topk_bits", "topk_passes", "topk_candidates",
                                                       "topk_sorted_rows")}
    assert got["join_kernel"] == -1
    assert got["sort_bits"] == got["sort_passes"] == got["sort_units"] == 0, got
    assert got["topk_bits"] == got["topk_passes"] == got["topk_candidates"] == got["topk_sorted_rows"] == 0, got
    assert got["window_units"] == units_of(n, T, max_units), got
    assert got["window_sorts"] == (sorts if n else 0) and got["window_partitions"] == partitions, got


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


def call(eng, T, tab, flags, ops, args, which, max_units=2048, twice=False, expect=None):
    """one rhj_window_cols_dev call on the table's columns (which[j]: the value column of op j, or None) against the oracle
    (expect: its answer for exactly these ops, where a test computed it for several calls at once)"""
    n = tab.n
    part, order = tab.host["part"], tab.host["order"]
    cols = [tab.host[w] if w else None for w in which]
    want, partitions = expect if expect is not None else WC.oracle(part, order, flags, ops, args, cols, n)
    outs = [Array(eng, n, off=3 + j) for j in range(len(ops))]
    runs = []
    for _ in range(2 if twice else 1):
        got = eng.window_cols_dev(tab.ptr("part"), tab.ptr("order"), n, flags, ops, args, [tab.ptr(w) if w else None for w in which],
                                  [o.ptr for o in outs])
        assert got == partitions
        check_info(eng, n, T, (part is not None) + (order is not None), partitions, max_units)
        runs.append([o.read().copy() for o in outs])
    for j, op in enumerate(ops):
        bad = np.nonzero(runs[0][j] != want[j])[0]
        assert len(bad) == 0, (f"op {op} (#{j}), flags {flags}, n {n}: {len(bad)} rows differ, first at row {bad[:5].tolist()}: "
                               f"{runs[0][j][bad[:5]].tolist()} for {want[j][bad[:5]].tolist()}")
        if twice:
            assert np.array_equal(runs[0][j], runs[1][j]), "two runs differ"
    for o in outs:
        o.free()


def three_calls(eng, T, tab, flags, offsets=(1, 1, 2, 3), max_units=2048):
    """every op: the ranks and the sum; the four extremes of one column; lag and lead under two offsets"""
    call(eng, T, tab, flags, RANKS, None, [None, None, None, "col0"], max_units)
    call(eng, T, tab, flags, EXTREMES, None, ["col0"] * 4, max_units)
    call(eng, T, tab, flags, SHIFTS, list(offsets), [None] * 4, max_units)


def small_sizes(T):
    return {"0": 0, "1": 1, "63": 63, "64": 64, "65": 65, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1}


@pytest.mark.parametrize("shape", WC.SHAPES)
@pytest.mark.parametrize("size", ["0", "1", "63", "64", "65", "T-1", "T", "T+1", "2T+1"])
def test_every_op_at_every_small_size_and_partition_shape(eng, T, size, shape):
    n = small_sizes(T)[size]
    i = WC.SHAPES.index(shape) + list(small_sizes(T)).index(size)             # orders, views and values rotate over the grid
    kind = WC.ORDERS[i % len(WC.ORDERS)]
    flags = WC.FLAGS[i % 4] if kind != "none" else 0
    tab = Table(eng, WC.make_part(shape, n, T), WC.make_order(kind, n), [WC.make_values(WC.VALUES[i % len(WC.VALUES)], n)])
    three_calls(eng, T, tab, flags)
    tab.close()


@pytest.mark.parametrize("kind", WC.ORDERS)
@pytest.mark.parametrize("shape", ["runsT-1", "zipf", None])
def test_order_columns_under_all_four_flag_combinations(eng, T, shape, kind):
    """constant: rank and dense rank are all 1; sixteen: peer runs crossing tiles; the extremes of both views in both directions; no
    partition column: one sort, the order column's own"""
    n = 2 * T + 1
    part = WC.make_part(shape, n, T) if shape else None
    order = WC.make_order(kind, n)
    tab = Table(eng, part, order, [WC.make_values("full64", n)])
    for flags in (WC.FLAGS if order is not None else (0,)):
        call(eng, T, tab, flags, RANKS, None, [None, None, None, "col0"])
        call(eng, T, tab, flags, SHIFTS, [1, 1, 5, 64], [None] * 4)
    if kind == "constant":
        outs, _ = WC.oracle(part, order, 0, [WC.RANK, WC.DENSE_RANK])
        assert (outs[0] == 1).all() and (outs[1] == 1).all()
    tab.close()


@pytest.mark.parametrize("values", WC.VALUES)
@pytest.mark.parametrize("shape", ["one", "runsT+1", "geometric"])
def test_value_columns(eng, T, shape, values):
    """full-range words: the sum wraps; the extremes under the four minimum / maximum ops; a constant; one column under two ops, two
    columns in one call"""
    n = 2 * T + 1
    tab = Table(eng, WC.make_part(shape, n, T), WC.make_order("sixteen", n), [WC.make_values(values, n), WC.make_values("extremes", n, seed=5)])
    for flags in (WC.SORT_I64, WC.SORT_DESC):
        call(eng, T, tab, flags, EXTREMES, None, ["col0"] * 4)
        call(eng, T, tab, flags, (WC.CUMSUM, WC.CUMSUM, WC.CUMMAX_I64, WC.CUMMIN_U64), None, ["col0", "col1", "col1", "col0"])
    tab.close()


@pytest.mark.parametrize("shape", ["one", "runs64", "runsT+1", "geometric", "each"])
def test_lag_and_lead_offsets(eng, T, shape):
    """1, 63, 64, T, and one larger than every partition"""
    n = 2 * T + 1
    tab = Table(eng, WC.make_part(shape, n, T), WC.make_order("distinct", n), [])
    call(eng, T, tab, WC.SORT_I64, SHIFTS, [1, 1, 63, 63], [None] * 4)
    call(eng, T, tab, WC.SORT_I64, SHIFTS, [64, 64, T, T], [None] * 4)
    call(eng, T, tab, 0, SHIFTS, [n, n, 1 << 40, (1 << 64) - 1], [None] * 4)
    call(eng, T, tab, 0, (WC.LAG_ROW, WC.LEAD_ROW), None, [None] * 2)            # args NULL: offset 1
    tab.close()


@pytest.mark.parametrize("max_units", [1, 3])
@pytest.mark.parametrize("shape,kind", [("one", "sixteen"), ("runsT-1", "distinct"), ("zipf", "sixteen"), ("each", "none"), ("edges", "extremes")])
def test_several_tiles_per_unit(eng, T, shape, kind, max_units):
    """70,000 rows under "sort.max_units" 1 -- one workgroup walks every tile -- and 3 -- several units of several tiles"""
    n = 70_000
    assert units_of(n, T, max_units) == max_units and -(-n // T) > 2 * max_units
    tab = Table(eng, WC.make_part(shape, n, T), WC.make_order(kind, n), [WC.make_values("full64", n)])
    with option(eng, "sort.max_units", max_units):
        three_calls(eng, T, tab, WC.SORT_I64 if kind != "none" else 0, (1, 64, T, T + 1), max_units)
    tab.close()


@pytest.mark.parametrize("shape", ["one", "zipf"])
def test_three_million_rows(eng, T, shape):
    """more units than CUs; one partition -- the carry crosses every unit -- and a few thousand Zipf partitions"""
    n = BIG
    assert units_of(n, T) > 512
    tab = Table(eng, WC.make_part(shape, n, T, groups=3000), WC.make_order("sixteen", n), [WC.make_values("full64", n)])
    ops = (WC.ROW_NUMBER, WC.DENSE_RANK, WC.CUMSUM, WC.CUMMAX_I64, WC.RANK, WC.LAG_ROW, WC.LEAD_ROW)
    args, which = [1, 1, 1, 1, 1, 1, T], [None, None, "col0", "col0", None, None, None]
    want, partitions = WC.oracle(tab.host["part"], tab.host["order"], WC.SORT_I64, ops, args, [tab.host[w] if w else None for w in which])
    assert partitions == (1 if shape == "one" else 3000)                       # the oracle once, for both calls
    call(eng, T, tab, WC.SORT_I64, ops[:4], args[:4], which[:4], expect=(want[:4], partitions))
    call(eng, T, tab, WC.SORT_I64, ops[4:], args[4:], which[4:], expect=(want[4:], partitions))
    tab.close()


def test_two_runs_are_bit_identical(eng, T):
    n = 2 * T + 1
    tab = Table(eng, WC.make_part("zipf", n, T), WC.make_order("sixteen", n), [WC.make_values("full64", n)])
    call(eng, T, tab, WC.SORT_DESC, RANKS, None, [None, None, None, "col0"], twice=True)
    call(eng, T, tab, WC.SORT_DESC, SHIFTS, [1, 2, 3, 4], [None] * 4, twice=True)
    tab.close()


def test_release_workspace_and_call_again(eng, T):
    n = T + 1
    tab = Table(eng, WC.make_part("geometric", n, T), WC.make_order("distinct", n), [WC.make_values("full64", n)])
    three_calls(eng, T, tab, 0)
    eng.release_workspace()
    three_calls(eng, T, tab, WC.SORT_I64)
    tab.close()


def test_other_calls_reset_the_window_names(eng, T):
    n = 65
    tab = Table(eng, WC.make_part("runs64", n, T), None, [])
    call(eng, T, tab, 0, (WC.ROW_NUMBER,), None, [None])
    assert eng.info("last.window_units") == 1 and eng.info("last.window_sorts") == 1 and eng.info("last.window_partitions") == 2
    out = Array(eng, n)
    eng.sort_cols_dev(tab.ptr("part"), None, n, 0, None, out.ptr)
    assert eng.info("last.window_units") == eng.info("last.window_sorts") == eng.info("last.window_partitions") == 0
    out.free()
    tab.close()


def test_invalid_arguments_are_refused_before_any_launch(eng, T):
    n = 65
    tab = Table(eng, WC.make_part("runs64", n, T), WC.make_order("sixteen", n), [WC.make_values("full64", n)])
    outs = [Array(eng, n, off=2), Array(eng, n, off=5)]
    p, o, c = tab.ptr("part"), tab.ptr("order"), tab.ptr("col0")
    u32s, u64s, ptrs = (lambda *x: (C.c_uint32 * len(x))(*x)), (lambda *x: (C.c_uint64 * len(x))(*x)), (lambda *x: (C.c_void_p * len(x))(*x))
    two = ptrs(outs[0].ptr, outs[1].ptr)
    parts = C.c_uint64(77)
    # (d_part, d_order, n, flags, ops, args, d_cols, nops, d_outs): the word the message must hold
    bad = [((p, o, n, 4, u32s(0, 1), None, None, 2, two), "flags"),
           ((p, o, n, 0x80000000, u32s(0, 1), None, None, 2, two), "flags"),
           ((p, o, 0, 8, u32s(0, 1), None, None, 2, two), "flags"),                   # ... also with no rows
           ((p, None, n, WC.SORT_DESC, u32s(0, 1), None, None, 2, two), "d_order"),
           ((p, None, n, WC.SORT_I64, u32s(0, 1), None, None, 2, two), "d_order"),
           ((p, o, n, 0, u32s(0, 1), None, None, 0, two), "nops"),
           ((p, o, n, 0, u32s(0, 1, 2, 0, 1), None, None, 5, ptrs(*[outs[0].ptr] * 5)), "nops"),
           ((p, o, n, 0, u32s(0, 10), None, None, 2, two), r"ops\[1\]"),
           ((p, o, n, 0, u32s(0xFFFFFFFF, 1), None, None, 2, two), r"ops\[0\]"),
           ((p, o, n, 0, u32s(WC.LAG_ROW, WC.LEAD_ROW), u64s(1, 0), None, 2, two), r"args\[1\]"),
           ((p, o, n, 0, u32s(WC.LAG_ROW, 0), u64s(0, 0), None, 2, two), r"args\[0\]"),
           ((p, o, n, 0, None, None, None, 2, two), "ops"),
           ((p, o, n, 0, u32s(0, 1), None, None, 2, None), "d_outs"),
           ((p, o, n, 0, u32s(0, 1), None, None, 2, ptrs(outs[0].ptr, None)), r"d_outs\[1\]"),
           ((p, o, n, 0, u32s(0, WC.CUMSUM), None, ptrs(None, None), 2, two), r"d_cols\[1\]"),
           ((p, o, n, 0, u32s(WC.CUMMAX_I64, WC.CUMSUM), None, None, 2, two), r"d_cols\[0\]"),
           ((p, o, n, 0, u32s(WC.CUMMAX_I64, WC.CUMSUM), None, ptrs(c, None), 2, two), r"d_cols\[1\]")]
    for args, word in bad:
        rc = eng.lib.rhj_window_cols_dev(eng.ctx, *args, C.byref(parts))
        assert rc == RHJ_E_INVALID, (rc, word)
        with pytest.raises(RhjError, match=r"rhj_window_cols_dev: .*" + word) as err:
            eng._chk(rc)
        assert err.value.code == RHJ_E_INVALID
    assert (outs[0].read() == GUARD).all() and (outs[1].read() == GUARD).all()          # nothing was launched
    # a column op with no rows needs no column; a row op's args are ignored for the other ops
    assert eng.lib.rhj_window_cols_dev(eng.ctx, p, o, 0, 0, u32s(WC.CUMSUM, 0), None, None, 2, two, C.byref(parts)) == 0 and parts.value == 0
    check_info(eng, 0, T, 0, 0)
    assert (outs[0].read() == GUARD).all() and (outs[1].read() == GUARD).all()
    assert eng.lib.rhj_window_cols_dev(eng.ctx, p, o, n, 0, u32s(WC.CUMSUM, WC.RANK), u64s(0, 0), ptrs(c, None), 2, two, None) == 0    # out_partitions NULL
    want, _ = WC.oracle(tab.host["part"], tab.host["order"], 0, [WC.CUMSUM, WC.RANK], None, [tab.host["col0"], None])
    assert np.array_equal(outs[0].read(), want[0]) and np.array_equal(outs[1].read(), want[1])
    for a in outs:
        a.free()
    tab.close()


def as_i64(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def test_window_columns_with_a_two_tensor_partition_and_a_lagged_payload(eng, T):
    n = 2 * T + 1
    rng = np.random.default_rng(3)
    a, b = rng.integers(-3, 4, n).astype(np.int64), rng.integers(0, 5, n).astype(np.int64) * (1 << 40)
    order = WC.make_order("sixteen", n)
    vals = WC.make_values("full64", n)
    part = (a.view(np.uint64) << np.uint64(3)) ^ (b.view(np.uint64) >> np.uint64(40))      # one word per distinct (a, b): the oracle's partitions
    assert len(np.unique(part)) == len(np.unique(np.stack([a, b]), axis=1).T)
    fill = -12345
    ta, tb, to, tv = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), as_i64(order), as_i64(vals)
    keep = [t.clone() for t in (ta, tb, to, tv)]
    got = eng.window_columns([ta, tb], to, [None, tv, tv, tv], ["rank", "cumsum", "lag", "lead"], descending=True, offsets=[1, 1, 2, 1], fill=fill)
    flags = WC.SORT_I64 | WC.SORT_DESC
    want, partitions = WC.oracle(part, order, flags, [WC.RANK, WC.CUMSUM, WC.LAG_ROW, WC.LEAD_ROW], [1, 1, 2, 1], [None, vals, None, None])
    assert [g.dtype for g in got] == [torch.int64] * 4 and [len(g) for g in got] == [n] * 4
    assert np.array_equal(got[0].cpu().numpy().view(np.uint64), want[0]) and np.array_equal(got[1].cpu().numpy().view(np.uint64), want[1])
    for g, rows in ((got[2], want[2]), (got[3], want[3])):
        there = rows != WC.NO_ROW
        exp = np.full(n, fill, dtype=np.int64)
        exp[there] = vals.view(np.int64)[rows[there].astype(np.int64)]
        assert (~there).any() and np.array_equal(g.cpu().numpy(), exp)
    # the row indices themselves, -1 at the ends; unsigned view; no partition
    rows, number = eng.window_columns(None, to, [None, None], ["lead", "row_number"], unsigned=True)
    want, _ = WC.oracle(None, order, 0, [WC.LEAD_ROW, WC.ROW_NUMBER])
    assert np.array_equal(rows.cpu().numpy(), want[0].view(np.int64)) and int(rows.min()) == -1
    assert np.array_equal(number.cpu().numpy().view(np.uint64), want[1])
    for t, k in zip((ta, tb, to, tv), keep):
        assert torch.equal(t, k)
    empty = torch.empty(0, dtype=torch.int64, device="cuda")
    assert [len(x) for x in eng.window_columns(empty, empty, [None, empty], ["rank", "cumsum"])] == [0, 0]


def test_topk_per_group_columns(eng, T):
    """k larger than a partition takes all of it; ties at the cut go to the rows earliest in the input"""
    n = 2 * T + 1
    part, order = WC.make_part("geometric", n, T), WC.make_order("sixteen", n)
    tp, to = as_i64(part), as_i64(order)
    sizes = np.unique(part, return_counts=True)[1]
    for k, desc in ((0, False), (1, False), (3, True), (100, False), (n + 5, True)):
        number, _ = WC.oracle(part, order, WC.SORT_I64 | (WC.SORT_DESC if desc else 0), [WC.ROW_NUMBER])
        want = np.nonzero(number[0] <= np.uint64(k))[0]
        got = eng.topk_per_group_columns(tp, to, k, descending=desc)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
        assert len(want) == int(np.minimum(sizes, k).sum())
    assert (sizes < 100).any() and (sizes > 100).any()
    # 16 order values over partitions of hundreds of rows: the cut at k = 100 falls inside runs of peers
    ranks, _ = WC.oracle(part, order, WC.SORT_I64, [WC.ROW_NUMBER, WC.RANK])
    cut = (ranks[0] == 100) & (ranks[1] < 100)
    assert cut.any()
