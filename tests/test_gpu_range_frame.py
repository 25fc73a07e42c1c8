"""GPU suite: the RANGE frame entry (rhj_frame_range_cols_dev, Engine.frame_range_columns) against the oracles of
tests/frame_range_cases.py.  Every comparison is exact, aligned with the input rows.  Every output lies between guard words, the
inputs are compared before and after, every case runs twice and the two runs are compared bit for bit, and "last.frame_range_*" and
the zeroed "last.*" of the other entries are asserted after each call.

The naive oracle answers every case but the large one, which goes against the searchsorted oracle.  Which of the five answers of a
two-sided minimum / maximum a case takes is counted from the oracle's positions (frame_range_cases.paths) and asserted."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import frame_cases as FC
import frame_range_cases as RC
from radixhashjoin_amd import Engine, RhjError
from radixhashjoin_amd.binding import RHJ_E_INVALID

pytestmark = pytest.mark.gpu

GUARD, NGUARD = FC.GUARD, FC.NGUARD
U = RC.UNBOUNDED
BIG = 3_000_000
ZEROED = ("sort_bits", "sort_passes", "sort_units", "topk_bits", "topk_passes", "topk_candidates", "topk_sorted_rows", "window_units",
          "window_sorts", "window_partitions", "asof_units", "asof_sorts", "asof_matched", "frame_units", "frame_sorts", "frame_scans",
          "frame_partitions")
OURS = ("frame_range_units", "frame_range_sorts", "frame_range_partitions", "frame_range_scans", "frame_range_levels")


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


def check_info(eng, n, T, sorts, partitions, scans, levels, max_units=2048):
    got = {name: eng.info("last." + name) for name in OURS + ("join_kernel",) + ZEROED}
    assert got["join_kernel"] == -1
    assert all(got[name] == 0 for name in ZEROED), got
    assert got["frame_range_units"] == units_of(n, T, max_units), got
    assert got["frame_range_sorts"] == (sorts if n else 0) and got["frame_range_partitions"] == partitions, got
    assert got["frame_range_scans"] == (scans if n else 0) and got["frame_range_levels"] == (levels if n else 0), got


class Table:
    """the input columns of a case in HBM, between guard words; read back and compared when the case is closed"""
    def __init__(self, eng, part, order, cols):
        self.eng = eng
        self.host = {"part": part, "order": order, **{f"col{j}": c for j, c in enumerate(cols)}}
        self.n = len(order)
        self.dev = {k: Array(eng, self.n, off=1 + i, data=a) for i, (k, a) in enumerate(self.host.items()) if a is not None}

    def ptr(self, name):
        return self.dev[name].ptr if name in self.dev else None

    def close(self):
        for k, a in self.dev.items():
            assert np.array_equal(a.read(), self.host[k]), f"the input column {k} was modified"
            a.free()


def call(eng, T, tab, flags, ops, pre, fol, which, max_units=2048, expect=None):
    """one rhj_frame_range_cols_dev call on the table's columns, run twice (which[j]: the value column of op j, or None; pre / fol: one
    distance per op, or None for the entry's default) against the naive oracle (expect: the answer, where a test has it from
    elsewhere)"""
    n = tab.n
    part, order = tab.host["part"], tab.host["order"]
    cols = [tab.host[w] if w else None for w in which]
    want, partitions = expect if expect is not None else RC.brute(part, order, flags, ops, pre, fol, cols)
    outs = [Array(eng, n, off=3 + j) for j in range(len(ops))]
    runs = []
    for _ in range(2):
        got = eng.frame_range_cols_dev(tab.ptr("part"), tab.ptr("order"), n, flags, ops, pre, fol, [tab.ptr(w) if w else None for w in which],
                                       [o.ptr for o in outs])
        assert got == partitions
        check_info(eng, n, T, 1 + (part is not None), partitions, RC.value_scans(ops, pre, fol), RC.levels(n, ops, pre, fol), max_units)
        runs.append([o.read().copy() for o in outs])
    for j, op in enumerate(ops):
        bad = np.nonzero(runs[0][j] != want[j])[0]
        assert len(bad) == 0, (f"op {op} (#{j}), frame ({pre[j] if pre else None}, {fol[j] if fol else None}), flags {flags}, n {n}: "
                               f"{len(bad)} rows differ, first at row {bad[:5].tolist()}: {runs[0][j][bad[:5]].tolist()} for "
                               f"{want[j][bad[:5]].tolist()}")
        assert np.array_equal(runs[0][j], runs[1][j]), "two runs differ"
    for o in outs:
        o.free()
    return runs[0]


def taken(tab, flags, ops, pre, fol):
    """the answers the two-sided minimum / maximum ops of a call take, counted from the oracle's positions"""
    total = {}
    for j, op in enumerate(ops):
        if op not in RC.EXTREMES or U in (pre[j], fol[j]):
            continue
        _, ps, pe, lo, hi = RC.positions(tab.host["part"], tab.host["order"], flags, pre[j], fol[j])
        for k, c in RC.paths(ps, pe, lo, hi).items():
            total[k] = total.get(k, 0) + c
    return total


ROWS4 = (RC.COUNT, RC.SUM, RC.FIRST_ROW, RC.LAST_ROW)
KINDS = ("near", "sixteen", "distinct", "extremes", "equal")
# distances that cut the data: a few rows of a "near" column, half and quarter ranges of full 64-bit words
NEAR = ([(2, 3), (10, 0), (0, 0), (U, 7)], [(5, 5), (70, 0), (0, U), (200, 300)])
WIDE = ([(1 << 62, 1 << 61), (1 << 63, 0), (0, (1 << 64) - 2), (U, 1)], [(1 << 63, 1 << 63), (0, 0), ((1 << 64) - 2, 5), (1 << 60, U)])


def row_counts(T):
    return {"1": 1, "2": 2, "63": 63, "64": 64, "65": 65, "127": 127, "128": 128, "129": 129, "T-1": T - 1, "T": T, "T+1": T + 1,
            "3T+17": 3 * T + 17}


def make_part(shape, n, rng):
    if shape == "none":
        return None
    if shape == "one":
        return np.full(n, 1 << 63, dtype=np.uint64)
    if shape == "1..70":
        return FC.dense_part(FC.sizes_1_to(70, n), rng)
    raise ValueError(shape)


@pytest.mark.parametrize("shape", ["none", "one", "1..70"])
@pytest.mark.parametrize("size", ["1", "2", "63", "64", "65", "127", "128", "129", "T-1", "T", "T+1", "3T+17"])
def test_every_op_at_every_row_count_and_partition_shape(eng, T, size, shape):
    """four ops with four different frames in one call, then the same column under the four extremes with four more; the order
    column's kind and the view go round with the case"""
    n = row_counts(T)[size]
    i = list(row_counts(T)).index(size) + ["none", "one", "1..70"].index(shape)
    rng = np.random.default_rng(200 + i)
    kind, flags = KINDS[i % 5], RC.FLAGS[i % 4]
    tab = Table(eng, make_part(shape, n, rng), RC.make_order(kind, n), [FC.make_values(("full64", "extremes", "mixed")[i % 3], n)])
    first, second = NEAR if kind == "near" else WIDE
    call(eng, T, tab, flags, ROWS4, [a for a, _ in first], [b for _, b in first], [None, "col0", None, None])
    call(eng, T, tab, flags, RC.EXTREMES, [a for a, _ in second], [b for _, b in second], ["col0"] * 4)
    tab.close()


@pytest.mark.parametrize("kind", ["distinct", "sixteen", "equal", "extremes"])
@pytest.mark.parametrize("flags", RC.FLAGS)
def test_order_columns_in_all_four_views(eng, T, kind, flags):
    """peer runs of sixteen values cross block, tile and unit boundaries; all-equal keys make every frame the whole partition at
    distance 0; the extreme words saturate both ends in every view"""
    n = 2 * T + 77
    rng = np.random.default_rng(7)
    parted = Table(eng, FC.dense_part([n // 2 - 5, 3, n - n // 2 + 2], rng), RC.make_order(kind, n), [FC.make_values("mixed", n, seed=2)])
    call(eng, T, parted, flags, (RC.SUM, RC.MIN_I64, RC.FIRST_ROW, RC.COUNT), [0, 1, 1 << 63, (1 << 64) - 2], [0, 5, 1, 0],
         ["col0", "col0", None, None])
    parted.close()
    one = Table(eng, None, RC.make_order(kind, n, seed=1), [FC.make_values("extremes", n)])
    call(eng, T, one, flags, (RC.MAX_U64, RC.MIN_U64, RC.LAST_ROW, RC.SUM), [0, (1 << 64) - 2, 5, 1], [0, 1 << 63, (1 << 64) - 2, 1 << 63],
         ["col0", "col0", None, "col0"])
    call(eng, T, one, flags, (RC.SUM, RC.MAX_I64), None, None, ["col0", "col0"])          # NULL distances: SQL's default frame
    one.close()


def interior_counts(n):
    """1, 2, 3, 2^l and 2^l + 1 whole blocks between a frame's ends, for every level l the table has at n rows"""
    top = (n - 1) // 64 - 1
    out = {c for c in (1, 2, 3) if c <= top}
    for l in range(top.bit_length()):
        out.update(c for c in (1 << l, (1 << l) + 1) if c <= top)
    return sorted(out)


@pytest.mark.parametrize("group", range(4))
@pytest.mark.parametrize("size", ["T+1", "3T+17"])
def test_each_answer_of_the_minimum_and_maximum_is_taken(eng, T, size, group):
    """one partition whose order column is a permutation of 0 .. n - 1, so a frame (a, b) is the positions [p - a, p + b]: a frame of 64
    (c + 1) positions holds c whole blocks between its ends from every position but one in 64.  Group 0 takes the four short answers,
    the other groups share the table ranges of every level"""
    n = row_counts(T)[size]
    rng = np.random.default_rng(11 + group)
    tab = Table(eng, None, rng.permutation(n).astype(np.uint64), [FC.make_values("mixed", n, seed=group)])
    counts = interior_counts(n)
    assert RC.levels(n, [RC.MIN_U64], [1], [1]) == ((n - 1) // 64 - 1).bit_length() >= 6 and len(counts) >= 11
    if group == 0:
        frames, need = [(2, 3), (20, 10), (0, 0), (63, 0)], {"start", "end", "walk", "neighbours"}
    else:
        mine = counts[group - 1::3]
        frames = [(64 * (c + 1) // 3, 64 * (c + 1) - 1 - 64 * (c + 1) // 3) for c in mine]
        need = {("table", c) for c in mine}
    frames = (frames + frames[:4])[:max(4, len(frames))]
    for at in range(0, len(frames), 4):
        four = (frames[at:at + 4] + frames[:4])[:4]
        pre, fol = [a for a, _ in four], [b for _, b in four]
        seen = taken(tab, 0, RC.EXTREMES, pre, fol)
        call(eng, T, tab, 0, RC.EXTREMES, pre, fol, ["col0"] * 4)
        need -= {k for k, c in seen.items() if c > 0}
    assert not need, f"no frame of the case takes {need}"
    tab.close()


def test_every_table_range_is_covered_by_the_groups(T):
    """the three table groups of the test above share out every count of interior_counts"""
    for n in (T + 1, 3 * T + 17):
        counts = interior_counts(n)
        assert sorted(c for g in (1, 2, 3) for c in counts[g - 1::3]) == counts
        top = (n - 1) // 64 - 1
        assert all(c in counts for l in range(top.bit_length()) for c in (1 << l, (1 << l) + 1) if c <= top) and {1, 2, 3} <= set(counts)


@pytest.mark.parametrize("marks", ["64", "T"])
def test_partition_heads_exactly_on_one_before_and_one_after_the_cuts(eng, T, marks):
    n = 3 * T + 17
    heads = FC.heads_around(n, (T,)) if marks == "T" else FC.heads_around(n, (64,))
    part = FC.dense_part(FC.sizes_with_heads_at(n, heads))
    tab = Table(eng, part, RC.make_order("near", n), [FC.make_values("mixed", n, seed=3)])
    pre, fol = [40, 700, 1, 0], [50, 600, 1, 1]
    seen = taken(tab, 0, (RC.MIN_U64, RC.MAX_I64), pre, fol)
    assert all(seen.get(k, 0) > 0 for k in ("start", "end") + (("walk", "neighbours", ("table", 1)) if marks == "T" else ())), seen
    call(eng, T, tab, 0, (RC.MIN_U64, RC.MAX_I64, RC.SUM, RC.COUNT), pre, fol, ["col0", "col0", "col0", None])
    call(eng, T, tab, RC.SORT_DESC, (RC.MAX_U64, RC.MIN_I64, RC.FIRST_ROW, RC.LAST_ROW), [0, 3 * T, 64, 2], [1, 2 * T, 0, 3], ["col0", "col0", None, None])
    tab.close()


@pytest.mark.parametrize("max_units", [1, 3])
def test_the_carry_crosses_tiles_inside_a_unit_and_units(eng, T, max_units):
    n = 7 * T - 3
    unit = -(-7 // max_units) * T
    rng = np.random.default_rng(31 + max_units)
    heads = FC.heads_around(n, (T, unit)) | FC.heads_around(min(n, 8 * 64), (64,))
    part = FC.dense_part(FC.sizes_with_heads_at(n, heads), rng)
    tab = Table(eng, part, RC.make_order("near", n), [FC.make_values("mixed", n, seed=max_units)])
    one = Table(eng, None, RC.make_order("near", n, seed=5), [FC.make_values("full64", n, seed=max_units)])
    with option(eng, "sort.max_units", max_units):
        assert units_of(n, T, max_units) == max_units
        call(eng, T, tab, RC.SORT_I64, (RC.MIN_I64, RC.MAX_U64, RC.SUM, RC.LAST_ROW), [2, 3 * T, U, 5], [3, 0, 5, U], ["col0", "col0", "col0", None],
             max_units)
        call(eng, T, one, RC.SORT_DESC, (RC.MIN_U64, RC.MAX_I64, RC.SUM, RC.COUNT), [6 * T + 1, 63, T - 1, U], [3 * T, 0, 1, U], ["col0"] * 3 + [None],
             max_units)
    tab.close()
    one.close()


def test_four_ops_four_frames_and_one_column_twice(eng, T):
    """every op of the call has a frame of its own; two ops share one value column and one frame, two more the column only"""
    n = T + 300
    rng = np.random.default_rng(3)
    col = FC.make_values("full64", n)
    tab = Table(eng, FC.dense_part(FC.sizes_1_to(70, n), rng), RC.make_order("near", n), [col, FC.make_values("mixed", n, seed=1)])
    got = call(eng, T, tab, RC.SORT_I64, (RC.SUM, RC.SUM, RC.MIN_I64, RC.MAX_I64), [7, 7, 0, 30], [0, 0, 9, 30], ["col0", "col0", "col0", "col0"])
    assert np.array_equal(got[0], got[1])
    call(eng, T, tab, 0, (RC.SUM, RC.MAX_U64, RC.MIN_U64, RC.SUM), [1, 20, 3, U], [1, 0, 40, U], ["col0", "col1", "col0", "col1"])
    tab.close()


@pytest.mark.parametrize("flags", [0, RC.SORT_I64 | RC.SORT_DESC])
def test_distinct_ranks_give_the_rows_frames_of_the_frame_entry(eng, T, flags):
    """the order column is each row's 0-based rank inside its partition: no peers, so RANGE (a, b) is ROWS (a, b), and the two
    entries' outputs are compared on the device's own results"""
    n = 2 * T + 9
    rng = np.random.default_rng(17)
    part = FC.dense_part(FC.sizes_1_to(130, n // 2) + [n - n // 2], rng)
    order = RC.rank_order(part, n, rng)
    tab = Table(eng, part, order, [FC.make_values("mixed", n, seed=4)])
    rows = [Array(eng, n, off=2 + j) for j in range(4)]
    rng_ = [Array(eng, n, off=5 + j) for j in range(4)]
    for ops in ((RC.COUNT, RC.SUM, RC.FIRST_ROW, RC.LAST_ROW), RC.EXTREMES):
        cols = [tab.ptr("col0")] * 4
        for pre, fol in ((0, 0), (1, 0), (2, 3), (63, 64), (200, 70), (U, 0), (0, U), (U, U), (U, 5), (300, U)):
            a = eng.frame_cols_dev(tab.ptr("part"), tab.ptr("order"), n, flags, ops, [pre] * 4, [fol] * 4, cols, [o.ptr for o in rows])
            b = eng.frame_range_cols_dev(tab.ptr("part"), tab.ptr("order"), n, flags, ops, [pre] * 4, [fol] * 4, cols, [o.ptr for o in rng_])
            assert a == b
            for j in range(4):
                assert np.array_equal(rows[j].read(), rng_[j].read()), (ops[j], pre, fol)
    for o in rows + rng_:
        o.free()
    tab.close()


def test_more_units_than_cus(eng, T):
    """3 x 10^6 rows in about n / 100 Zipf partitions, int64 order values in a range of 2^40, against the searchsorted oracle"""
    n = BIG
    assert units_of(n, T) > 512
    rng = np.random.default_rng(43)
    ids = n // 100
    weight = 1.0 / np.arange(1, ids + 1) ** 0.9
    part = rng.choice(ids, n, p=weight / weight.sum()).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    order = rng.integers(-(1 << 39), 1 << 39, n).view(np.uint64)
    col = FC.make_values("mixed", n)
    d = (1 << 40) // 300
    ops, pre, fol = [RC.SUM, RC.COUNT, RC.MAX_I64, RC.FIRST_ROW], [d, d, d // 2, d // 2], [0, 0, d // 2, d // 2]
    want = RC.fast(part, order, RC.SORT_I64, ops, pre, fol, [col] * 4)
    assert int(want[0][1].max()) > 3 * 64                                   # the largest partitions' frames span whole blocks
    tab = Table(eng, part, order, [col])
    call(eng, T, tab, RC.SORT_I64, ops, pre, fol, ["col0", None, "col0", None], expect=want)
    tab.close()


def test_invalid_arguments_and_no_rows(eng, T):
    n = 100
    tab = Table(eng, np.zeros(n, dtype=np.uint64), np.arange(n, dtype=np.uint64), [np.arange(n, dtype=np.uint64)])
    out = Array(eng, n)
    P, O, X = tab.ptr("part"), tab.ptr("order"), tab.ptr("col0")
    me = "rhj_frame_range_cols_dev: "

    def refused(message, *args):
        with pytest.raises(RhjError) as err:
            eng.frame_range_cols_dev(*args)
        assert err.value.code == RHJ_E_INVALID and me + message in str(err.value), str(err.value)

    refused("unknown flags", P, O, n, 4, [RC.COUNT], None, None, None, [out.ptr])
    refused("unknown flags", P, O, 0, 1 << 31, [RC.COUNT], None, None, None, [out.ptr])
    refused("d_order is null", P, None, n, 0, [RC.COUNT], None, None, None, [out.ptr])
    refused("d_order is null", None, None, n, 0, [RC.SUM], [1], [1], [X], [out.ptr])
    refused("d_order is null", P, None, 0, RC.SORT_DESC, [RC.COUNT], None, None, None, [out.ptr])
    refused("nops must be 1 .. RHJ_FRAME_MAX_OPS", P, O, n, 0, [], None, None, None, [])
    refused("nops must be 1 .. RHJ_FRAME_MAX_OPS", P, O, n, 0, [RC.COUNT] * 5, None, None, None, [out.ptr] * 5)
    parts = C.c_uint64(77)
    for message, ops, outs in (("ops is null", None, (C.c_void_p * 1)(out.ptr)), ("d_outs is null", (C.c_uint32 * 1)(RC.COUNT), None)):
        rc = eng.lib.rhj_frame_range_cols_dev(eng.ctx, P, O, n, 0, ops, None, None, None, 1, outs, C.byref(parts))     # (the binding would say nops 0)
        assert rc == RHJ_E_INVALID
        with pytest.raises(RhjError, match=me + message):
            eng._chk(rc)
    refused("d_outs[1] is null", P, O, n, 0, [RC.COUNT, RC.COUNT], None, None, None, [out.ptr, None])
    refused("ops[1] is not an RHJ_FRAME_* op", P, O, n, 0, [RC.COUNT, RC.LAST_ROW + 1], None, None, None, [out.ptr] * 2)
    for op in (RC.SUM,) + RC.EXTREMES:
        refused("d_cols[1] is null for a column op", P, O, n, 0, [RC.COUNT, op], None, None, [None, None], [out.ptr] * 2)
        refused("d_cols[0] is null for a column op", P, O, n, 0, [op], None, None, None, [out.ptr])
    assert (out.read() == GUARD).all()                                   # nothing was launched
    # no rows: RHJ_OK, no launch, 0 partitions -- also without an order column, and for a column op without a column
    assert eng.frame_range_cols_dev(None, None, 0, 0, [RC.SUM], None, None, None, [out.ptr]) == 0
    check_info(eng, 0, T, 0, 0, 0, 0)
    assert (out.read() == GUARD).all()
    # the context is usable afterwards; out_partitions may be NULL; the default frame over distinct keys is the running sum
    x = tab.host["col0"]
    col, one = (C.c_void_p * 1)(X), (C.c_void_p * 1)(out.ptr)
    assert eng.lib.rhj_frame_range_cols_dev(eng.ctx, P, O, n, 0, (C.c_uint32 * 1)(RC.SUM), None, None, col, 1, one, None) == 0
    assert np.array_equal(out.read(), np.cumsum(x, dtype=np.uint64))
    check_info(eng, n, T, 2, 1, 1, 0)
    # ... and every other entry zeroes the five names
    eng.frame_cols_dev(P, O, n, 0, [RC.COUNT], None, None, None, [out.ptr])
    assert [eng.info("last." + name) for name in OURS] == [0] * 5 and eng.info("last.frame_units") == 1
    out.free()
    tab.close()


def test_torch_entry(eng, T):
    n = T + 300
    rng = np.random.default_rng(23)
    a, b = rng.integers(0, 7, n), rng.integers(-3, 4, n)
    order = rng.integers(-500, 500, n)
    x = FC.make_values("mixed", n).view(np.int64)
    dev = lambda h: torch.from_numpy(np.ascontiguousarray(h)).to("cuda")
    pair = (a * 16 + (b + 3)).astype(np.uint64)                             # equal exactly where both columns are
    ops = [RC.SUM, RC.MIN_I64, RC.MAX_I64, RC.LAST_ROW]
    want, _ = RC.brute(pair, order.view(np.uint64), RC.SORT_I64 | RC.SORT_DESC, ops, [40, 20, U, 0], [0, 20, 0, 10], [x.view(np.uint64)] * 3 + [None])
    got = eng.frame_range_columns([dev(a), dev(b)], dev(order), [dev(x)] * 3 + [None], ["sum", "min", "max", "last_row"], [40, 20, None, 0],
                                  [0, 20, 0, 10], descending=True)
    assert [g.dtype for g in got] == [torch.int64] * 4
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy().view(np.uint64), w)
    check_info(eng, n, T, 2, len(np.unique(pair)), 4, RC.levels(n, ops, [40, 20, U, 0], [0, 20, 0, 10]))
    want, _ = RC.brute(a.astype(np.uint64), order.view(np.uint64), 0, [RC.MIN_U64, RC.COUNT, RC.FIRST_ROW], [U, U, 3], [0, U, 0],
                       [x.view(np.uint64), None, None])
    got = eng.frame_range_columns(dev(a), dev(order), [dev(x), None, None], ["min", "count", "first_row"], [None, None, 3], [0, None, 0], unsigned=True)
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy().view(np.uint64), w)
    got = eng.frame_range_columns(None, dev(order), [dev(x)], ["sum"])      # the defaults: SQL's default frame, peers share a value
    want, _ = RC.brute(None, order.view(np.uint64), RC.SORT_I64, [RC.SUM], None, None, [x.view(np.uint64)])
    assert np.array_equal(got[0].cpu().numpy().view(np.uint64), want[0])
    with pytest.raises(ValueError, match=r"^cols\[0\]: 5 elements, order has "):
        eng.frame_range_columns(None, dev(order), [dev(x[:5])], ["sum"])
    empty = torch.empty(0, dtype=torch.int64, device="cuda")
    assert [t.numel() for t in eng.frame_range_columns(empty, empty, [empty], ["sum"])] == [0]
