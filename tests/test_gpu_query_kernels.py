"""GPU suite: the query-layer kernels of the C-ABI (rhj_col_filter, rhj_gather_tuples, rhj_pairs_split,
rhj_gather_u64, rhj_rows_filter_equal, rhj_sum_gather) bit-exact against numpy restatements of the
reference loops they replace (Query.cpp:66-74,96-146; structs.cpp:217-243; intermediate.cpp:72-105)."""
import numpy as np
import pytest

from oracle.pyoracle import PAIR, TUPLE
from radixhashjoin_amd.binding import RHJ_E_INVALID, RhjError

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 100_003, 3_000_000])
def test_col_filter_and_chain(engine, n):
    rng = np.random.default_rng(n)
    col = rng.integers(0, 1000, n, dtype=np.uint64)
    dcol, drows, drows2 = engine.to_device(col), engine.alloc(8 * n), engine.alloc(8 * n)
    for op, val, f in (("<", 500, lambda v: v < 500), (">", 998, lambda v: v > 998), ("=", 7, lambda v: v == 7), (">", 5000, lambda v: v > 5000)):
        m = engine.col_filter(dcol, None, n, op, val, drows)
        exp = np.nonzero(f(col))[0].astype(np.uint64)
        assert m == len(exp)
        got = np.sort(drows.to_numpy(np.uint64, m))
        assert np.array_equal(got, exp)
        # a second filter applied to the surviving rows (several filters on one alias)
        m2 = engine.col_filter(dcol, drows, m, ">", 100, drows2)
        exp2 = exp[col[exp.astype(np.int64)] > 100]
        assert m2 == len(exp2) and np.array_equal(np.sort(drows2.to_numpy(np.uint64, m2)), exp2)


def test_gather_tuples_split_gather_sum(engine):
    rng = np.random.default_rng(3)
    nrows, n = 50_000, 333_333
    col = rng.integers(0, 1 << 64, nrows, dtype=np.uint64)
    rows = rng.integers(0, nrows, n, dtype=np.uint64)
    dcol, drows, dt = engine.to_device(col), engine.to_device(rows), engine.alloc(16 * n)
    for pos in (False, True):
        engine.gather_tuples(dcol, drows, n, pos, dt)
        t = dt.to_numpy(TUPLE, n)
        assert np.array_equal(t["payload"], col[rows.astype(np.int64)])
        assert np.array_equal(t["key"], np.arange(n, dtype=np.uint64) if pos else rows)
    pairs = np.empty(n, dtype=PAIR)
    pairs["keyR"], pairs["keyS"] = rng.integers(0, 1 << 64, n, dtype=np.uint64), rng.integers(0, 1 << 64, n, dtype=np.uint64)
    dp, dr, ds = engine.to_device(pairs), engine.alloc(8 * n), engine.alloc(8 * n)
    engine.pairs_split(dp, n, dr, ds)
    assert np.array_equal(dr.to_numpy(np.uint64, n), pairs["keyR"]) and np.array_equal(ds.to_numpy(np.uint64, n), pairs["keyS"])
    dd = engine.alloc(8 * n)
    engine.gather_u64(dcol, drows, n, dd)
    assert np.array_equal(dd.to_numpy(np.uint64, n), col[rows.astype(np.int64)])
    assert engine.sum_gather(dcol, drows, n) == int(col[rows.astype(np.int64)].sum(dtype=np.uint64))     # wraps mod 2^64
    assert engine.sum_gather(dcol, drows, 0) == 0


def test_rows_filter_equal(engine):
    rng = np.random.default_rng(4)
    n = 200_001
    colA, colB = rng.integers(0, 50, 1000, dtype=np.uint64), rng.integers(0, 50, 2000, dtype=np.uint64)
    rA, rB = rng.integers(0, 1000, n, dtype=np.uint64), rng.integers(0, 2000, n, dtype=np.uint64)
    d = [engine.to_device(x) for x in (colA, rA, colB, rB)]
    dpos = engine.alloc(8 * n)
    m = engine.rows_filter_equal(d[0], d[1], d[2], d[3], n, dpos)
    exp = np.nonzero(colA[rA.astype(np.int64)] == colB[rB.astype(np.int64)])[0].astype(np.uint64)
    assert m == len(exp) and np.array_equal(np.sort(dpos.to_numpy(np.uint64, m)), exp)


# ---- edges: more than one grid-stride trip, NULL row lists, the full 64-bit range, the return paths --------------------------
POISON = 0xA5A5A5A5A5A5A5A5
TOP, HALF = (1 << 64) - 1, 1 << 63
# every kernel runs at most 2048 blocks x 256 threads: 524,288 elements per trip.  One short of a full trip, exactly one, one
# element into the second (for the compacting kernels: the second, padded ballot trip with one live lane), two trips + 1.
TRIP = 2048 * 256
TRIP_SIZES = [TRIP - 1, TRIP, TRIP + 1, 2 * TRIP + 1]


def poisoned(engine, n_words):
    """an output buffer with known contents: released blocks are handed out again, and what an earlier call left in one
    could pass for this call's output"""
    return engine.to_device(np.full(max(n_words, 2), POISON, dtype=np.uint64))


def keep_fn(op, val):
    val = np.uint64(val)
    return {"<": lambda v: v < val, ">": lambda v: v > val, "=": lambda v: v == val}[op]


@pytest.mark.parametrize("n", TRIP_SIZES)
def test_grid_stride_trips(engine, n):
    rng = np.random.default_rng(n)
    ncol = 100_003
    col = rng.integers(0, 1 << 64, ncol, dtype=np.uint64)
    rows = rng.integers(0, ncol, n, dtype=np.uint64)
    rows[-1] = 5                                                           # the last element passes `= col[5]` below
    ri = rows.astype(np.int64)
    dcol, drows = engine.to_device(col), engine.to_device(rows)
    # sum_gather, gather_u64, gather_tuples
    assert engine.sum_gather(dcol, drows, n) == int(col[ri].sum(dtype=np.uint64))
    dd = poisoned(engine, n)
    engine.gather_u64(dcol, drows, n, dd)
    assert np.array_equal(dd.to_numpy(np.uint64, n), col[ri])
    for pos in (False, True):
        dt = poisoned(engine, 2 * n)
        engine.gather_tuples(dcol, drows, n, pos, dt)
        t = dt.to_numpy(TUPLE, n)
        assert np.array_equal(t["payload"], col[ri])
        assert np.array_equal(t["key"], np.arange(n, dtype=np.uint64) if pos else rows)
    # pairs_split
    pairs = np.empty(n, dtype=PAIR)
    pairs["keyR"], pairs["keyS"] = rng.integers(0, 1 << 64, n, dtype=np.uint64), rng.integers(0, 1 << 64, n, dtype=np.uint64)
    dp, dr, ds = engine.to_device(pairs), poisoned(engine, n), poisoned(engine, n)
    engine.pairs_split(dp, n, dr, ds)
    assert np.array_equal(dr.to_numpy(np.uint64, n), pairs["keyR"]) and np.array_equal(ds.to_numpy(np.uint64, n), pairs["keyS"])
    # rows_filter_equal: one position in four survives, in every trip
    colA, colB = rng.integers(0, 4, 1000, dtype=np.uint64), rng.integers(0, 4, 2000, dtype=np.uint64)
    rA, rB = rng.integers(0, 1000, n, dtype=np.uint64), rng.integers(0, 2000, n, dtype=np.uint64)
    rB[-1] = np.nonzero(colB == colA[int(rA[-1])])[0][0]                   # the last position survives
    d = [engine.to_device(x) for x in (colA, rA, colB, rB)]
    dpos = poisoned(engine, n)
    m = engine.rows_filter_equal(d[0], d[1], d[2], d[3], n, dpos)
    exp = np.nonzero(colA[rA.astype(np.int64)] == colB[rB.astype(np.int64)])[0].astype(np.uint64)
    assert m == len(exp) and exp[-1] == n - 1 and np.array_equal(np.sort(dpos.to_numpy(np.uint64, m)), exp)
    # col_filter through a row list (unsorted, rows repeat)
    dout = poisoned(engine, n)
    for op, val in (("<", HALF), (">", HALF), ("=", int(col[5]))):
        m = engine.col_filter(dcol, drows, n, op, val, dout)
        exp = np.sort(rows[keep_fn(op, val)(col[ri])])
        assert m == len(exp) and np.array_equal(np.sort(dout.to_numpy(np.uint64, m)), exp)


def test_null_row_lists(engine):
    """a NULL row list stands for the identity 0..n-1 (include/rhj.h)"""
    rng = np.random.default_rng(11)
    n = 70_001
    colA, colB = rng.integers(0, 4, n, dtype=np.uint64), rng.integers(0, 4, n + 9, dtype=np.uint64)
    rA, rB = rng.integers(0, n, n, dtype=np.uint64), rng.integers(0, n + 9, n, dtype=np.uint64)
    dA, dB, drA, drB = (engine.to_device(x) for x in (colA, colB, rA, rB))
    ident = np.arange(n)
    for a, b in ((None, drB), (drA, None), (None, None)):
        dpos = poisoned(engine, n)
        m = engine.rows_filter_equal(dA, a, dB, b, n, dpos)
        exp = np.nonzero(colA[ident if a is None else rA.astype(np.int64)] == colB[ident if b is None else rB.astype(np.int64)])[0]
        assert m == len(exp) and 0 < m < n and np.array_equal(np.sort(dpos.to_numpy(np.uint64, m)), exp.astype(np.uint64))
    wide = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    dw = engine.to_device(wide)
    assert engine.sum_gather(dw, None, n) == sum(int(v) for v in wide) % (1 << 64)
    for pos in (False, True):
        dt = poisoned(engine, 2 * n)
        engine.gather_tuples(dw, None, n, pos, dt)
        t = dt.to_numpy(TUPLE, n)
        assert np.array_equal(t["payload"], wide) and np.array_equal(t["key"], np.arange(n, dtype=np.uint64))


@pytest.fixture(scope="module")
def wide_column(engine):
    """100,003 values over the whole 64-bit range; 0, 2^63 - 1, 2^63 and 2^64 - 1 occur several times each"""
    rng = np.random.default_rng(12)
    n = 100_003
    col = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    col[rng.permutation(n)[:40]] = np.tile(np.array([0, HALF - 1, HALF, TOP], dtype=np.uint64), 10)
    return col, engine.to_device(col)


@pytest.mark.parametrize("op", ["<", ">", "="])
@pytest.mark.parametrize("val", [0, HALF - 1, HALF, TOP])
def test_col_filter_full_width(engine, wide_column, op, val):
    col, dcol = wide_column
    n = len(col)
    keep = keep_fn(op, val)(col)
    # unsigned: < 0 and > 2^64 - 1 keep no row; about half of the rows lie on either side of 2^63
    assert keep.sum() == sum(1 for v in col.tolist() if (v < val if op == "<" else v > val if op == ">" else v == val))
    dout = poisoned(engine, 2 * n)
    m = engine.col_filter(dcol, None, n, op, val, dout)
    assert m == keep.sum() and np.array_equal(np.sort(dout.to_numpy(np.uint64, m)), np.nonzero(keep)[0].astype(np.uint64))
    # a row list that is unsorted and repeats rows: every occurrence of a surviving row comes out
    rows = np.random.default_rng(13).integers(0, n, 2 * n, dtype=np.uint64)
    m = engine.col_filter(dcol, engine.to_device(rows), 2 * n, op, val, dout)
    exp = np.sort(rows[keep[rows.astype(np.int64)]])
    assert m == len(exp) and np.array_equal(np.sort(dout.to_numpy(np.uint64, m)), exp)


def test_col_filter_keeps_every_row_or_none(engine, wide_column):
    col, _ = wide_column
    n = len(col)
    inner = np.where((col == 0) | (col == TOP), np.uint64(HALF), col)      # neither 0 nor 2^64 - 1
    dcol, dout = engine.to_device(inner), poisoned(engine, n)
    for op, val in ((">", 0), ("<", TOP)):
        assert engine.col_filter(dcol, None, n, op, val, dout) == n
        assert np.array_equal(np.sort(dout.to_numpy(np.uint64, n)), np.arange(n, dtype=np.uint64))
    for op, val in (("<", 0), (">", TOP), ("=", 0), ("=", TOP)):
        dout = poisoned(engine, n)
        assert engine.col_filter(dcol, None, n, op, val, dout) == 0
        assert np.all(dout.to_numpy(np.uint64, n) == POISON)               # nothing was written


def test_sum_gather_wraps(engine):
    rng = np.random.default_rng(14)
    n = 100_000
    near = np.uint64(TOP) - rng.integers(0, 1000, n, dtype=np.uint64)      # all within 1000 of 2^64: the sum wraps ~n times
    col = near.tolist()
    exact = sum(col)
    assert exact >> 64 >= n - 1
    dcol = engine.to_device(near)
    assert engine.sum_gather(dcol, None, n) == exact % (1 << 64)
    rows = rng.integers(0, n, 3 * n, dtype=np.uint64)
    assert engine.sum_gather(dcol, engine.to_device(rows), 3 * n) == sum(col[r] for r in rows.tolist()) % (1 << 64)


@pytest.mark.parametrize("n", [0, 1])
def test_zero_and_one_element(engine, n):
    col, rows = np.array([7, TOP, 7], dtype=np.uint64), np.array([1, 2], dtype=np.uint64)
    dcol, drows = engine.to_device(col), engine.to_device(rows)
    for rin, r in ((None, 0), (drows, 1)):                                 # the one row in play: 0 (value 7) or 1 (2^64 - 1)
        for op, val, hit in (("=", int(col[r]), True), ("<", int(col[r]), False), (">", int(col[r]) - 1, True)):
            dout = poisoned(engine, 2)
            m = engine.col_filter(dcol, rin, n, op, val, dout)
            assert m == (n if hit else 0)
            assert dout.to_numpy(np.uint64, 2).tolist() == ([r, POISON] if m else [POISON, POISON])
        dout = poisoned(engine, 2)
        m = engine.rows_filter_equal(dcol, rin, dcol, None, n, dout)        # col[r] == col[0] only for r = 0
        assert m == (n if r == 0 else 0) and dout.to_numpy(np.uint64, 2).tolist() == ([0, POISON] if m else [POISON, POISON])
        assert engine.sum_gather(dcol, rin, n) == (int(col[r]) if n else 0)
        for pos in (False, True):
            dt = poisoned(engine, 4)
            engine.gather_tuples(dcol, rin, n, pos, dt)
            assert dt.to_numpy(np.uint64, 4).tolist() == ([0 if pos else r, int(col[r])] if n else [POISON] * 2) + [POISON] * 2
    dd = poisoned(engine, 2)
    engine.gather_u64(dcol, drows, n, dd)
    assert dd.to_numpy(np.uint64, 2).tolist() == ([TOP, POISON] if n else [POISON, POISON])
    dp, dr, ds = engine.to_device(np.array([3, TOP - 1, 5, 6], dtype=np.uint64)), poisoned(engine, 2), poisoned(engine, 2)
    engine.pairs_split(dp, n, dr, ds)
    assert dr.to_numpy(np.uint64, 2).tolist() == ([3, POISON] if n else [POISON] * 2)
    assert ds.to_numpy(np.uint64, 2).tolist() == ([TOP - 1, POISON] if n else [POISON] * 2)
    if n == 0:                                                             # with no element, no array has to exist
        assert engine.col_filter(None, None, 0, "<", 1, None) == 0 and engine.rows_filter_equal(None, None, None, None, 0, None) == 0
        assert engine.sum_gather(None, None, 0) == 0
        engine.gather_tuples(None, None, 0, True, None); engine.gather_u64(None, None, 0, None); engine.pairs_split(None, 0, None, None)


@pytest.mark.parametrize("op", ["!", "\0", "~", "L"])
def test_col_filter_bad_op(engine, op):
    dcol, dout = engine.to_device(np.arange(4, dtype=np.uint64)), poisoned(engine, 4)
    with pytest.raises(RhjError) as e:
        engine.col_filter(dcol, None, 4, op, 2, dout)
    assert e.value.code == RHJ_E_INVALID
    assert np.all(dout.to_numpy(np.uint64, 4) == POISON)
    assert engine.col_filter(dcol, None, 4, "<", 2, dout) == 2             # the context goes on working
