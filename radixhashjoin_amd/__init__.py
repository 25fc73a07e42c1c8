"""radixhashjoin_amd -- MI355X (gfx950) radix hash join engine.

The product is the C-ABI shared library ``librhj_hip.so`` (hand-written HIP kernels, see
``csrc/`` and ``include/rhj.h``) plus the C++ host mirror of the reference's
``relation / relation_info / Result / JobScheduler`` surface in ``host/``.  This Python package is
only the thin ctypes binding used by tests, ``bench.py`` and the multi-GPU driver; there is NO
CPU fallback: if the HIP library is missing or no GPU is present, construction of an
:class:`Engine` raises.

From torch: ``idx_R, idx_S = Engine(0).join_columns(keys_R, keys_S)`` joins two int64 key tensors on the engine's device
(``rhj_join_cols_dev``: the relations as columns, rowID = index); ``Engine(0).semi_join_columns(keys_R, keys_S, anti=False)``
returns the indices of the keys of R that occur (``anti=True``: do not occur) in S (``rhj_semi_join_cols_dev``);
``idx_R, idx_S = Engine(0).outer_join_columns(keys_R, keys_S, how="left")`` is the left, right or full outer join: the matched index
pairs first, then the unmatched rows of the preserved side(s) with -1 on the missing side (``rhj_outer_join_cols_dev``);
``count, sums = Engine(0).join_sum_columns(keys_R, keys_S, weights)`` is COUNT(*) and SUM(weights[k][i]) over the join's pairs
without the pairs (``rhj_join_sum_cols_dev``); ``mult, total = Engine(0).join_multiplicity_columns(keys_R, keys_S, weights_S=None)``
is, per key of R, how many keys of S equal it -- or the sum of their weights (``rhj_join_mult_cols_dev``);
``idx_S, matched, values = Engine(0).lookup_columns(keys_R, keys_S, values_S, fill=0, which="first")`` is the lookup of every key of
R in S, aligned with R: the first (or last) index in S, -1 where there is none, and S's value tensors gathered by it
(``rhj_lookup_cols_dev``, ``rhj_gather_cols_fill``);
``unique_keys, counts, sums = Engine(0).group_by_columns(keys, weights)`` is GROUP BY on one key tensor: its distinct values, their
counts and the per-group sums of the weight tensors (``rhj_group_sum_cols_dev``) -- with ``ops=["min", "max", "sum"]`` the per-group
minimum, maximum or sum per weight tensor (``rhj_group_agg_cols_dev``);
``unique_keys, counts, vals, rows = Engine(0).group_by_columns_arg(keys, [t], ["max"], ties="last")`` is which row holds each group's
minimum or maximum -- the latest record per key -- and ``idx = Engine(0).drop_duplicates_columns(keys, keep="first")`` the rows
pandas' drop_duplicates keeps (``rhj_group_arg_cols_dev``);
``keys, count, sums_R, sums_S = Engine(0).join_group_by_columns(keys_R, keys_S, weights_R, weights_S, how="inner")`` is the join
with GROUP BY on the key: per join value COUNT(*) and the SUMs of both sides' weights over its pairs, without the pairs
(``rhj_group_join_cols_dev``); ``ops_R`` / ``ops_S`` make a column a minimum or maximum there too (``rhj_group_join_agg_cols_dev``).
Composite keys: every one of these takes a list of up to four key tensors per side wherever it takes a key tensor (``ON r.a = s.a
AND r.b = s.b``, ``GROUP BY a, b``); ``packed_R, packed_S, plan = Engine(0).pack_keys([a, b], [c, d])`` is the step they share -- one
exact 64-bit key per row (``rhj_keys_pack_dev``), and ``plan.unpack(packed)`` gives the columns back (``rhj_keys_unpack_dev``).
Order: ``sorted_keys, perm, gathered = Engine(0).sort_columns(keys, values, descending=False)`` is ORDER BY on a key tensor -- a stable
radix sort, ``perm`` the stable argsort, ``values[k][perm]`` beside it; a list of key tensors is ``ORDER BY k0, k1, ..``;
``Engine(0).argsort_columns(keys)`` returns ``perm`` alone (``rhj_sort_cols_dev``).
``top_keys, idx, gathered = Engine(0).topk_columns(keys, k, values, descending=False)`` is ORDER BY .. LIMIT k -- the first k entries of
that sort without sorting the column (a radix select in front of the sort), and ``value, row = Engine(0).kth_value_columns(keys, k)``
the k-th smallest key and its row, a median or a quantile, with nothing of size k written (``rhj_topk_cols_dev``).
Window functions: ``number, running = Engine(0).window_columns(k, t, [None, x], ["row_number", "cumsum"])`` is ROW_NUMBER() and a
running SUM(x) OVER (PARTITION BY k ORDER BY t), one tensor per op aligned with the rows -- also rank, dense_rank, cummin / cummax and
lag / lead (``rhj_window_cols_dev``); ``Engine(0).topk_per_group_columns(k, t, 3)`` the rows with ROW_NUMBER <= 3.
As-of join: ``idx_S, matched, values = Engine(0).asof_join_columns(t_R, t_S, by_R=sym_R, by_S=sym_S, values_S=[bid])`` is, for every
row of R, the row of S with the same ``by`` whose ``on`` is the nearest at or before it (``direction="forward"``: at or after), -1
where there is none, aligned with R -- ``pandas.merge_asof`` on unsorted tensors, with ``allow_exact_matches`` and ``tolerance``
(``rhj_asof_cols_dev``).
Framed window aggregates: ``moving, size = Engine(0).frame_columns(k, t, [x, None], ["max", "count"], [9, None], [0, None])`` is
MAX(x) over the last ten rows of each partition and the partition's size, aligned with the rows -- sliding ROWS frames for count, sum,
min / max and the frame's first / last row, a sliding min / max at the same cost for every width (``rhj_frame_cols_dev``);
``Engine(0).ntile_columns(k, t, 4)`` is NTILE(4).
RANGE frames: ``Engine(0).frame_range_columns(sym, t, [x, None], ["sum", "count"], 5_000_000_000)`` is the sum and the count of the same
symbol's rows of the last 5 seconds -- the frame a value distance on the order key, peers always inside (``rhj_frame_range_cols_dev``).
Range join: ``idx_R, idx_S = Engine(0).range_join_columns(lo_R, hi_R, t_S, by_R=sym_R, by_S=sym_S)`` is every pair with the same ``by``
and ``lo_R[i] <= t_S[j] <= hi_R[i]``, ordered by i and then by (t_S[j], j) -- a defined order, bit-identical from run to run;
``offsets, first, rows_S, total = Engine(0).range_join_csr_columns(..)`` the same as runs of S in sorted order, 16 bytes per row of R
and 8 per row of S however many pairs there are; ``Engine(0).band_join_columns(t_R, t_S, below, above, ..)`` the band join
``t_R[i] - below <= t_S[j] <= t_R[i] + above`` with saturating ends (``rhj_range_join_cols_dev``, ``rhj_range_expand_dev``).
"""
from .binding import (  # noqa: F401
    AGG_MAX_I64,
    AGG_MAX_U64,
    AGG_MIN_I64,
    AGG_MIN_U64,
    AGG_SUM,
    ANTI,
    ARG_MAX_I64,
    ARG_MAX_U64,
    ARG_MIN_I64,
    ARG_MIN_U64,
    ARG_ROW,
    ARG_TIE_FIRST,
    ARG_TIE_LAST,
    ASOF_FORWARD,
    ASOF_I64,
    ASOF_STRICT,
    ASOF_TOLERANCE,
    PAIR,
    RANGE_BAND,
    RANGE_HI_OPEN,
    RANGE_I64,
    RANGE_LO_OPEN,
    TUPLE,
    DeviceBuffer,
    Engine,
    FRAME_COUNT,
    FRAME_FIRST_ROW,
    FRAME_LAST_ROW,
    FRAME_MAX_I64,
    FRAME_MAX_OPS,
    FRAME_MAX_U64,
    FRAME_MIN_I64,
    FRAME_MIN_U64,
    FRAME_SUM,
    FRAME_UNBOUNDED,
    GJ_INNER,
    GJ_LEFT,
    GROUP_ARG_MAX_COLS,
    GROUP_JOIN_MAX_COLS,
    GROUP_MAX_COLS,
    KEYS_DICT,
    KEYS_MAX_COLS,
    KEYS_NO_UNPACK,
    KEYS_RANGE,
    KeyPlan,
    KeysLayout,
    LOOKUP_FIRST,
    LOOKUP_LAST,
    LOOKUP_MAX_COLS,
    NO_ROW,
    OUTER_FULL,
    OUTER_LEFT,
    OUTER_RIGHT,
    Opts,
    RhjError,
    SEMI,
    SORT_DESC,
    SORT_I64,
    SUM_MAX_COLS,
    Timings,
    WINDOW_MAX_OPS,
    WIN_CUMMAX_I64,
    WIN_CUMMAX_U64,
    WIN_CUMMIN_I64,
    WIN_CUMMIN_U64,
    WIN_CUMSUM,
    WIN_DENSE_RANK,
    WIN_LAG_ROW,
    WIN_LEAD_ROW,
    WIN_RANK,
    WIN_ROW_NUMBER,
    lib_path,
    load_library,
    mix64,
    keys_layout,
    unmix64,
)

__all__ = ["Engine", "Opts", "Timings", "DeviceBuffer", "RhjError", "TUPLE", "PAIR", "lib_path", "load_library", "mix64", "unmix64", "SEMI", "ANTI", "OUTER_LEFT", "OUTER_RIGHT", "OUTER_FULL", "NO_ROW", "SUM_MAX_COLS", "GROUP_MAX_COLS", "GROUP_JOIN_MAX_COLS", "GJ_INNER", "GJ_LEFT", "AGG_SUM", "AGG_MIN_U64", "AGG_MAX_U64", "AGG_MIN_I64", "AGG_MAX_I64", "KeyPlan", "KeysLayout", "keys_layout", "KEYS_MAX_COLS", "KEYS_NO_UNPACK", "KEYS_RANGE", "KEYS_DICT", "LOOKUP_FIRST", "LOOKUP_LAST", "LOOKUP_MAX_COLS", "ARG_MIN_U64", "ARG_MAX_U64", "ARG_MIN_I64", "ARG_MAX_I64", "ARG_ROW", "ARG_TIE_FIRST", "ARG_TIE_LAST", "GROUP_ARG_MAX_COLS", "SORT_I64", "SORT_DESC", "WINDOW_MAX_OPS", "WIN_ROW_NUMBER", "WIN_RANK", "WIN_DENSE_RANK", "WIN_LAG_ROW", "WIN_LEAD_ROW", "WIN_CUMSUM", "WIN_CUMMIN_U64", "WIN_CUMMAX_U64", "WIN_CUMMIN_I64", "WIN_CUMMAX_I64", "ASOF_I64", "ASOF_FORWARD", "ASOF_STRICT", "ASOF_TOLERANCE", "FRAME_MAX_OPS", "FRAME_UNBOUNDED", "FRAME_COUNT", "FRAME_SUM", "FRAME_MIN_U64", "FRAME_MAX_U64", "FRAME_MIN_I64", "FRAME_MAX_I64", "FRAME_FIRST_ROW", "FRAME_LAST_ROW", "RANGE_I64", "RANGE_LO_OPEN", "RANGE_HI_OPEN", "RANGE_BAND"]
__version__ = "0.1.0"
