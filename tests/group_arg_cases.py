"""What the group-by argmin / argmax suites share (test_group_arg_abi.py, test_gpu_group_arg.py): the numpy oracle.  Nothing of the
product is used, and nothing of group_agg_cases.side_oracle: per column ONE lexicographic sort of the tuples by (group key, column
word in the op's order, rowID in the tie's order) and the first or last tuple of every group's run -- the tuple a reader of the
contract would pick by hand.  The column word is ordered as uint64 for the U64 ops and as int64 for the I64 ops; rowIDs always as
uint64."""
import numpy as np

from radixhashjoin_amd import ARG_MAX_I64, ARG_MAX_U64, ARG_MIN_I64, ARG_MIN_U64, ARG_ROW, ARG_TIE_FIRST, ARG_TIE_LAST

MASK64 = (1 << 64) - 1
I64_MIN, I64_MAX = 1 << 63, (1 << 63) - 1                                  # as 64-bit words
VALUE_OPS = [ARG_MIN_U64, ARG_MAX_U64, ARG_MIN_I64, ARG_MAX_I64]
# the word a minimum / maximum sweep starts from: a column that holds nothing else is where a row sweep may lose its row
IDENTITY = {ARG_MIN_U64: MASK64, ARG_MAX_U64: 0, ARG_MIN_I64: I64_MAX, ARG_MAX_I64: I64_MIN}
_IS_MAX = {ARG_MIN_U64: False, ARG_MAX_U64: True, ARG_MIN_I64: False, ARG_MAX_I64: True}
_VIEW = {ARG_MIN_U64: np.uint64, ARG_MAX_U64: np.uint64, ARG_MIN_I64: np.int64, ARG_MAX_I64: np.int64}


def arg_oracle(values, rows, cols, ops, ties):
    """(keys ascending, counts, [extremes as uint64 words, None for ARG_ROW], [rowIDs as uint64]).  values: uint64 keys; rows: the
    rowID of every tuple; cols: uint64 columns indexed by rowID (None under ARG_ROW); column j under ops[j] / ties[j]"""
    values = np.asarray(values, dtype=np.uint64)
    rid = np.asarray(rows).astype(np.uint64)
    keys, counts = np.unique(values, return_counts=True)
    if len(keys) == 0:
        empty = np.zeros(0, dtype=np.uint64)
        return keys, counts.astype(np.uint64), [None if op == ARG_ROW else empty for op in ops], [empty for _ in ops]
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    last = np.cumsum(counts) - 1
    vals, out_rows, by_row = [], [], None
    for c, op, tie in zip(cols, ops, ties):
        assert tie in (ARG_TIE_FIRST, ARG_TIE_LAST)
        if op == ARG_ROW:                                                  # the rowIDs themselves: ascending, the run's first or last
            by_row = np.lexsort((rid, values)) if by_row is None else by_row
            pick = by_row[first if tie == ARG_TIE_FIRST else last]
            vals.append(None)
            out_rows.append(rid[pick])
            continue
        word = np.asarray(c, dtype=np.uint64)[rid.astype(np.int64)]
        # a minimum is the run's first tuple, a maximum its last: the rowID order is turned round where the tuple wanted among equal
        # words would otherwise stand at the wrong end of them
        want_first_of_run = not _IS_MAX[op]
        rid_ascending = (tie == ARG_TIE_FIRST) == want_first_of_run
        order = np.lexsort((rid if rid_ascending else ~rid, word.view(_VIEW[op]), values))
        pick = order[first if want_first_of_run else last]
        vals.append(word[pick])
        out_rows.append(rid[pick])
    return keys, counts.astype(np.uint64), vals, out_rows


def tying_groups(values, rows, col, op):
    """per key (ascending): how many tuples of the group hold the group's extreme of col under op"""
    keys, _, (ext,), _ = arg_oracle(values, rows, [col], [op], [ARG_TIE_FIRST])
    g = np.searchsorted(keys, values)
    at = np.asarray(col, dtype=np.uint64)[np.asarray(rows).astype(np.int64)] == ext[g]
    return np.bincount(g[at], minlength=len(keys))
