"""What the two group-id GPU suites share (test_gpu_group_ids.py, test_gpu_group_join_ids.py): an id array with guard words behind
it and a sentinel in every word, and the check of ids against a call's own outputs.  Nothing of the product is used: the check is
numpy on what the call wrote, so it does not depend on the order of groups."""
import numpy as np

SENTINEL = np.uint64(0xA5A5A5A55A5A5A5A)                                   # what an id word holds before the call; no group index, not all ones
GUARD, NGUARD = np.uint64(0xFEEDFACECAFEBEEF), 64                          # words behind the array
NO_GROUP = np.uint64((1 << 64) - 1)


class IdArray:
    """rows id words pre-set to SENTINEL, NGUARD guard words behind them"""
    def __init__(self, eng, rows):
        self.rows = rows
        fill = np.full(rows + NGUARD, SENTINEL, dtype=np.uint64)
        fill[rows:] = GUARD
        self.buf = eng.to_device(fill)

    def read(self):
        a = self.buf.to_numpy(np.uint64, self.rows + NGUARD)
        assert (a[self.rows:] == GUARD).all(), "a word at or past gid_rows was written"
        return a[:self.rows]

    def free(self):
        self.buf.free()


def raw(buf, groups):
    """the first `groups` words of an output array, in the call's own order"""
    return buf.to_numpy(np.uint64, groups) if groups else np.zeros(0, dtype=np.uint64)


def check_ids(gid, rows, values, keys, counts, groups):
    """gid: the id array as read; rows / values: the rowID and value of every tuple THAT HAS A GROUP; keys / counts: the call's
    outputs in its own order (counts may be None).  The issue's check: ids below groups, keys[gid[rows]] == values, and the bincount
    of the ids is the count column."""
    ids = gid[rows]
    bad = int((ids >= np.uint64(groups)).sum())
    print(f"rows with a group {len(rows)} groups {groups} ids out of range {bad}")
    assert bad == 0
    ids = ids.astype(np.int64)
    assert len(keys) == groups and np.array_equal(keys[ids], values)
    if counts is not None:
        assert np.array_equal(np.bincount(ids, minlength=groups).astype(np.uint64), counts)
