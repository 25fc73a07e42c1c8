"""The sort entry's oracle and case generators (numpy only; shares nothing with the product).

Oracle: np.argsort(t(keys), kind="stable"), t the view -- the words as uint64, or with the sign bit flipped for the int64 order --
and, for descending, the bitwise complement of the transformed word: the complement reverses the key order and nothing else, so a
stable argsort of it keeps ties in input order, which is what the entry promises in both directions."""
import numpy as np

SORT_I64, SORT_DESC = 1, 2                    # include/rhj.h RHJ_SORT_*
FLAGS = (0, SORT_I64, SORT_DESC, SORT_I64 | SORT_DESC)
BIAS = np.uint64(1 << 63)
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
GUARD = np.uint64(0xDEADBEEFCAFEF00D)
NGUARD = 16


def transform(keys, flags):
    """the uint64 word whose ascending unsigned order is the order asked for"""
    t = np.asarray(keys, dtype=np.uint64)
    if flags & SORT_I64:
        t = t ^ BIAS
    if flags & SORT_DESC:
        t = ~t
    return t


def oracle_perm(keys, flags):
    return np.argsort(transform(keys, flags), kind="stable").astype(np.uint64)


def oracle_bits(keys, flags):
    """the width the probe must find: 0 when max == min in the view, else 64 - clz(max - min)"""
    if len(keys) == 0:
        return 0
    t = np.asarray(keys, dtype=np.uint64) ^ (BIAS if flags & SORT_I64 else np.uint64(0))
    return int(int(t.max()) - int(t.min())).bit_length()


DISTS = ("full64", "sixteen", "constant", "sorted", "reverse", "small_signed", "extremes", "middle_digit", "top_byte")


def make_keys(dist, n, seed=0):
    """n uint64 words of the named distribution"""
    rng = np.random.default_rng(1000 * (DISTS.index(dist) + 1) + n % 977 + seed)
    if dist == "full64":                      # 8-bit digits: 8 passes
        return rng.integers(0, 1 << 64, n, dtype=np.uint64)
    if dist == "sixteen":                     # long tie runs: the stability test proper
        vals = rng.integers(0, 1 << 64, 16, dtype=np.uint64)
        return vals[rng.integers(0, 16, n)]
    if dist == "constant":                    # 0 passes
        return np.full(n, 0x0123456789ABCDEF, dtype=np.uint64)
    if dist == "sorted":
        return np.sort(rng.integers(0, 1 << 40, n, dtype=np.uint64))
    if dist == "reverse":
        return np.sort(rng.integers(0, 1 << 40, n, dtype=np.uint64))[::-1].copy()
    if dist == "small_signed":                # int64 in -3 .. 3: signed 3 bits, unsigned 64
        return rng.integers(-3, 4, n, dtype=np.int64).view(np.uint64)
    if dist == "extremes":                    # both views' extremes mixed into random words: base subtraction wraps
        k = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        special = np.array([0, (1 << 63) - 1, 1 << 63, (1 << 64) - 1], dtype=np.uint64)
        where = rng.random(n) < 0.25
        k[where] = special[rng.integers(0, 4, int(where.sum()))]
        if n >= 4:
            k[rng.permutation(n)[:4]] = special
        return k
    if dist == "middle_digit":                # r1 << 16 | 0x55 << 8 | r2: a middle digit that is one bin
        r1 = rng.integers(0, 256, n, dtype=np.uint64)
        r2 = rng.integers(0, 256, n, dtype=np.uint64)
        return (r1 << np.uint64(16)) | np.uint64(0x55 << 8) | r2
    if dist == "top_byte":                    # keys that differ only in their top byte
        return (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(56)) | np.uint64(0x00A5A5A5A5A5A5A5)
    raise ValueError(dist)


def wide_rows(n, seed=0):
    """explicit rowIDs: opaque payloads with duplicates and values >= 2^32"""
    rng = np.random.default_rng(n + 31 + seed)
    r = rng.integers(0, 1 << 64, max(n // 3, 1), dtype=np.uint64)
    return r[rng.integers(0, len(r), n)]
