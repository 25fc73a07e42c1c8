"""The top-k entries' oracle and case generators (numpy only; shares nothing with the product).

Oracle: the first min(k, n) entries of the sort's oracle, sort_cases.oracle_perm -- a stable argsort in the chosen view, so ties
keep their input order in both directions, also at the cut.  Two distributions beside sort_cases.DISTS:
  "outliers"  all but 10 keys below 2^8 and 10 keys near 2^40: every upper digit keeps almost every row a candidate, then the digits
              run out inside a tie run;
  "cut_run"   a sorted-then-shuffled column in which ONE value fills the middle third of the ranks, so that a k near n / 2 falls
              inside its run (cut_run_bounds: the ranks the run covers, ascending unsigned), and the run's rows lie all over the
              input -- in every tile."""
import numpy as np

import sort_cases as SC

DISTS = SC.DISTS + ("outliers", "cut_run")
RUN_VALUE = np.uint64(1 << 39)


def make_keys(dist, n, seed=0):
    """n uint64 words of the named distribution"""
    if dist in SC.DISTS:
        return SC.make_keys(dist, n, seed)
    rng = np.random.default_rng(1000 * (DISTS.index(dist) + 1) + n % 977 + seed)
    if dist == "outliers":
        k = rng.integers(0, 1 << 8, n, dtype=np.uint64)
        far = rng.permutation(n)[:10]
        k[far] = np.uint64(1 << 40) - rng.integers(1, 1 << 8, len(far), dtype=np.uint64)
        return k
    if dist == "cut_run":
        k = np.sort(rng.integers(0, 1 << 40, n, dtype=np.uint64))
        lo, hi = cut_run_bounds(n)
        k[:lo] = k[:lo] % RUN_VALUE                                      # below the run's value ...
        k[hi:] = RUN_VALUE + np.uint64(1) + k[hi:] % RUN_VALUE           # ... and above it
        k[lo:hi] = RUN_VALUE
        return k[rng.permutation(n)]
    raise ValueError(dist)


def cut_run_bounds(n):
    """[lo, hi): the ranks "cut_run"'s run value takes in unsigned ascending order"""
    return n // 3, max(n - n // 3, n // 3 + 1) if n else 0


def oracle_topk(keys, k, flags):
    """the rows of the first min(k, n) tuples of the sort"""
    return SC.oracle_perm(keys, flags)[:min(k, len(keys))]


def run_of(keys, flags, rank):
    """[first, last]: the ranks of the tie run that the tuple of rank `rank` stands in"""
    t = np.sort(SC.transform(keys, flags))
    return int(np.searchsorted(t, t[rank], "left")), int(np.searchsorted(t, t[rank], "right")) - 1
