"""The entry runner of the keyed-table GPU suites (test_gpu_keyed_table_adversarial.py, test_gpu_ladder.py): every columnar entry
over one keyed_table_cases.Case under one forced path, against keyed_table_cases.Oracle.  A plain module, no conftest: the files
that use it import it.

PATHS names the paths, Forced arms one on a context and asserts the state words a call reports, Device holds a case's columns in HBM,
Run holds one case on the device and has one method per entry; run_entries calls them all.  Every output array has guard words behind
it, every comparison is exact (these are integers), the pair multiset is the C oracle's.

Run(..., state=) takes the expected state of every call as a function of one_sided; without it a call must report what its path gives
on an input that takes no repeat (Forced.state).  Run(..., twice=True) makes every call a second time on the same context, re-armed:
the same checks again, and the same words where the entry promises them (lookup, group_arg, join_mult, join_sum).  Run.seen records
"last.join_kernel" / "last.semi_tables" / "last.group_rounds" / "last.outer_sweeps" per call, so that two runs of one input under two
paths can be compared."""
import collections

import numpy as np

import keyed_table_cases as K
from group_arg_cases import arg_oracle
from group_ids_cases import GUARD, NGUARD, NO_GROUP, SENTINEL, IdArray, check_ids
from oracle.pyoracle import TUPLE
from radixhashjoin_amd import (AGG_MAX_U64, AGG_MIN_I64, AGG_SUM, ANTI, ARG_MAX_U64, ARG_MIN_I64, ARG_ROW, ARG_TIE_FIRST, ARG_TIE_LAST,
                               GJ_INNER, GJ_LEFT, LOOKUP_FIRST, LOOKUP_LAST, OUTER_FULL, OUTER_LEFT, OUTER_RIGHT, PAIR, SEMI, Opts)
from test_gpu_group_arg import check_exact as check_arg_exact
from test_gpu_group_sum import Outputs
from test_gpu_lookup import oracle as lookup_oracle
from test_gpu_outer_join import check as check_outer_sections, sort_pairs

U64 = np.uint64
JK_SEMI, JK_AGG, JK_MULT, JK_GROUP, JK_GJOIN, JK_LOOKUP = 12, 13, 14, 15, 16, 17
GROUP_OPS = [AGG_SUM, AGG_MIN_I64, AGG_MAX_U64]
GJ_OPS_R, GJ_OPS_S = [AGG_SUM], [AGG_MIN_I64]      # (S's minimum: a LEFT group without a tuple of S must hold the op's identity)
ARG_OPS = [ARG_MIN_I64, ARG_MAX_U64, ARG_ROW, ARG_ROW]                     # MIN and MAX of ONE pointer, the group's first and last row
ARG_TIES = [ARG_TIE_FIRST, ARG_TIE_LAST, ARG_TIE_FIRST, ARG_TIE_LAST]
STAMP = U64(0xDEADBEEFDEADBEEF)                    # what an output word holds before the call
GID_SLACK = 8                                      # words of an id array that no rowID names

# path -> (plan, "partition.narrow", "partition.countfree", "partition.mix"); -1 leaves an option at its default.  What must have run:
# the plan's passes; narrow partitions at the level asked (16-byte tuples otherwise); count-free pass 1 on both sides where asked;
# columns read directly ("last.cols_*" 1) by the narrow two-pass paths and converted first (2) by every other one.
Path = collections.namedtuple("Path", "plan narrow countfree mix")
PATHS = {
    "unpartitioned": Path(Opts(0, 0, 0), -1, -1, -1),
    "one-pass": Path(Opts(1, 4, 0), -1, -1, -1),
    "two-pass-16B": Path(Opts(2, 8, 8), 0, -1, -1),
    "two-pass-narrow1": Path(Opts(2, 8, 8), 1, -1, -1),
    "two-pass-narrow2": Path(Opts(2, 8, 8), 2, 0, -1),
    "two-pass-countfree": Path(Opts(2, 8, 8), 2, 1, -1),
    "raw-one-pass": Path(Opts(1, 4, 0), -1, -1, 0),
    "raw-narrow2": Path(Opts(2, 8, 8), 2, 0, 0),
}
EXACT_PATHS = [p for p in PATHS if p != "two-pass-countfree"]
PATTERN = {0: 0, 4: 9, 16: 0xBEEF}                 # the partition the crafted keys of a plan of rb bits share
STATE = ("last.narrow", "last.countfree_R", "last.countfree_S", "last.cols_R", "last.cols_S")


class Forced:
    """the options of one path on a context, re-armed before every call and reset to the defaults on exit"""
    OPTIONS = ("partition.narrow", "partition.countfree", "partition.mix")

    def __init__(self, eng, name):
        self.eng, self.name, self.path = eng, name, PATHS[name]
        self.plan = self.path.plan
        self.rb = K.radix_bits(self.plan)
        self.mixes = self.rb != 0 and self.path.mix != 0                    # unpartitioned plans and "partition.mix" 0 do not mix
        self.pattern = PATTERN[self.rb]

    def __enter__(self):
        self.arm()
        return self

    def __exit__(self, *exc):
        for k in self.OPTIONS:
            self.eng.set_option(k, -1)
        return False

    def arm(self):
        self.eng.set_option("partition.narrow", self.path.narrow)
        self.eng.set_option("partition.countfree", self.path.countfree)
        self.eng.set_option("partition.mix", self.path.mix)

    def state(self, one_sided=False):
        """the STATE words of a call that takes no repeat under this path"""
        p = self.path
        narrow, cf = max(p.narrow, 0), 1 if p.countfree == 1 else 0
        cols = 1 if narrow else 2
        return (narrow, cf, 0 if one_sided else cf, cols, 0 if one_sided else cols)

    def assert_ran(self, kernel, state):
        """state: the STATE words expected of the call just made"""
        e, p = self.eng, self.path
        got = {k: e.info(k) for k in STATE + ("partition.mix",)}
        got["passes"] = e.timings()["passes"]
        print(f"{self.name}: kernel {e.info('last.join_kernel')} {got}")
        exp = dict(zip(STATE, state))
        exp.update({"passes": self.plan.passes, "partition.mix": 0 if p.mix == 0 else 1})
        assert got == exp
        if kernel is not None:
            assert e.info("last.join_kernel") == kernel


class Device:
    """a case's columns in HBM; ids=False: the calls get NULL id columns"""

    def __init__(self, eng, case, ids):
        up = eng.to_device
        self.vR, self.vS = up(case.valR), up(case.valS)
        self.iR, self.iS = (up(case.idR), up(case.idS)) if ids else (None, None)
        self.cR, self.cS = [up(c) for c in case.colsR], [up(c) for c in case.colsS]

    def free(self):
        for b in [self.vR, self.vS, self.iR, self.iS] + self.cR + self.cS:
            if b is not None:
                b.free()


class AosEngine:
    """an Engine whose columnar entries take the 16-byte entry of the same phase on the case's tuples (value = .payload, rowID =
    .key); everything else is the Engine's"""
    BOTH = {"join_cols_dev": "join_dev", "outer_join_cols_dev": "outer_join_dev", "join_mult_cols_dev": "join_mult_dev",
            "lookup_cols_dev": "lookup_dev", "group_join_agg_ids_cols_dev": "group_join_agg_ids_dev"}      # (vR, iR, nR, vS, iS, nS, ...)
    NO_ID_S = {"semi_join_cols_dev": "semi_join_dev", "join_sum_cols_dev": "join_sum_dev"}                  # (vR, iR, nR, vS, nS, ...)
    R_ONLY = {"group_agg_ids_cols_dev": "group_agg_ids_dev", "group_arg_cols_dev": "group_arg_dev"}         # (vR, iR, nR, ...)

    def __init__(self, eng, case):
        self.eng = eng
        R, S = np.empty(len(case.valR), dtype=TUPLE), np.empty(len(case.valS), dtype=TUPLE)
        R["key"], R["payload"], S["key"], S["payload"] = case.idR, case.valR, case.idS, case.valS
        self.R, self.S = R, S
        self.dR, self.dS = eng.to_device(R), eng.to_device(S)

    def free(self):
        self.dR.free()
        self.dS.free()

    def __getattr__(self, name):
        eng = self.eng
        if name in self.BOTH:
            return lambda vR, iR, nR, vS, iS, nS, *a, **k: getattr(eng, self.BOTH[name])(self.dR, nR, self.dS, nS, *a, **k)
        if name in self.NO_ID_S:
            return lambda vR, iR, nR, vS, nS, *a, **k: getattr(eng, self.NO_ID_S[name])(self.dR, nR, self.dS, nS, *a, **k)
        if name in self.R_ONLY:
            return lambda vR, iR, nR, *a, **k: getattr(eng, self.R_ONLY[name])(self.dR, nR, *a, **k)
        return getattr(eng, name)


class Guarded:
    """`words` output words pre-set to STAMP, NGUARD guard words behind them"""

    def __init__(self, eng, words):
        self.cap, self.words = words, max(words + (words & 1), 2)           # (whole 16-byte pairs)
        fill = np.full(self.words + NGUARD, STAMP, dtype=U64)
        fill[self.words:] = GUARD
        self.buf = eng.to_device(fill)

    def read(self, dtype, count):
        """the first `count` items; asserts the guard words"""
        a = self.buf.to_numpy(U64, self.words + NGUARD)
        assert (a[self.words:] == GUARD).all() and (a[self.cap:self.words] == STAMP).all(), "a word at or past the capacity was written"
        return a[:self.words].view(dtype)[:count].copy()

    def free(self):
        self.buf.free()


class OuterExpected:
    """what test_gpu_outer_join.check reads of its oracle"""

    def __init__(self, pairs, orc):
        self.pairs, self.r_only, self.s_only = sort_pairs(pairs), orc.r_only(), orc.s_only()

    def sections(self, how):
        return (len(self.pairs), len(self.r_only) if how & OUTER_LEFT else 0, len(self.s_only) if how & OUTER_RIGHT else 0)


def tables_expected(case, f, side):
    """"last.semi_tables" of a sweep whose tables are built on `side`: 1 where every partition fits a table (markers, chain: asserted
    on the CPU), what the close rule gives for the one unpartitioned task otherwise"""
    keys = case.valS if side == "S" else case.valR
    return K.tables_closed(keys) if f.rb == 0 else 1


def rounds_expected(case, f):
    return K.group_rounds(case.valR) if f.rb == 0 else 1


def by_key(keys, *words):
    order = np.argsort(keys, kind="stable")
    return [keys[order]] + [w[order] for w in words]


def same_words(a, b):
    """two results of one call, as nested lists of arrays and integers"""
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_words(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


class Run:
    """one case on the device under the path f; one method per entry, each exact against the oracle.  ids=False: NULL id columns
    (the rowID of a tuple is its index).  The id columns of a case may hold a rowID that indexes nothing (ladder_cases.wide): the
    methods that read a column or an array by rowID say so and are not for such a case."""
    ENTRIES = ("pair", "semi", "anti", "outer_left", "outer_right", "outer_full", "join_sum", "mult", "mult_weighted", "lookup_first",
               "lookup_last", "group_ids", "group_arg", "gjoin_inner", "gjoin_left")

    def __init__(self, f, oracle, case, ids, state=None, twice=False, arm=True, aos=False, follow=None):
        self.f, self.plan, self.c_oracle = f, f.plan, oracle
        self.case = case = case if ids else K.null_ids(case)
        self.nR, self.nS = len(case.valR), len(case.valS)
        self.orc = K.Oracle(case)
        self.dev = Device(f.eng, case, ids)
        self.e = AosEngine(f.eng, case) if aos else f.eng                   # aos: the 16-byte entries (which need ids)
        assert ids or not aos
        self.follow, self.current = follow, None                           # follow(name): called behind every call of entry `name`
        self.state = state if state is not None else f.state
        self.twice, self.rearm = twice, arm
        self.tabS, self.tabR, self.rounds = tables_expected(case, f, "S"), tables_expected(case, f, "R"), rounds_expected(case, f)
        self.seen = {}
        self.bufs = []
        self._pairs = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False

    def free(self):
        self.dev.free()
        if isinstance(self.e, AosEngine):
            self.e.free()
        for b in self.bufs:
            b.free()
        self.bufs = []

    def out(self, words):
        self.bufs.append(Guarded(self.e, words))
        return self.bufs[-1]

    def outputs(self, capacity, ncols):
        self.bufs.append(Outputs(self.e, capacity, ncols))
        return self.bufs[-1]

    def id_array(self, rows):
        self.bufs.append(IdArray(self.e, rows + GID_SLACK))
        return self.bufs[-1]

    def ran(self, name, kernel, one_sided=False, tables=0, rounds=0, sweeps=None):
        """after a call: the state words, the kernel and what it built"""
        e = self.e
        self.f.assert_ran(kernel, self.state(one_sided))
        assert e.info("last.semi_tables") == tables and e.info("last.group_rounds") == rounds
        if sweeps is not None:
            assert e.info("last.outer_sweeps") == sweeps
        self.seen[self.current or name] = (e.info("last.join_kernel"), e.info("last.semi_tables"), e.info("last.group_rounds"), e.info("last.outer_sweeps"))

    def call(self, once, same=False):
        """arm, call and check; with twice a second time -- re-armed, the same checks, and with `same` the same words"""
        if self.rearm:
            self.f.arm()
        first = once()
        if self.follow:
            self.follow(self.current)
        if self.twice:
            self.f.arm()
            again = once()
            if same:
                assert same_words(first, again), "the second call on the same context gave other words"
            if self.follow:
                self.follow(self.current)
        return first

    def run(self, name):
        """the entry `name`; its output arrays are freed behind it"""
        self.current, kept = name, len(self.bufs)
        try:
            return getattr(self, name)()
        finally:
            for b in self.bufs[kept:]:
                b.free()
            del self.bufs[kept:]

    # ---- the pair join: the baseline ---------------------------------------------------------------------------------------------
    def expected_pairs(self):
        if self._pairs is None:
            case = self.case
            R, S = np.empty(self.nR, dtype=TUPLE), np.empty(self.nS, dtype=TUPLE)
            R["key"], R["payload"], S["key"], S["payload"] = case.idR, case.valR, case.idS, case.valS
            self._pairs = self.c_oracle.join(R, S)
            assert len(self._pairs) == self.orc.pair_count() > 0
        return self._pairs

    def pair(self):
        e, dev, exp = self.e, self.dev, self.expected_pairs()
        npairs = len(exp)
        out = self.out(2 * npairs)

        def once():
            assert e.join_cols_dev(dev.vR, dev.iR, self.nR, dev.vS, dev.iS, self.nS, out.buf, npairs, opts=self.plan) == npairs
            assert np.array_equal(sort_pairs(out.read(PAIR, npairs)), sort_pairs(exp))
            self.ran("pair", None)
        self.call(once)

    # ---- semi and anti: k_semi_bkt, 8-byte rowIDs ----------------------------------------------------------------------------------
    def semi(self, kind=SEMI):
        e, dev = self.e, self.dev
        exp = self.orc.semi_ids(kind == ANTI)
        out = self.out(self.nR)

        def once():
            n = e.semi_join_cols_dev(dev.vR, dev.iR, self.nR, dev.vS, self.nS, kind, out.buf, self.nR, opts=self.plan)
            got = np.sort(out.read(U64, n))
            print(f"semi kind {kind}: {n} ids, expected {len(exp)}, tables {e.info('last.semi_tables')} (expected {self.tabS})")
            assert n == len(exp) and np.array_equal(got, exp)
            self.ran("anti" if kind == ANTI else "semi", JK_SEMI, tables=self.tabS)
        self.call(once)

    def anti(self):
        self.semi(ANTI)

    # ---- outer joins: k_semi_bkt's pair forms behind the pair join -----------------------------------------------------------------
    def outer(self, how):
        e, dev = self.e, self.dev
        oexp = OuterExpected(self.expected_pairs(), self.orc)
        cap = sum(oexp.sections(OUTER_FULL))
        out = self.out(2 * cap)
        name = {OUTER_LEFT: "outer_left", OUTER_RIGHT: "outer_right", OUTER_FULL: "outer_full"}[how]

        def once():
            n, sec = e.outer_join_cols_dev(dev.vR, dev.iR, self.nR, dev.vS, dev.iS, self.nS, how, out.buf, cap, opts=self.plan)
            check_outer_sections(out.read(PAIR, n), n, sec, how, oexp)
            self.ran(name, None, tables=max(self.tabS if how & OUTER_LEFT else 0, self.tabR if how & OUTER_RIGHT else 0),
                     sweeps=2 if how == OUTER_FULL else 1)
        self.call(once)

    def outer_left(self):
        self.outer(OUTER_LEFT)

    def outer_right(self):
        self.outer(OUTER_RIGHT)

    def outer_full(self):
        self.outer(OUTER_FULL)

    # ---- COUNT and SUMs over the join: k_agg_bkt (the columns are read at R's rowIDs) ------------------------------------------------
    def join_sum(self, ncols=2):
        e, dev = self.e, self.dev
        exp = self.orc.join_sums(ncols)

        def once():
            got = e.join_sum_cols_dev(dev.vR, dev.iR, self.nR, dev.vS, self.nS, dev.cR[:ncols], self.nR if ncols else 0, opts=self.plan)
            print(f"join_sum {got} expected {exp}")
            assert got[0] == exp[0] and list(got[1]) == list(exp[1])
            self.ran("join_sum", JK_AGG, tables=self.tabS)
            return [got[0], list(got[1])]
        self.call(once, same=True)

    def join_sum_plain(self):
        self.join_sum(0)

    # ---- per-row multiplicity: k_mult_bkt, plain and weighted (d_out is indexed by R's rowID, the weights by S's) ------------------------
    def mult(self, weighted=False):
        e, dev, nR, nS = self.e, self.dev, self.nR, self.nS
        exp_out, exp_total = self.orc.mult(nR, 0 if weighted else None)
        out = self.out(nR)

        def once():
            total = e.join_mult_cols_dev(dev.vR, dev.iR, nR, dev.vS, dev.iS, nS, out.buf, nR, dev.cS[0] if weighted else None,
                                         nS if weighted else 0, opts=self.plan)
            got = out.read(U64, nR)
            print(f"join_mult weighted {weighted}: total {total} expected {exp_total}, wrong words {int((got != exp_out).sum())}")
            assert total == exp_total and np.array_equal(got, exp_out)
            self.ran("mult_weighted" if weighted else "mult", JK_MULT, tables=self.tabS)
            return [total, got]
        self.call(once, same=True)

    def mult_weighted(self):
        self.mult(True)

    # ---- the lookup join: one partner rowID of S per rowID of R (d_out is indexed by R's rowID) --------------------------------------------
    def lookup(self, which):
        e, dev, case, nR, nS = self.e, self.dev, self.case, self.nR, self.nS
        exp_out, exp_matched = lookup_oracle(case.valR, case.idR.astype(np.int64), case.valS, case.idS, which, nR)
        assert 0 < exp_matched < nR
        out = self.out(nR)

        def once():
            matched = e.lookup_cols_dev(dev.vR, dev.iR, nR, dev.vS, dev.iS, nS, out.buf, nR, which, opts=self.plan)
            got = out.read(U64, nR)
            print(f"lookup which {which}: matched {matched} expected {exp_matched}, wrong words {int((got != exp_out).sum())}")
            assert matched == exp_matched and np.array_equal(got, exp_out)
            self.ran("lookup_first" if which == LOOKUP_FIRST else "lookup_last", JK_LOOKUP, tables=self.tabS)
            return [matched, got]
        self.call(once, same=True)

    def lookup_first(self):
        self.lookup(LOOKUP_FIRST)

    def lookup_last(self):
        self.lookup(LOOKUP_LAST)

    # ---- GROUP BY on R with the group of every row: k_group_bkt ------------------------------------------------------------------------
    def group_ids(self):
        e, dev, case, nR = self.e, self.dev, self.case, self.nR
        keys, counts, aggs = self.orc.groups(GROUP_OPS)
        G = len(keys)
        o, gid = self.outputs(G, len(GROUP_OPS)), self.id_array(nR)

        def once():
            groups = e.group_agg_ids_cols_dev(dev.vR, dev.iR, nR, dev.cR, GROUP_OPS, nR, o.keys, o.counts, o.sums, G, gid.buf, nR,
                                              opts=self.plan)
            assert groups == G
            raw_keys, raw_cnt = o.keys.to_numpy(U64, G), o.counts.to_numpy(U64, G)
            got = o.read(G)                                                # (sorted by key; asserts the guards)
            print(f"group_agg: {groups} groups, rounds {e.info('last.group_rounds')} (expected {self.rounds}), "
                  f"keys not among the payloads {int((~np.isin(got[0], keys)).sum())}")
            assert np.array_equal(got[0], keys), "the group keys are not the caller's payloads"
            assert np.array_equal(got[1], counts)
            for j in range(len(GROUP_OPS)):
                assert np.array_equal(got[2][j], aggs[j]), f"column {j}"
            g = gid.read()
            check_ids(g[:nR], self.orc.R.ids, case.valR, raw_keys, raw_cnt, G)   # ids up to the permutation of d_out_keys
            assert (g[nR:] == SENTINEL).all(), "an id word that no rowID names was written"
            self.ran("group_ids", JK_GROUP, one_sided=True, rounds=self.rounds)
        self.call(once)

    def group_agg_plain(self):
        """rhj_group_agg_cols_dev with no column and no ids: keys and counts (no rowID is used as an index)"""
        e, dev, nR = self.e, self.dev, self.nR
        keys, counts, _ = self.orc.groups([])
        G = len(keys)
        o = self.outputs(G, 0)

        def once():
            assert e.group_agg_cols_dev(dev.vR, dev.iR, nR, (), None, 0, o.keys, o.counts, (), G, opts=self.plan) == G
            got = o.read(G)
            assert np.array_equal(got[0], keys) and np.array_equal(got[1], counts)
            self.ran("group_agg_plain", JK_GROUP, one_sided=True, rounds=self.rounds)
            return [got[0], got[1]]
        self.call(once, same=True)

    # ---- the row of every group's extreme: k_group_bkt<., GB_ARG>, rows filled by global atomics ----------------------------------------
    def group_arg(self, ops=ARG_OPS, ties=ARG_TIES):
        e, dev, case, nR = self.e, self.dev, self.case, self.nR
        k = len(ops)
        cols = [None if op == ARG_ROW else case.colsR[0] for op in ops]
        exp = arg_oracle(case.valR, case.idR, cols, ops, ties)
        G = len(exp[0])
        o = self.outputs(G, 2 * k)                                          # k value arrays, k rows arrays, guards behind each
        d_cols = [None if op == ARG_ROW else dev.cR[0] for op in ops]
        col_rows = nR if any(c is not None for c in d_cols) else 0

        def once():
            groups = e.group_arg_cols_dev(dev.vR, dev.iR, nR, d_cols, ops, ties, col_rows, o.keys, o.counts, o.sums[:k], o.sums[k:], G,
                                          opts=self.plan)
            assert groups == G
            got = o.read(G)
            check_arg_exact(got, exp, ops)                                 # (a ROW column's value array must still hold its guard word)
            self.ran("group_arg", JK_GROUP, one_sided=True, rounds=self.rounds)
            return list(got[:2]) + [a for a, op in zip(got[2][:k], ops) if op != ARG_ROW] + list(got[2][k:])
        return self.call(once, same=True)

    def group_arg_rows(self):
        return self.group_arg([ARG_ROW, ARG_ROW], [ARG_TIE_FIRST, ARG_TIE_LAST])

    # ---- join with GROUP BY on the key, both modes: k_gjoin_bkt ------------------------------------------------------------------------
    def gjoin(self, mode):
        e, dev, nR, nS = self.e, self.dev, self.nR, self.nS
        keys, cntR, cntS, aggsR, aggsS = self.orc.group_join(mode == GJ_LEFT, GJ_OPS_R, GJ_OPS_S)
        G = len(keys)
        assert G > 0
        o = self.outputs(G, 3)                                              # keys, cntR; cntS, R's column, S's column
        gR, gS = self.id_array(nR), self.id_array(nS)

        def once():
            groups = e.group_join_agg_ids_cols_dev(dev.vR, dev.iR, nR, dev.vS, dev.iS, nS, dev.cR[:1], GJ_OPS_R, nR, dev.cS[:1], GJ_OPS_S,
                                                   nS, mode, o.keys, o.counts, o.sums[0], o.sums[1:2], o.sums[2:3], G, gR.buf, nR, gS.buf,
                                                   nS, opts=self.plan)
            assert groups == G
            raw = [b.to_numpy(U64, G) for b in o.all()]
            got = o.read(G)
            print(f"group_join mode {mode}: {groups} groups, rounds {e.info('last.group_rounds')} (expected {self.rounds})")
            assert np.array_equal(got[0], keys), "the group keys are not the caller's payloads"
            for name, a, b in zip(("cntR", "cntS", "aggR", "aggS"), [got[1]] + got[2], (cntR, cntS, aggsR[0], aggsS[0])):
                assert np.array_equal(a, b), name
            for side, ida, n, cnt in ((self.orc.R, gR, nR, raw[1]), (self.orc.S, gS, nS, raw[2])):
                g = ida.read()
                has = np.isin(side.val, keys)
                check_ids(g[:n], side.ids[has], side.val[has], raw[0], cnt, G)
                rest = np.ones(n, dtype=bool)
                rest[side.ids[has]] = False
                assert (g[:n][rest] == NO_GROUP).all()
                assert (g[n:] == SENTINEL).all(), "an id word at or past the side's rows was written"
            self.ran("gjoin_left" if mode == GJ_LEFT else "gjoin_inner", JK_GJOIN, rounds=self.rounds)
        self.call(once)

    def gjoin_inner(self):
        self.gjoin(GJ_INNER)

    def gjoin_left(self):
        self.gjoin(GJ_LEFT)

    def gjoin_plain(self, mode=GJ_INNER):
        """rhj_group_join_agg_cols_dev with no column and no ids: keys and both counts (no rowID is used as an index)"""
        e, dev, nR, nS = self.e, self.dev, self.nR, self.nS
        keys, cntR, cntS, _, _ = self.orc.group_join(mode == GJ_LEFT, [], [])
        G = len(keys)
        o = self.outputs(G, 1)

        def once():
            groups = e.group_join_agg_cols_dev(dev.vR, dev.iR, nR, dev.vS, dev.iS, nS, (), None, 0, (), None, 0, mode, o.keys, o.counts,
                                               o.sums[0], (), (), G, opts=self.plan)
            assert groups == G
            got = o.read(G)
            assert np.array_equal(got[0], keys) and np.array_equal(got[1], cntR) and np.array_equal(got[2][0], cntS)
            self.ran("gjoin_plain", JK_GJOIN, rounds=self.rounds)
            return [got[0], got[1], got[2][0]]
        self.call(once, same=True)


def run_entries(f, oracle, case, ids, **kw):
    """every entry over one case under the path f, against the oracle; -> Run.seen"""
    with Run(f, oracle, case, ids, **kw) as r:
        for name in Run.ENTRIES:
            r.run(name)
        return r.seen


def run_case(f, oracle, case, **kw):
    for ids in (True, False):
        run_entries(f, oracle, case, ids, **kw)
