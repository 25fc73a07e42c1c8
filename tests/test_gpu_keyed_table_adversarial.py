"""GPU suite: adversarial keys for the five keyed-table kernels -- k_semi_bkt (its id form and the two outer-join pair forms),
k_agg_bkt, k_mult_bkt, k_group_bkt, k_gjoin_bkt -- through every path that feeds them.

The inputs come from keyed_table_cases.py (checked on the CPU by test_keyed_table_cases.py): values built in the space the kernel
sees, h = rhj_mix64(payload) or the payload itself where nothing mixes, so that they sit where the shared LDS table can go wrong --
the all-ones word that marks an empty slot and its neighbours (markers), the marker key in the first, the middle or the last of
several tables of a task (marker_and_tables), 3,000 distinct keys in ONE start slot whose chain begins at slot 0, wraps from slot 8191
to 0 or ends exactly at slot 8191, probed by absent keys of the same and of an inner start slot (chain), and table sides of 4095 ...
8193 distinct keys, where a table closes (fill_edge).

Every case goes through join_cols_dev (filled: the baseline the pair suite trusts), semi_join_cols_dev (SEMI, ANTI),
outer_join_cols_dev (three modes, the section checks of test_gpu_outer_join.check), join_sum_cols_dev (2 columns), join_mult_cols_dev
(with and without weights), group_agg_ids_cols_dev on R (SUM, MIN_I64, MAX_U64) and group_join_agg_ids_cols_dev (INNER, LEFT; a column per
side), each with explicit ids (a permutation) and with NULL ids.  Results equal keyed_table_cases.Oracle exactly -- these are integers --,
the pair multiset the C oracle's; reported group keys are the caller's payloads in every path; every call asserts the path that ran
(passes, "last.narrow", "last.countfree_*", "last.cols_*", "partition.mix") and its "last.semi_tables" / "last.group_rounds".

How many tables a task builds, from rhj_internal.h: a k_semi_bkt / k_agg_bkt / k_mult_bkt table takes whole tiles of SEMI_BUILD_TILE =
AGG_BUILD_TILE = 1024 tuples while filled + 1024 <= SEMI_FILL = AGG_FILL = 4608, i.e. while filled <= 3584 distinct keys.  With all
keys distinct that is true after 1, 2 and 3 tiles (1024, 2048, 3072) and false after the 4th (4096): a table holds 4096 keys, a task
builds ceil(n / 4096) tables.  The count is read between two barriers after every tile, so with repeated keys or the all-ones key
(which fills no slot) it still depends on the input order only: keyed_table_cases.tables_closed restates the rule and the assertions
are exact, not ranges.  k_group_bkt / k_gjoin_bkt build a class of R's keys per round and split a class that holds more than AGG_FILL =
4608 distinct keys by the next bit of mix64(key ^ salt): the rounds of a partition depend on its keys' hashes alone
(keyed_table_cases.group_rounds), again exact.  Both are 1 for markers and chain, whose partitions fit four tiles.

The count-free path (narrow 2, "partition.countfree" 1) gives every (pass-1 unit, digit) run a fixed region: at these sizes a unit is
one 4096-tuple tile and a region holds 64 tuples (cf_geometry: 16 + 10 * sqrt(16) + 1, rounded up to lines of 32).  `markers` keeps
every run far below that, and the case asserts "last.countfree_*" == 1.  `chain` cannot: its 3,858 table-side rows share one partition,
so one digit, and 64 per 4096 rows would take 250,000 rows of input -- chain runs on the exact paths only."""
import collections

import numpy as np
import pytest

import keyed_table_cases as K
from group_ids_cases import NO_GROUP, IdArray, check_ids
from oracle.pyoracle import TUPLE
from radixhashjoin_amd import (AGG_MAX_U64, AGG_MIN_I64, AGG_SUM, ANTI, GJ_INNER, GJ_LEFT, OUTER_FULL, OUTER_LEFT, OUTER_RIGHT, PAIR, SEMI,
                               Engine, Opts)
from test_gpu_outer_join import check as check_outer_sections, sort_pairs

pytestmark = pytest.mark.gpu
U64 = np.uint64
JK_SEMI, JK_AGG, JK_MULT, JK_GROUP, JK_GJOIN = 12, 13, 14, 15, 16
GROUP_OPS = [AGG_SUM, AGG_MIN_I64, AGG_MAX_U64]
GJ_OPS_R, GJ_OPS_S = [AGG_SUM], [AGG_MIN_I64]      # (S's minimum: a LEFT group without a tuple of S must hold the op's identity)

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


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


class Forced:
    """the options of one path on a context, re-armed before every call and reset to the defaults on exit"""

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
        for k in ("partition.narrow", "partition.countfree", "partition.mix"):
            self.eng.set_option(k, -1)
        return False

    def arm(self):
        self.eng.set_option("partition.narrow", self.path.narrow)
        self.eng.set_option("partition.countfree", self.path.countfree)
        self.eng.set_option("partition.mix", self.path.mix)

    def assert_ran(self, kernel, one_sided=False):
        e, p = self.eng, self.path
        narrow, cf = max(p.narrow, 0), 1 if p.countfree == 1 else 0
        cols = 1 if narrow else 2
        got = {k: e.info(k) for k in ("last.narrow", "last.countfree_R", "last.countfree_S", "last.cols_R", "last.cols_S", "partition.mix")}
        got["passes"] = e.timings()["passes"]
        print(f"{self.name}: kernel {e.info('last.join_kernel')} {got}")
        assert got == {"passes": self.plan.passes, "last.narrow": narrow, "last.countfree_R": cf, "last.countfree_S": 0 if one_sided else cf,
                       "last.cols_R": cols, "last.cols_S": 0 if one_sided else cols, "partition.mix": 0 if p.mix == 0 else 1}
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


def run_entries(f, oracle, case, ids):
    """every entry over one case under the path f, against the oracle"""
    e, plan = f.eng, f.plan
    case = case if ids else K.null_ids(case)
    nR, nS = len(case.valR), len(case.valS)
    orc = K.Oracle(case)
    dev = Device(e, case, ids)
    tabS, tabR, rounds = tables_expected(case, f, "S"), tables_expected(case, f, "R"), rounds_expected(case, f)
    bufs = []

    def alloc(words):
        bufs.append(e.alloc(8 * max(words, 1)))
        return bufs[-1]
    try:
        # ---- the pair join: the baseline -------------------------------------------------------------------------------------
        R, S = np.empty(nR, dtype=TUPLE), np.empty(nS, dtype=TUPLE)
        R["key"], R["payload"], S["key"], S["payload"] = case.idR, case.valR, case.idS, case.valS
        exp_pairs = oracle.join(R, S)
        npairs = orc.pair_count()
        assert len(exp_pairs) == npairs and npairs > 0
        out = alloc(2 * npairs)
        f.arm()
        assert e.join_cols_dev(dev.vR, dev.iR, nR, dev.vS, dev.iS, nS, out, npairs, opts=plan) == npairs
        assert np.array_equal(sort_pairs(out.to_numpy(PAIR, npairs)), sort_pairs(exp_pairs))
        f.assert_ran(None)
        assert e.info("last.semi_tables") == 0 and e.info("last.group_rounds") == 0

        # ---- semi and anti: k_semi_bkt, 8-byte rowIDs --------------------------------------------------------------------------
        out = alloc(nR)
        for kind in (SEMI, ANTI):
            exp = orc.semi_ids(kind == ANTI)
            f.arm()
            n = e.semi_join_cols_dev(dev.vR, dev.iR, nR, dev.vS, nS, kind, out, nR, opts=plan)
            got = np.sort(out.to_numpy(U64, n))
            print(f"semi kind {kind}: {n} ids, expected {len(exp)}, tables {e.info('last.semi_tables')} (expected {tabS})")
            assert n == len(exp) and np.array_equal(got, exp)
            f.assert_ran(JK_SEMI)
            assert e.info("last.semi_tables") == tabS

        # ---- outer joins: k_semi_bkt's pair forms behind the pair join ---------------------------------------------------------
        oexp = OuterExpected(exp_pairs, orc)
        cap = sum(oexp.sections(OUTER_FULL))
        out = alloc(2 * cap)
        for how in (OUTER_LEFT, OUTER_RIGHT, OUTER_FULL):
            f.arm()
            n, sec = e.outer_join_cols_dev(dev.vR, dev.iR, nR, dev.vS, dev.iS, nS, how, out, cap, opts=plan)
            check_outer_sections(out.to_numpy(PAIR, n), n, sec, how, oexp)
            f.assert_ran(None)
            assert e.info("last.outer_sweeps") == (2 if how == OUTER_FULL else 1)
            assert e.info("last.semi_tables") == max(tabS if how & OUTER_LEFT else 0, tabR if how & OUTER_RIGHT else 0)

        # ---- COUNT and SUMs over the join: k_agg_bkt ---------------------------------------------------------------------------
        f.arm()
        got = e.join_sum_cols_dev(dev.vR, dev.iR, nR, dev.vS, nS, dev.cR[:2], nR, opts=plan)
        exp = orc.join_sums(2)
        print(f"join_sum {got} expected {exp}")
        assert got[0] == exp[0] and got[1] == exp[1]
        f.assert_ran(JK_AGG)
        assert e.info("last.semi_tables") == tabS

        # ---- per-row multiplicity: k_mult_bkt, plain and weighted ----------------------------------------------------------------
        out = alloc(nR)
        for weighted in (False, True):
            exp_out, exp_total = orc.mult(nR, 0 if weighted else None)
            f.arm()
            total = e.join_mult_cols_dev(dev.vR, dev.iR, nR, dev.vS, dev.iS, nS, out, nR, dev.cS[0] if weighted else None,
                                         nS if weighted else 0, opts=plan)
            got = out.to_numpy(U64, nR)
            print(f"join_mult weighted {weighted}: total {total} expected {exp_total}, wrong words {int((got != exp_out).sum())}")
            assert total == exp_total and np.array_equal(got, exp_out)
            f.assert_ran(JK_MULT)
            assert e.info("last.semi_tables") == tabS

        # ---- GROUP BY on R with the group of every row: k_group_bkt ----------------------------------------------------------------
        keys, counts, aggs = orc.groups(GROUP_OPS)
        G = len(keys)
        o_keys, o_cnt, o_aggs, gid = alloc(G), alloc(G), [alloc(G) for _ in GROUP_OPS], IdArray(e, nR)
        try:
            f.arm()
            groups = e.group_agg_ids_cols_dev(dev.vR, dev.iR, nR, dev.cR, GROUP_OPS, nR, o_keys, o_cnt, o_aggs, G, gid.buf, nR, opts=plan)
            assert groups == G
            raw_keys, raw_cnt = o_keys.to_numpy(U64, G), o_cnt.to_numpy(U64, G)
            got = by_key(raw_keys, raw_cnt, *[a.to_numpy(U64, G) for a in o_aggs])
            print(f"group_agg: {groups} groups, rounds {e.info('last.group_rounds')} (expected {rounds}), "
                  f"keys not among the payloads {int((~np.isin(got[0], keys)).sum())}")
            assert np.array_equal(got[0], keys), "the group keys are not the caller's payloads"
            assert np.array_equal(got[1], counts)
            for j in range(len(GROUP_OPS)):
                assert np.array_equal(got[2 + j], aggs[j]), f"column {j}"
            check_ids(gid.read(), orc.R.ids, case.valR, raw_keys, raw_cnt, G)        # ids up to the permutation of d_out_keys
            f.assert_ran(JK_GROUP, one_sided=True)
            assert e.info("last.group_rounds") == rounds and e.info("last.semi_tables") == 0
        finally:
            gid.free()

        # ---- join with GROUP BY on the key, both modes: k_gjoin_bkt ----------------------------------------------------------------
        for mode in (GJ_INNER, GJ_LEFT):
            keys, cntR, cntS, aggsR, aggsS = orc.group_join(mode == GJ_LEFT, GJ_OPS_R, GJ_OPS_S)
            G = len(keys)
            assert G > 0
            o = [alloc(G) for _ in range(5)]                                # keys, cntR, cntS, R's column, S's column
            gR, gS = IdArray(e, nR), IdArray(e, nS)
            try:
                f.arm()
                groups = e.group_join_agg_ids_cols_dev(dev.vR, dev.iR, nR, dev.vS, dev.iS, nS, dev.cR[:1], GJ_OPS_R, nR, dev.cS[:1], GJ_OPS_S, nS,
                                                       mode, o[0], o[1], o[2], o[3:4], o[4:5], G, gR.buf, nR, gS.buf, nS, opts=plan)
                assert groups == G
                raw = [b.to_numpy(U64, G) for b in o]
                got = by_key(*raw)
                print(f"group_join mode {mode}: {groups} groups, rounds {e.info('last.group_rounds')} (expected {rounds})")
                assert np.array_equal(got[0], keys), "the group keys are not the caller's payloads"
                for name, a, b in zip(("cntR", "cntS", "aggR", "aggS"), got[1:], (cntR, cntS, aggsR[0], aggsS[0])):
                    assert np.array_equal(a, b), name
                for side, g, cnt in ((orc.R, gR.read(), raw[1]), (orc.S, gS.read(), raw[2])):
                    has = np.isin(side.val, keys)
                    check_ids(g, side.ids[has], side.val[has], raw[0], cnt, G)
                    rest = np.ones(len(g), dtype=bool)
                    rest[side.ids[has]] = False
                    assert (g[rest] == NO_GROUP).all()
                f.assert_ran(JK_GJOIN)
                assert e.info("last.group_rounds") == rounds and e.info("last.semi_tables") == 0
            finally:
                gR.free()
                gS.free()
    finally:
        dev.free()
        for b in bufs:
            b.free()


def run_case(f, oracle, case):
    for ids in (True, False):
        run_entries(f, oracle, case, ids)


# ---- markers: every path -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", K.MARKER_VARIANTS)
@pytest.mark.parametrize("path", list(PATHS))
def test_markers(eng, oracle, path, variant):
    """the empty marker as the kernel sees it -- unmix64(all ones) where the path mixes, the raw all-ones payload where it does not --,
    its neighbours and the raw payloads 0 / all ones / unmix64(0), on R only, on S only and on both"""
    with Forced(eng, path) as f:
        case = K.markers(f.rb, f.pattern, f.mixes, variant)
        marker = K.payload_of(K.ONES, f.mixes)
        assert any(int(p) == int(marker) for p, _, _ in case.info["markers"])
        run_case(f, oracle, case)


# ---- chains: every path but the count-free one (see the module's docstring) ----------------------------------------------------------
@pytest.mark.parametrize("table_side", ["S", "R"])
@pytest.mark.parametrize("variant", K.CHAIN_VARIANTS)
@pytest.mark.parametrize("path", EXACT_PATHS)
def test_chain(eng, oracle, path, variant, table_side):
    """3,000 distinct keys in one start slot, on the table side of the semi / sum / mult kernels (S) and of the group kernels and the
    right outer sweep (R); absent keys that must walk to the empty slot behind the chain and answer no"""
    with Forced(eng, path) as f:
        run_case(f, oracle, K.chain(f.rb, f.pattern, f.mixes, variant, table_side))


# ---- several tables per task: the unpartitioned path, where the table side is read in input order -------------------------------------
@pytest.mark.parametrize("table_side", ["S", "R"])
@pytest.mark.parametrize("probes", K.MARKER_PROBES)
@pytest.mark.parametrize("position", K.MARKER_POSITIONS)
def test_marker_and_tables(eng, oracle, position, probes, table_side):
    """the marker key of the table side in the first, the second or the last of three tables, or absent; 0, 1 or 5 probes of it"""
    with Forced(eng, "unpartitioned") as f:
        case = K.marker_and_tables(position, probes, table_side)
        assert tables_expected(case, f, table_side) == 3                    # ceil(9000 / 4096), ceil(9001 / 4096)
        run_case(f, oracle, case)


@pytest.mark.parametrize("table_side", ["S", "R"])
@pytest.mark.parametrize("edge", K.FILL_EDGES, ids=[str(x) for x in K.FILL_EDGES])
def test_fill_edge(eng, oracle, edge, table_side):
    """where a table closes: 4095, 4096 (one table), 4097 (a second table of one key), 8192, 8193 distinct keys; 4096 distinct keys and
    10,000 repeats of one of them behind them"""
    with Forced(eng, "unpartitioned") as f:
        case = K.fill_edge(edge, table_side)
        assert tables_expected(case, f, table_side) == {4095: 1, 4096: 1, 4097: 2, 8192: 2, 8193: 3, "4096+repeats": 2}[edge]
        run_case(f, oracle, case)


def test_one_pass_pair_join_reports_its_own_count_free_state(eng, oracle):
    """a pair join under a one-pass plan runs without a partition phase of its own: "last.countfree_*" must be its zeros, not the ones
    of the count-free join before it (they were, and every path assertion after a count-free case read them)"""
    case = K.markers(16, PATTERN[16], True, 0)
    with Forced(eng, "two-pass-countfree") as f:
        run_entries(f, oracle, case, True)
        assert eng.info("last.countfree_R") == 1 and eng.info("last.countfree_S") == 1
    with Forced(eng, "one-pass") as f:
        dev = Device(eng, case, False)
        try:
            assert eng.join_cols_dev(dev.vR, None, len(case.valR), dev.vS, None, len(case.valS), opts=f.plan) == K.Oracle(case).pair_count()
            f.assert_ran(None)
        finally:
            dev.free()
