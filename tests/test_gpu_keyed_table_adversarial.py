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
(with and without weights), lookup_cols_dev (FIRST, LAST), group_agg_ids_cols_dev on R (SUM, MIN_I64, MAX_U64), group_arg_cols_dev on R
(MIN_I64 and MAX_U64 of one column pointer, the group's first and last row; k_group_bkt<., GB_ARG>, whose rows arrays are filled by
global atomics) and group_join_agg_ids_cols_dev (INNER, LEFT; a column per side), each with explicit ids (a permutation) and with NULL
ids.  The runner and its helpers live in keyed_entries.py, which test_gpu_ladder.py shares.  Results equal keyed_table_cases.Oracle exactly -- these are integers --,
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
so one digit, and 64 per 4096 rows would take 250,000 rows of input -- chain runs on the exact paths only here; under the count-free
path it overflows on both sides and takes the two-repeat rung of the ladder, which is test_gpu_ladder.py's subject."""
import pytest

import keyed_table_cases as K
from keyed_entries import EXACT_PATHS, PATHS, PATTERN, Device, Forced, run_case, run_entries, tables_expected

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from radixhashjoin_amd import Engine
    e = Engine(0)
    yield e
    e.close()


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
            f.assert_ran(None, f.state())
        finally:
            dev.free()
