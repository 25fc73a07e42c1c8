"""GPU suite: every operator through every rung of the repeat ladder of partition_and_join (rhj_api.hip), at
10^4 rows and below.

A call that starts in the narrow format with a count-free pass 1 can run its partition phase and the phase behind it up to three
times: after a count-free overflow of R, of S or of both one after the other, after a rowID >= 2^32, and after an overflow of R
followed by a wide rowID of S that the first attempt never looked at.  The loop is shared by the eight phases (join_phase, semi_phase,
outer_phase, agg_phase, mult_phase, lookup_phase, group_phase, gjoin_phase); what makes a repeat right is not: each phase zeroes or
refills its own outputs, counters and guard flags on every attempt, and the back-off words live in the context and outlive the call.

Every call here is armed with "partition.narrow" 2, "partition.countfree" 1 and "partition.countfree2" 0 (the one-writer pass 2 is
test_gpu_cf_walk's subject) under Opts(2, 8, 8).  Under forced options the narrow format applies from 1,024 tuples; a relation below
4,096 rows is one pass-1 unit whose (unit, digit) region holds cf_cases.cap(4096, 8) = 64 tuples, so 64 rows of one pass-1 digit fit
and the 65th repeats the call.  ladder_cases.py builds the inputs (checked on the CPU by test_ladder_cases.py), keyed_entries.py runs
the entries.

The rungs and the state words ("last.narrow", "last.countfree_R", "last.countfree_S", "last.cols_R", "last.cols_S") each must report
-- ladder_cases.expect; read from partition_phase / partition_and_join and confirmed here:

    rung              input                           narrow cf_R cf_S cols  partition phases
    full              cap on R and on S                  2     1    1   1, 1   1
    S+1               cap + 1 on S                       2     1    2   1, 1   2, R stands (cf_keep_R)
    R+1               cap + 1 on R                       2     2    1   1, 1   2, S runs again, count-free
    both+1            cap + 1 on both                    2     2    2   1, 1   3, the loop's maximum
    chain             K.chain, 2,304 ... 2,717 rows of
                      one digit on both sides            2     2    2   1, 1   3
    wide R / wide S   rowID 2^32, no overflow            0     0    0   2, 2   2
    S+1, wide R       the flag's bit 0 is read first     0     0    0   2, 2   2; no streak, no back-off
    R+1, wide S       S's kernels return at once in
                      attempt 1, the id shows in 2       0     0    0   2, 2   3; cf_skip[R] armed

A one-sided operator (group_agg_ids, group_arg, group_agg) partitions R alone: it takes the R rungs and reports 0 in S's words.  A
16-byte entry reads no column: "last.cols_*" are 0.

Every case asserts the result against the oracle, exactly; the guard words behind every output (and the id words that no rowID
names); the state words above, exactly; "last.join_kernel", "last.semi_tables", "last.group_rounds" and "last.outer_sweeps" equal to
what the exact path reports for the same input (narrow 2 without the count-free pass; 16 bytes for a wide id); the same call a second
time, re-armed: the same words (bit-identical for lookup, group_arg, join_mult, join_sum); and behind each of the two the same entry
on K.markers, re-armed, which must be exact and report (2, 1, 1, 1, 1): its own state, not the previous call's.

Which assertion catches a phase that skipped its re-initialisation on a repeat (argued from the code, no kernel was weakened):
  * join_phase / outer_phase: the result counter and the task count (the 64-byte counter block) -- a count that went on from the
    abandoned attempt overflows the capacity, which is exactly the pair count; outer_phase's sweep count is asserted ("last.outer_sweeps"
    1 or 2: it is zeroed per attempt, not per call);
  * semi_phase: the id counter -- the ids of the abandoned attempt would stand in front of the right ones and the count would double;
  * agg_phase / mult_phase: COUNT, the sums and the total are accumulated by atomics from zero; d_out of join_mult is zeroed per
    attempt -- a word that kept the abandoned attempt's partial multiplicity is compared with the oracle's;
  * lookup_phase: d_out is set to all ones per attempt and filled by atomic minima / maxima -- a word of the abandoned attempt could
    only be hidden if it were the right one already, the matched count not at all;
  * group_phase: the group counter; for group_arg the rows arrays, which the owners re-seed: an abandoned attempt's rows[g] word belongs
    to ANOTHER group of the repeat (the group order differs), so a minimum that was not re-seeded shows as a wrong row of that group;
    the id words of group_agg_ids are written again by every tuple;
  * gjoin_phase: both id arrays are filled with all ones per attempt -- checked on every word no group names; the group counter as
    above;
  * every phase: its guard flag word, which a repeat must clear -- a stale narrow flag would repeat the call until the loop gives up
    ("overflow flag after the exact repeat").
The chain rungs abandon two attempts whose kernels of the side that overflowed ran to the end on 2,300 rows of garbage cursors: the
massive case of all the above.

The back-off is per context and per SIDE, not per operator: after S+1 through any operator the next two calls that ask for a
count-free pass 1 on S -- two-sided calls of any operator under a narrow fused plan -- run S with exact cursors ("last.countfree_S" 0)
and the third reports 1, R's word staying 1 throughout.  A one-sided operator never asks cf_side_for about S (partition_phase skips S
under ctx->one_sided), so it consumes nothing of S's back-off; it does consume R's.  An unpartitioned or one-pass call asks about
neither.  After "R+1, wide S" the next two eligible calls report "last.countfree_R" 0: the only observable that tells that rung from a
plain wide one.  set_option("partition.countfree", 1) clears the back-off.

Out of scope: the narrow back-off (narrow_skip) acts in automatic mode only, which needs 8 * 10^6 tuples; count-free pass 2 stays 0."""
import pytest

import keyed_table_cases as K
import ladder_cases as LC
from group_arg_cases import arg_oracle
from keyed_entries import PATTERN, Forced, Run
from radixhashjoin_amd import ARG_MIN_I64, ARG_ROW, ARG_TIE_FIRST, ARG_TIE_LAST, Engine, RhjError
from radixhashjoin_amd.binding import RHJ_E_INVALID

pytestmark = pytest.mark.gpu
PAT = PATTERN[16]
BASES = {"one-unit": (3000, 2500), "partial-unit": (9000, 7000)}          # R, S: 1 and 1 units; 3 and 2, the last one partial
RUNGS = {"full": ("both", 0), "S+1": ("S", 1), "R+1": ("R", 1), "both+1": ("both", 1)}
ONE_SIDED = ("group_ids", "group_arg", "group_agg_plain", "group_arg_rows")
PLAIN_STATE = (2, 1, 1, 1, 1)
# every columnar entry, and the forms that read no column and write no id (rhj_group_agg_cols_dev, rhj_group_join_agg_cols_dev, ...)
ALL = Run.ENTRIES + ("join_sum_plain", "group_agg_plain", "group_arg_rows", "gjoin_plain")
# the entries whose contract lets a rowID index nothing, by the side that may hold the wide id
WIDE = {"R": ("pair", "semi", "anti", "outer_left", "outer_right", "outer_full", "join_sum_plain", "group_agg_plain", "gjoin_plain",
              "group_arg_rows"),
        "S": ("pair", "outer_left", "outer_right", "outer_full", "lookup_first", "lookup_last", "mult", "gjoin_plain")}


class Ladder(Forced):
    """narrow 2, count-free pass 1 forced, count-free pass 2 off"""
    OPTIONS = Forced.OPTIONS + ("partition.countfree2",)

    def __init__(self, eng):
        super().__init__(eng, "two-pass-countfree")
        self.name = "ladder"

    def arm(self):
        super().arm()
        self.eng.set_option("partition.countfree2", 0)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    for k in Ladder.OPTIONS:
        e.set_option(k, -1)
    e.close()


@pytest.fixture(scope="module")
def cases():
    """name -> Case: built once, shared, never written"""
    cache = {}

    def base(name, variant):
        return K.markers(16, PAT, True, variant, n_ordinary=BASES[name])

    def get(*key):
        if key not in cache:
            kind = key[0]
            if kind == "plain":
                c = K.markers(16, PAT, True, 0)
                c = c._replace(info=LC.plain_info(c))
            elif kind == "rung":                                           # ("rung", base, rung, variant)
                c = LC.rung(base(key[1], key[3]), *RUNGS[key[2]], PAT)
            elif kind == "chain":                                          # ("chain", variant, table side)
                c = K.chain(16, PAT, True, key[1], key[2])
                c = c._replace(info=LC.chain_info(c))
            else:                                                          # ("wide", side, *the key of the case below)
                inner = get(*key[2:])
                n = len(inner.valR if key[1] == "R" else inner.valS)
                c = LC.wide(inner, key[1], n // 3)
            cache[key] = c
        return cache[key]
    return get


def expected(case, aos=False):
    """one_sided -> the state words of a call on this case"""
    def state(one_sided=False):
        s = LC.expect(case.info, one_sided)[0]
        return s[:3] + (0, 0) if aos else s
    return state


def exact_seen(eng, oracle, case, ids, entries, aos=False):
    """what the exact path reports for the same input: narrow 2 with the pass-1 histogram, or 16 bytes where an id is wide"""
    with Forced(eng, "two-pass-16B" if case.info.get("wide") else "two-pass-narrow2") as f:
        state = (lambda one_sided=False: f.state(one_sided)[:3] + (0, 0)) if aos else None
        with Run(f, oracle, case, ids, state=state, aos=aos) as r:
            for name in entries:
                r.run(name)
            return dict(r.seen)


def climb(eng, oracle, cases, case, ids, entries, aos=False):
    """the entries over one rung: each exact, twice, with the same entry on K.markers behind every call"""
    exact = exact_seen(eng, oracle, case, ids, entries, aos)
    f = Ladder(eng)
    with f, Run(f, oracle, cases("plain"), ids, state=lambda one_sided=False: LC.expect(cases("plain").info, one_sided)[0]) as plain:
        with Run(f, oracle, case, ids, state=expected(case, aos), twice=True, aos=aos, follow=plain.run) as r:
            for name in entries:
                r.run(name)
            assert r.seen == exact
            return len(entries)


# ---- the overflow rungs: every entry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", [True, False], ids=["ids", "null"])
@pytest.mark.parametrize("base", list(BASES))
@pytest.mark.parametrize("rung", list(RUNGS))
def test_overflow_rungs(eng, oracle, cases, rung, base, ids):
    """64 rows of one digit in one unit on both sides (no repeat), 65 on S, on R, on both; the three marker variants rotate over the
    rungs.  The one-sided entries report R's word and 0 for S whatever S holds."""
    variant = (list(RUNGS).index(rung) + list(BASES).index(base)) % 3
    case = cases("rung", base, rung, variant)
    assert LC.expect(case.info)[0] == {"full": (2, 1, 1, 1, 1), "S+1": (2, 1, 2, 1, 1), "R+1": (2, 2, 1, 1, 1), "both+1": (2, 2, 2, 1, 1)}[rung]
    climb(eng, oracle, cases, case, ids, ALL)


@pytest.mark.parametrize("ids", [True, False], ids=["ids", "null"])
@pytest.mark.parametrize("table_side", ["S", "R"])
@pytest.mark.parametrize("variant", K.CHAIN_VARIANTS)
def test_chain_takes_two_repeats(eng, oracle, cases, variant, table_side, ids):
    """the massive overflow: more than 2,300 rows of one pass-1 digit on both sides against a region of 64"""
    case = cases("chain", variant, table_side)
    assert LC.expect(case.info) == ((2, 2, 2, 1, 1), (2, 2)) and LC.expect(case.info, True) == ((2, 2, 0, 1, 0), (2, 0))
    climb(eng, oracle, cases, case, ids, ALL)


# ---- the 16-byte entries: each of the eight phases once --------------------------------------------------------------------------------
def test_sixteen_byte_entries_on_one_overflow(eng, oracle, cases):
    """join_dev, semi_join_dev, outer_join_dev, join_sum_dev, join_mult_dev, lookup_dev, group_join_agg_ids_dev on the S+1 rung,
    group_agg_ids_dev and group_arg_dev -- which have no S -- on the R+1 rung"""
    two = ("pair", "semi", "outer_full", "join_sum", "mult_weighted", "lookup_last", "gjoin_left")
    climb(eng, oracle, cases, cases("rung", "one-unit", "S+1", 1), True, two, aos=True)
    climb(eng, oracle, cases, cases("rung", "one-unit", "R+1", 2), True, ("group_ids", "group_arg"), aos=True)


# ---- a rowID of 2^32 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("below", ["plain", "S+1", "R+1"])
@pytest.mark.parametrize("side", ["R", "S"])
def test_wide_rowid(eng, oracle, cases, side, below):
    """one rowID of 2^32 on a side, alone or beside an overflow of either side: the call ends at 16 bytes and reports (0, 0, 0, 2, 2);
    group_arg's rows hold 2^32 itself, not its truncation"""
    inner = ("plain",) if below == "plain" else ("rung", "one-unit", below, 0)
    case = cases("wide", side, *inner)
    assert LC.expect(case.info)[0] == (0, 0, 0, 2, 2)
    if side == "R":                                                        # (the oracle the rows are compared with names 2^32)
        rows = arg_oracle(case.valR, case.idR, [None], [ARG_ROW], [ARG_TIE_LAST])[3][0]
        assert int(rows.max()) == 1 << 32 and int(case.idR[case.info["wide_row"]]) == 1 << 32
    climb(eng, oracle, cases, case, True, WIDE[side])


@pytest.mark.parametrize("entry", ["join_sum", "mult_weighted", "group_arg_min"])
def test_wide_rowid_is_still_refused_where_it_indexes_a_column(eng, oracle, cases, entry):
    """the "row at col_rows" contract behind a narrow first attempt: the 16-byte repeat refuses the row with RHJ_E_INVALID, and the
    context goes on"""
    side = "S" if entry == "mult_weighted" else "R"
    case = cases("wide", side, "plain")
    f = Ladder(eng)
    with f, Run(f, oracle, case, True) as r, Run(f, oracle, cases("plain"), True, state=lambda one_sided=False: LC.expect(cases("plain").info, one_sided)[0]) as plain:
        dev, nR, nS = r.dev, r.nR, r.nS
        out = r.outputs(nR, 2)
        for _ in range(2):
            f.arm()
            with pytest.raises(RhjError) as err:
                if entry == "join_sum":
                    eng.join_sum_cols_dev(dev.vR, dev.iR, nR, dev.vS, nS, dev.cR[:1], nR, opts=f.plan)
                elif entry == "mult_weighted":
                    eng.join_mult_cols_dev(dev.vR, dev.iR, nR, dev.vS, dev.iS, nS, out.keys, nR, dev.cS[0], nS, opts=f.plan)
                else:
                    eng.group_arg_cols_dev(dev.vR, dev.iR, nR, [dev.cR[0]], [ARG_MIN_I64], [ARG_TIE_FIRST], nR, out.keys, out.counts,
                                           out.sums[:1], out.sums[1:], nR, opts=f.plan)
            assert err.value.code == RHJ_E_INVALID
            got = tuple(eng.info(k) for k in LC.STATE[:3])
            print(f"{entry}: refused, state {got}")
            assert got == (0, 0, 0)                                        # the refusal came from the 16-byte repeat
            out.read(0)                                                    # the guard words
            plain.run({"join_sum": "join_sum", "mult_weighted": "mult_weighted", "group_arg_min": "group_arg"}[entry])


# ---- the back-off: per context and per side, across operators --------------------------------------------------------------------------
BACKOFF = [("semi", ["group_ids", "pair", "group_arg", "lookup_first", "gjoin_inner", "mult"]),
           ("gjoin_left", ["mult", "group_agg_plain", "join_sum", "outer_full", "group_ids"]),
           ("lookup_last", ["outer_left", "anti", "gjoin_plain", "pair"]),
           ("outer_right", ["group_arg", "group_ids", "mult_weighted", "semi", "join_sum", "lookup_first"])]


def unarmed(eng, oracle, case, ids=True, state=None, path=None):
    """a Run that never sets an option (path: the plan of another path, whose options stay unset)"""
    f = Ladder(eng) if path is None else Forced(eng, path)
    return Run(f, oracle, case, ids, state=state, arm=False)


@pytest.mark.parametrize("first,then", BACKOFF, ids=[a for a, _ in BACKOFF])
def test_back_off_of_S_crosses_operators(eng, oracle, cases, first, then):
    """S+1 through one operator; then, never re-armed: an unpartitioned and a one-pass call (they consume nothing), and other operators
    on K.markers -- the first two two-sided ones run S with exact cursors, the next ones count-free again; the one-sided ones report
    R's word, 1, and leave S's back-off alone"""
    box = {}
    with unarmed(eng, oracle, cases("rung", "one-unit", "S+1", 0), state=lambda one_sided=False: (2, 1, 2, 1, 1)) as a, \
            unarmed(eng, oracle, cases("plain"), state=lambda one_sided=False: box["state"](one_sided)) as b, \
            unarmed(eng, oracle, cases("plain"), path="unpartitioned") as u, unarmed(eng, oracle, cases("plain"), path="one-pass") as o:
        Ladder(eng).arm()
        try:
            a.run(first)
            u.run("pair")
            u.run("semi")
            o.run("gjoin_inner")
            o.run("group_ids")
            left, met = 2, []
            for name in then:
                one = name in ONE_SIDED
                cf_S = 0 if one else (0 if left > 0 else 1)
                box["state"] = lambda one_sided=False, cf_S=cf_S: (2, 1, cf_S, 1, 0 if one_sided else 1)
                b.run(name)
                if not one:
                    left = max(left - 1, 0)
                    met.append(cf_S)
            assert met[:3] == [0, 0, 1] and all(m == 1 for m in met[2:])
        finally:
            for k in Ladder.OPTIONS:
                eng.set_option(k, -1)


def test_back_off_of_R_is_consumed_by_one_sided_operators_too(eng, oracle, cases):
    """R+1 through a group-by; then a join and a group-by run R with exact cursors, and the call behind them count-free"""
    box = {}
    with unarmed(eng, oracle, cases("rung", "one-unit", "R+1", 1), state=lambda one_sided=False: (2, 2, 0, 1, 0) if one_sided else None) as a, \
            unarmed(eng, oracle, cases("plain"), state=lambda one_sided=False: box["state"](one_sided)) as b:
        Ladder(eng).arm()
        try:
            a.run("group_arg")
            for name, cf_R in (("lookup_first", 0), ("group_ids", 0), ("group_arg", 1), ("semi", 1)):
                box["state"] = lambda one_sided=False, cf_R=cf_R: (2, cf_R, 0 if one_sided else 1, 1, 0 if one_sided else 1)
                b.run(name)
        finally:
            for k in Ladder.OPTIONS:
                eng.set_option(k, -1)


@pytest.mark.parametrize("entry", ["pair", "outer_full", "lookup_first", "mult", "gjoin_plain"])
def test_overflow_of_R_then_wide_id_of_S_arms_the_back_off_of_R(eng, oracle, cases, entry):
    """three partition phases in one call: R overflows in attempt 1, where the kernels of S return at once; the wide id of S shows in
    attempt 2; the call ends at 16 bytes.  R's back-off was armed on the way: the next two eligible calls report "last.countfree_R" 0.
    A plain wide id, and an overflow of S beside a wide id of R, arm nothing.  Setting "partition.countfree" clears the back-off."""
    box = {}
    plain_state = lambda one_sided=False: box["state"](one_sided)
    with unarmed(eng, oracle, cases("wide", "S", "rung", "one-unit", "R+1", 0), state=lambda one_sided=False: (0, 0, 0, 2, 2)) as a, \
            unarmed(eng, oracle, cases("wide", "S", "plain"), state=lambda one_sided=False: (0, 0, 0, 2, 2)) as w, \
            unarmed(eng, oracle, cases("plain"), state=plain_state) as b:
        assert LC.expect(a.case.info) == ((0, 0, 0, 2, 2), (2, 0)) and LC.expect(w.case.info) == ((0, 0, 0, 2, 2), (0, 0))
        f = Ladder(eng)
        f.arm()
        try:
            w.run(entry)                                                   # a plain wide id: nothing armed
            box["state"] = lambda one_sided=False: PLAIN_STATE
            b.run(entry)
            a.run(entry)                                                   # R+1, wide S
            box["state"] = lambda one_sided=False: (2, 0, 1, 1, 1)
            b.run(entry)
            b.run("semi")
            box["state"] = lambda one_sided=False: PLAIN_STATE
            b.run(entry)
            a.run(entry)                                                   # armed again ...
            f.arm()                                                        # ... and cleared by the option
            b.run(entry)
        finally:
            for k in Ladder.OPTIONS:
                eng.set_option(k, -1)


def test_overflow_of_S_beside_a_wide_id_of_R_arms_nothing(eng, oracle, cases):
    with unarmed(eng, oracle, cases("wide", "R", "rung", "one-unit", "S+1", 0), state=lambda one_sided=False: (0, 0, 0, 2, 2)) as a, \
            unarmed(eng, oracle, cases("plain"), state=lambda one_sided=False: PLAIN_STATE) as b:
        assert LC.expect(a.case.info) == ((0, 0, 0, 2, 2), (0, 0))
        Ladder(eng).arm()
        try:
            for entry in ("pair", "semi", "outer_left", "gjoin_plain"):
                a.run(entry)
                b.run(entry)
        finally:
            for k in Ladder.OPTIONS:
                eng.set_option(k, -1)
