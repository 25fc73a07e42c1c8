"""The cases of tests/pipeline_cases.py are what tests/test_gpu_host_pipeline.py says they are: every precondition a GPU case
relies on -- the pair count relative to the optimistic page, the chunk that holds the wide rowID, the chunks that hold matches,
the chunk geometry, the gates -- checked here with the CPU oracle and numpy alone, so that an edited builder cannot quietly turn
a case into a different case."""
import numpy as np
import pytest

import pipeline_cases as pc


def test_geometry_and_gates_restate_the_host_code():
    """the numbers DESIGN §7 and the issue quote, from the restated arithmetic"""
    assert pc.N_BIG == 64 * (1 << 20) // 16 - 1024                            # the smallest side whose page is 64 MiB
    assert pc.geometry(pc.N_BIG) == (12, 352_256, 12, 318_464)
    assert pc.geometry(786_444) == (12, 69_632, 12, 20_492)                  # the raggedest last chunk the 65 536 clamp allows
    assert pc.geometry(16 * 65_536 + 16, max_chunks=16)[2] == 16 and pc.geometry(pc.N_BIG, max_chunks=16)[2] == 16
    assert pc.geometry(pc.N_BIG, max_chunks=2)[2] == 2
    assert pc.geometry(40_000_000 - 1_234_567, 8 << 20)[2] == 4              # the sizes of the large tests, default knobs
    assert pc.geometry(65_535) == (0, 0, 0, 0)
    assert pc.chunks_of(pc.N_BIG, 65_536, 12, nR=300_000) == 12
    assert pc.chunks_of(pc.N_BIG, 65_536, 12, nR=32_767) == 0 and pc.chunks_of(pc.N_BIG, 65_536, 12, nR=32_768) == 12
    assert pc.chunks_of(262_143, 65_536, 12, nR=pc.N_BIG) == 0 and pc.chunks_of(262_144, 65_536, 12, nR=pc.N_BIG) == 4
    assert pc.chunks_of(pc.N_BIG - 1, 65_536, 12, nR=300_000) == 0
    assert pc.chunks_of(1_000_000, 65_536, 12, nR=1_000_000) == 0             # 16 MB page: the plain path
    assert pc.chunks_of(40_000_000, 8 << 20, 12) == 4


def test_the_runs_cover_every_case_once():
    in_runs = [name for run in pc.RUNS for name in pc.steps_of(run)]
    assert set(in_runs) == set(pc.CASES)
    assert pc.ONLY_IN_SEQUENCES == {n for n in pc.CASES if n not in pc.RUNS}
    for run in pc.RUNS:                                                        # one process, one value of each knob
        knobs = [pc.CASES[n]["env"] for n in pc.steps_of(run)]
        assert all(k == knobs[0] for k in knobs)
        assert pc.env_of(run)["RHJ_PIPE_MIN_CHUNK"] == "65536"
    assert pc.steps_of("context_reuse")[0] == pc.steps_of("context_reuse")[-1]
    k4, k12 = pc.CASES["reuse_k4"], pc.CASES["reuse_k12"]
    assert (k4["pipelined"], pc.CASES["reuse_plain"]["pipelined"], k12["pipelined"]) == (4, 0, 12)
    assert pc.page_pairs(k12["nR"], k12["nS"]) < pc.page_pairs(k4["nR"], k4["nS"])    # the pair buffer of join 1 is larger than join 3's page


@pytest.mark.parametrize("below, at", pc.GATE_PAIRS)
def test_gate_pairs_straddle_their_gate(below, at):
    b, a = pc.CASES[below], pc.CASES[at]
    gate = a["gate"]
    assert b["gate"] == gate
    gb, ga = pc.gates(b["nR"], b["nS"]), pc.gates(a["nR"], a["nS"])
    assert all(ga.values()) and not gb[gate] and all(v for k, v in gb.items() if k != gate)
    assert abs(a["nR"] - b["nR"]) + abs(a["nS"] - b["nS"]) == 1               # one tuple apart
    assert b["pipelined"] == 0 and a["pipelined"] == pc.geometry(a["nS"])[2] >= 2
    assert b["plan"] == a["plan"] == (2, 8, 8)


@pytest.mark.parametrize("name", list(pc.CASES))
def test_case_preconditions(name, oracle):
    R, S, plan, options, expect = pc.build_case(name)
    nR, nS = len(R), len(S)
    assert (nR, nS) == (expect["nR"], expect["nS"]) and plan == expect["plan"]
    assert options == [("partition.narrow", expect["narrow"])]
    k0, chunk, K, last = pc.geometry(nS, pc.MIN_CHUNK, expect["max_chunks"])
    if "geometry" in expect:
        assert (k0, chunk, K, last) == expect["geometry"]
    # the path: only a gate, an overfull page or a wide rowID in the narrow format takes a join off the pipelined path
    wide_in_narrow = "wide" in expect and expect["narrow"] > 0 and plan[0] == 2
    stays = all(pc.gates(nR, nS).values()) and expect["count"] in ("within", "full", "zero") and not wide_in_narrow
    assert expect["pipelined"] == (K if stays else 0)
    assert expect["last_narrow"] == (0 if plan[0] != 2 or wide_in_narrow else expect["narrow"])
    # the pair count, from the oracle
    count, _ = oracle.join_count_checksum(R, S)
    assert pc.count_class(count, nR, nS) == expect["count"], (count, pc.page_pairs(nR, nS))
    # rowIDs: positions, but for the one wide rowID, which sits in the chunk the case names and in a pair
    ids = np.arange(nS, dtype=np.uint64)
    assert np.array_equal(R["key"], np.arange(nR, dtype=np.uint64))
    hit = np.isin(S["payload"], R["payload"])
    if "wide" in expect:
        rowid, chunk_index = expect["wide"]
        at = np.flatnonzero(S["key"] != ids)
        assert len(at) == 1 and S["key"][at[0]] == rowid >= 1 << 32 and at[0] // chunk == chunk_index >= 1 and hit[at[0]]
    else:
        assert np.array_equal(S["key"], ids)
    # which chunks hold matches
    with_matches = sorted(set((np.flatnonzero(hit) // max(chunk, 1)).tolist()))
    if expect["count"] == "zero":
        assert with_matches == []
    elif "match_chunks" in expect:
        assert with_matches == expect["match_chunks"] and (with_matches[0] in (0, K - 1))
    elif K:
        assert with_matches == list(range(K))
    if "skew_chunk" in expect:                               # one value, held once by R, fills the chunk
        v = np.unique(S["payload"][pc.chunk_slice(expect, expect["skew_chunk"])])
        assert len(v) == 1 and np.count_nonzero(R["payload"] == v[0]) == 1
        assert len(np.unique(R["payload"])) == nR and hit.all()
    if "first" in expect:                                    # the page cases: every S tuple a foreign key, `first` + `last` of them to the R value held twice
        vals, n = np.unique(R["payload"], return_counts=True)
        assert hit.all() and np.count_nonzero(n == 2) == 1 and n.max() == 2
        to_twice = np.flatnonzero(S["payload"] == vals[n == 2][0]) // chunk
        assert (np.count_nonzero(to_twice == 0), np.count_nonzero(to_twice == K - 1)) == (expect["first"], expect["last"])
        assert len(to_twice) == expect["first"] + expect["last"] == count - nS
    if expect.get("twice"):                                  # 5 % of R's values appear twice
        _, n = np.unique(R["payload"], return_counts=True)
        assert np.count_nonzero(n == 2) == expect["twice"] and abs(expect["twice"] / len(n) - 0.05) < 1e-4
    if expect.get("miss_every"):
        assert not hit[:: expect["miss_every"]].any() and np.count_nonzero(hit) == nS - len(hit[:: expect["miss_every"]])
    if name == "many_to_many":
        assert count == 3 * nS


def test_same_inputs_where_the_cases_say_so():
    for a, b in (("fk_S_large_narrow2", "fk_S_large_narrow0"), ("fk_S_large_narrow2", "fk_S_large_narrow1")):
        (Ra, Sa, *_), (Rb, Sb, *_) = pc.build_case(a), pc.build_case(b)
        assert np.array_equal(Ra, Rb) and np.array_equal(Sa, Sb)
    Rw, Sw, *_ = pc.build_case("wide_S_rowid_narrow")
    Ro, So, *_ = pc.build_case("wide_S_rowid_narrow_original")
    assert np.array_equal(Rw, Ro) and np.array_equal(Sw["payload"], So["payload"])
    assert np.count_nonzero(Sw["key"] != So["key"]) == 1
