"""The cases of tests/test_gpu_host_pipeline.py that drive rhj_join's PIPELINED host path (join_host_pipelined in
radixhashjoin_amd/csrc/rhj_api.hip) at the smallest sizes that reach it, and the child process that runs one of them.

A plain module: tests/test_pipeline_cases.py checks every case's preconditions with the CPU oracle alone (no GPU), and
tests/test_gpu_host_pipeline.py starts `python tests/pipeline_cases.py NAME` once per case, because the environment knobs
that shrink the path (RHJ_PIPE_MIN_CHUNK, RHJ_PIPE_CHUNKS) are read once per process.

Tuples are {key = rowID, payload = join value}; a pair is (rowID of R, rowID of S).  S rowIDs are positions (but for the one
wide rowID some cases plant), so the chunk an S tuple travels in is rowID // chunk.
"""
import functools
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TUPLE = np.dtype([("key", "<u8"), ("payload", "<u8")])
MIN_CHUNK = 65_536                   # the floor of RHJ_PIPE_MIN_CHUNK, which every child runs under
MAX_CHUNKS = 12                      # the default of RHJ_PIPE_CHUNKS
PAGE_SLACK = 1024                    # the optimistic result page holds max(nR, nS) + 1024 pairs
PAGE_MIN_BYTES = 64 << 20            # PagePrefault starts no page below this, and without a page nothing is pipelined
N_BIG = 4_193_280                    # the smallest max(nR, nS) with (max + 1024) * 16 >= 64 MiB
PLAN = (2, 8, 8)


# ---- the chunk arithmetic and the gates of join_host_pipelined, restated --------------------------------------------------
def geometry(nS, min_chunk=MIN_CHUNK, max_chunks=MAX_CHUNKS):
    """(K0, chunk, K, tuples in the last chunk): K0 = min(max_chunks, nS // min_chunk) chunks are asked for, a chunk is
    ceil(nS / K0) rounded up to a multiple of 4096 tuples, and K = ceil(nS / chunk) chunks come out"""
    k0 = min(max_chunks, nS // min_chunk)
    if k0 < 1:
        return 0, 0, 0, 0
    chunk = (-(-nS // k0) + 4095) // 4096 * 4096
    k = -(-nS // chunk)
    return k0, chunk, k, nS - (k - 1) * chunk


def gates(nR, nS, min_chunk=MIN_CHUNK):
    """the three conditions under which rhj_join pipelines at all"""
    return {"nS": nS >= 4 * min_chunk, "nR": nR >= min_chunk // 2, "page": page_pairs(nR, nS) * 16 >= PAGE_MIN_BYTES}


def chunks_of(nS, min_chunk=MIN_CHUNK, max_chunks=MAX_CHUNKS, nR=None):
    """what "last.pipelined" must report for a join that stays on the pipelined path: the number of S chunks, 0 when a gate
    keeps the join off the path (nR = None: R is taken to pass its gates)"""
    k0, _, k, _ = geometry(nS, min_chunk, max_chunks)
    if k0 < 2 or not all(gates(nS if nR is None else nR, nS, min_chunk).values()):
        return 0
    return k


def page_pairs(nR, nS):
    return max(nR, nS) + PAGE_SLACK


def count_class(count, nR, nS):
    """where a pair count stands relative to the optimistic page"""
    page = page_pairs(nR, nS)
    if count == 0:
        return "zero"
    if count < page:
        return "within"
    if count == page:
        return "full"
    if count == page + 1:
        return "one_over"
    return "well_over" if count >= 2 * page else "over"


# ---- join values ----------------------------------------------------------------------------------------------------------
def mix(x):
    """splitmix64's finaliser, a bijection of uint64: distinct k give distinct join values with no pattern in any bit"""
    with np.errstate(over="ignore"):
        z = np.asarray(x, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def val(k):
    """the join value of key number k (k < 2^40)"""
    return mix(np.asarray(k, dtype=np.uint64) + np.uint64(1))


def miss(k):
    """a join value no key number below 2^40 has"""
    return mix(np.asarray(k, dtype=np.uint64) + np.uint64(1 + (1 << 40)))


def rel(values):
    t = np.empty(len(values), dtype=TUPLE)
    t["key"] = np.arange(len(values), dtype=np.uint64)
    t["payload"] = values
    return t


def r_of(rng, nR, twice=0, copies=1):
    """(R, D): D distinct key numbers 0 .. D-1, each `copies` times, the first `twice` of them once more, in random order"""
    assert (nR - twice) % copies == 0
    d = (nR - twice) // copies
    k = np.concatenate([np.tile(np.arange(d, dtype=np.uint64), copies), np.arange(twice, dtype=np.uint64)])
    return rel(val(rng.permutation(k))), d


def chunk_slice(spec, i):
    _, chunk, k, _ = geometry(spec["nS"], MIN_CHUNK, spec["max_chunks"])
    i = i % k
    return slice(i * chunk, min((i + 1) * chunk, spec["nS"]))


# ---- builders: (spec, rng) -> (R, S) --------------------------------------------------------------------------------------
def b_fk(spec, rng):
    """foreign keys into R; spec: twice (R values that occur twice), miss_every (every n-th S value misses R)"""
    R, d = r_of(rng, spec["nR"], twice=spec.get("twice", 0))
    fk = rng.integers(0, d, spec["nS"], dtype=np.uint64)
    v = val(fk)
    if spec.get("miss_every"):
        v[:: spec["miss_every"]] = miss(fk[:: spec["miss_every"]])
    S = rel(v)
    if "wide" in spec:
        rowid, chunk_index = spec["wide"]
        S["key"][chunk_slice(spec, chunk_index).start + 1234] = rowid
    return R, S


def b_one_chunk_matches(spec, rng):
    """only the S tuples of chunk spec["match_chunks"][0] match R (each once); every other S value is disjoint from R"""
    R, d = r_of(rng, spec["nR"])
    fk = rng.integers(0, d, spec["nS"], dtype=np.uint64)
    v = miss(fk)
    sl = chunk_slice(spec, spec["match_chunks"][0])
    v[sl] = val(fk[sl])
    return R, rel(v)


def b_no_match(spec, rng):
    R, d = r_of(rng, spec["nR"])
    return R, rel(miss(rng.integers(0, d, spec["nS"], dtype=np.uint64)))


def b_skewed(spec, rng):
    """chunk spec["skew_chunk"] of S is one single value that R holds once (one partition, many probe tasks); the other
    chunks are Zipf(0.9) foreign keys: rank r (from 1) with probability ~ r^-0.9, ranks mapped to key numbers at random"""
    R, d = r_of(rng, spec["nR"])
    cdf = np.cumsum(np.arange(1, d + 1, dtype=np.float64) ** -0.9)
    rank = np.searchsorted(cdf, rng.random(spec["nS"]) * cdf[-1]).clip(0, d - 1)
    fk = rng.permutation(d).astype(np.uint64)[rank]
    fk[chunk_slice(spec, spec["skew_chunk"])] = fk[0]
    return R, rel(val(fk))


def b_page(spec, rng):
    """every S tuple is a foreign key into R, and exactly spec["first"] + spec["last"] of them, in the first and in the
    last chunk, reference the one R value that occurs twice: |R join S| = nS + first + last"""
    R, d = r_of(rng, spec["nR"], twice=1)
    fk = rng.integers(1, d, spec["nS"], dtype=np.uint64)
    for i, n in ((0, spec["first"]), (-1, spec["last"])):
        sl = chunk_slice(spec, i)
        fk[sl.start + rng.choice(sl.stop - sl.start, n, replace=False)] = 0
    return R, rel(val(fk))


def b_many(spec, rng):
    """every R value three times, every S tuple a foreign key: 3 * nS pairs"""
    R, d = r_of(rng, spec["nR"], copies=3)
    return R, rel(val(rng.integers(0, d, spec["nS"], dtype=np.uint64)))


# ---- the cases ------------------------------------------------------------------------------------------------------------
CASES = {}


def case(name, build, nR, nS, count, pipelined=True, plan=PLAN, narrow=2, last_narrow=None, max_chunks=MAX_CHUNKS, **more):
    """count: the count_class the oracle must find; pipelined: whether the join must stay on the pipelined path; narrow: the
    forced "partition.narrow" (these sizes never get the narrow format by themselves); last_narrow: "last.narrow" afterwards"""
    assert name not in CASES
    spec = dict(name=name, build=build, nR=nR, nS=nS, count=count, plan=plan, narrow=narrow, max_chunks=max_chunks,
                seed=1000 + len(CASES), **more)
    spec["last_narrow"] = (narrow if plan[0] == 2 else 0) if last_narrow is None else last_narrow
    spec["pipelined"] = chunks_of(nS, MIN_CHUNK, max_chunks, nR) if pipelined else 0
    spec["env"] = {"RHJ_PIPE_CHUNKS": str(max_chunks)} if max_chunks != MAX_CHUNKS else {}
    CASES[name] = spec


WIDE = (1 << 40) + 5
# -- must pipeline
for _n in (2, 1, 0):
    case(f"fk_S_large_narrow{_n}", b_fk, 300_000, N_BIG, "within", narrow=_n, twice=14_285, miss_every=7, seed_as="fk_S_large_narrow2")
case("fk_S_small", b_fk, N_BIG, 786_444, "within", geometry=(12, 69_632, 12, 20_492))
case("one_pass", b_fk, 300_000, N_BIG, "within", plan=(1, 8, 0), twice=14_285, miss_every=7)
case("max_chunks", b_fk, 300_000, N_BIG, "within", max_chunks=16, miss_every=7, geometry=(16, 262_144, 16, 261_120))
case("two_chunks", b_fk, 300_000, N_BIG, "within", max_chunks=2, miss_every=7, geometry=(2, 2_097_152, 2, 2_096_128))
case("matches_only_in_last_chunk", b_one_chunk_matches, 300_000, N_BIG, "within", match_chunks=[11])
case("matches_only_in_first_chunk", b_one_chunk_matches, 300_000, N_BIG, "within", match_chunks=[0])
case("skewed_chunk", b_skewed, 300_000, N_BIG, "within", skew_chunk=5)
case("wide_S_rowid_16_byte", b_fk, 300_000, N_BIG, "within", narrow=0, miss_every=7, wide=(WIDE, 3))
case("page_exactly_full", b_page, 300_000, N_BIG, "full", first=512, last=512)
# -- must leave the pipelined path
case("page_one_over_last", b_page, 300_000, N_BIG, "one_over", pipelined=False, first=512, last=513)
case("page_one_over_first", b_page, 300_000, N_BIG, "one_over", pipelined=False, first=513, last=512)
case("many_to_many", b_many, 300_000, N_BIG, "well_over", pipelined=False)
case("wide_S_rowid_narrow", b_fk, 300_000, N_BIG, "within", pipelined=False, last_narrow=0, miss_every=7, wide=((1 << 32) + 9, 2))
case("wide_S_rowid_narrow_original", b_fk, 300_000, N_BIG, "within", miss_every=7, seed_as="wide_S_rowid_narrow")
# -- the gates: (just outside, just inside)
case("gate_nS_below", b_fk, N_BIG, 4 * MIN_CHUNK - 1, "within", miss_every=7, gate="nS")
case("gate_nS_at", b_fk, N_BIG, 4 * MIN_CHUNK, "within", miss_every=7, gate="nS", geometry=(4, 65_536, 4, 65_536))
case("gate_nR_below", b_fk, MIN_CHUNK // 2 - 1, N_BIG, "within", miss_every=7, gate="nR")
case("gate_nR_at", b_fk, MIN_CHUNK // 2, N_BIG, "within", miss_every=7, gate="nR")
case("gate_page_below", b_fk, 300_000, N_BIG - 1, "within", miss_every=7, gate="page")
case("gate_page_at", b_fk, 300_000, N_BIG, "within", miss_every=7, gate="page", geometry=(12, 352_256, 12, 318_464))
# -- others
case("no_match_at_all", b_no_match, 300_000, N_BIG, "zero")
case("reuse_k4", b_fk, N_BIG + 500_000, 300_000, "within", miss_every=7, geometry=(4, 77_824, 4, 66_528))
case("reuse_plain", b_fk, 1_000_000, 1_000_000, "within", miss_every=7)
case("reuse_k12", b_fk, 300_000, N_BIG, "within", twice=14_285, miss_every=7)

GATE_PAIRS = [("gate_nS_below", "gate_nS_at"), ("gate_nR_below", "gate_nR_at"), ("gate_page_below", "gate_page_at")]

# what one child process runs, in order, on ONE context; a name that is not listed here runs alone
SEQUENCES = {
    "wide_S_rowid_narrow": ["wide_S_rowid_narrow", "wide_S_rowid_narrow_original"],          # the fall-back is per join
    "context_reuse": ["reuse_k4", "reuse_plain", "reuse_k12", "page_one_over_last", "reuse_k4"],
}
ONLY_IN_SEQUENCES = {"wide_S_rowid_narrow_original", "reuse_k4", "reuse_plain", "reuse_k12"}
RUNS = [n for n in CASES if n not in ONLY_IN_SEQUENCES] + ["context_reuse"]               # the children of the GPU test


def steps_of(run):
    return SEQUENCES.get(run, [run])


def env_of(run):
    env = {"RHJ_PIPE_MIN_CHUNK": str(MIN_CHUNK)}
    for name in steps_of(run):
        env.update(CASES[name]["env"])
    return env


@functools.lru_cache(maxsize=2)
def _build(name):
    spec = CASES[name]
    rng = np.random.default_rng(CASES[spec.get("seed_as", name)]["seed"])
    R, S = spec["build"](spec, rng)
    assert len(R) == spec["nR"] and len(S) == spec["nS"]
    return R, S


def build_case(name):
    """-> (R, S, opts, options, expect): the relations (deterministic: a fixed seed per case), the plan as the fields of
    rhj_opts (passes, bits1, bits2), the set_option calls to make first, and the case's entry of CASES -- which path must
    run ("pipelined": the chunks "last.pipelined" must report), "last_narrow", "plan", and the class of the pair count"""
    spec = CASES[name]
    R, S = _build(name)
    return R, S, spec["plan"], [("partition.narrow", spec["narrow"])], spec


# ---- the child ------------------------------------------------------------------------------------------------------------
def main(run):
    from oracle.pyoracle import Oracle, sorted_pairs
    from radixhashjoin_amd import Engine, Opts
    assert os.environ.get("RHJ_PIPE_MIN_CHUNK") == str(MIN_CHUNK), "the parent sets the knobs: they are read once per process"
    assert os.environ.get("RHJ_PIPE_CHUNKS", str(MAX_CHUNKS)) == env_of(run).get("RHJ_PIPE_CHUNKS", str(MAX_CHUNKS))
    oracle, engine, out, first = Oracle(), Engine(0), [], {}
    try:
        for name in steps_of(run):
            R, S, plan, options, expect = build_case(name)
            for option, value in options:
                engine.set_option(option, value)
            t0 = time.perf_counter()
            got = engine.join(R, S, Opts(*plan))
            t1 = time.perf_counter()
            info = {k: engine.info(k) for k in ("last.pipelined", "last.narrow", "last.join_kernel")}
            t = engine.timings()
            with ThreadPoolExecutor(1) as pool:              # (sorting releases the interpreter lock: both arrays at once)
                sorting = pool.submit(sorted_pairs, got)
                exp = first[name][0] if name in first else sorted_pairs(oracle.join(R, S))
                got = sorting.result()
            same = bool(np.array_equal(got, first[name][1])) if name in first else None     # the same join again on this context
            first.setdefault(name, (exp, got))
            step = {"case": name, "count": len(got), "oracle_count": len(exp), "equal": bool(np.array_equal(got, exp)),
                    "plan": [t["passes"], t["bits1"], t["bits2"]], "join_seconds": round(t1 - t0, 3), **info}
            if same is not None:
                step["same_as_first"] = same
            if "wide" in expect:
                step["wide_rowid_pairs"] = int(np.count_nonzero(got["keyS"] == np.uint64(expect["wide"][0])))
            out.append(step)
    finally:
        engine.close()
    print(json.dumps({**out[0], "run": run, "then": out[1:]}))


if __name__ == "__main__":
    main(sys.argv[1])
