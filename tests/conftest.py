import atexit
import functools
import json
import os
import re
import shutil
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "slow: long-running CPU test, skipped unless RHJ_SLOW=1")


def pytest_sessionstart(session):
    """Built artefacts are git-ignored: if this checkout has not been built yet, build it (hipcc cross-compiles
    gfx950 without a GPU; the oracle needs only gcc)."""
    need = [os.path.join(ROOT, "radixhashjoin_amd", "librhj_hip.so"), os.path.join(ROOT, "oracle", "liborc.so"),
            os.path.join(ROOT, "radixhashjoin_amd", "host", "join_gpu"),
            os.path.join(ROOT, "radixhashjoin_amd", "host", "host_driver"),
            os.path.join(ROOT, "radixhashjoin_amd", "host", "query_unit"),
            os.path.join(ROOT, "radixhashjoin_amd", "host", "sharded_host")]
    if not all(os.path.exists(p) for p in need):
        import __graft_entry__
        __graft_entry__.build()


def pytest_collection_modifyitems(config, items):
    if os.environ.get("RHJ_SLOW") == "1":
        return
    skip = pytest.mark.skip(reason="set RHJ_SLOW=1 to run")
    for it in items:
        if "slow" in it.keywords:
            it.add_marker(skip)


@pytest.fixture(scope="session")
def oracle():
    """The CPU restatement (oracle/rhj_oracle.c) -- the checker, never the thing under test on GPU."""
    from oracle.pyoracle import Oracle
    return Oracle()


@pytest.fixture(scope="session")
def reference():
    """The real reference compiled into oracle/_ref (present in the build container and, as a
    prebuilt binary, on the GPU box); tests that need it skip when it is absent."""
    from oracle.pyoracle import Reference, ref_available
    if not ref_available():
        pytest.skip("oracle/_ref/libref_rhj.so not built")
    return Reference()


@pytest.fixture(scope="session")
def synthetic_golden():
    with open(os.path.join(GOLDEN, "synthetic.json")) as f:
        return json.load(f)


@pytest.fixture(scope="session")
def small_joins():
    with open(os.path.join(GOLDEN, "small_joins.json")) as f:
        meta = json.load(f)["calls"]
    return meta, load_npz_parts("small_joins")


# A committed file stays within 1 MiB: larger fixtures are stored in parts, <name>.part0, <name>.part1, ... (byte ranges of
# a relation file; disjoint sets of arrays of an .npz), and put back together here.
PART = re.compile(r"(.+)\.part(\d+)(\.npz)?$")


def load_npz_parts(stem):
    """{array name: array} of tests/golden/<stem>.part<k>.npz"""
    parts = sorted((int(m.group(2)), f) for f in os.listdir(GOLDEN) for m in [PART.match(f)]
                   if m and m.group(1) == stem and m.group(3))
    assert parts and [k for k, _ in parts] == list(range(len(parts))), stem
    out = {}
    for _, f in parts:
        with np.load(os.path.join(GOLDEN, f)) as z:
            out.update({k: z[k] for k in z.files})
    return out


@functools.lru_cache(maxsize=None)
def golden_workdir():
    """working directory for the binaries that read the golden workloads (`small/rN`, `edge/eN` relative to it): a
    temporary copy of tests/golden/small and tests/golden/edge with every relation file whole again, removed at exit"""
    d = tempfile.mkdtemp(prefix="rhj_golden_")
    atexit.register(shutil.rmtree, d, True)
    for sub in ("small", "edge"):
        src, dst = os.path.join(GOLDEN, sub), os.path.join(d, sub)
        os.makedirs(dst)
        parts = {}
        for f in sorted(os.listdir(src)):
            m = PART.match(f)
            if m:
                parts.setdefault(m.group(1), []).append((int(m.group(2)), f))
            else:
                shutil.copyfile(os.path.join(src, f), os.path.join(dst, f))
        for name, ps in parts.items():
            assert [k for k, _ in sorted(ps)] == list(range(len(ps))), name
            with open(os.path.join(dst, name), "wb") as out:
                for _, f in sorted(ps):
                    with open(os.path.join(src, f), "rb") as part:
                        out.write(part.read())
    return d


@pytest.fixture(scope="session")
def tiny_vectors():
    return np.load(os.path.join(GOLDEN, "tiny_vectors.npz"))


@pytest.fixture(scope="session")
def engine():
    """One rhj_ctx on cuda:0 through the C-ABI.  Fails loudly if the HIP library is missing."""
    from radixhashjoin_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def make_inputs(o, spec):
    """inputs of a tests/golden/synthetic.json case (generators of SURVEY.md App. A)"""
    if spec["S"] == "const":
        return o.gen_const(spec["nR"], spec["value"]), o.gen_const(spec["nS"], spec["value"])
    R = o.gen_R(spec["nR"], spec["D"])
    if spec["S"] == "chain":
        return R, o.gen_S_chain(spec["nS"], spec["D"])
    if spec["S"] == "disjoint":
        return R, o.gen_S_disjoint(spec["nS"], spec["D"])
    raise ValueError(spec["S"])


@pytest.fixture(scope="session")
def reference_recorded():
    """what the real reference returned for the inputs of test_oracle.py's *_vs_reference tests
    (tests/golden/make_reference_recorded.py): checked everywhere, also where oracle/_ref is not built"""
    with open(os.path.join(GOLDEN, "reference_recorded.json")) as f:
        return json.load(f)


def digest(a):
    """sha256 of an array's bytes (reference_recorded.json stores digests, not the arrays)"""
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


NEXT_PRIME_XS = list(range(0, 2000)) + [4095, 4096, 65535, 65536, 10**6, 10**6 + 3]
HASH_RELATION_NS = [0, 1, 7, 8, 9, 1000, 100003]


def random_join_trials(seed=7, trials=40):
    """(R, S) of test_random_joins_vs_reference: sizes below 3000, join-value domains from 1 to 2^62"""
    from oracle.pyoracle import TUPLE
    rng = np.random.default_rng(seed)
    for _ in range(trials):
        nR, nS = int(rng.integers(0, 3000)), int(rng.integers(0, 3000))
        dom = int(rng.choice([1, 3, 50, 1000, 1 << 20, 1 << 62]))
        R = np.empty(nR, dtype=TUPLE); S = np.empty(nS, dtype=TUPLE)
        R["key"] = rng.permutation(nR); S["key"] = rng.permutation(nS)
        R["payload"] = rng.integers(0, dom, nR, dtype=np.uint64); S["payload"] = rng.integers(0, dom, nS, dtype=np.uint64)
        yield R, S


def small_call_arrays(npz, i):
    from oracle.pyoracle import PAIR, TUPLE
    def tup(tag, a, b, dt):
        x = np.empty(len(npz[f"call{i}__{tag}_{a}"]), dtype=dt)
        x[a] = npz[f"call{i}__{tag}_{a}"]
        x[b] = npz[f"call{i}__{tag}_{b}"]
        return x
    return tup("R", "key", "payload", TUPLE), tup("S", "key", "payload", TUPLE), tup("P", "keyR", "keyS", PAIR)
