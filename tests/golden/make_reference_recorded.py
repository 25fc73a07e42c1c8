#!/usr/bin/env python3
"""Generate tests/golden/reference_recorded.json from the REAL reference (oracle/_ref/libref_rhj.so, built by
oracle/Makefile where the reference checkout is present):

    make -C oracle liborc.so ref
    python tests/golden/make_reference_recorded.py

For the exact inputs of tests/test_oracle.py's *_vs_reference tests it records what the reference returns: next_prime
values, sha256 digests of the hash_relation / single_partition outputs, and per random join the count, head_null and
the sha256 of the pairs in the reference's page order.  Data only; the tests compare the oracle against it.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
from conftest import HASH_RELATION_NS, NEXT_PRIME_XS, digest, random_join_trials  # noqa: E402
from oracle.pyoracle import Oracle, Reference, ref_available  # noqa: E402


def main():
    if not ref_available():
        raise SystemExit("oracle/_ref/libref_rhj.so not built (make -C oracle ref, with the reference checkout present)")
    o, ref = Oracle(), Reference()
    out = {"source": "oracle/_ref/libref_rhj.so (the reference's own Result.cpp / structs.cpp / auxFun.cpp)",
           "next_prime": [[x, int(ref.next_prime(x))] for x in NEXT_PRIME_XS], "hash_relation": {}, "random_joins": []}
    for n in HASH_RELATION_NS:
        R = o.gen_R(n, max(n // 3, 1))
        b, hb = ref.hash_relation(R)
        c, hc = ref.single_partition(R)
        out["hash_relation"][str(n)] = {"hash_relation": [digest(b), digest(hb)], "single_partition": [digest(c), digest(hc)]}
    for R, S in random_join_trials():
        pr, cnt, head_null, _ = ref.join(R, S)
        out["random_joins"].append({"nR": len(R), "nS": len(S), "count": int(cnt), "head_null": bool(head_null),
                                    "pairs_sha256": digest(pr)})
    with open(os.path.join(HERE, "reference_recorded.json"), "w") as f:      # one line per key / per record
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: " + (json.dumps(v) if k != "random_joins" else
                                     "[\n" + ",\n".join("  " + json.dumps(r) for r in v) + "\n ]") for k, v in out.items()) + "\n}\n")


if __name__ == "__main__":
    main()
