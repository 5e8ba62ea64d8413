"""Writes cut_weight_vectors.json (tests/test_cut_weight_gpu.py) from the pure-Python oracle, no GPU:

    python tests/golden/make_cut_weight_golden.py

BLS12-381 only -- the one base field whose multiplier columns are cut (csrc/field.h).  A 64-coefficient commitment
and every FK20 proof of one polynomial on the domains of 2 and 8 points, all in the trapdoor form (p(tau) G1 and
((p(tau) - p(z)) / (tau - z)) G1), which needs no key."""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import py_oracle as O  # noqa: E402

CURVE = "bls12_381"
TAU = 0x1f2e3d4c5b6a79880123456789abcdef0fedcba987654321


def pt(p):
    return None if p is None else [hex(p[0]), hex(p[1])]


def main():
    cv = O.curve(CURVE)
    rng = random.Random(0xc07)
    coeffs = [rng.randrange(cv.r) for _ in range(64)]
    out = {"curve": CURVE, "tau": hex(TAU),
           "commit": {"coeffs": [hex(c) for c in coeffs],
                      "commitment": pt(O.normalize(O.commit_trapdoor(coeffs, TAU, cv), cv))},
           "open_domain": []}
    for log_n in (1, 3):
        n = 1 << log_n
        w = cv.root_of_unity(n)
        p = [rng.randrange(cv.r) for _ in range(n)]
        proofs = [pt(O.normalize(O.open_trapdoor([p], pow(w, i, cv.r), 1, TAU, cv), cv)) for i in range(n)]
        out["open_domain"].append({"log_n": log_n, "w": hex(w), "coeffs": [hex(c) for c in p], "proofs": proofs})
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "cut_weight_vectors.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
