#!/usr/bin/env python3
"""Generates tests/golden/g1_bytes_vectors.json: compressed G1 points (ZCash's 48 bytes on bls12_381, gnark's 32 on
bn254) with their affine coordinates, and one blob per way a decompression can fail, from kzg_snark_amd/curve.py's
single-point helpers alone (seeded; data, not code).

    python tests/golden/make_g1_bytes_golden.py

Per curve:
  points     [k] G and -[k] G for a dozen k: {"k", "blob", "x", "y"}; both signs of y occur
  infinity   the blob of the point at infinity
  status1    malformed blobs, one per sub-case: {"case", "blob"}
  status2    well-formed blobs whose x has no point (x^3 + b is not a square), both sign flags
  status3    bls12_381 only: points of the curve outside the subgroup of prime order -- cofactor-torsion points
             T = [r] Q of random points Q of the curve, sums P + T with P in G1, and the point (0, 2) of order 3 --
             {"case", "blob", "x", "y"}: they decompress (status 0) without the subgroup check
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from kzg_snark_amd import curve as C  # noqa: E402


def random_curve_point(cv, rng):
    while True:
        x = rng.randrange(cv.p)
        y = C.sqrt_fp((x * x * x + cv.b) % cv.p, cv.p)
        if y is not None:
            return (x, y if rng.randrange(2) else cv.p - y, 1)


def with_flags(x, flags, cv):
    size = C.g1_compressed_size(cv)
    bits = 3 if cv.name == "bls12_381" else 2
    return ((flags << (8 * size - bits)) | x).to_bytes(size, "big").hex()


def vectors(cv, rng):
    G = C.g1_group(cv)
    g = (cv.g1[0], cv.g1[1], 1)
    bls = cv.name == "bls12_381"
    fin_small, fin_large, inf_flags = (4, 5, 6) if bls else (2, 3, 1)
    out = {"size": C.g1_compressed_size(cv), "points": [], "status1": [], "status2": [], "status3": []}
    for k in [1, 2, 3, 5, 7, 0xffff, cv.r - 1, cv.r - 2] + [rng.randrange(cv.r) for _ in range(4)]:
        pt = G.multiply(g, k)
        for q in (pt, G.neg(pt)) if k < 8 else (pt,):
            out["points"].append({"k": hex(k), "neg": q is not pt, "blob": C.compress_g1(q, cv).hex(), "x": hex(q[0]),
                                  "y": hex(q[1])})
    assert {int(p["y"], 16) > (cv.p - 1) // 2 for p in out["points"]} == {True, False}
    out["infinity"] = C.compress_g1(G.Z, cv).hex()
    x_good = g[0]
    # x >= p that would ALSO be a non-residue: the first failure (bad encoding) wins
    x_big = next(x for x in range(cv.p, cv.p + 64) if C.sqrt_fp((x ** 3 + cv.b) % cv.p, cv.p) is None)
    assert x_big.bit_length() <= cv.p.bit_length()
    s1 = [("infinity with a stray low bit", with_flags(1, inf_flags, cv)),
          ("infinity with a stray high bit", with_flags(1 << (cv.p.bit_length() - 1), inf_flags, cv)),
          ("x = p", with_flags(cv.p, fin_small, cv)),
          ("x >= p and x^3 + b not a square", with_flags(x_big, fin_large, cv)),
          ("x all ones", with_flags((1 << (8 * out["size"] - (3 if bls else 2))) - 1, fin_small, cv))]
    if bls:
        s1 += [("compressed bit clear", with_flags(x_good, 0, cv)),
               ("compressed bit clear, sign set", with_flags(x_good, 1, cv)),
               ("uncompressed infinity flag", with_flags(0, 2, cv)),
               ("infinity with the sign bit", with_flags(0, 7, cv))]
    else:
        s1 += [("flags 00", with_flags(x_good, 0, cv)), ("all zero", with_flags(0, 0, cv))]
    out["status1"] = [{"case": c, "blob": b} for c, b in s1]
    while len(out["status2"]) < 4:
        x = rng.randrange(cv.p)
        if C.sqrt_fp((x ** 3 + cv.b) % cv.p, cv.p) is None:
            out["status2"].append({"case": "x^3 + b not a square", "blob": with_flags(x, fin_large if len(out["status2"]) & 1 else fin_small, cv)})
    if bls:
        def entry(case, pt):
            assert C.on_curve_g1(pt, cv) and not C.in_subgroup_g1(pt, cv)
            return {"case": case, "blob": C.compress_g1(pt, cv).hex(), "x": hex(pt[0]), "y": hex(pt[1])}
        for i in range(3):
            q = random_curve_point(cv, rng)
            t = G.multiply(q, cv.r)
            assert t[2] == 1
            out["status3"].append(entry(f"random point of the curve {i}", q))
            out["status3"].append(entry(f"its cofactor-torsion part [r] Q {i}", t))
            out["status3"].append(entry(f"P + T {i}", G.add(G.multiply(g, rng.randrange(1, cv.r)), t)))
        out["status3"].append(entry("the point (0, 2) of order 3", (0, 2, 1)))
    # every vector is what the helpers say it is
    for p in out["points"]:
        assert C.decompress_g1_status(bytes.fromhex(p["blob"]), cv) == ((int(p["x"], 16), int(p["y"], 16), 1), 0)
    for want, key in ((1, "status1"), (2, "status2"), (3, "status3")):
        for e in out[key]:
            assert C.decompress_g1_status(bytes.fromhex(e["blob"]), cv)[1] == want, e
    return out


if __name__ == "__main__":
    rng = random.Random(0x67316279)
    data = {name: vectors(C.CURVES[name], rng) for name in ("bls12_381", "bn254")}
    data["pins"] = {"bls12_381_generator": "97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac58"
                                           "6c55e83ff97a1aeffb3af00adb22c6bb",
                    "bls12_381_infinity": "c0" + "00" * 47}
    path = os.path.join(HERE, "g1_bytes_vectors.json")
    with open(path, "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")
