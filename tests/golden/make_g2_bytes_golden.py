#!/usr/bin/env python3
"""Writes g2_bytes_vectors.json, the golden vectors of the compressed-G2 tests, from kzg_snark_amd/curve.py's
single-point helpers.  Run from the repository root:  python tests/golden/make_g2_bytes_golden.py"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from kzg_snark_amd import curve as C          # noqa: E402

# independent of this code base: the published compressed generator of BLS12-381's G2
BLS_G2_GENERATOR = ("93e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e"
                    "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8")


def entry(pt, cv, **more):
    d = {"x0": hex(pt[0][0]), "x1": hex(pt[0][1]), "y0": hex(pt[1][0]), "y1": hex(pt[1][1]),
         "blob": C.compress_g2(pt, cv).hex()}
    d.update(more)
    return d


def rhs(x, cv):
    K = C._Fp2(cv.p)
    return K.add(K.mul(K.mul(x, x), x), cv.b2)


def real_rhs_points(cv, want=2):
    """points whose x^3 + b' lies in Fp: for x = x0 + x1 i the imaginary part 3 x0^2 x1 - x1^3 + b'.c1 vanishes when
    x0^2 = (x1^3 - b'.c1) / (3 x1); walk x1 = 1, 2, ... and keep those for which that is a residue, until `want` of
    each kind (the real part a residue of Fp: a real y; a non-residue: a purely imaginary y) are found"""
    p, out, kinds = cv.p, [], {"residue": 0, "non-residue": 0}
    x1 = 0
    while min(kinds.values()) < want:
        x1 += 1
        x0 = C.sqrt_fp((x1 ** 3 - cv.b2[1]) * pow(3 * x1, -1, p) % p, p)
        if x0 is None:
            continue
        a = rhs((x0, x1), cv)
        assert a[1] == 0
        kind = "residue" if C.sqrt_fp(a[0], p) is not None else "non-residue"
        if kinds[kind] >= want:
            continue
        y = C.sqrt_fp2(a, p)
        assert (y[1] == 0) == (kind == "residue") and (y[0] == 0) == (kind == "non-residue")
        if kinds[kind] % 2:
            y = C._Fp2(p).neg(y)
        kinds[kind] += 1
        out.append(entry(((x0, x1), y, (1, 0)), cv, kind=kind))
    return out


def build(cv):
    p = cv.p
    G = C.g2_group(cv)
    K = C._Fp2(p)
    g = (cv.g2[0], cv.g2[1], (1, 0))
    rng = random.Random(0x92 + len(cv.name))
    size = C.g2_compressed_size(cv)
    half = size // 2
    bls = cv.name == "bls12_381"
    pts = [g, G.neg(g)] + [G.multiply(g, rng.randrange(1, cv.r)) for _ in range(6)]
    # eight points of G2 under "points"; a point whose y has y.c1 = 0 (the second arm of "larger") cannot be had in G2 by
    # search, so those are points of the twist under "real_rhs" (status 0 without the subgroup check, 3 with it)
    real = real_rhs_points(cv)
    points = [entry(q, cv) for q in pts]
    assert {C._fp2_larger(q[1], p) for q in pts} == {True, False}
    finite = 0x80                                            # finite, the smaller y, in either format
    out = {"points": points, "infinity": C.compress_g2(G.Z, cv).hex(), "real_rhs": real}
    gen_blob = bytearray(C.compress_g2(g, cv))
    no_root = None
    x = 1
    while no_root is None:                                   # an x = (x, 0) with no point above it
        x += 1
        if C.sqrt_fp2(rhs((x, 0), cv), p) is None:
            no_root = x
    s1 = []
    b = bytearray(gen_blob); b[0] &= 0x1f if bls else 0x3f
    s1.append({"case": "top bits 00 (compressed bit clear)", "blob": bytes(b).hex()})
    if bls:
        b = bytearray(gen_blob); b[0] = (b[0] & 0x1f) | 0x20
        s1.append({"case": "compressed bit clear, sign bit set", "blob": bytes(b).hex()})
        b = bytearray(size); b[0] = 0xe0
        s1.append({"case": "infinity with the sign bit", "blob": bytes(b).hex()})
    b = bytearray(size); b[0] = 0xc0 if bls else 0x40; b[size - 1] = 1
    s1.append({"case": "infinity with a stray bit in x.c0", "blob": bytes(b).hex()})
    b = bytearray(size); b[0] = 0xc0 if bls else 0x40; b[half - 1] = 1
    s1.append({"case": "infinity with a stray bit in x.c1", "blob": bytes(b).hex()})
    b = bytearray(p.to_bytes(half, "big") + (1).to_bytes(half, "big")); b[0] |= finite
    s1.append({"case": "x.c1 = p", "blob": bytes(b).hex()})
    b = bytearray((1).to_bytes(half, "big") + p.to_bytes(half, "big")); b[0] |= finite
    s1.append({"case": "x.c0 = p", "blob": bytes(b).hex()})
    b = bytearray((0).to_bytes(half, "big") + (p + no_root).to_bytes(half, "big")); b[0] |= finite
    assert p + no_root < 1 << (8 * half)
    s1.append({"case": "x.c0 = p + %d: not below p, and no root either (first failure wins)" % no_root, "blob": bytes(b).hex()})
    b = bytearray((0).to_bytes(half, "big") + no_root.to_bytes(half, "big"))
    s1.append({"case": "top bits 00 on an x with no root (first failure wins)", "blob": bytes(b).hex()})
    s2 = []
    for larger in (False, True):
        b = bytearray((0).to_bytes(half, "big") + no_root.to_bytes(half, "big"))
        b[0] |= (0x80 | (0x20 if larger else 0)) if bls else (0xc0 if larger else 0x80)
        s2.append({"case": "x = %d: x^3 + b' is not a square" % no_root, "blob": bytes(b).hex()})
    while len(s2) < 4:
        x = (rng.randrange(p), rng.randrange(p))
        if C.sqrt_fp2(rhs(x, cv), p) is None:
            b = bytearray(x[1].to_bytes(half, "big") + x[0].to_bytes(half, "big")); b[0] |= finite
            s2.append({"case": "random x with no root", "blob": bytes(b).hex()})
    s3 = []
    while len(s3) < 3:
        x = (rng.randrange(p), rng.randrange(p))
        y = C.sqrt_fp2(rhs(x, cv), p)
        if y is None:
            continue
        q = (x, y, (1, 0))
        t = G.multiply(q, cv.r)
        assert t[2] == (1, 0)
        for pt, what in ((q, "a random point of the twist"), (t, "its cofactor part [r] Q"),
                         (G.add(G.multiply(g, rng.randrange(1, cv.r)), t), "P + [r] Q, P in G2")):
            assert not C.in_subgroup_g2(pt, cv)
            s3.append({"case": what, "blob": C.compress_g2(pt, cv).hex()})
    for e in real:                                           # the special branches of the root, off the subgroup too
        pt = ((int(e["x0"], 16), int(e["x1"], 16)), (int(e["y0"], 16), int(e["y1"], 16)), (1, 0))
        assert C.on_curve_g2(pt, cv) and not C.in_subgroup_g2(pt, cv)
        s3.append({"case": "x^3 + b' in Fp, a %s: %s y" % (e["kind"], "real" if e["kind"] == "residue" else "imaginary"),
                   "blob": e["blob"]})
    out.update(status1=s1, status2=s2, status3=s3)
    for st, lst in ((1, s1), (2, s2), (3, s3)):
        for e in lst:
            assert C.decompress_g2_status(bytes.fromhex(e["blob"]), cv) == (None, st), e["case"]
    for e in points:
        assert C.decompress_g2_status(bytes.fromhex(e["blob"]), cv)[1] == 0
    return out


def main():
    doc = {"pins": {"bls12_381_g2_generator": BLS_G2_GENERATOR}, "bn254": build(C.BN254), "bls12_381": build(C.BLS12_381)}
    assert doc["bls12_381"]["points"][0]["blob"] == BLS_G2_GENERATOR
    with open(os.path.join(HERE, "g2_bytes_vectors.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
