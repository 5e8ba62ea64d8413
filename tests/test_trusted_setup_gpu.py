"""GPU tests of trusted-setup files (KZG.save_trusted_setup / load_trusted_setup / check_key): n1 = 64
G1 points in both bases and n2 = 9 G2 powers, on both curves.  Expected points come from setup / setup_lagrange /
setup_g2 with the same tau, expected bytes from curve.py's compression."""
import random

import numpy as np
import pytest

from g2_bytes_cases import subgroup_matrix_g2
from kzg_snark_amd import curve as C

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
TAU = 0x7a11_5eed_0bad_cafe_1234_5678_9abc
N1, N2 = 64, 9
FIXED_R = 0x1f2e3d4c5b6a79880123456789abcdef


@pytest.fixture(scope="module")
def kzgs():
    from kzg_snark_amd.kzg import KZG
    return {c: KZG(c) for c in CURVES}


class Honest:
    def __init__(self, kzg, tmp):
        self.kzg = kzg
        self.ck = kzg.setup(N1 - 1, tau=TAU)[0]
        self.lk = kzg.setup_lagrange(N1, tau=TAU)[0]
        self.g2 = kzg.setup_g2(N2, TAU)
        self.mono, self.lag = list(self.ck), list(self.lk)
        self.path = str(tmp / f"{kzg.curve_type}.txt")
        kzg.save_trusted_setup(self.path, self.ck, self.g2)
        self.lines = open(self.path).read().splitlines()

    def write(self, tmp_path, lines, name="edited.txt"):
        path = str(tmp_path / name)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        return path


@pytest.fixture(scope="module")
def honest(kzgs, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("setup")
    return {c: Honest(kzgs[c], tmp) for c in CURVES}


@pytest.mark.parametrize("curve", CURVES)
def test_save_then_load(kzgs, honest, curve):
    kzg, h = kzgs[curve], honest[curve]
    cv = kzg._cv
    assert h.g2[0] == kzg.G2 and h.g2[1] == kzg.multiply(kzg.G2, TAU) and len(h.g2) == N2
    want = ([str(N1), str(N2)] + [C.compress_g1(p, cv).hex() for p in h.lag] + [C.compress_g2(q, cv).hex() for q in h.g2]
            + [C.compress_g1(p, cv).hex() for p in h.mono])
    assert h.lines == want
    for r in (FIXED_R, None):
        ts = kzg.load_trusted_setup(h.path, r=r)
        assert list(ts.monomial) == h.mono and list(ts.lagrange) == h.lag and ts.g2 == h.g2
        assert ts.lagrange.n == N1 and ts.lagrange.w == h.lk.w
        assert ts.rk == h.g2[1] and ts.rk_l(4) == h.g2[4] == kzg.coset_verification_key(4, TAU)
        with pytest.raises(ValueError, match="9 G2 powers"):
            ts.rk_l(16)
        assert kzg.check_key(ts.monomial, ts.g2, ts.lagrange, r=r) is True
        assert kzg.check_key(ts.monomial, ts.g2, r=r) is True
    assert kzg.check_key(h.mono, h.g2) is True                                    # a key as a list of points
    assert kzg.check_key(h.ck, h.g2[:2], h.lk) is True


@pytest.mark.parametrize("curve", CURVES)
def test_check_key_rejects_every_broken_setup(kzgs, honest, curve, tmp_path):
    kzg, h = kzgs[curve], honest[curve]
    cv = kzg._cv
    lag0, g20, mono0 = 2, 2 + N1, 2 + N1 + N2                       # first line of each section
    hx1 = lambda p: C.compress_g1(p, cv).hex()
    other_tau = TAU + 1
    other_ck = kzg.setup(N1 - 1, tau=other_tau)[0]
    bits = N1.bit_length() - 1
    brp = [int(format(i, "0%db" % bits)[::-1], 2) for i in range(N1)]
    broken = {}
    lines = list(h.lines); lines[mono0 + 5] = hx1(kzg.add(h.mono[5], kzg.G1))
    broken["S_5 + G1"] = (lines, "G1 powers")
    lines = list(h.lines); lines[mono0] = hx1(kzg.multiply(kzg.G1, 2))
    broken["S_0 is not G1"] = (lines, "first G1 power")
    lines = list(h.lines); lines[g20 + 6] = C.compress_g2(kzg.multiply(kzg.G2, 12345), cv).hex()
    broken["another subgroup point for a G2 power"] = (lines, "G2 powers")
    lines = list(h.lines); lines[g20:mono0] = [C.compress_g2(q, cv).hex() for q in kzg.setup_g2(N2, other_tau)]
    broken["G1 and G2 sections of different tau"] = (lines, "G1 powers")
    lines = list(h.lines); lines[lag0:g20] = [h.lines[lag0 + brp[i]] for i in range(N1)]
    broken["the Lagrange section bit-reversed"] = (lines, "Lagrange")
    lines = list(h.lines); lines[lag0 + 10], lines[lag0 + 11] = lines[lag0 + 11], lines[lag0 + 10]
    broken["two Lagrange neighbours swapped"] = (lines, "Lagrange")
    for what, (lines, part) in broken.items():
        path = h.write(tmp_path, lines)
        for r in (FIXED_R, None):
            with pytest.raises(ValueError, match="do not describe one tau.*" + part):
                kzg.load_trusted_setup(path, r=r)
        ts = kzg.load_trusted_setup(path, check=False)
        for r in (FIXED_R, None):
            assert kzg.check_key(ts.monomial, ts.g2, ts.lagrange, r=r) is False, what
    # the same through lists of points, without a file
    bad = list(h.mono); bad[5] = kzg.add(bad[5], kzg.G1)
    assert kzg.check_key(bad, h.g2) is False
    assert kzg.check_key(other_ck, h.g2) is False and kzg.check_key(h.ck, kzg.setup_g2(N2, other_tau)) is False
    bad = list(h.g2); bad[0] = kzg.multiply(kzg.G2, 2)
    assert kzg.check_key(h.ck, bad) is False
    bad = list(h.g2); bad[N2 - 1] = bad[N2 - 2]
    assert kzg.check_key(h.ck, bad) is False


@pytest.mark.parametrize("curve", CURVES)
def test_a_g2_line_outside_the_subgroup(kzgs, honest, curve, tmp_path):
    kzg, h = kzgs[curve], honest[curve]
    cv = kzg._cv
    t = next(pt for pt, ok, what in subgroup_matrix_g2(curve) if what.startswith("T"))
    q = kzg._g2.add(h.g2[3], t)
    lines = list(h.lines)
    lines[2 + N1 + 3] = C.compress_g2(q, cv).hex()
    path = h.write(tmp_path, lines)
    with pytest.raises(ValueError, match=r"G2 section: point 3 has status 3"):
        kzg.load_trusted_setup(path)
    with pytest.raises(ValueError, match=r"G2 section: point 3 has status 3"):
        kzg.load_trusted_setup(path, check=False)
    ts = kzg.load_trusted_setup(path, check_subgroup=False, check=False)
    assert ts.g2[3] == q and ts.g2[:3] == h.g2[:3] and list(ts.monomial) == h.mono
    # a G1 line that names no point: the section, the index and the status
    lines = list(h.lines)
    lines[2 + N1 + N2 + 7] = "00" * (len(lines[-1]) // 2)
    with pytest.raises(ValueError, match=r"G1 monomial section: .*point 7 has status 1"):
        kzg.load_trusted_setup(h.write(tmp_path, lines))


@pytest.mark.parametrize("curve", CURVES)
def test_bit_reversed_lagrange_order(kzgs, honest, curve, tmp_path):
    kzg, h = kzgs[curve], honest[curve]
    path = str(tmp_path / "brp.txt")
    kzg.save_trusted_setup(path, h.ck, h.g2, lagrange_order="bit_reversed")
    lines = open(path).read().splitlines()
    assert lines != h.lines and sorted(lines) == sorted(h.lines) and lines[2 + N1:] == h.lines[2 + N1:]
    assert lines[2 + 1] == h.lines[2 + N1 // 2]
    ts = kzg.load_trusted_setup(path, lagrange_order="bit_reversed", r=FIXED_R)
    assert list(ts.lagrange) == h.lag and list(ts.monomial) == h.mono and ts.g2 == h.g2
    with pytest.raises(ValueError, match="Lagrange"):
        kzg.load_trusted_setup(path)
    with pytest.raises(ValueError, match="lagrange_order"):
        kzg.load_trusted_setup(path, lagrange_order="reversed")


def test_end_to_end_from_the_file_alone(kzgs, honest):
    """No tau after the file is written: commitments, cells and proofs from the loaded keys verify against the loaded
    G2 powers (bls12_381, n1 = 64, cosets of l = 4 on the domain of 128 points)."""
    kzg, h = kzgs["bls12_381"], honest["bls12_381"]
    ts = kzg.load_trusted_setup(h.path)
    ck, lk = ts.monomial, ts.lagrange
    r = kzg.curve_order
    n, l, N = N1, 4, 2 * N1
    cosets = N // l
    rng = random.Random(77)
    # one opening at a point
    poly = [rng.randrange(r) for _ in range(n)]
    z, xi = rng.randrange(r), rng.randrange(r)
    comm = kzg.commit(ck, [poly])
    proof = kzg.open(ck, [poly], z, xi)
    value = sum(c * pow(z, k, r) for k, c in enumerate(poly)) % r
    assert kzg.check(ts.rk, comm, z, [value], proof, xi)
    assert not kzg.check(ts.rk, comm, z, [(value + 1) % r], proof, xi)
    # coset proofs through verify_cosets with [tau^4] G2 from the file
    proofs, values = kzg.open_cosets_each(ck, [poly], l, n=n, N=N, with_values=True)
    args = (comm, [0] * cosets, list(range(cosets)), values[0], proofs[0], l, N)
    assert kzg.verify_cosets(ck, ts.rk_l(l), *args) is True
    assert kzg.verify_cosets(ck, ts.rk_l(l + 1), *args) is False
    # EIP-7594 by name: a blob, its commitment from the loaded Lagrange key, its cells and proofs
    w_N = int(kzg.Fq.root_of_unity(N))
    assert lk.w == pow(w_N, N // n, r)
    elements = [rng.randrange(r) for _ in range(n)]
    blob = b"".join(e.to_bytes(32, "big") for e in elements)
    bits = n.bit_length() - 1
    natural = [elements[int(format(t, "0%db" % bits)[::-1], 2)] for t in range(n)]
    commitment = kzg.compress_g1(kzg.commit_evaluations(lk, [natural]))[0]
    cells, cell_proofs = kzg.compute_cells_and_kzg_proofs(ck, [blob], l, n=n, N=N)
    idx = list(range(cosets))
    assert kzg.verify_cell_kzg_proof_batch(ck, ts.rk_l(l), [commitment] * cosets, idx, cells[0], cell_proofs[0], l, N) is True
    swapped = list(cells[0]); swapped[0], swapped[1] = swapped[1], swapped[0]
    assert kzg.verify_cell_kzg_proof_batch(ck, ts.rk_l(l), [commitment] * cosets, idx, swapped, cell_proofs[0], l, N) is False
    with pytest.raises(ValueError, match="9 G2 powers"):
        ts.rk_l(16)
