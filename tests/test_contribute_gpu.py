"""GPU tests of setup contributions (KZG.unit_setup / contribute / verify_contribution / verify_contributions): a
powers-of-tau ceremony of two or three participants from tau = 1, against setups generated from the product of the
secrets, and a coordinator's rejections."""
import numpy as np
import pytest

import g_mul_cases as gm

pytestmark = pytest.mark.gpu

CURVES = gm.CURVES
S1, S2, S3 = 0x1d2c3b4a59687766554433221100ffee, 0x0123456789abcdef0f1e2d3c4b5a6978, 0xc0ffee1234567


@pytest.fixture(scope="module")
def kzgs():
    from kzg_snark_amd.kzg import KZG
    return {c: KZG(c) for c in CURVES}


_CHAIN = {}


def chain(kzg):
    """unit_setup(16, 3) and the setups after S1 and after S2 with their contributions, computed once per curve"""
    if kzg.curve_type not in _CHAIN:
        s0 = kzg.unit_setup(16, 3)
        s1, c1 = kzg.contribute(s0, S1)
        s2, c2 = kzg.contribute(s1, S2)
        _CHAIN[kzg.curve_type] = (s0, s1, s2, c1, c2)
    return _CHAIN[kzg.curve_type]


def same_key(a, b):
    (xa, ia), (xb, ib) = a.srs.export(), b.srs.export()
    return np.array_equal(xa, xb) and np.array_equal(ia, ib)


def with_point(kzg, key, index, pt, lagrange=False):
    """a copy of the key with point `index` replaced"""
    from kzg_snark_amd import _native
    from kzg_snark_amd.kzg import CommitmentKey, LagrangeKey
    ctx = kzg._context()
    pts = _native.limbs_to_points(*key.srs.export())
    pts[index] = pt
    srs = ctx.srs_load_g1(*_native.points_to_limbs(pts, ctx.fp_limbs))
    return LagrangeKey(ctx, srs, key.n, key.w) if lagrange else CommitmentKey(ctx, srs)


@pytest.mark.parametrize("curve", CURVES)
def test_two_contributions_are_the_setup_of_the_product(kzgs, curve, tmp_path):
    from kzg_snark_amd.kzg import Contribution, TrustedSetup
    kzg = kzgs[curve]
    r = kzg.curve_order
    s0, s1, s2, c1, c2 = chain(kzg)
    assert len(s0.monomial) == 16 and s0.g2 == [kzg.G2] * 3 and s0.monomial[:] == [kzg.G1] * 16
    assert s0.lagrange[0] == kzg.G1 and s0.lagrange[1:] == [kzg.Z1] * 15             # L_i(1) = [i = 0]
    tau = S1 * S2 % r
    assert isinstance(s2, TrustedSetup) and isinstance(c2, Contribution)
    assert same_key(s2.monomial, kzg.setup(15, tau)[0])
    assert s2.g2 == kzg.setup_g2(3, tau)
    assert same_key(s2.lagrange, kzg.setup_lagrange(16, tau)[0]) and s2.lagrange.n == 16
    assert same_key(s1.monomial, kzg.setup(15, S1)[0]) and s1.g2 == kzg.setup_g2(3, S1)
    assert c1 == (kzg._g2.multiply(kzg.G2, S1), kzg._g1.multiply(kzg.G1, S1))
    assert c2 == (kzg._g2.multiply(kzg.G2, S2), kzg._g1.multiply(kzg.G1, tau))
    assert kzg.verify_contribution(s0, s1, c1, r=11) is True and kzg.verify_contribution(s1, s2, c2, r=12) is True
    # a contributed setup round-trips through its file
    path = str(tmp_path / "setup.txt")
    kzg.save_trusted_setup(path, s2.monomial, s2.g2)
    back = kzg.load_trusted_setup(path, check=True, r=5)
    assert same_key(back.monomial, s2.monomial) and same_key(back.lagrange, s2.lagrange) and back.g2 == s2.g2
    assert kzg.verify_contribution(s1, back, c2, r=13) is True
    # a secret nobody gave: drawn, used, not kept
    s3, c3 = kzg.contribute(s2)
    assert kzg.verify_contribution(s2, s3, c3) is True and c3.tau_g1 != c2.tau_g1


@pytest.mark.parametrize("curve", CURVES)
def test_a_coordinator_rejects_what_is_not_a_contribution(kzgs, curve):
    from kzg_snark_amd.kzg import Contribution, TrustedSetup
    kzg = kzgs[curve]
    r = kzg.curve_order
    s0, s1, s2, c1, c2 = chain(kzg)
    G1, G2 = kzg._g1, kzg._g2
    stray1, stray2 = G1.multiply(kzg.G1, 0xbad), G2.multiply(kzg.G2, 0xbad)

    def verdict(before=s1, after=s2, c=c2):
        return kzg.verify_contribution(before, after, c, r=21)

    assert verdict() is True
    assert verdict(c=Contribution(c1.pubkey, c2.tau_g1)) is False                      # the pubkey of another secret
    assert verdict(c=Contribution(kzg.Z2, c2.tau_g1)) is False                         # an infinite pubkey
    assert verdict(c=Contribution(c2.pubkey, kzg.Z1)) is False
    outside = [pt for pt, what in gm.points(curve, 2) if what == "outside the subgroup"][0]
    assert verdict(c=Contribution(outside, c2.tau_g1)) is False                        # a pubkey outside G2
    for index in (1, 15):                                                              # one monomial point replaced
        bad = TrustedSetup(with_point(kzg, s2.monomial, index, stray1), s2.lagrange, s2.g2)
        assert verdict(after=bad) is False
    # index 1 replaced consistently with the contribution's own tau_g1 still breaks the chain of the key
    bad = TrustedSetup(with_point(kzg, s2.monomial, 1, stray1), s2.lagrange, s2.g2)
    assert verdict(after=bad, c=Contribution(c2.pubkey, stray1)) is False
    assert verdict(after=TrustedSetup(s2.monomial, s2.lagrange, [s2.g2[0], s2.g2[1], stray2])) is False   # a G2 power
    assert verdict(after=TrustedSetup(s2.monomial, s2.lagrange, [s2.g2[0], stray2, s2.g2[2]])) is False
    assert verdict(after=TrustedSetup(s2.monomial, with_point(kzg, s2.lagrange, 7, stray1, lagrange=True), s2.g2)) is False
    # `after` shorter than `before`: the same secrets over a smaller setup are a valid setup of another length
    t0 = kzg.unit_setup(8, 3)
    t1, _ = kzg.contribute(t0, S1)
    t2, d2 = kzg.contribute(t1, S2)
    assert d2 == c2 and kzg.verify_contribution(t1, t2, d2, r=21) is True
    assert verdict(after=t2) is False
    assert verdict(after=TrustedSetup(s2.monomial, s2.lagrange, s2.g2[:2])) is False
    for secret in (0, r, -1, r + 5):
        with pytest.raises(ValueError, match="secret must be in"):
            kzg.contribute(s0, secret)
    assert same_key(kzg.contribute(s0, r - 1)[0].monomial, kzg.setup(15, r - 1)[0])


@pytest.mark.parametrize("curve", CURVES)
def test_a_transcript_is_one_pairing_call_with_one_verdict_per_link(kzgs, curve, monkeypatch):
    kzg = kzgs[curve]
    s0, s1, s2, c1, c2 = chain(kzg)
    s3, c3 = kzg.contribute(s2, S3)
    ctx = kzg._context()
    calls = []
    real = ctx.pairing_check

    def counted(g1_xy, g1_inf, g2_xy, g2_inf, k):
        calls.append((len(g1_xy) // k, k))
        return real(g1_xy, g1_inf, g2_xy, g2_inf, k)

    monkeypatch.setattr(ctx, "pairing_check", counted)
    first = s0.monomial[1]
    links = [c1, c2, c3]
    assert kzg.verify_contributions(first, links) == [True, True, True]
    assert calls == [(3, 2)]                                                           # one call, three equations
    assert kzg.verify_contributions(first, []) == [] and len(calls) == 1
    # link i reads c_i and c_(i-1).tau_g1: swapping positions a and b changes links a, a + 1, b, b + 1
    for a, b in ((1, 2), (0, 1), (0, 2)):
        swapped = list(links)
        swapped[a], swapped[b] = swapped[b], swapped[a]
        touched = {a, a + 1, b, b + 1}
        assert kzg.verify_contributions(first, swapped) == [i not in touched for i in range(3)], (a, b)
    assert kzg.verify_contributions(kzg._g1.multiply(kzg.G1, 2), links) == [False, True, True]
    assert len(calls) == 5
    monkeypatch.undo()
    assert kzg.verify_contributions(first, links[:1], pairing="host") == [True]
    # an infinite point makes a link False, whatever its partner
    from kzg_snark_amd.kzg import Contribution
    assert kzg.verify_contributions(kzg.Z1, [Contribution(kzg.Z2, kzg.Z1)]) == [False]
