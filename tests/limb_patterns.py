"""Adversarial limb patterns for the unsaturated-limb fields of csrc/field.h (a plain helper module, no fixtures).

An element is N limbs of L bits, value = sum l[j] 2^(L j); the lower N-1 limbs of a normalised element are below 2^L
and the top limb takes whatever is left.  Uniformly random field elements fill a 64-bit product column to about a
quarter of its capacity and never sit at the top of a lazy range; the integers produced here do both on purpose."""
import random


def to_limbs(x, L, N):
    """normalised limb image of x >= 0 (the top limb takes the excess; it must fit 32 bits)"""
    mask = (1 << L) - 1
    out = [(x >> (L * j)) & mask for j in range(N - 1)]
    top = x >> (L * (N - 1))
    assert 0 <= top < (1 << 32), "value does not fit the representation"
    return out + [top]


def from_limbs(limbs, L):
    """value of ANY limb vector (limbs may exceed 2^L)"""
    return sum(int(v) << (L * j) for j, v in enumerate(limbs))


def _largest_at_top(bound, L, N):
    """the value <= bound with the same top limb as `bound` and as many all-ones limbs below it as that allows"""
    mask = (1 << L) - 1
    limbs = to_limbs(bound, L, N)
    for j in range(N - 2, -1, -1):
        if limbs[j] == mask:
            continue
        if limbs[j] > 0:
            limbs[j] -= 1
            for i in range(j):
                limbs[i] = mask
        break
    return from_limbs(limbs, L)


def fixed_patterns(p, L, N, K):
    """the deterministic part: integers in [0, K*p)"""
    mask = (1 << L) - 1
    bound = K * p - 1
    shift = L * (N - 1)
    ones = (1 << shift) - 1                              # all lower limbs 2^L - 1
    top = bound >> shift
    vals = [bound, _largest_at_top(bound, L, N), 0, 1, p, p - 1, p + 1, 2 * p - 1, 2 * p - 2, (K - 1) * p, K * p - 2]
    for t in (top - 1, top - 2, top // 2, 0):            # all-ones below a top limb just under the bound's
        if t >= 0:
            vals.append((t << shift) | ones)
    for j in range(N - 1):                               # a single limb at its maximum; all but one
        vals.append(mask << (L * j))
        if top >= 1:
            vals.append(((top - 1) << shift) | (ones ^ (mask << (L * j))))
    alt = sum(mask << (L * j) for j in range(0, N - 1, 2))
    vals += [alt, ones ^ alt]
    if top >= 1:
        vals += [((top - 1) << shift) | alt, ((top - 1) << shift) | (ones ^ alt)]
    seen, out = set(), []
    for v in vals:
        if 0 <= v <= bound and v not in seen:
            seen.add(v)
            out.append(v)
    return out


def random_mixtures(p, L, N, K, count, seed):
    """seeded mixtures: every lower limb is all-ones (3 in 5), zero or random; the top limb is at, just under or
    anywhere below the top limb of K*p - 1"""
    rng = random.Random(seed)
    mask = (1 << L) - 1
    bound = K * p - 1
    shift = L * (N - 1)
    top = bound >> shift
    out = []
    while len(out) < count:
        v = 0
        for j in range(N - 1):
            c = rng.randrange(5)
            limb = mask if c < 3 else 0 if c == 3 else rng.randrange(mask + 1)
            v |= limb << (L * j)
        t = rng.choice([top, max(top - 1, 0), max(top - 1, 0), rng.randrange(top + 1)])
        v |= t << shift
        if v <= bound:
            out.append(v)
    return out


def near_all_ones(p, L, N, K, count, seed):
    """all lower limbs 2^L - 1 but one or two random ones, under the top limb of K*p - 1.  The quotient digits m_k of a
    Montgomery product depend on the low limbs only; varying them while every column stays (nearly) full of maximal
    a*b products is what finds a column that is one m*p product too full."""
    rng = random.Random(seed)
    mask = (1 << L) - 1
    shift = L * (N - 1)
    top = (K * p - 1) >> shift
    out = []
    for i in range(count):
        v = (1 << shift) - 1
        for j in ([0], [i % (N - 1)], [0, 1 + i % (N - 2)])[i % 3]:
            v = (v & ~(mask << (L * j))) | (rng.randrange(mask + 1) << (L * j))
        out.append(v | (max(top - 1, 0) << shift))
    return out


def adversarial(p, L, N, K, count=0, seed=0):
    """integers < K*p with adversarial limb images: the fixed patterns, then `count` seeded mixtures"""
    return fixed_patterns(p, L, N, K) + (random_mixtures(p, L, N, K, count, seed) if count else [])


def header_layout(struct_name):
    """(L, N) of one field as kzg_snark_amd/csrc/curve_constants.h declares them (struct BnFr / BnFp / BlsFr / BlsFp),
    read from the header's text so that no test keeps a copy of the layout"""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kzg_snark_amd", "csrc", "curve_constants.h")
    with open(path) as f:
        text = f.read()
    body = text[text.index("struct %s {" % struct_name):]
    body = body[:body.index("};")]
    return (int(re.search(r"constexpr int L = (\d+);", body).group(1)),
            int(re.search(r"constexpr int N = (\d+);", body).group(1)))
