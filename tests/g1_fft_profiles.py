"""Keys and polynomials DESIGNED to drive the G1 transform (g1_level_kernel / launch_levels, csrc/domain.hip) and the
FK20 code around it through the exceptional branches of Ec::add -- an infinite operand on either side, P + P, P + (-P)
-- and a CPU census of which butterfly takes which branch.  Pure Python on ints mod r: no GPU, no library.

Every point of these tests is a known multiple of G: a key is a list of scalars a_t (0 is the point at infinity), a
polynomial a list of coefficients, and what the device must return is [k] G for a scalar k taken from the DEFINITION:

    proof_scalar          q = (p - rho) / (X^l - z^l) by long division, k = sum_t q_t a_t.  This holds for ANY key,
                          not only powers of a tau: FK20 uses linearity alone, h_u = sum_(t >= (u+1) l) c_t a_(t-(u+1)l)
                          and pi(z) = sum_u h_u z^(l u) = sum_t q_t a_t.
    lagrange_key_scalars  n^-1 sum_j w^(-ij) a_j

    dit_census    replays the schedule of g1_level_kernel on scalars (bit-reversed load; level s pairs i0 = b 2^(s+1) + k
                  with i0 + 2^s, twiddle root^(k len / 2^(s+1))) and counts (level, class, unit twiddle) per butterfly.
                  It serves coverage claims only (tests/test_g1_fft_profiles_host.py), never an expected value.
    fk20_stages   the inputs of the three transforms of one opening (table, size-2m inverse, final) in scalars, for the
                  census; straus_census the same for the chain of dom_hadsum_kernel
    *_cases       the inputs tests/test_g1_transforms_gpu.py runs, so that the host test pins the set the GPU sees"""
import random
from collections import Counter

CURVES = ["bls12_381", "bn254"]
TAU = 0x5eed_1234_abcd_0987_6543_21fe_dcba
CLASSES = ("A_inf", "B_inf", "both_inf", "A==B", "A==-B", "generic")
EXCEPTIONAL = CLASSES[:5]
BASE_KEYS = ("tau", "constant", "alternating", "root_low", "root_high", "some_inf", "all_inf")
PAIR_KEYS = ("const_along_j", "opposite_pairs")              # l >= 2: sub-tables that coincide / are opposite


def bitrev(i, log_len):
    return int(format(i, "0%db" % log_len)[::-1], 2) if log_len else 0


def dft(vec, root, r):
    """X_k = sum_j vec_j root^(jk), by the definition"""
    n = len(vec)
    pw = [pow(root, e, r) for e in range(n)]
    return [sum(v * pw[j * k % n] for j, v in enumerate(vec) if v) % r for k in range(n)]


# ---- the census ----------------------------------------------------------------------------------------------------

def classify(A, B, r):
    """the branch Ec::add(A, B) takes first (B: the second operand, twiddle applied)"""
    if A == 0:
        return "both_inf" if B == 0 else "A_inf"
    if B == 0:
        return "B_inf"
    if A == B:
        return "A==B"
    if (A + B) % r == 0:
        return "A==-B"
    return "generic"


def dit_census(vec, root, r):
    """(Counter[(level, class, unit)], natural-order output) of the radix-2 DIT transform of `vec` with `root`, the
    schedule of g1_level_kernel: unit is True for twiddle index k = 0 (the kernel skips the scalar multiple)."""
    n = len(vec)
    log_len = n.bit_length() - 1
    assert n == 1 << log_len and log_len >= 1
    buf = [0] * n
    for i, v in enumerate(vec):
        buf[bitrev(i, log_len)] = v % r
    seen = Counter()
    for s in range(log_len):
        h = 1 << s
        for b in range(n >> (s + 1)):
            for k in range(h):
                i0 = (b << (s + 1)) + k
                tw = pow(root, k * (n >> (s + 1)), r)
                A, B = buf[i0], buf[i0 + h] * tw % r
                seen[(s, classify(A, B, r), k == 0)] += 1
                buf[i0], buf[i0 + h] = (A + B) % r, (A - B) % r
    return seen, buf


def cells(log_len):
    """every (level, class, unit) a transform of 2^log_len points has: level 0 has the unit twiddle only"""
    return {(s, c, u) for s in range(log_len) for c in CLASSES for u in (True, False) if u or s > 0}


def build_level_vector(log_len, root, s, r, seed, shift=0, last_zero=False):
    """A natural-order input whose butterfly (b, k) of level s is of class CLASSES[(b + k + shift) % 6]: the state at
    the entry of level s is chosen, the levels below it are inverted.  last_zero: the input's last entry is 0 (what
    FK20 forces on h); that is one linear condition on the B operands of the last block, met by solving for the first
    of them that the asked classes leave finite (at level 0 it is the entry itself, so the last butterfly's B is
    infinite whatever is asked)."""
    n = 1 << log_len
    h = 1 << s
    rng = random.Random(seed)
    b_last = (n >> (s + 1)) - 1
    free = [k for k in range(h) if CLASSES[(b_last + k + shift) % 6] not in ("B_inf", "both_inf")]
    pivot = free[0] if free else None

    def state(pivot_value):
        buf = [0] * n
        for b in range(n >> (s + 1)):
            last = last_zero and b == b_last
            for k in range(h):
                cls = CLASSES[(b + k + shift) % 6]
                tw = pow(root, k * (n >> (s + 1)), r)
                B = rng.randrange(1, r)
                A = rng.randrange(1, r)
                if last and k == pivot:
                    B = pivot_value
                if cls in ("B_inf", "both_inf"):
                    B = 0
                if cls == "A==B":
                    A = tw * B % r
                elif cls == "A==-B":
                    A = -tw * B % r
                elif cls in ("A_inf", "both_inf"):
                    A = 0
                i0 = (b << (s + 1)) + k
                buf[i0], buf[i0 + h] = A, B
        return buf

    def invert(buf):
        inv2 = pow(2, -1, r)
        for t in range(s - 1, -1, -1):
            ht = 1 << t
            for b in range(n >> (t + 1)):
                for k in range(ht):
                    i0 = (b << (t + 1)) + k
                    tw_inv = pow(root, -(k * (n >> (t + 1))), r)
                    x0, x1 = buf[i0], buf[i0 + ht]
                    buf[i0], buf[i0 + ht] = (x0 + x1) * inv2 % r, (x0 - x1) * inv2 % r * tw_inv % r
        return [buf[bitrev(i, log_len)] for i in range(n)]

    if not last_zero:
        return invert(state(None))
    st = rng.getstate()
    f0 = invert(state(0))[n - 1]
    rng.setstate(st)
    f1 = invert(state(1))[n - 1]
    rng.setstate(st)
    b0 = 0 if f1 == f0 else -f0 * pow(f1 - f0, -1, r) % r
    x = invert(state(b0))
    assert x[n - 1] == 0
    return x


# ---- the definitions -------------------------------------------------------------------------------------------------

def coset_quotient(coeffs, l, a, r):
    """quotient of p by X^l - a, long division: q_t = c_(t+l) + a q_(t+l)"""
    c = [int(x) % r for x in coeffs]
    q = [0] * max(len(c) - l, 0)
    for t in range(len(q) - 1, -1, -1):
        q[t] = (c[t + l] + (a * q[t + l] if t + l < len(q) else 0)) % r
    return q


def proof_scalar(key, coeffs, l, z, r):
    """k with proof = [k] G for the coset {z zeta^j, j < l} (l = 1: the point z) under the key [a_t] G"""
    q = coset_quotient(coeffs, l, pow(z, l, r), r)
    assert len(q) <= len(key)
    return sum(x * a for x, a in zip(q, key)) % r


def coset_proof_scalars(key, coeffs, l, N, w, r):
    """the N/l proofs of kzg_open_cosets (coset i starts at w^i); l = 1, N = n: kzg_open_domain's"""
    return [proof_scalar(key, coeffs, l, pow(w, i, r), r) for i in range(N // l)]


def lagrange_key_scalars(key, w, r):
    n = len(key)
    ninv = pow(n, -1, r)
    return [x * ninv % r for x in dft(key, pow(w, -1, r), r)]


# ---- FK20 in scalars, stage by stage (census only) -------------------------------------------------------------------

def fk20_stages(key, coeffs, log_n, log_l, log_N, w, cv):
    """The inputs of the transforms of one kzg_open_cosets call (l = 1, N = n: kzg_open_domain), as csrc/domain.hip
    states them: {"table": [(vector, root)] * l, "inverse": (vector, root), "final": (vector, root)}, the Straus
    operands "scalars"[i][j], "points"[i][j] of output i < 2m, and "proofs", the final transform's output."""
    r = cv.r
    n, l = 1 << log_n, 1 << log_l
    m, mm = n >> log_l, 2 * (n >> log_l)
    omega = cv.root_of_unity(mm)
    c = [int(x) % r for x in coeffs] + [0] * (n - len(coeffs))
    tables, S, chat = [], [], []
    for j in range(l):
        s_hat = [key[(m - 2 - u) * l + j] % r if u + 2 <= m else 0 for u in range(mm)]
        tables.append((s_hat, omega))
        S.append(dft(s_hat, omega, r))
        chat.append(dft([c[s * l + j] for s in range(m)] + [0] * m, omega, r))
    mminv = pow(mm, -1, r)
    scalars = [[chat[j][i] * mminv % r for j in range(l)] for i in range(mm)]
    points = [[S[j][i] for j in range(l)] for i in range(mm)]
    u_hat = [sum(e * p for e, p in zip(scalars[i], points[i])) % r for i in range(mm)]
    omega_inv = pow(omega, -1, r)
    u = dft(u_hat, omega_inv, r)
    L = (1 << log_N) >> log_l
    h = [u[m - 1 + t] if t + 2 <= m else 0 for t in range(L)]
    wl = pow(w, l, r)
    return {"table": tables, "inverse": (u_hat, omega_inv), "final": (h, wl), "scalars": scalars, "points": points,
            "proofs": dft(h, wl, r)}


def straus_census(scalars, points, r):
    """the additions of dom_hadsum_kernel's chain over one group: acc = 2 acc per bit, then acc += P_jj for every set
    bit, classified as classify(acc, P_jj)"""
    seen = Counter()
    acc = 0
    for bit in range(255, -1, -1):
        acc = 2 * acc % r
        for e, p in zip(scalars, points):
            if (e >> bit) & 1:
                seen[classify(acc, p % r, r)] += 1
                acc = (acc + p) % r
    return seen


# ---- profiles --------------------------------------------------------------------------------------------------------

def key_profiles(log_n, log_l, cv, seed=1):
    """{name: (scalars a_t, tau or None)} for a key of n = 2^log_n points used with cosets of l = 2^log_l"""
    r = cv.r
    n, l = 1 << log_n, 1 << log_l
    mm = 2 * (n >> log_l)
    rng = random.Random(seed * 1000 + log_n * 10 + log_l)
    omega = cv.root_of_unity(mm)

    def powers(tau):
        return ([pow(tau, t, r) for t in range(n)], tau % r)

    out = {
        "tau": powers(TAU),
        "constant": powers(1),                                # all G
        "alternating": powers(r - 1),                         # +-G: tau = -1
        "root_low": powers(pow(omega, mm // 4, r)),           # tau of order 4: a key of period 4
        "root_high": powers(pow(omega, 3, r)),                # tau a primitive 2m-th root (omega itself: no A = -B)
        "all_inf": ([0] * n, None),
    }
    some = [pow(TAU, t, r) for t in range(n)]
    for t in {0, 3, n // 2, n // 2 + 1, n - 2, n - 1}:
        some[t] = 0
    some[5 % n] = some[2]                                     # and a repeated point
    out["some_inf"] = (some, None)
    if l >= 2:
        base = [rng.randrange(1, r) for _ in range(n // l)]
        out["const_along_j"] = ([base[t // l] for t in range(n)], None)          # the l sub-tables coincide
        opp = [rng.randrange(1, r) for _ in range(n)]
        for s in range(n // l):
            opp[s * l + 1] = -opp[s * l] % r                                     # sub-tables 0 and 1 are opposite
        out["opposite_pairs"] = (opp, None)
    return out


def poly_from_h(h, tau, l, r):
    """coefficients whose FK20 vector under the key [tau^t] G is h (h_u = sum_(t >= (u+1) l) c_t tau^(t-(u+1)l); the
    last entry of h must be 0): c_(ul) = h_(u-1) - tau^l h_u, zero elsewhere, c_0 free (0 here)"""
    m = len(h)
    assert h[m - 1] % r == 0
    tl = pow(tau, l, r)
    c = [0] * (m * l)
    for u in range(1, m):
        c[u * l] = (h[u - 1] - tl * h[u]) % r
    return c


def h_profiles(log_m, w, r, seed=2):
    """{name: h} of m = 2^log_m entries, the last one 0: inputs of the final transform (root w)"""
    m = 1 << log_m
    out = {"h_constant": [1] * (m - 1) + [0], "h_alternating": [(-1) ** u % r for u in range(m - 1)] + [0]}
    for e in range(m):
        out["h_geometric_%d" % e] = [pow(w, -e * u, r) for u in range(m - 1)] + [0]
    for p in range(m - 1):
        out["h_spike_%d" % p] = [int(u == p) for u in range(m)]
    for s in range(log_m):
        for shift in (range(6) if s == log_m - 1 else (0, 3)):        # the top level has one butterfly per twiddle
            out["h_level_%d_%d" % (s, shift)] = build_level_vector(log_m, w, s, r, seed * 100 + s, shift, last_zero=True)
    return out


def poly_profiles(log_n, cv, seed=3):
    """{name: coefficients} of length <= n that need no tau"""
    r = cv.r
    n = 1 << log_n
    rng = random.Random(seed * 100 + log_n)
    omega = cv.root_of_unity(2 * n)
    c = rng.randrange(2, r)
    out = {
        "random": [rng.randrange(r) for _ in range(n)],
        "zero": [0] * n,
        "empty": [],
        "all_equal": [c] * n,
        "all_minus_one": [r - 1] * n,
        "single_0": [c],
        "single_1": [0, c],
        "single_mid": [0] * (n // 2) + [1],
        "single_last": [0] * (n - 1) + [c],
    }
    for e in (0, 1, 2, n // 2, n, 2 * n - 1):
        out["geometric_%d" % e] = [pow(omega, -e * j, r) for j in range(n)]
    return out


def lagrange_cases(log_n, cv):
    """{name: key scalars} for kzg_srs_lagrange on loaded keys of n = 2^log_n points (the transform is free: any
    vector is a key)"""
    r = cv.r
    n = 1 << log_n
    w = cv.root_of_unity(n)
    winv = pow(w, -1, r)
    out = {k: v[0] for k, v in key_profiles(log_n, 0, cv).items()}
    for e in range(n):
        out["geometric_%d" % e] = [pow(w, e * t, r) for t in range(n)]
    for p in range(n):
        out["spike_%d" % p] = [int(t == p) for t in range(n)]
    for s in range(log_n):
        for shift in (0, 3):
            out["level_%d_%d" % (s, shift)] = build_level_vector(log_n, winv, s, r, 40 + s, shift)
    return out


def domain_cases(log_n, cv, full):
    """[(key name, key scalars, {poly name: coefficients})] for kzg_open_domain at n = 2^log_n.  full: every key with
    every tau-free polynomial; otherwise each key with a rotating third of them.  The tau-generated key also gets the
    polynomials built from a target h."""
    r = cv.r
    n = 1 << log_n
    w = cv.root_of_unity(n)
    polys = poly_profiles(log_n, cv)
    names = sorted(polys)
    out = []
    for q, (kname, (key, tau)) in enumerate(sorted(key_profiles(log_n, 0, cv).items())):
        take = names if full else [p for t, p in enumerate(names) if t % 3 == q % 3 or p in ("zero", "all_equal")]
        chosen = {p: polys[p] for p in take}
        if kname == "tau":
            for hname, h in h_profiles(log_n, w, r).items():
                chosen[hname] = poly_from_h(h, tau, 1, r)
        out.append((kname, key, chosen))
    return out


def coset_cases(log_n, log_l, cv):
    """[(key name, key scalars, {poly name: coefficients})] for kzg_open_cosets at n = 2^log_n, l = 2^log_l"""
    r = cv.r
    n, l = 1 << log_n, 1 << log_l
    rng = random.Random(500 + log_n * 10 + log_l)
    polys = poly_profiles(log_n, cv)
    keys = key_profiles(log_n, log_l, cv)
    base = {p: polys[p] for p in ("random", "all_equal", "single_mid", "geometric_1", "zero")}
    if l >= 2:
        pair = [rng.randrange(1, r) for _ in range(n)]
        for s in range(n // l):
            pair[s * l + 1] = pair[s * l]                    # c_(sl) = c_(sl+1): equal scalars for sub-tables 0 and 1
        base["pair_equal"] = pair
        base["pair_only"] = [pair[t] if t % l < 2 else 0 for t in range(n)]
    m = n // l
    if m >= 2:
        w_m = cv.root_of_unity(m)
        hs = h_profiles(log_n - log_l, w_m, r)
        tau_h = {k: poly_from_h(hs[k], TAU, l, r) for k in sorted(hs) if k.endswith("_0") or k == "h_alternating"}
    else:
        tau_h = {}
    out = []
    for kname in sorted(keys):
        key, tau = keys[kname]
        chosen = dict(base)
        if kname == "tau":
            chosen.update(tau_h)
        elif kname in ("root_low", "root_high", "some_inf", "all_inf"):
            chosen = {p: base[p] for p in ("all_equal", "geometric_1", "single_mid")}
        out.append((kname, key, chosen))
    return out
