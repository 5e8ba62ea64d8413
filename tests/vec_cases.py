"""The launch plans of the Fr vector primitives (csrc/poly.hip, last section: vec_prefix_product_t, vec_inverse_t,
vec_mul_powers_t and their kernels) restated as functions of n, the plain-integer definitions of what the calls compute,
and the inputs tests/test_vec_edges_gpu.py runs.  Pure Python: no GPU, no library, no torch.

    prefix_levels    the level sizes m = [n, ceil(n / LC), ..] of the prefix product, down to one chunk
    inverse_threads  T of the batch inversion; inverse_batch(n, t) the elements thread t inverts with one exponentiation
    powers_threads   T = 2^lt of vec_mul_powers: thread t walks t, t + T, .. with p *= s^T
    ref_*            the definitions, on integers mod r
    *_cases          labelled inputs with the expected output; tests/test_vec_cases_host.py pins what they reach

Every expected list is written down from the definition of the case (a closed form where the case has one, the ref_*
function otherwise); the host test shows that the closed forms are the ref_* values too."""
import functools
import random
from collections import namedtuple

LC = 32                  # csrc/poly.hip: constexpr uint32_t LC -- elements per thread / per chunk of the three primitives
DOT_G = 6                # csrc/poly.hip: constexpr uint32_t DOT_G -- lincomb terms that share one Montgomery reduction
MAXK = 64                # csrc/poly.hip: constexpr uint32_t MAXK -- terms one lincomb call takes
INVERSE_BLOCK = 64       # threads per block of vec_inverse_kernel (dim3(64))
POWERS_LT0 = 7           # vec_mul_powers_t: `uint32_t lt = 7` -- 128 threads at the least
MAX_N = 40000            # no vector case is longer

PREFIX_NS = (1, 31, 32, 33, 1023, 1024, 1025, 32767, 32768, 32769)
PREFIX_MARKS = (0, 31, 32, 1023, 1024, 32767, 32768)          # and n - 2, n - 1: where a single element differs
INVERSE_NS = (1, 31, 32, 33, 2047, 2048, 2049, 4097, 40000)
POWERS_NS = (1, 127, 128, 129, 4095, 4096, 4097, 8192, 8193)
ALIAS_NS = (1, 33, 257, 1025)


# ---- the launch plans ------------------------------------------------------------------------------------------------

def prefix_levels(n):
    """vec_prefix_product_t: m = {n}; while (m.back() > LC) m.push_back(ceil(m.back() / LC))"""
    m = [n]
    while m[-1] > LC:
        m.append((m[-1] + LC - 1) // LC)
    return m


def inverse_threads(n):
    """vec_inverse_t (out != a): ceil(chunks / 64) blocks of 64 threads, chunks = ceil(n / LC)"""
    chunks = (n + LC - 1) // LC
    return INVERSE_BLOCK * ((chunks + INVERSE_BLOCK - 1) // INVERSE_BLOCK)


def inverse_batch(n, t):
    """vec_inverse_kernel: thread t takes t, t + T, t + 2T, .. below n"""
    return list(range(t, n, inverse_threads(n)))


def powers_threads(n):
    """vec_mul_powers_t: lt = 7; while ((LC << lt) < n && lt < 24) ++lt; T = 1 << lt"""
    lt = POWERS_LT0
    while (LC << lt) < n and lt < 24:
        lt += 1
    return 1 << lt


# ---- the definitions -------------------------------------------------------------------------------------------------

def ref_prefix(a, r):
    """out[i] = prod_(j < i) a[j]"""
    out, acc = [], 1
    for x in a:
        out.append(acc)
        acc = acc * x % r
    return out


def ref_inverse(a, r):
    """out[i] = a[i]^-1, 0 -> 0"""
    return [pow(x, -1, r) if x else 0 for x in a]


def ref_mul_powers(a, s, c0, r):
    """out[i] = a[i] c0 s^i, s^i by a running product (s^0 = 1 for every s, 0 included)"""
    out, p = [], c0 % r
    for x in a:
        out.append(x * p % r)
        p = p * s % r
    return out


def ref_op(op, a, b, r):
    if op == "add":
        return [(x + y) % r for x, y in zip(a, b)]
    if op == "sub":
        return [(x - y) % r for x, y in zip(a, b)]
    assert op == "mul"
    return [x * y % r for x, y in zip(a, b)]


def ref_lincomb(n, vecs, lens, scalars, r):
    """out[i] = sum_j scalars[j] vecs[j][i], a vector counting as zero from lens[j] on"""
    assert len(vecs) == len(lens) == len(scalars) <= MAXK
    return [sum(s * v[i] for v, ln, s in zip(vecs, lens, scalars) if i < ln) % r for i in range(n)]


def fourth_root_of_unity(r):
    """w of order 4 in Fr (w^2 = -1): both scalar fields have r = 1 mod 4"""
    assert r % 4 == 1
    for g in range(2, 100):
        w = pow(g, (r - 1) // 4, r)
        if w * w % r == r - 1:
            return w
    raise AssertionError("no quadratic non-residue below 100")


# ---- shared random material: one vector per field, its prefix products and inverses computed once ------------------

@functools.lru_cache(maxsize=None)
def _base(r):
    rng = random.Random(r % 1000003)
    a = [rng.randrange(2, r - 1) for _ in range(MAX_N)]        # neither 0 nor 1 nor r - 1: the cases place those
    return a, ref_prefix(a, r), ref_inverse(a, r)


def base_vector(r, n):
    return _base(r)[0][:n]


Case = namedtuple("Case", "label a want")


# ---- prefix product --------------------------------------------------------------------------------------------------

def prefix_marks(n):
    return sorted({p for p in PREFIX_MARKS + (n - 2, n - 1) if 0 <= p < n})


def prefix_cases(n, r):
    a, pre, _ = _base(r)
    a, pre = a[:n], pre[:n]
    v = a[0]                                                   # the non-one value: random, not 0, 1 or r - 1
    cases = [Case("random", a, pre),
             Case("ones", [1] * n, [1] * n),
             Case("minus-ones", [r - 1] * n, [1 if i % 2 == 0 else r - 1 for i in range(n)])]
    for p in prefix_marks(n):
        # 1 up to and including p (exclusive product), v after it
        cases.append(Case(f"non-one@{p}", [1] * p + [v] + [1] * (n - p - 1), [1] * (p + 1) + [v] * (n - p - 1)))
        # exact up to and including p, 0 after it
        cases.append(Case(f"zero@{p}", a[:p] + [0] + a[p + 1:], pre[:p + 1] + [0] * (n - p - 1)))
    return cases


# ---- inverse ---------------------------------------------------------------------------------------------------------

def inverse_chosen_threads(n):
    """thread 0, one in the middle and the last of the threads that hold two elements or more (none: [])"""
    T = inverse_threads(n)
    if n <= T:
        return []
    last = min(T, n - T) - 1                                   # the largest t with t + T < n
    return sorted({0, last // 2, last})


def inverse_tail_thread(n):
    """the last thread whose batch is a single element, or None: with n <= T every thread that has work has one
    element, past T the threads t >= n - T do"""
    T = inverse_threads(n)
    t = min(n, T) - 1
    return t if len(inverse_batch(n, t)) == 1 else None


def inverse_cases(n, r):
    a, _, inv = _base(r)
    a, inv = a[:n], inv[:n]

    def zeroed(label, idx):
        az, want = list(a), list(inv)
        for i in idx:
            az[i] = want[i] = 0
        return Case(label, az, want)

    lone = (3 * n) // 4                                        # where the single non-zero element stands
    cases = [Case("random", a, inv),
             Case("zeros", [0] * n, [0] * n),
             Case("minus-ones", [r - 1] * n, [r - 1] * n),     # (-1)^-1 = -1
             Case(f"one-non-zero@{lone}", [0] * lone + [a[lone]] + [0] * (n - lone - 1),
                  [0] * lone + [inv[lone]] + [0] * (n - lone - 1))]
    for t in inverse_chosen_threads(n):
        batch = inverse_batch(n, t)
        cases.append(zeroed(f"thread{t}:whole-batch-zero", batch))
        cases.append(zeroed(f"thread{t}:first-zero", [min(batch)]))
        cases.append(zeroed(f"thread{t}:last-zero", [max(batch)]))
    t = inverse_tail_thread(n)
    if t is not None:
        cases.append(zeroed(f"thread{t}:tail-single-zero", inverse_batch(n, t)))
    return cases


# ---- powers ----------------------------------------------------------------------------------------------------------

def powers_scalars(r):
    """(label, s, c0): every s with a random c0, every c0 with a random s, and (0, 0)"""
    rng = random.Random(r % 1000003 + 1)
    rs, rc = rng.randrange(2, r - 1), rng.randrange(2, r - 1)
    pairs = [(f"s={ls},c0=random", s, rc) for ls, s in
             (("0", 0), ("1", 1), ("r-1", r - 1), ("i", fourth_root_of_unity(r)), ("random", rs))]
    pairs += [(f"s=random,c0={lc}", rs, c) for lc, c in (("0", 0), ("1", 1), ("r-1", r - 1))]
    pairs.append(("s=0,c0=0", 0, 0))
    return pairs


def powers_cases(n, r):
    a = base_vector(r, n)
    cases = []
    for label, s, c0 in powers_scalars(r):
        if s == 0:                                             # 0^0 = 1: out[0] = a[0] c0 and nothing else survives
            want = [a[0] * c0 % r] + [0] * (n - 1)
        else:
            want = ref_mul_powers(a, s, c0, r)
        cases.append(Case(label, a, want))
    return cases
