"""The launch plans of the evaluation-form path (csrc/lagrange.hip: lagr_sums_kernel, lagr_batch_sums_kernel and the
chunk loop of fr_eval_lagrange_batch_t; csrc/blob.hip: blob_intake_kernel, blob_output_kernel) restated as functions,
the plain-integer definitions of what the calls compute, and the inputs tests/test_lagrange_edges_gpu.py and
tests/test_blob_stride_gpu.py run.  Pure Python: no GPU, no library, no torch.

    sums_plan, sums_place     the reduction pass of one vector: workgroups, passes of its strided loop, who takes index i
    batch_plan, batch_place   the batched pass: the loop ends at lens[j], so the passes depend on the vector
    batch_chunks              the (j0, cb) of the chunk loop, from b, n and the tuning key
    blob_plan                 workgroups and passes of the two byte kernels
    ref_*                     the definitions, on integers mod r
    *_TABLE, *_vectors        labelled inputs; tests/test_lagrange_cases_host.py pins what they reach

A point is written ("random",), ("zero",) or ("w", m) for w^m; a vector is (len, point)."""
import random

SUM_TB = 128                       # csrc/lagrange.hip: constexpr uint32_t SUM_TB -- threads per workgroup of both passes
SUM_MAXG = 2048                    # csrc/lagrange.hip: constexpr uint32_t SUM_MAXG -- workgroups of lagr_sums_kernel
BATCH_MAXG = 32                    # csrc/lagrange.hip: constexpr uint32_t BATCH_MAXG -- workgroups per vector, batched
BATCH_MAX_CHUNK = 65535            # csrc/lagrange.hip: constexpr size_t BATCH_MAX_CHUNK -- gridDim.y holds the vector
BATCH_SCRATCH_BYTES = 1 << 30      # csrc/lagrange.hip: constexpr size_t BATCH_SCRATCH_BYTES -- den + inv of one chunk
BLOB_MAXG = 8192                   # csrc/blob.hip: intake_launch, output_launch: std::min<size_t>(.., 8192) workgroups
BLOB_TB = 256                      # csrc/blob.hip: intake_launch, output_launch: dim3(256)
WAVE = 64


def _ceil(a, b):
    return (a + b - 1) // b


# ---- the launch plans ------------------------------------------------------------------------------------------------

def sums_groups(n):
    """value_pass: groups = min(SUM_MAXG, ceil(n / SUM_TB))"""
    return min(SUM_MAXG, _ceil(n, SUM_TB))


def sums_plan(n):
    """(groups, passes) of lagr_sums_kernel: every thread walks i, i + groups * SUM_TB, .. below n"""
    groups = sums_groups(n)
    return groups, _ceil(n, groups * SUM_TB)


def sums_place(n, i):
    """(pass, group, wave, lane) of the thread that takes index i of lagr_sums_kernel"""
    assert 0 <= i < n
    step = sums_groups(n) * SUM_TB
    t = i % step
    return i // step, t // SUM_TB, t % SUM_TB // WAVE, t % WAVE


def batch_groups(n):
    """fr_eval_lagrange_batch_t: groups = min(BATCH_MAXG, ceil(n / SUM_TB)), the grid's x"""
    return min(BATCH_MAXG, _ceil(n, SUM_TB))


def batch_plan(n, plen):
    """(groups, passes) of lagr_batch_sums_kernel over one vector: the loop runs below plen = lens[j], not n"""
    groups = batch_groups(n)
    return groups, _ceil(plen, groups * SUM_TB)


def batch_place(n, plen, i):
    """(pass, group, wave, lane) of the thread that takes index i, or None: no thread reads i >= plen"""
    assert 0 <= i < n
    if i >= plen:
        return None
    step = batch_groups(n) * SUM_TB
    t = i % step
    return i // step, t // SUM_TB, t % SUM_TB // WAVE, t % WAVE


def batch_pass_threads(n, plen, p):
    """the threads of one vector that take pass p (they are threads 0 .. count - 1 of the grid's x)"""
    step = batch_groups(n) * SUM_TB
    return max(0, min(step, plen - p * step))


def batch_pass_groups(n, plen, p):
    """the workgroups with at least one thread in pass p"""
    return _ceil(batch_pass_threads(n, plen, p), SUM_TB)


def batch_chunks(b, n, tuning=0):
    """fr_eval_lagrange_batch_t: chunk = tuning or max(1, BATCH_SCRATCH_BYTES / (n * 64)), at most b and
    BATCH_MAX_CHUNK; the list of (j0, cb)"""
    if b == 0:
        return []
    chunk = tuning if tuning > 0 else max(1, BATCH_SCRATCH_BYTES // (n * 64))
    chunk = min(chunk, b, BATCH_MAX_CHUNK)
    return [(j0, min(chunk, b - j0)) for j0 in range(0, b, chunk)]


def blob_plan(total):
    """(blocks, passes) of blob_intake_kernel / blob_output_kernel: idx += blocks * BLOB_TB below total"""
    blocks = min(_ceil(total, BLOB_TB), BLOB_MAXG)
    return blocks, _ceil(total, blocks * BLOB_TB)


# ---- the definitions -------------------------------------------------------------------------------------------------

def _batch_inverse(d, r):
    """d[i]^-1 for non-zero d[i], with one modular inversion (Montgomery's trick)"""
    pre, acc = [], 1
    for v in d:
        pre.append(acc)
        acc = acc * v % r
    inv = pow(acc, -1, r)
    out = [0] * len(d)
    for i in range(len(d) - 1, -1, -1):
        out[i] = inv * pre[i] % r
        inv = inv * d[i] % r
    return out


def ref_barycentric(vals, n, w, z, r):
    """p(z) of the interpolant of len(vals) <= n values over {w^i} (zero from len(vals) on):
    (z^n - 1)/n * sum_i vals[i] w^i / (z - w^i); for z = w^m the value vals[m] itself, 0 past the end"""
    assert len(vals) <= n
    in_domain = pow(z, n, r) == 1
    wi, d, x = [], [], 1
    for i in range(len(vals)):
        if x == z:
            return vals[i] % r
        wi.append(x)
        d.append((z - x) % r)
        x = x * w % r
    if in_domain:                                              # z = w^m with m >= len(vals)
        return 0
    inv = _batch_inverse(d, r)
    s = 0
    for v, x, iv in zip(vals, wi, inv):
        s += v * x % r * iv
    return (pow(z, n, r) - 1) * pow(n, -1, r) % r * (s % r) % r


def ref_quotient_on_domain(P, n, w, z, r):
    """(y, q): y = p(z) and the quotient (p(X) - y)/(X - z) as values on the domain, q_i = (P_i - y)/(w^i - z); for
    z = w^m the term q_m = sum_(i != m) (P_i - y) w^i / (z (z - w^i)) (EIP-4844,
    compute_quotient_eval_within_domain)"""
    P = [v % r for v in P] + [0] * (n - len(P))
    y = ref_barycentric(P, n, w, z, r)
    wi, x = [], 1
    for _ in range(n):
        wi.append(x)
        x = x * w % r
    m = wi.index(z) if z in wi else None
    d = [(x - z) % r if i != m else 1 for i, x in enumerate(wi)]
    inv = _batch_inverse(d, r)
    q = [(P[i] - y) * inv[i] % r for i in range(n)]
    if m is not None:
        zinv = pow(z, -1, r)
        q[m] = sum((P[i] - y) * wi[i] % r * zinv % r * (r - inv[i]) for i in range(n) if i != m) % r
    return y, q


def ref_lagrange_scalars(n, w, tau, r):
    """L_i(tau) = (tau^n - 1)/n * w^i / (tau - w^i), e_m for tau = w^m"""
    wi, x = [], 1
    for _ in range(n):
        wi.append(x)
        x = x * w % r
    if tau in wi:
        return [1 if x == tau else 0 for x in wi]
    c = (pow(tau, n, r) - 1) * pow(n, -1, r) % r
    inv = _batch_inverse([(tau - x) % r for x in wi], r)
    return [c * x % r * iv % r for x, iv in zip(wi, inv)]


def two_point_value(v0, v1, z, r):
    """the interpolant of (v0, v1) over {1, -1} at z: (v0 + v1)/2 + (v0 - v1) z/2"""
    half = pow(2, -1, r)
    return ((v0 + v1) * half + (v0 - v1) * half % r * z) % r


def point(spec, w, r, rng):
    if spec[0] == "random":
        return rng.randrange(2, r)
    if spec[0] == "zero":
        return 0
    assert spec[0] == "w"
    return pow(w, spec[1], r)


def random_values(rng, n, r, runs=()):
    """n random elements with r - 1 on every [a, b) of `runs`"""
    v = [rng.randrange(r) for _ in range(n)]
    for a, b in runs:
        for i in range(max(a, 0), min(b, n)):
            v[i] = r - 1
    return v


def batch_vectors(table, log_n, w, r, seed):
    """(vecs, zs, want) of a batched call from a table of (len, point): random values with runs of r - 1 around the
    ends of the passes, expected values by ref_barycentric"""
    n = 1 << log_n
    rng = random.Random(seed)
    step = batch_groups(n) * SUM_TB
    runs = [(0, 3)] + [(e - 2, e + 2) for e in range(step, n + 1, step)]
    vecs, zs = [], []
    for ln, spec in table:
        vecs.append(random_values(rng, ln, r, runs))
        zs.append(point(spec, w, r, rng))
    want = [ref_barycentric(v, n, w, z, r) for v, z in zip(vecs, zs)]
    return vecs, zs, want


# ---- (a) the batched pass at two and at four passes ------------------------------------------------------------------

BATCH13_LOG_N = 13                 # n = 8192: 32 workgroups, step 4096, two passes
BATCH13_TABLE = (
    ("full:random", 8192, ("random",)),
    ("full:last-of-pass-0", 8192, ("w", 4095)),
    ("full:first-of-pass-1", 8192, ("w", 4096)),
    ("full:last-of-pass-1", 8192, ("w", 8191)),
    ("one-pass-exactly:random", 4096, ("random",)),
    ("one-thread-in-pass-1:random", 4097, ("random",)),
    ("one-thread-in-pass-1:it-finds-z", 4097, ("w", 4096)),
    ("one-thread-in-pass-1:z-past-the-end", 4097, ("w", 5000)),
    ("one-group-in-pass-1:random", 4224, ("random",)),
    ("all-but-one:last-value", 8191, ("w", 8190)),
    ("one-value:z=0", 1, ("zero",)),
    ("no-values:z-in-domain", 0, ("w", 3)),
)
BATCH14_LOG_N = 14                 # n = 16384: four passes
BATCH14_TABLE = (
    ("full:random", 16384, ("random",)),
    ("one-thread-in-pass-3:it-finds-z", 12289, ("w", 12288)),
    ("three-passes-exactly:random", 12288, ("random",)),
)
BATCH_TUNED_CHUNK = 5              # the same calls again in chunks of 5

# ---- (b) the grid's y limit ------------------------------------------------------------------------------------------

YLIMIT_LOG_N = 1
YLIMIT_B = 65537
YLIMIT_STRIDE = 3
YLIMIT_POINTS = ("random", "one", "minus-one", "zero")        # vector j takes YLIMIT_POINTS[j % 4]; r - 1 is w


def ylimit_len(j):
    """0, 1, 2 in turn, started so that both vectors of the second chunk (65535, 65536) hold values"""
    return (j + 1) % 3


def ylimit_batch(r, seed):
    """(lens, v0, v1, zs, want): want by the closed form for two points, a value beyond lens[j] counting as zero"""
    rng = random.Random(seed)
    lens, v0, v1, zs, want = [], [], [], [], []
    for j in range(YLIMIT_B):
        ln = ylimit_len(j)
        a, b = rng.randrange(r), rng.randrange(r)
        z = {"random": rng.randrange(2, r - 1), "one": 1, "minus-one": r - 1, "zero": 0}[YLIMIT_POINTS[j % 4]]
        lens.append(ln)
        v0.append(a)
        v1.append(b)
        zs.append(z)
        want.append(two_point_value(a if ln > 0 else 0, b if ln > 1 else 0, z, r))
    return lens, v0, v1, zs, want


# ---- (c) in-domain index past the end, across chunk edges ------------------------------------------------------------

PAST_LOG_N = 5
PAST_CHUNK = 3                     # 7 vectors: chunks of 3, 3 and 1
PAST_TABLE = (                     # (len, m): z = w^m with m >= len > 0 (value 0) or m = len - 1 (the last value)
    (1, 1), (17, 16), (16, 16), (32, 31), (31, 31), (12, 20), (1, 0),
)

# ---- (d) scratch growth with work queued -----------------------------------------------------------------------------

SMALL_LOG_N = 3
SMALL_TABLE = (("small:random", 8, ("random",)), ("small:in-domain", 5, ("w", 2)))

# ---- (e) the single vector at two passes -----------------------------------------------------------------------------

SINGLE_LOG_N = 19                  # n = 2^19: 2048 workgroups, step 2^18, two passes
SINGLE_SHORT = (1 << 18) + 1       # one thread in the second pass
SINGLE_TABLE = (
    ("full:random", 1 << 19, ("random",)),
    ("full:z-in-pass-1", 1 << 19, ("w", (1 << 18) + 77)),
    ("short:random", SINGLE_SHORT, ("random",)),
    ("short:z-is-the-last-value", SINGLE_SHORT, ("w", 1 << 18)),
    ("short:z-past-the-end", SINGLE_SHORT, ("w", (1 << 18) + 1)),
)

# ---- (f) the opening and the key against the definition --------------------------------------------------------------

OPEN_LOG_N = 10                    # n = 1024: 8 workgroups of the reduction pass, one pass
OPEN_LENS = (1024, 700)            # k = 2, ragged
OPEN_POINTS = (("random",), ("zero",), ("w", 0), ("w", 127), ("w", 128), ("w", 255), ("w", 256), ("w", 1023))
KEY_TAU_EXPONENTS = (0, 255, 256, 1023)
MAXK = 64                          # csrc/lagrange.hip, open_evals_t: `if (k > 64)` -- vectors of one opening


def combine(vecs, lens, xi, n, r):
    """P = sum_j xi^(j+1) f_j, a vector counting as zero from lens[j] on"""
    P, xp = [0] * n, 1
    for v, ln in zip(vecs, lens):
        xp = xp * xi % r
        for i in range(ln):
            P[i] = (P[i] + xp * v[i]) % r
    return P


def proof_scalar(P, n, w, z, tau, r):
    """(y, s): the opening of P at z is [s] G1 with s = sum_i q_i L_i(tau)"""
    y, q = ref_quotient_on_domain(P, n, w, z, r)
    return y, sum(a * b for a, b in zip(q, ref_lagrange_scalars(n, w, tau, r))) % r


# ---- the blob kernels past one pass ----------------------------------------------------------------------------------

BLOB_LOG_N = 12
BLOB_B = 513                       # total = 2^21 + 4096 elements: the second pass is the last blob
BLOB_TOTAL = BLOB_B << BLOB_LOG_N
BLOB_PLANTED = (0, (1 << 21) - 1, 1 << 21, BLOB_TOTAL - 1)    # flat indices: both ends of both passes
BLOB_PLANTED_BLOBS = (0, 511, 512)
BLOB_LONE = 1 << 21                # the first element of the second pass, alone
