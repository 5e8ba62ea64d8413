"""What tests/test_lagrange_edges_gpu.py and tests/test_blob_stride_gpu.py cover, pinned on the CPU: the constants of
tests/lagrange_cases.py are those of csrc/lagrange.hip and csrc/blob.hip, the definitions are the oracle's interpolant,
and every labelled case hits the regime its label names.  An edit of the kernels' constants or of the case tables that
makes a case test nothing fails here."""
import os
import random
import re

import pytest

import lagrange_cases as L
from oracle import py_oracle as O

FIELDS = {"bls12_381": O.BLS12_381, "bn254": O.BN254}
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kzg_snark_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_constants_are_the_sources():
    src = source("lagrange.hip")
    for name in ("SUM_TB", "SUM_MAXG", "BATCH_MAXG"):
        found = re.findall(r"^constexpr uint32_t %s = (\d+);" % name, src, flags=re.M)
        assert [int(x) for x in found] == [getattr(L, name)], name
    found = re.findall(r"^constexpr size_t BATCH_MAX_CHUNK = (\d+);", src, flags=re.M)
    assert [int(x) for x in found] == [L.BATCH_MAX_CHUNK]
    found = re.findall(r"^constexpr size_t BATCH_SCRATCH_BYTES = \(size_t\)1 << (\d+);", src, flags=re.M)
    assert [1 << int(x) for x in found] == [L.BATCH_SCRATCH_BYTES]
    # the plans around the constants
    assert len(re.findall(r"groups = std::min<uint32_t>\(SUM_MAXG, \((?:uint32_t\)\(\()?n \+ SUM_TB - 1\) / SUM_TB\)",
                          src)) == 3                            # value_pass and the two scratch sizes
    assert len(re.findall(r"groups = std::min<uint32_t>\(BATCH_MAXG, \(uint32_t\)\(\(n \+ SUM_TB - 1\) / SUM_TB\)\)",
                          src)) == 1
    assert re.search(r"size_t chunk = c->tune_eval_batch_chunk > 0 \? \(size_t\)c->tune_eval_batch_chunk\s*"
                     r": std::max<size_t>\(1, BATCH_SCRATCH_BYTES / \(n \* 64\)\);\s*"
                     r"chunk = std::min<size_t>\(\{chunk, b, BATCH_MAX_CHUNK\}\);", src)
    assert re.search(r"lagr_sums_kernel<F>, dim3\(groups\), dim3\(SUM_TB\)", src)
    assert re.search(r"lagr_batch_sums_kernel<F>, dim3\(groups, \(uint32_t\)cb\), dim3\(SUM_TB\)", src)
    assert re.search(r"i < n; i \+= stride\)", src) and re.search(r"i < plen; i \+= step\)", src)
    assert re.search(r"if \(k > %d\) return set_err\(c, KZG_ERR_ARG, \"kzg_open_evals" % L.MAXK, src)
    assert L.WAVE == 64 and "threadIdx.x & 63u, wave = threadIdx.x >> 6" in src
    # the two literals of each of the two blob launches
    blob = source("blob.hip")
    found = re.findall(r"blocks = \(uint32_t\)std::min<size_t>\(\(total \+ (\d+)\) / (\d+), (\d+)\);", blob)
    assert found == [(str(L.BLOB_TB - 1), str(L.BLOB_TB), str(L.BLOB_MAXG))] * 2
    for kernel in ("blob_intake_kernel", "blob_output_kernel"):
        assert re.findall(r"hipLaunchKernelGGL\(%s<F>, dim3\(blocks\), dim3\((\d+)\)" % kernel, blob) == \
            [str(L.BLOB_TB)], kernel
        assert re.findall(r"__launch_bounds__\((\d+)\) void %s" % kernel, blob) == [str(L.BLOB_TB)], kernel
    assert len(re.findall(r"idx < total; idx \+= step\)", blob)) == 2


def test_the_plans():
    assert L.sums_plan(1 << 12) == (32, 1) and L.sums_plan(1 << 18) == (2048, 1)
    assert L.sums_plan((1 << 18) + 1) == (2048, 2) and L.sums_plan(1 << 19) == (2048, 2)
    assert L.sums_plan(2) == (1, 1) and L.sums_plan(129) == (2, 1) and L.sums_plan(1 << 20) == (2048, 4)
    assert L.sums_place(1 << 20, 12345) == (0, 96, 0, 57)      # the one large in-domain index of the older tests
    assert L.sums_place(1 << 19, (1 << 18) + 77) == (1, 0, 1, 13)
    assert L.batch_plan(1 << 12, 1 << 12) == (32, 1)           # the largest domain of the older tests: one pass
    assert L.batch_plan(1 << 13, 1 << 13) == (32, 2) and L.batch_plan(1 << 14, 1 << 14) == (32, 4)
    assert L.batch_plan(2, 2) == (1, 1) and L.batch_plan(32, 0) == (1, 0)
    assert L.batch_place(8192, 8192, 4096) == (1, 0, 0, 0) and L.batch_place(8192, 4096, 4096) is None
    for n in (2, 32, 8192):                                    # every index is some thread's, once
        step = L.batch_groups(n) * L.SUM_TB
        places = [L.batch_place(n, n, i) for i in range(n)]
        assert len(set(places)) == n
        assert all(p * step + g * L.SUM_TB + wv * L.WAVE + ln == i for i, (p, g, wv, ln) in enumerate(places))
        if n <= L.BATCH_MAXG * L.SUM_TB:                        # within one pass of either form the walks are the same
            assert places == [L.sums_place(n, i) for i in range(n)]
    assert L.batch_chunks(0, 2) == [] and L.batch_chunks(5, 32, 2) == [(0, 2), (2, 2), (4, 1)]
    assert L.batch_chunks(3, 1 << 24) == [(0, 1), (1, 1), (2, 1)]              # a vector's scratch alone is 1 GiB
    assert L.batch_chunks(70000, 1 << 13) == [(j, min(2048, 70000 - j)) for j in range(0, 70000, 2048)]
    assert L.blob_plan(65 * 256) == (65, 1) and L.blob_plan(1 << 21) == (8192, 1)
    assert L.blob_plan((1 << 21) + 1) == (8192, 2) and L.blob_plan(1 << 26) == (8192, 32)


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_the_definitions_are_the_oracles_interpolant(field):
    cv = FIELDS[field]
    r = cv.r
    rng = random.Random(31)
    for n in (2, 4, 16, 64):
        w = cv.root_of_unity(n)
        points = [rng.randrange(r), 0, 1, w, pow(w, n - 1, r), pow(w, n // 2, r), pow(w, n // 2 + 1, r)]
        for ln in sorted({n, n // 2 + 1, n // 2, 1, 0}):
            vals = L.random_values(rng, ln, r, [(0, 1)])
            coeffs = O.ifft_ff(vals + [0] * (n - ln), w, r)
            for z in points:
                y = L.ref_barycentric(vals, n, w, z, r)
                assert y == O.poly_eval(coeffs, z, r), (n, ln, z)
                qc, pz = O.poly_divide_linear(coeffs, z, r)
                y2, q = L.ref_quotient_on_domain(vals, n, w, z, r)
                assert y2 == y == pz
                assert q == O.fft_ff(qc + [0] * (n - len(qc)), w, r), (n, ln, z)
        # the key's scalars: sum_i f_i L_i(tau) = p(tau), at a tau outside the domain and at every tau inside
        vals = L.random_values(rng, n, r)
        coeffs = O.ifft_ff(list(vals), w, r)
        for tau in [rng.randrange(r)] + [pow(w, m, r) for m in range(n)]:
            lam = L.ref_lagrange_scalars(n, w, tau, r)
            assert sum(a * b for a, b in zip(vals, lam)) % r == O.poly_eval(coeffs, tau, r)
        assert L.ref_lagrange_scalars(n, w, pow(w, n - 1, r), r) == [0] * (n - 1) + [1]
    assert L.two_point_value(5, 9, 1, r) == 5 and L.two_point_value(5, 9, r - 1, r) == 9
    assert L.two_point_value(5, 9, 0, r) == 7 and cv.root_of_unity(2) == r - 1
    # the opening's scalar: [s] G1 is the coefficient opening, s = q(tau)
    n, w = 16, cv.root_of_unity(16)
    vecs, lens, xi, tau = [L.random_values(rng, 16, r), L.random_values(rng, 9, r)], [16, 9], rng.randrange(r), 987654321
    P = L.combine(vecs, lens, xi, n, r)
    assert P == [(xi * vecs[0][i] + (xi * xi * vecs[1][i] if i < 9 else 0)) % r for i in range(16)]
    for z in (rng.randrange(r), pow(w, 5, r)):
        qc, pz = O.poly_divide_linear(O.ifft_ff(list(P), w, r), z, r)
        assert L.proof_scalar(P, n, w, z, tau, r) == (pz, O.poly_eval(qc, tau, r))


def labelled(table):
    labels = [row[0] for row in table]
    assert len(set(labels)) == len(labels)
    return {row[0]: row[1:] for row in table}


def test_the_batched_cases_hit_the_passes_they_name():
    n = 1 << L.BATCH13_LOG_N
    step = L.batch_groups(n) * L.SUM_TB
    assert (n, L.batch_groups(n), step) == (8192, 32, 4096)
    t = labelled(L.BATCH13_TABLE)
    assert [(ln, z) for ln, z in t.values()] == [
        (8192, ("random",)), (8192, ("w", 4095)), (8192, ("w", 4096)), (8192, ("w", 8191)), (4096, ("random",)),
        (4097, ("random",)), (4097, ("w", 4096)), (4097, ("w", 5000)), (4224, ("random",)), (8191, ("w", 8190)),
        (1, ("zero",)), (0, ("w", 3))]                          # the issue's table, in its order
    passes = {k: L.batch_plan(n, ln)[1] for k, (ln, _) in t.items()}
    assert passes == {"full:random": 2, "full:last-of-pass-0": 2, "full:first-of-pass-1": 2, "full:last-of-pass-1": 2,
                      "one-pass-exactly:random": 1, "one-thread-in-pass-1:random": 2,
                      "one-thread-in-pass-1:it-finds-z": 2, "one-thread-in-pass-1:z-past-the-end": 2,
                      "one-group-in-pass-1:random": 2, "all-but-one:last-value": 2, "one-value:z=0": 1,
                      "no-values:z-in-domain": 0}

    def place(label):
        ln, z = t[label]
        return L.batch_place(n, ln, z[1])

    assert place("full:last-of-pass-0") == (0, 31, 1, 63)      # the last thread of the grid, first pass
    assert place("full:first-of-pass-1") == (1, 0, 0, 0)       # the first thread, second pass
    assert place("full:last-of-pass-1") == (1, 31, 1, 63)
    assert place("one-thread-in-pass-1:it-finds-z") == (1, 0, 0, 0)
    assert place("one-thread-in-pass-1:z-past-the-end") is None and 5000 >= 4097 > 0
    assert place("all-but-one:last-value") == (1, 31, 1, 62)
    assert place("no-values:z-in-domain") is None
    for k, (ln, _) in t.items():
        if k.startswith("one-thread-in-pass-1"):                # the second pass is one thread's
            assert L.batch_pass_threads(n, ln, 0) == step and L.batch_pass_threads(n, ln, 1) == 1
        if k.startswith("one-group-in-pass-1"):                 # or one whole workgroup's and nobody else's
            assert L.batch_pass_threads(n, ln, 1) == L.SUM_TB and L.batch_pass_groups(n, ln, 1) == 1
        if k.startswith("one-pass-exactly"):
            assert L.batch_pass_threads(n, ln, 0) == step and L.batch_pass_threads(n, ln, 1) == 0
    assert L.batch_pass_threads(n, 8191, 1) == step - 1 and L.batch_pass_groups(n, 8191, 1) == 32
    # the runs of r - 1 lie across the end of every pass
    r = FIELDS["bn254"].r
    v = L.random_values(random.Random(1), n, r, [(0, 3), (4094, 4098), (8190, 8194)])
    assert [i for i, x in enumerate(v) if x == r - 1] == [0, 1, 2, 4094, 4095, 4096, 4097, 8190, 8191]
    # four passes
    n = 1 << L.BATCH14_LOG_N
    t = labelled(L.BATCH14_TABLE)
    assert L.batch_groups(n) * L.SUM_TB == 4096
    assert [L.batch_plan(n, ln)[1] for ln, _ in t.values()] == [4, 4, 3]
    assert L.batch_place(n, 12289, 12288) == (3, 0, 0, 0) and L.batch_pass_threads(n, 12289, 3) == 1
    assert L.batch_pass_threads(n, 12288, 2) == 4096 and L.batch_pass_threads(n, 12288, 3) == 0
    assert t["one-thread-in-pass-3:it-finds-z"] == (12289, ("w", 12288))
    # the same calls in chunks: the default is one chunk, the tuned run has an edge inside either batch
    assert L.batch_chunks(12, 1 << 13) == [(0, 12)] and L.batch_chunks(3, 1 << 14) == [(0, 3)]
    assert L.batch_chunks(12, 1 << 13, L.BATCH_TUNED_CHUNK) == [(0, 5), (5, 5), (10, 2)]      # sizes (5, 5, 2)
    assert L.batch_chunks(5, 32, 2) == [(0, 2), (2, 2), (4, 1)]                # the older test's chunks, b = 5
    # scratch growth: the small call fits what no call of the cases above has grown, the large one does not
    assert L.SMALL_LOG_N == 3 and [ln for _, ln, _ in L.SMALL_TABLE] == [8, 5]
    small = (8 * 32 + 2 * 8 * 64 + 2 * 1 * 2 * 9 * 4 + 31) // 32 * 32 + 2 * 4
    large = 8192 * 32 + 12 * 8192 * 64
    assert small < large


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_the_y_limit_batch_straddles_the_grid(field):
    r = FIELDS[field].r
    assert L.batch_chunks(L.YLIMIT_B, 1 << L.YLIMIT_LOG_N) == [(0, 65535), (65535, 2)]
    assert L.YLIMIT_STRIDE > 2
    lens, v0, v1, zs, want = L.ylimit_batch(r, 1)
    assert len(lens) == L.YLIMIT_B == 65537 and set(lens) == {0, 1, 2}
    assert lens[:6] == [1, 2, 0, 1, 2, 0]
    edge = (65534, 65535, 65536)                               # the last of the first launch, the two of the second
    assert [lens[j] for j in edge] == [0, 1, 2]
    assert [L.YLIMIT_POINTS[j % 4] for j in edge] == ["minus-one", "zero", "random"]
    assert [zs[j] for j in edge[:2]] == [r - 1, 0] and zs[65536] not in (0, 1, r - 1)
    # a second launch that read the first launch's points or vectors would give other values
    assert zs[0] != zs[65535] and zs[1] != zs[65536]
    assert want[65535] == v0[65535] * pow(2, -1, r) % r and want[65535] != 0
    assert want[65536] != L.two_point_value(v0[65536], v1[65536], zs[1], r)
    assert want[65536] != L.two_point_value(v0[1], v1[1], zs[65536], r)
    # every (len, point) pair occurs; the closed form is the definition
    assert {(lens[j], j % 4) for j in range(L.YLIMIT_B)} == {(a, b) for a in range(3) for b in range(4)}
    for j in list(range(24)) + list(range(65530, 65537)):
        assert want[j] == L.ref_barycentric([v0[j], v1[j]][:lens[j]], 2, r - 1, zs[j], r), j


def test_the_past_the_end_cases_are_past_the_end():
    n = 1 << L.PAST_LOG_N
    assert L.batch_chunks(len(L.PAST_TABLE), n, L.PAST_CHUNK) == [(0, 3), (3, 3), (6, 1)]
    kinds = []
    for ln, m in L.PAST_TABLE:
        assert 0 < ln <= n and 0 <= m < n and (m >= ln or m == ln - 1)
        kinds.append("past" if m >= ln else "last")
        assert (L.batch_place(n, ln, m) is None) == (m >= ln)
    assert kinds == ["past", "last", "past", "last", "past", "past", "last"]
    for j0, cb in L.batch_chunks(len(L.PAST_TABLE), n, L.PAST_CHUNK)[:2]:      # both kinds in a chunk of several
        assert {"past", "last"} == set(kinds[j0:j0 + cb])
    assert (32, 31) in L.PAST_TABLE and (1, 31) not in L.PAST_TABLE and (1, 1) in L.PAST_TABLE


def test_the_single_vector_cases_hit_the_second_pass():
    n = 1 << L.SINGLE_LOG_N
    assert L.sums_plan(n) == (L.SUM_MAXG, 2) and L.sums_plan(n // 2) == (L.SUM_MAXG, 1)
    t = labelled(L.SINGLE_TABLE)
    assert L.SINGLE_SHORT == (1 << 18) + 1
    assert {k: ln for k, (ln, _) in t.items()} == {
        "full:random": n, "full:z-in-pass-1": n, "short:random": L.SINGLE_SHORT,
        "short:z-is-the-last-value": L.SINGLE_SHORT, "short:z-past-the-end": L.SINGLE_SHORT}
    assert L.sums_place(n, t["full:z-in-pass-1"][1][1]) == (1, 0, 1, 13)
    assert L.sums_place(n, t["short:z-is-the-last-value"][1][1]) == (1, 0, 0, 0)
    assert t["short:z-is-the-last-value"][1][1] == L.SINGLE_SHORT - 1
    assert t["short:z-past-the-end"][1][1] == L.SINGLE_SHORT           # the first index read as zero
    assert L.sums_place(n, L.SINGLE_SHORT)[0] == 1


def test_the_opening_cases_and_the_blob_batch():
    n = 1 << L.OPEN_LOG_N
    assert L.sums_plan(n) == (8, 1) and L.OPEN_LENS == (1024, 700)
    ms = [z[1] for z in L.OPEN_POINTS if z[0] == "w"]
    assert ms == [0, 127, 128, 255, 256, 1023] and L.OPEN_POINTS[:2] == (("random",), ("zero",))
    # the last lane of a workgroup and the first of the next, of the two kernels' workgroups (128 and 256 threads)
    assert [L.sums_place(n, m)[1:] for m in ms] == [(0, 0, 0), (0, 1, 63), (1, 0, 0), (1, 1, 63), (2, 0, 0), (7, 1, 63)]
    assert [m // 256 for m in L.KEY_TAU_EXPONENTS] == [0, 0, 1, 3] and L.KEY_TAU_EXPONENTS == (0, 255, 256, 1023)
    # the blob batch: the second pass is exactly the last blob
    total = L.BLOB_B << L.BLOB_LOG_N
    assert total == L.BLOB_TOTAL == (1 << 21) + 4096 and (L.BLOB_LOG_N, L.BLOB_B) == (12, 513)
    blocks, passes = L.blob_plan(total)
    step = blocks * L.BLOB_TB
    assert (blocks, passes, step) == (8192, 2, 1 << 21) and total - step == 4096 == 1 << L.BLOB_LOG_N
    assert L.blob_plan(total - 4096) == (8192, 1)
    assert L.BLOB_PLANTED == (0, step - 1, step, total - 1) and L.BLOB_LONE == step
    assert tuple(sorted({i >> L.BLOB_LOG_N for i in L.BLOB_PLANTED})) == L.BLOB_PLANTED_BLOBS == (0, 511, 512)
    assert [i // step for i in L.BLOB_PLANTED] == [0, 0, 1, 1]
