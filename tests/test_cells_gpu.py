"""GPU tests of EIP-7594 cells as bytes: kzg_fr_to_blob* against the restatement
(tests/cells_restated.py) and as the exact inverse of kzg_blob_to_fr; the four calls of the specification against the
existing coset engines (open_cosets_each, check_coset, kzg_verify_cosets, recover_cosets) in the restated numbering;
the batch challenge against hashlib.  Equality of integers and bytes everywhere."""
import random

import numpy as np
import pytest

import blob_restated as B
import cells_restated as CR

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
TAU = 0x5eed_1234_abcd_0987_6543_21fe_dcba
SHAPES = [(8, 2, 16), (64, 4, 128), (8, 2, 8), (8, 2, 32)]      # (n, l, N): N = 2n twice, N = n and N = 4n once each


@pytest.fixture(scope="module")
def kzgs():
    from kzg_snark_amd.kzg import KZG
    return {c: KZG(c) for c in CURVES}


def element_bytes(values):
    return b"".join(int(v).to_bytes(32, "big") for v in values)


# ---- 1. kzg_fr_to_blob ------------------------------------------------------------------------------------------------
def value_rows(rng, b, n, r):
    rows = [[rng.randrange(r) for _ in range(n)] for _ in range(b)]
    rows[0][0], rows[b - 1][n - 1] = 0, r - 1
    return rows


def device_fr_to_blob(ctx, vals, log_n, bit_reversed):
    """the _device form between guard bytes: (uint8[b, 32 n], status uint8[b])"""
    import torch
    b, n = vals.shape[0], 1 << log_n
    dev = f"cuda:{ctx.device}"
    d_vals = torch.from_numpy(np.ascontiguousarray(vals).view(np.int64)).to(dev)
    d_out = torch.from_numpy(np.full(32 + b * n * 32 + 32, 0x5a, dtype=np.uint8)).to(dev)
    d_status = torch.from_numpy(np.full(32 + b + 32, 0x5a, dtype=np.uint8)).to(dev)
    torch.cuda.synchronize(ctx.device)
    ctx.fr_to_blob_device(d_vals.data_ptr(), log_n, b, bit_reversed, d_out.data_ptr() + 32, d_status.data_ptr() + 32)
    ctx.synchronize()
    out, status = d_out.cpu().numpy(), d_status.cpu().numpy()
    assert (out[:32] == 0x5a).all() and (out[-32:] == 0x5a).all()
    assert (status[:32] == 0x5a).all() and (status[32 + b:] == 0x5a).all()
    return out[32:-32].reshape(b, 32 * n), status[32:32 + b]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("log_n,b", [(1, 3), (9, 3)])          # six lanes; 1536: above one workgroup, no power of two
@pytest.mark.parametrize("bit_reversed", [False, True])
def test_fr_to_blob_equals_the_restatement_and_inverts_the_intake(kzgs, native, curve, log_n, b, bit_reversed):
    ctx = kzgs[curve]._context()
    r, n = B.R[curve], 1 << log_n
    rng = random.Random(log_n * 10 + b + bit_reversed)
    rows = value_rows(rng, b, n, r)
    vals = native.ints_to_limbs([v for row in rows for v in row]).reshape(b, n, 4)
    want, want_status = CR.fr_to_blob(rows, curve, bit_reversed)
    assert want_status == [0] * b
    for out, status in (ctx.fr_to_blob(vals, log_n, bit_reversed), device_fr_to_blob(ctx, vals, log_n, bit_reversed)):
        assert not status.any()
        assert [row.tobytes() for row in out] == want
        back, back_status = ctx.blob_to_fr(out, log_n, bit_reversed)            # the exact inverse on canonical rows
        assert not back_status.any() and np.array_equal(back, vals)
    if bit_reversed:
        facade = kzgs[curve].values_to_blob(vals, n)
        assert facade == want and facade == kzgs[curve].values_to_blob(rows, n)
        assert np.array_equal(kzgs[curve].blob_to_values(facade, n), vals)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("log_n,b", [(1, 3), (9, 3)])
def test_fr_to_blob_marks_the_row_of_an_element_equal_to_r(kzgs, native, curve, log_n, b):
    ctx = kzgs[curve]._context()
    r, n = B.R[curve], 1 << log_n
    rng = random.Random(log_n + 77)
    for row_at, elem_at in ((0, 0), (1, n - 1), (b - 1, n // 2)):
        rows = value_rows(rng, b, n, r)
        rows[row_at][elem_at] = r
        vals = native.ints_to_limbs([v for row in rows for v in row]).reshape(b, n, 4)
        for bit_reversed in (False, True):
            want, want_status = CR.fr_to_blob(rows, curve, bit_reversed)
            at = CR.brp(elem_at, log_n) if bit_reversed else elem_at             # byte element `at` reads value elem_at
            for out, status in (ctx.fr_to_blob(vals, log_n, bit_reversed),
                                device_fr_to_blob(ctx, vals, log_n, bit_reversed)):
                assert list(np.flatnonzero(status)) == [row_at] == list(np.flatnonzero(want_status))
                assert status[row_at] == 1
                assert not out[row_at, 32 * at:32 * at + 32].any()               # zero bytes
                assert [row.tobytes() for row in out] == want                    # everything else still correct
    with pytest.raises(ValueError, match="row 1"):
        bad = value_rows(rng, 2, n, r)
        bad[1][0] = r
        kzgs[curve].values_to_blob(bad, n)


def test_fr_to_blob_argument_errors_and_empty_batches(kzgs, native):
    ctx = kzgs["bls12_381"]._context()
    lib, vp = native.lib(), native._as_vp
    vals, out, status = np.zeros((1, 2, 4), dtype=np.uint64), np.zeros((1, 64), dtype=np.uint8), np.zeros(1, np.uint8)
    assert lib.kzg_fr_to_blob(ctx._h, 1, vp(vals), 1, 1, vp(out), vp(status)) == 0
    assert lib.kzg_fr_to_blob(ctx._h, 0, vp(vals), 1, 1, vp(out), vp(status)) == -1           # log_n = 0
    assert lib.kzg_fr_to_blob(ctx._h, 25, vp(vals), 1, 1, vp(out), vp(status)) == -1          # log_n = 25
    assert lib.kzg_fr_to_blob(ctx._h, 24, vp(vals), 5, 1, vp(out), vp(status)) == -1          # 5 * 2^24 > 2^26
    assert lib.kzg_fr_to_blob(ctx._h, 1, None, 0, 1, None, None) == 0                         # b = 0: no work
    assert lib.kzg_fr_to_blob_device(ctx._h, 1, 48, 1, 1, 64, 64) == -1                       # d_vals not 32-aligned
    assert lib.kzg_fr_to_blob_device(ctx._h, 1, 64, 1, 1, 72, 64) == -1                       # d_bytes not 16-aligned
    assert lib.kzg_fr_to_blob(ctx._h, 1, vp(vals), 1, 1, vp(out), vp(status)) == 0            # still usable


def test_pending_commits_stay_pending_and_correct_across_fr_to_blob(kzgs, native):
    import torch
    curve = "bls12_381"
    kzg = kzgs[curve]
    ctx = kzg._context()
    L, r = ctx.fp_limbs, B.R[curve]
    n = 1 << 12
    ck = kzg.setup(n - 1, tau=TAU)[0]
    rng = np.random.default_rng(6)
    polys = rng.integers(0, 1 << 63, size=(2, n, 4), dtype=np.uint64)
    polys[..., 3] %= np.uint64(r >> 192)
    want_xy, want_inf = ctx.commit(ck.srs, polys, [n, n], n)
    d = torch.from_numpy(polys.view(np.int64)).to(f"cuda:{ctx.device}")
    torch.cuda.synchronize(ctx.device)
    out_xy = np.zeros((2, 2 * L), dtype=np.uint64)
    out_inf = np.full(2, 9, dtype=np.uint8)
    ctx.commit_device_async(ck.srs, d.data_ptr(), [n, n], n, out_xy, out_inf)
    out, status = ctx.fr_to_blob(polys.reshape(2 * n // 8, 8, 4), 3, True)
    assert len(ctx._inflight) == 1 and (out_inf == 9).all()               # not retired: delivered at the flush
    ctx.commit_flush()
    assert (out_xy == want_xy).all() and (out_inf == want_inf).all()
    rows = [native.limbs_to_ints(row) for row in polys.reshape(-1, 8, 4)]
    assert [row.tobytes() for row in out] == CR.fr_to_blob(rows, curve, True)[0] and not status.any()


# ---- 2. compute_cells / compute_cells_and_kzg_proofs ---------------------------------------------------------------------
class Case:
    """One (curve, n, l, N): key, blobs and what the existing engines say about them, computed once"""

    def __init__(self, kzg, curve, n, l, N, randoms):
        self.kzg, self.curve, self.n, self.l, self.N, self.C = kzg, curve, n, l, N, N // l
        r = self.r = B.R[curve]
        rng = random.Random(n * 1000 + N + len(curve))
        self.ck, _ = kzg.setup(n - 1, tau=TAU)
        self.rk_l = kzg.coset_verification_key(l, TAU)
        self.w = int(kzg.Fq.root_of_unity(N))
        w_n = pow(self.w, N // n, r)
        log_n = n.bit_length() - 1
        rows = [[rng.randrange(r) for _ in range(n)] for _ in range(randoms)] + [[0] * n, [r - 1] * n]
        self.blobs = [element_bytes(row) for row in rows]
        # the coefficients by the inverse transform written out: blob element i is p(w_n^brp(i))
        inv_n = pow(n, -1, r)
        self.coeffs = []
        for row in rows:
            natural = B.intake(element_bytes(row), n, curve)[0]
            self.coeffs.append([sum(natural[t] * pow(w_n, -t * k % n, r) for t in range(n)) * inv_n % r
                                for k in range(n)])
        self.ref_proofs, self.ref_values = kzg.open_cosets_each(self.ck, self.coeffs, l, n=n, N=N, with_values=True)
        self.commitments = kzg.commit(self.ck, self.coeffs)
        self.cells, self.proofs = kzg.compute_cells_and_kzg_proofs(self.table, self.blobs, l, N=N)


    @property
    def table(self):
        """asked for at every use: the facade keeps two tables and closes the ones it drops"""
        return self.kzg.coset_table(self.ck, self.n, self.l)


@pytest.fixture(scope="module")
def cases(kzgs):
    made = {}

    def get(curve, shape, randoms=1):
        key = (curve, shape)
        if key not in made:
            made[key] = Case(kzgs[curve], curve, *shape, randoms=randoms)
        return made[key]
    return get


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("shape", SHAPES)
def test_cells_and_proofs_equal_the_coset_engine_in_the_restated_numbering(cases, curve, shape):
    cs = cases(curve, shape, randoms=2 if shape == SHAPES[0] else 1)
    kzg, n, l, N, C = cs.kzg, cs.n, cs.l, cs.N, cs.C
    b = len(cs.blobs)
    assert len(cs.cells) == len(cs.proofs) == b
    for j in range(b):
        assert cs.cells[j] == CR.cells_of_coset_values(cs.ref_values[j], l)
        want = kzg.compress_g1(cs.ref_proofs[j])
        assert cs.proofs[j] == [want[CR.coset_of_cell(c, C)] for c in range(C)]
        assert all(isinstance(x, bytes) and len(x) == 32 * l for x in cs.cells[j]) and len(cs.cells[j]) == C
    zero, top = b - 2, b - 1
    assert cs.cells[zero] == [bytes(32 * l)] * C                               # the zero blob
    assert cs.proofs[zero] == kzg.compress_g1([(1, 1, 0)]) * C                 # proofs at infinity
    assert cs.cells[top] == [element_bytes([cs.r - 1] * l)] * C                # the constant r - 1
    # the other entries give the same bytes
    assert kzg.compute_cells(cs.blobs, n, l, N=N) == cs.cells
    assert kzg.compute_cells_and_kzg_proofs(cs.ck, cs.blobs, l, n=n, N=N, w=cs.w) == (cs.cells, cs.proofs)
    # on the blob's own domain the cells are the blob cut in pieces
    if N == n:
        assert [b"".join(cells) for cells in cs.cells] == cs.blobs


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("shape", SHAPES)
def test_every_cell_and_proof_passes_the_host_check(cases, curve, shape):
    """check_coset (two pairings of pairing.py per cell) on what the call returned, decoded by the restatement"""
    cs = cases(curve, shape, randoms=2 if shape == SHAPES[0] else 1)
    kzg, l, C, r = cs.kzg, cs.l, cs.C, cs.r
    zeta = pow(cs.w, C, r)
    for j in range(len(cs.blobs)):
        points = kzg.decompress_g1(cs.proofs[j])
        for c in range(C):
            h = pow(cs.w, CR.coset_of_cell(c, C), r)
            values = CR.coset_values_of_cell(cs.cells[j][c], l)
            assert kzg.check_coset(cs.ck, cs.rk_l, [cs.commitments[j]], h, [values], points[c], 1, zeta), (j, c)


@pytest.mark.parametrize("curve", CURVES)
def test_compute_cells_names_the_blob_with_an_element_above_r(cases, curve):
    cs = cases(curve, SHAPES[0], randoms=2)
    bad = list(cs.blobs)
    bad[1] = bad[1][:32 * 3] + cs.r.to_bytes(32, "big") + bad[1][32 * 4:]
    with pytest.raises(ValueError, match="blob 1: element 3 "):
        cs.kzg.compute_cells(bad, cs.n, cs.l, N=cs.N)
    with pytest.raises(ValueError, match="blob 1: element 3 "):
        cs.kzg.compute_cells_and_kzg_proofs(cs.table, bad, cs.l, N=cs.N)
    with pytest.raises(ValueError):
        cs.kzg.compute_cells_and_kzg_proofs(cs.table, cs.blobs, cs.l, n=2 * cs.n, N=cs.N)   # not the table's n
    with pytest.raises(ValueError):
        cs.kzg.compute_cells_and_kzg_proofs(cs.table, cs.blobs, 2 * cs.l, N=cs.N)           # not the table's l
    assert cs.kzg.compute_cells_and_kzg_proofs(cs.table, [], cs.l, N=cs.N) == ([], [])


# ---- 3. verify_cell_kzg_proof_batch ------------------------------------------------------------------------------------------
def batch_of(cs, rng):
    """every cell of the two random blobs, shuffled, with repeats: (commitments, cell indices, cells, proofs)"""
    comms = [cs.kzg.compress_g1([c])[0] for c in cs.commitments]
    picks = [(j, c) for j in range(2) for c in range(cs.C)]
    picks += [picks[3], picks[cs.C + 1], picks[3]]
    rng.shuffle(picks)
    return ([comms[j] for j, _ in picks], [c for _, c in picks], [cs.cells[j][c] for j, c in picks],
            [cs.proofs[j][c] for j, c in picks])


@pytest.mark.parametrize("curve", CURVES)
def test_verify_cell_batch_accepts_and_rejects(cases, curve, monkeypatch):
    cs = cases(curve, SHAPES[0], randoms=2)
    kzg, n, l, N, C, r = cs.kzg, cs.n, cs.l, cs.N, cs.C, cs.r
    comms, idx, cells, proofs = batch_of(cs, random.Random(9))
    K = len(idx)
    assert K == 2 * C + 3

    seen = []
    real = kzg._cell_batch_rho

    def recording(*args):
        seen.append(real(*args))
        return seen[-1]
    monkeypatch.setattr(kzg, "_cell_batch_rho", recording)

    def verdict(comms=comms, idx=idx, cells=cells, proofs=proofs, **kw):
        return kzg.verify_cell_kzg_proof_batch(cs.ck, cs.rk_l, comms, idx, cells, proofs, l, N, **kw)

    assert verdict() is True
    distinct, comm_idx = CR.dedup(comms)
    assert len(distinct) == 2
    want_rho = CR.rho(n, l, distinct, comm_idx, idx, cells, proofs, curve)
    assert seen == [want_rho]                                                  # the challenge is the restatement's
    assert verdict(pairing="host") is True
    assert verdict(cells=np.frombuffer(b"".join(cells), dtype=np.uint8).reshape(K, 32 * l), w=cs.w, n=n) is True

    flipped = list(cells)
    raw = bytearray(flipped[5])
    raw[31] ^= 1                                                               # one byte of one cell
    flipped[5] = bytes(raw)
    assert max(CR.coset_values_of_cell(flipped[5], l)) < r
    assert verdict(cells=flipped) is False
    a, b2 = next((a, b2) for a in range(K) for b2 in range(K) if proofs[a] != proofs[b2])
    swapped = list(proofs)
    swapped[a], swapped[b2] = proofs[b2], proofs[a]
    assert verdict(proofs=swapped) is False                                    # one proof swapped with another's
    shifted = list(idx)
    shifted[2] = (shifted[2] + 1) % C
    assert verdict(idx=shifted) is False                                       # a cell index off by one
    with_r = list(cells)
    with_r[K - 1] = with_r[K - 1][:32] + r.to_bytes(32, "big") + with_r[K - 1][64:]
    assert verdict(cells=with_r) is False                                      # an element >= r
    keep = 0x7f if curve == "bls12_381" else 0x3f                              # ZCash: bit 7; gnark: both top bits
    cleared = [bytes([comms[0][0] & keep]) + comms[0][1:]] + comms[1:]
    assert kzg.decompress_g1(cleared[:1], strict=False)[1][0] == 1
    assert verdict(comms=cleared) is False                                     # a commitment with a bad flag byte
    assert verdict(pairing="host", cells=flipped) is False

    assert kzg.verify_cell_kzg_proof_batch(cs.ck, cs.rk_l, [], [], [], [], l, N) is True     # no cells
    for bad in (dict(comms=comms[:-1]), dict(proofs=proofs + proofs[:1]), dict(cells=cells[:-1]), dict(idx=idx[:-1]),
                dict(cells=[cells[0][:-1]] + cells[1:]), dict(comms=[comms[0] + b"\x00"] + comms[1:]),
                dict(idx=[C] + idx[1:]), dict(idx=[-1] + idx[1:]), dict(pairing="both")):
        with pytest.raises(ValueError):
            verdict(**bad)


@pytest.mark.parametrize("curve", CURVES)
def test_verify_cosets_bytes_returns_the_points_of_verify_cosets(cases, native, curve):
    cs = cases(curve, SHAPES[0], randoms=2)
    kzg, l, N, C, r = cs.kzg, cs.l, cs.N, cs.C, cs.r
    ctx = kzg._context()
    comms, idx, cells, proofs = batch_of(cs, random.Random(10))
    K = len(idx)
    distinct, comm_idx = CR.dedup(comms)
    G = ctx.g1_bytes
    cxy, cinf, cst = ctx.g1_decompress(np.frombuffer(b"".join(distinct), dtype=np.uint8).reshape(-1, G))
    pxy, pinf, pst = ctx.g1_decompress(np.frombuffer(b"".join(proofs), dtype=np.uint8).reshape(-1, G))
    assert not cst.any() and not pst.any()
    coset_idx = [CR.coset_of_cell(c, C) for c in idx]
    values = native.ints_to_limbs([v for cell in cells for v in CR.coset_values_of_cell(cell, l)]).reshape(K, l, 4)
    arr = np.frombuffer(b"".join(cells), dtype=np.uint8).reshape(K, 32 * l)
    key = kzg._key(cs.ck)
    rho = 0x1234567 + len(curve)
    args = (key.srs, N.bit_length() - 1, l.bit_length() - 1, cs.w, cxy, cinf, comm_idx, coset_idx)
    want_xy, want_inf = ctx.verify_cosets(*args, values, pxy, pinf, rho)
    xy, inf, status = ctx.verify_cosets_bytes(*args, arr, pxy, pinf, rho, bit_reversed=True)
    assert status == 0 and np.array_equal(xy, want_xy) and np.array_equal(inf, want_inf) and not inf.any()
    # natural order in: the same values written in the library's order
    natural = np.frombuffer(b"".join(element_bytes(CR.coset_values_of_cell(cell, l)) for cell in cells),
                            dtype=np.uint8).reshape(K, 32 * l)
    xy, inf, status = ctx.verify_cosets_bytes(*args, natural, pxy, pinf, rho, bit_reversed=False)
    assert status == 0 and np.array_equal(xy, want_xy) and np.array_equal(inf, want_inf)
    # an element >= r in the last cell: a verdict, both points at infinity
    bad = arr.copy()
    bad[K - 1, 32 * (l - 1):] = np.frombuffer(r.to_bytes(32, "big"), dtype=np.uint8)
    xy, inf, status = ctx.verify_cosets_bytes(*args, bad, pxy, pinf, rho)
    assert status == 1 and list(inf) == [1, 1] and not xy.any()
    xy, inf, status = ctx.verify_cosets_bytes(*args, arr, pxy, pinf, rho)      # the context is usable afterwards
    assert status == 0 and np.array_equal(xy, want_xy)


# ---- 4. recover_cells_and_kzg_proofs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_recover_cells_is_the_identity_on_computed_cells(cases, curve):
    cs = cases(curve, SHAPES[0], randoms=2)
    kzg, n, l, N, C = cs.kzg, cs.n, cs.l, cs.N, cs.C
    rng = random.Random(11)
    order = list(range(C))
    rng.shuffle(order)
    for K in (C // 2, C // 2 + 1, C):
        idx = order[:K]
        given = [[cells[c] for c in idx] for cells in cs.cells]
        assert kzg.recover_cells_and_kzg_proofs(cs.table, idx, given, l, N=N) == (cs.cells, cs.proofs), K
    idx = order[:C // 2]
    given = [[cells[c] for c in idx] for cells in cs.cells]
    assert kzg.recover_cells_and_kzg_proofs(cs.ck, idx, given, l, n=n, N=N, w=cs.w) == (cs.cells, cs.proofs)

    def recover(idx, given):
        return kzg.recover_cells_and_kzg_proofs(cs.table, idx, given, l, N=N)

    few = order[:C // 2 - 1]
    with pytest.raises(ValueError, match="cannot determine"):
        recover(few, [[cells[c] for c in few] for cells in cs.cells])
    rep = order[:C // 2] + order[:1]
    with pytest.raises(ValueError, match="repeated"):
        recover(rep, [[cells[c] for c in rep] for cells in cs.cells])
    more = order[:C // 2 + 1]
    given = [[cells[c] for c in more] for cells in cs.cells]
    raw = bytearray(given[1][2])
    raw[63] ^= 1                                                               # the lowest byte of its second element
    given[1][2] = bytes(raw)
    with pytest.raises(ValueError, match="polynomial 1 lie on no polynomial"):
        recover(more, given)
    given[1][2] = given[1][2][:32] + cs.r.to_bytes(32, "big")
    with pytest.raises(ValueError, match=f"blob 1: cell {more[2]} "):
        recover(more, given)
    with pytest.raises(ValueError):
        recover([C] + more[1:], given)                                         # an index out of range
    with pytest.raises(ValueError):
        recover(more, [g[:-1] for g in given])                                 # fewer cells than indices
    with pytest.raises(ValueError):
        recover(more, [])                                                      # no blob
