"""Drop-in for the reference's kzg.py `KZG` class: same constructor, attributes and
method signatures (kzg.py:18-288), with the data-parallel work -- SRS generation,
commit and open -- executed by the gfx950 engine through the C ABI.

    KZG(curve_type="bn254")                          kzg.py:18
      .G1 .G2 .Z1 .Z2 .multiply .add .neg .eq .pairing .curve_order .Fq .R .X     kzg.py:40-54
    setup(max_degree) -> (ck, tau_G2)                kzg.py:56
    commit(ck, polynomials) -> [point]               kzg.py:80
    open(ck, polynomials, z, xi) -> point            kzg.py:122
    check(rk, commitments, z, evaluations, proof, xi) -> bool            kzg.py:161
    batch_check(rk, commitments_list, z_list, evaluations_list, proof_list, xi_list, r=None)   kzg.py:213
    verify_cosets / verify_domain: any number of coset (or single-point) claims folded on the device, two pairings
    pairing_check / pairing_product: pairing-product equations on the device, the verdict the verifiers below end with
    verify_points / verify_blobs: the same for claims at arbitrary points (blob proofs), evaluate_evaluations_each
    compress_g1 / decompress_g1 / in_subgroup: 48- / 32-byte points and subgroup membership, on the device
    blob_to_kzg_commitment / compute_blob_kzg_proof / verify_blob_kzg_proof_batch: EIP-4844's calls, bytes in and out
    (blob_to_values / blob_challenges: the device intake of blob bytes and the SHA-256 challenges on their own)
    multiply_each / multiply_each_g2 / scale_key: [k_i] P_i per point on the device, the products kept apart
    unit_setup / contribute / verify_contribution / verify_contributions: a powers-of-tau ceremony on top of them

Points are py_ecc-shaped 3-tuples, always normalised: (x, y, 1), infinity (1, 1, 0).
The reference returns un-normalised projective triples whose representative
depends on py_ecc's operation order; equality there is `eq`, here plain `==` works
too.  There is no CPU fallback for commit/open/setup: they raise
_native.NativeUnavailable without the shared library and a GPU."""
import secrets
from collections import namedtuple
from collections.abc import Sequence
from contextlib import contextmanager

import numpy as np

from . import _native
from . import curve as _curve
from .field import GF, Polynomial, PolynomialRing


def _lru_get(cache, key, capacity, fresh, make, close):
    """cache[key], moved to most recently used, when fresh(entry) says it still stands; else make(), stored in its
    place once close() has released least recently used entries down to capacity - 1.  A stale entry is dropped,
    not closed: its holder may still use it."""
    hit = cache.get(key)
    if hit is not None and fresh(hit):
        cache[key] = cache.pop(key)                                # most recently used last
        return hit
    entry = make()
    cache.pop(key, None)
    while len(cache) >= capacity:
        close(cache.pop(next(iter(cache))))
    cache[key] = entry
    return entry


# what open_multi returns: the two proof points, the challenge used and the values, evaluations[i] along point_sets[i]
OpenMulti = namedtuple("OpenMulti", "W W2 zeta evaluations")
# what a participant publishes beside the new setup (KZG.contribute): [s] G2 and the new [tau] G1
Contribution = namedtuple("Contribution", "pubkey tau_g1")


@contextmanager
def _bad_input_is_value_error():
    """the library's KZG_ERR_ARG (-1: an input it refuses, named in the message) as the facade's ValueError"""
    try:
        yield
    except _native.NativeError as e:
        if e.code == -1:
            raise ValueError(str(e)) from e
        raise


class CommitmentKey(Sequence):
    """The `ck` of the reference: a sequence of G1 points [tau^i G1] (kzg.py:70-72).

    Lives on the device (kzg_srs handle) in the engine's table layout; indexing
    and iteration export points lazily so code that only passes `ck` around and
    takes len(ck) (every in-tree caller) never materialises 2^20 tuples."""

    def __init__(self, ctx, srs):
        self._ctx = ctx
        self.srs = srs
        self._cache = {}

    def __len__(self):
        return self.srs.n

    def __getitem__(self, i):
        if isinstance(i, slice):
            idx = range(*i.indices(len(self)))
            return [self[j] for j in idx]
        n = len(self)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError("commitment key index out of range")
        if i not in self._cache:
            start = (i // 1024) * 1024
            count = min(1024, n - start)
            xy, inf = self.srs.export(start, count)
            self._cache.update(enumerate(_native.limbs_to_points(xy, inf), start))
        return self._cache[i]


class LagrangeKey(CommitmentKey):
    """A commitment key in the Lagrange basis of the domain {w^i, i < n}: the points [L_i(tau)] G1.  A Sequence of
    points like CommitmentKey; commit_evaluations / open_evaluations take VALUES f[i] = p(w^i) against it."""

    def __init__(self, ctx, srs, n, w):
        super().__init__(ctx, srs)
        self.n = int(n)
        self.w = int(w)
        self.log_n = self.n.bit_length() - 1


class DomainTable:
    """The FK20 table of one monomial key and domain size n (KZG.domain_table): what open_domain needs to compute all
    n proofs on a domain at once.  Holds 2n affine points on the device.  KZG.coset_table makes one for cosets of l
    points (open_cosets); domain_table's tables have l = 1."""

    def __init__(self, ctx, table, n, l=1):
        self._ctx = ctx
        self.table = table
        self.n = int(n)
        self.log_n = self.n.bit_length() - 1
        self.l = int(l)
        self.log_l = self.l.bit_length() - 1

    def __len__(self):
        return self.n


def parse_trusted_setup(text, g1_size, g2_size):
    """The text of a trusted-setup file (c-kzg-4844's trusted_setup.txt layout) -> (n1, n2, lagrange, g2, monomial),
    the three sections as uint8 arrays [n1, g1_size], [n2, g2_size], [n1, g1_size] of compressed points, nothing
    decoded.  Line 1: n1, line 2: n2 (decimal), then n1 + n2 + n1 lines of hex, one compressed point each: the G1
    Lagrange points, the G2 powers, the G1 powers.  Blank lines and surrounding whitespace are skipped; n1 must be a
    power of two.  Anything else raises ValueError naming the line (as counted in the file) or the section."""
    lines = [(no, ln.strip()) for no, ln in enumerate(text.splitlines(), 1) if ln.strip()]
    if len(lines) < 2:
        raise ValueError("trusted setup: the file ends before the two counts (lines 1 and 2)")
    counts = []
    for (no, ln), what in zip(lines[:2], ("n1, the number of G1 points", "n2, the number of G2 points")):
        if not ln.isdigit():
            raise ValueError(f"trusted setup, line {no}: expected {what} in decimal, found {ln[:40]!r}")
        counts.append(int(ln))
    n1, n2 = counts
    if n1 < 1 or n1 & (n1 - 1):
        raise ValueError(f"trusted setup, line {lines[0][0]}: n1 = {n1} is not a power of two")
    if n2 < 1:
        raise ValueError(f"trusted setup, line {lines[1][0]}: n2 = {n2}: at least the G2 generator is needed")
    body = lines[2:]
    sections = (("G1 Lagrange", n1, g1_size), ("G2", n2, g2_size), ("G1 monomial", n1, g1_size))
    want = 2 * n1 + n2
    out, at = [], 0
    for name, count, size in sections:
        rows = body[at:at + count]
        if len(rows) < count:
            raise ValueError(f"trusted setup: the file is truncated in the {name} section: {len(rows)} of {count} "
                             f"points ({len(body)} point lines where n1 = {n1}, n2 = {n2} announce {want})")
        blob = bytearray()
        for k, (no, ln) in enumerate(rows):
            if len(ln) != 2 * size:
                raise ValueError(f"trusted setup, line {no} ({name} section, point {k}): {len(ln)} hex digits, "
                                 f"expected {2 * size}")
            try:
                blob += bytes.fromhex(ln)
            except ValueError:
                raise ValueError(f"trusted setup, line {no} ({name} section, point {k}): not hexadecimal") from None
        out.append(np.frombuffer(bytes(blob), dtype=np.uint8).reshape(count, size))
        at += count
    if len(body) > want:
        raise ValueError(f"trusted setup, line {body[want][0]}: {len(body) - want} lines more than the counts "
                         f"n1 = {n1}, n2 = {n2} announce")
    return n1, n2, out[0], out[1], out[2]


def format_trusted_setup(lagrange, g2, monomial):
    """The text parse_trusted_setup reads, from the three sections as arrays (or lists) of compressed points."""
    rows = [bytes(b).hex() for sec in (lagrange, g2, monomial) for b in sec]
    return "\n".join([str(len(monomial)), str(len(g2))] + rows) + "\n"


def bit_reverse_rows(rows):
    """rows[bitrev(i)] at i, for a power-of-two number of rows (its own inverse)"""
    n = len(rows)
    bits = n.bit_length() - 1
    idx = [int(format(i, "0%db" % bits)[::-1], 2) if bits else 0 for i in range(n)]
    return rows[idx]


class TrustedSetup:
    """What KZG.load_trusted_setup returns: .monomial (CommitmentKey [tau^i G1]), .lagrange (LagrangeKey over the
    n1-th root of unity), .g2 (the points [tau^j G2]), .rk = g2[1] and .rk_l(l) = g2[l], the verification keys."""

    def __init__(self, monomial, lagrange, g2):
        self.monomial, self.lagrange, self.g2 = monomial, lagrange, list(g2)

    @property
    def rk(self):
        return self.rk_l(1)

    def rk_l(self, l):
        l = int(l)
        if not 0 <= l < len(self.g2):
            raise ValueError(f"the setup holds {len(self.g2)} G2 powers: [tau^{l}] G2 needs at least {l + 1}")
        return self.g2[l]


class KZG:
    def __init__(self, curve_type="bn254"):
        if curve_type not in _curve.CURVES:
            raise ValueError(f"Unsupported curve type: {curve_type}")          # kzg.py:37
        self.curve_type = curve_type
        cv = _curve.CURVES[curve_type]
        self._cv = cv
        self._g1 = _curve.g1_group(cv)
        self._g2 = _curve.g2_group(cv)
        # curve operations with py_ecc's names (kzg.py:40-49)
        self.G1 = (cv.g1[0], cv.g1[1], 1)
        self.G2 = (cv.g2[0], cv.g2[1], (1, 0))
        self.Z1 = self._g1.Z
        self.Z2 = self._g2.Z
        self.curve_order = cv.r
        # field and polynomial ring (kzg.py:52-54)
        self.Fq = GF(cv.r)
        self.R = PolynomialRing(self.Fq, "X")
        self.X = self.R.gen()
        self._ctx = None
        self._loaded = {}          # id(list ck) -> (CommitmentKey, fingerprint); at most _KEY_CACHE entries, LRU
        self._tables = {}          # (id(CommitmentKey), n[, l]) -> (CommitmentKey, DomainTable); _TABLE_CACHE, LRU

    # ---- py_ecc-shaped single-point operations (host; used by the verifiers) ------
    def _grp(self, pt):
        return self._g2 if isinstance(pt[0], tuple) else self._g1

    def multiply(self, pt, n):
        return self._grp(pt).multiply(pt, int(n) % self.curve_order if int(n) >= self.curve_order else int(n))

    def add(self, p1, p2):
        return self._grp(p1).add(p1, p2)

    def neg(self, pt):
        return self._grp(pt).neg(pt)

    def eq(self, p1, p2):
        return self._grp(p1).eq(p1, p2)

    def pairing(self, Q, P):
        """pairing(G2_point, G1_point) as used at kzg.py:208-209, 285-286."""
        from .pairing import pairing as _pairing
        return _pairing(Q, P, self._cv)

    # ---- engine plumbing ------------------------------------------------------------
    def _context(self):
        if self._ctx is None:
            self._ctx = _native.get_context(self.curve_type)
        return self._ctx

    _TABLE_CACHE = 2               # FK20 tables kept per (key, n) (2^20: 235 MB on BLS12-381)
    _KEY_CACHE = 2                 # device tables kept for list-form keys (a 2^20-point table is 1.7 GiB)

    @staticmethod
    def _fingerprint(ck):
        """Length plus up to 16 sampled points: guards the id()-keyed cache against a recycled id
        and against in-place edits of the list (not a hash of every point: that would cost as much
        as the upload the cache avoids)."""
        n = len(ck)
        if n == 0:
            return (0,)
        step = max(1, n // 15)
        return (n,) + tuple(tuple(int(c) for c in ck[i]) for i in sorted({*range(0, n, step), n - 1}))

    def _key(self, ck):
        """Device handle for a commitment key given as CommitmentKey or as a plain
        sequence of point tuples (what the reference's callers hold)."""
        if isinstance(ck, CommitmentKey):
            return ck
        fp = self._fingerprint(ck)

        def load():
            ctx = self._context()
            xy, inf = _native.points_to_limbs(ck, ctx.fp_limbs, self._g1.normalize)
            return CommitmentKey(ctx, ctx.srs_load_g1(xy, inf)), fp

        return _lru_get(self._loaded, id(ck), self._KEY_CACHE, lambda e: e[1] == fp, load,
                        lambda e: e[0].srs.close())[0]

    def _coeffs(self, poly):
        """Coefficient ints of a polynomial given as a list, our Polynomial, or any
        object with .list() (a Sage polynomial); trailing zeros dropped like R(poly)."""
        r = self.curve_order
        if isinstance(poly, Polynomial):
            return poly.c
        if isinstance(poly, np.ndarray) and poly.dtype == np.uint64 and poly.ndim == 2 and poly.shape[1] == 4:
            # buffer fast path (as in fft_ff): canonical little-endian limbs, no per-element Python objects;
            # trailing zero coefficients dropped like everywhere else
            if poly.shape[0] and poly[-1].any():                  # the usual case: nothing to trim, nothing to scan
                return np.ascontiguousarray(poly)
            nz = np.flatnonzero(poly.any(axis=1))
            return np.ascontiguousarray(poly[:int(nz[-1]) + 1 if nz.size else 0])
        if isinstance(poly, (list, tuple)):
            c = [int(x) % r for x in poly]
        else:
            c = [int(x) % r for x in poly.list()]
        while c and c[-1] == 0:
            c.pop()
        return c

    def _pack(self, coeff_lists):
        stride = max((len(c) for c in coeff_lists), default=0)
        stride = max(stride, 1)
        if len(coeff_lists) == 1 and isinstance(coeff_lists[0], np.ndarray) and len(coeff_lists[0]):
            return coeff_lists[0].reshape(1, stride, 4), [stride], stride          # one buffer: handed over as it is
        arr = np.zeros((len(coeff_lists), stride, 4), dtype=np.uint64)
        for i, c in enumerate(coeff_lists):
            if len(c):
                arr[i, :len(c)] = c if isinstance(c, np.ndarray) else _native.ints_to_limbs(c)
        return arr, [len(c) for c in coeff_lists], stride

    _points = staticmethod(_native.limbs_to_points)

    def _canon(self, v):
        """a scalar argument (z, xi, h: an int or a field element) as its canonical int (kzg.py:144-145)"""
        return int(self.Fq(v))

    def _tau(self, tau):
        """the secret of a setup: the one given (reproducible tests), else sampled (kzg.py:67), as an int mod r"""
        if tau is None:
            tau = self.Fq.random_element()
        return int(tau) % self.curve_order

    @staticmethod
    def _upload(ctx, arr):
        """A host array of canonical words as an int64 tensor on the context's GPU.  The context runs on its own
        stream ("stream ordering"), so the device is synchronised before the engine may read it --
        and whatever else torch had queued, a zero fill of a result tensor say."""
        import torch
        d = torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to(f"cuda:{ctx.device}", non_blocking=False)
        torch.cuda.synchronize(ctx.device)
        return d

    # ---- the scheme -----------------------------------------------------------------
    def setup(self, max_degree, tau=None):
        """kzg.py:56-78.  `tau` may be supplied for reproducible tests (the reference
        samples it at :67 and discards it; so do we when it is not given)."""
        tau = self._tau(tau)
        ctx = self._context()
        srs = ctx.srs_generate(_native.int_to_words(tau), int(max_degree) + 1)      # kzg.py:69-72
        tau_G2 = self.multiply(self.G2, tau)                                         # kzg.py:75
        return (CommitmentKey(ctx, srs), tau_G2)

    # ---- on-disk commitment key: build the SRS once, reload it later -----------
    #   bytes 0..7   magic b"KZGSRS1\0"      bytes 8..11  curve id (u32 LE: 0 bn254, 1 bls12_381)
    #   bytes 12..15 uint64 limbs per coordinate (u32 LE)   bytes 16..23 number of points n (u64 LE)
    #   then n * 2 * limbs little-endian uint64 (affine x | y, canonical), then n infinity-flag bytes
    #   version 2 (save_key(compressed=True)): magic b"KZGSRS2\0", the same 16 header bytes, then n compressed points
    #   of 8 * limbs bytes each (include/kzg_mi355x.h: ZCash's 48 bytes for bls12_381, gnark's 32 for bn254); the
    #   points are decompressed -- and checked for subgroup membership -- on the device when the file is loaded
    _MAGIC = b"KZGSRS1\0"
    _MAGIC_COMPRESSED = b"KZGSRS2\0"

    def save_key(self, ck, path, chunk=1 << 16, compressed=False):
        key = self._key(ck)
        ctx = self._context()
        n, L = len(key), ctx.fp_limbs
        with open(path, "wb") as f:
            f.write(self._MAGIC_COMPRESSED if compressed else self._MAGIC)
            f.write(int(ctx.curve_id).to_bytes(4, "little") + int(L).to_bytes(4, "little") + int(n).to_bytes(8, "little"))
            if compressed:
                for start in range(0, n, chunk):
                    f.write(key.srs.export_compressed(start, min(chunk, n - start)).tobytes())
                return
            flags = []
            for start in range(0, n, chunk):
                xy, inf = key.srs.export(start, min(chunk, n - start))
                f.write(np.ascontiguousarray(xy, dtype="<u8").tobytes())
                flags.append(inf)
            f.write(np.concatenate(flags).astype(np.uint8).tobytes())

    def load_key(self, path, check_subgroup=True):
        """check_subgroup applies to version-2 (compressed) files: every point must lie in the prime-order subgroup.
        A point that does not decompress, or fails that check, raises ValueError naming its index."""
        ctx = self._context()
        with open(path, "rb") as f:
            head = f.read(24)
            if head[:8] not in (self._MAGIC, self._MAGIC_COMPRESSED):
                raise ValueError("not a KZG SRS file")
            cid, L, n = (int.from_bytes(head[8:12], "little"), int.from_bytes(head[12:16], "little"),
                         int.from_bytes(head[16:24], "little"))
            if cid != ctx.curve_id or L != ctx.fp_limbs:
                raise ValueError("SRS file belongs to another curve")
            if head[:8] == self._MAGIC_COMPRESSED:
                blobs = np.frombuffer(f.read(n * ctx.g1_bytes), dtype=np.uint8)
                if blobs.size != n * ctx.g1_bytes:
                    raise ValueError("SRS file is shorter than its header says")
                with _bad_input_is_value_error():
                    return CommitmentKey(ctx, ctx.srs_load_g1_compressed(blobs.reshape(n, ctx.g1_bytes), check_subgroup))
            xy = np.frombuffer(f.read(n * 2 * L * 8), dtype="<u8").reshape(n, 2 * L).astype(np.uint64)
            inf = np.frombuffer(f.read(n), dtype=np.uint8).copy()
        return CommitmentKey(ctx, ctx.srs_load_g1(np.ascontiguousarray(xy), inf))

    # ---- compressed points and subgroup membership, any number of points per call on the device -------------------
    def compress_g1(self, points):
        """points: a list of point tuples, or (xy, inf) arrays in the C layout -> list of bytes objects (48 bytes each
        on bls12_381, ZCash's format; 32 on bn254, gnark's).  A point off the curve raises ValueError."""
        xy, inf = self._g1_arrays(points, "points")
        with _bad_input_is_value_error():
            out = self._context().g1_compress(xy, inf)
        return [row.tobytes() for row in out]

    def decompress_g1(self, blobs, check_subgroup=True, strict=True):
        """blobs: a list of bytes objects or a uint8[n, size] array -> list of points.  strict: the first blob that is
        malformed, names no point of the curve or (check_subgroup) a point outside the prime-order subgroup raises
        ValueError with its index and the reason; strict=False returns (points, status) instead, status a uint8 array
        (curve.G1_STATUS_TEXT) and None in place of a failed point."""
        ctx = self._context()
        if isinstance(blobs, np.ndarray):
            arr = np.ascontiguousarray(blobs, dtype=np.uint8).reshape(-1, ctx.g1_bytes)
        else:
            blobs = [bytes(b) for b in blobs]
            for i, b in enumerate(blobs):
                if len(b) != ctx.g1_bytes:
                    raise ValueError(f"compressed point {i}: {len(b)} bytes, expected {ctx.g1_bytes}")
            arr = np.frombuffer(b"".join(blobs), dtype=np.uint8).reshape(len(blobs), ctx.g1_bytes)
        xy, inf, status = ctx.g1_decompress(arr, check_subgroup)
        bad = np.flatnonzero(status)
        if strict and bad.size:
            i = int(bad[0])
            raise ValueError(f"compressed point {i}: {_curve.G1_STATUS_TEXT[int(status[i])]}")
        points = self._points(xy, inf)
        if strict:
            return points
        for i in bad:
            points[int(i)] = None
        return points, status

    def in_subgroup(self, points):
        """bool array: point i is on the curve AND in the subgroup of prime order (infinity: True).  BLS12-381's G1
        has cofactor 0x396c8c005555e1568c00aaab0000aaab; on bn254 every point of the curve is in the subgroup."""
        xy, inf = self._g1_arrays(points, "points")
        return self._context().g1_check_subgroup(xy, inf) == 0

    # ---- the G2 forms (kzg_g2_*): the same argument and error conventions ------------------------------
    def _g2_arrays(self, points, what):
        """points: a list of G2 point tuples, or (xy uint64[n, 4L], inf uint8[n] | None) in the C layout -> (xy, inf)."""
        L = (self._cv.p.bit_length() + 63) // 64
        if isinstance(points, tuple) and len(points) == 2 and isinstance(points[0], np.ndarray):
            xy = np.ascontiguousarray(points[0], dtype=np.uint64).reshape(-1, 4 * L)
            inf = None if points[1] is None else np.ascontiguousarray(points[1], dtype=np.uint8).reshape(-1)
            if inf is not None and inf.size != xy.shape[0]:
                raise ValueError(f"{what}: {inf.size} infinity flags for {xy.shape[0]} points")
            return xy, inf
        return _native.g2_points_to_limbs([self._g2.normalize(pt) for pt in points], L)

    def compress_g2(self, points):
        """points: a list of G2 point tuples, or (xy, inf) arrays in the C layout -> list of bytes objects (96 bytes
        each on bls12_381, ZCash's format; 64 on bn254, gnark's).  A point off the twist raises ValueError."""
        xy, inf = self._g2_arrays(points, "points")
        with _bad_input_is_value_error():
            out = self._context().g2_compress(xy, inf)
        return [row.tobytes() for row in out]

    def decompress_g2(self, blobs, check_subgroup=True, strict=True):
        """blobs: a list of bytes objects or a uint8[n, size] array -> list of G2 points.  strict: the first blob that
        is malformed, names no point of the twist or (check_subgroup) a point outside the prime-order subgroup raises
        ValueError with its index and the reason; strict=False returns (points, status) instead, status a uint8 array
        (curve.G2_STATUS_TEXT) and None in place of a failed point."""
        ctx = self._context()
        if isinstance(blobs, np.ndarray):
            arr = np.ascontiguousarray(blobs, dtype=np.uint8).reshape(-1, ctx.g2_bytes)
        else:
            blobs = [bytes(b) for b in blobs]
            for i, b in enumerate(blobs):
                if len(b) != ctx.g2_bytes:
                    raise ValueError(f"compressed G2 point {i}: {len(b)} bytes, expected {ctx.g2_bytes}")
            arr = np.frombuffer(b"".join(blobs), dtype=np.uint8).reshape(len(blobs), ctx.g2_bytes)
        xy, inf, status = ctx.g2_decompress(arr, check_subgroup)
        bad = np.flatnonzero(status)
        if strict and bad.size:
            i = int(bad[0])
            raise ValueError(f"compressed G2 point {i}: {_curve.G2_STATUS_TEXT[int(status[i])]}")
        points = _native.limbs_to_g2_points(xy, inf)
        if strict:
            return points
        for i in bad:
            points[int(i)] = None
        return points, status

    def in_subgroup_g2(self, points):
        """bool array: point i is on the twist AND in the subgroup of prime order (infinity: True).  The twists of
        both curves have a cofactor: a random point of either twist is outside G2."""
        xy, inf = self._g2_arrays(points, "points")
        return self._context().g2_check_subgroup(xy, inf) == 0

    # ---- trusted-setup files and keys checked on the device --------------------------------------------
    def setup_g2(self, count, tau, device=False):
        """[tau^j] G2, j < count, on the host with curve.py: pure Python, one scalar multiplication per point -- for
        tests and small ceremonies, NOT a data-parallel path (a real setup publishes its G2 powers; nobody knows tau).
        device=True computes the same list on the device: kzg_g2_mul_powers on `count` copies of the generator."""
        tau = self._tau(tau)
        if device:
            xy, inf = self._g2_arrays([self.G2] * int(count), "setup_g2")
            return _native.limbs_to_g2_points(*self._context().g2_mul_powers(xy, inf, tau, 1))
        out, t = [], 1
        for _ in range(int(count)):
            out.append(self.multiply(self.G2, t) if t else self.Z2)
            t = t * tau % self.curve_order
        return out

    def _lagrange_of(self, key):
        n = len(key)
        log_n, w = self._domain(n, None)
        ctx = self._context()
        return LagrangeKey(ctx, ctx.srs_lagrange(key.srs, log_n, w), n, w)

    # ---- per-point scalar multiplication and setup contributions (kzg_g1_mul_* / kzg_g2_mul_*) ---------
    @staticmethod
    def _scalar_rows(scalars, n, who):
        """n scalars, ints in [0, 2^256) taken as they stand (NOT reduced modulo r), as uint64[n, 4]"""
        if isinstance(scalars, np.ndarray) and scalars.dtype == np.uint64:
            rows = np.ascontiguousarray(scalars).reshape(-1, 4)
        else:
            ks = [int(k) for k in scalars]
            for i, k in enumerate(ks):
                if not 0 <= k < 1 << 256:
                    raise ValueError(f"{who}: scalar {i} is not in [0, 2^256)")
            rows = _native.ints_to_limbs(ks) if ks else np.zeros((0, 4), dtype=np.uint64)
        if rows.shape[0] != n:
            raise ValueError(f"{who}: {rows.shape[0]} scalars for {n} points")
        return rows

    def _multiply_each(self, group, points, scalars, who):
        as_arrays = isinstance(points, tuple) and len(points) == 2 and isinstance(points[0], np.ndarray)
        xy, inf = (self._g1_arrays if group == 1 else self._g2_arrays)(points, who)
        rows = self._scalar_rows(scalars, xy.shape[0], who)
        ctx = self._context()
        with _bad_input_is_value_error():
            out = (ctx.g1_mul_each if group == 1 else ctx.g2_mul_each)(xy, inf, rows)
        if as_arrays:
            return out
        return self._points(*out) if group == 1 else _native.limbs_to_g2_points(*out)

    def multiply_each(self, points, scalars):
        """[k_i] P_i for every i, on the device, the products kept apart.  points: a list of G1 point tuples, or
        (xy, inf) arrays in the C layout; the result is of the same kind.  scalars: ints in [0, 2^256), each taken as it
        stands -- NOT reduced modulo r, so a point outside the prime-order subgroup is multiplied by the integer given
        (multiply() reduces).  A point off the curve or with a coordinate >= p raises ValueError naming its index."""
        return self._multiply_each(1, points, scalars, "multiply_each")

    def multiply_each_g2(self, points, scalars):
        """multiply_each for points of the twist (G2 tuples, or (xy, inf) arrays in kzg_pairing_check's layout)."""
        return self._multiply_each(2, points, scalars, "multiply_each_g2")

    def lincomb_g2(self, points, scalars):
        """sum_i [k_i] Q_i as ONE point of the twist, on the device (kzg_g2_lincomb).  points: a list of
        G2 point tuples, or (xy, inf) arrays in kzg_pairing_check's layout; scalars: ints in [0, 2^256), each taken as
        it stands -- NOT reduced modulo r.  The sum is exact for every point of the twist, in the subgroup or not.  No
        points give infinity.  A point off the twist or with a coordinate >= p raises ValueError naming its index."""
        xy, inf = self._g2_arrays(points, "lincomb_g2")
        rows = self._scalar_rows(scalars, xy.shape[0], "lincomb_g2")
        with _bad_input_is_value_error():
            out_xy, out_inf = self._context().g2_lincomb(xy, inf, rows)
        return _native.limbs_to_g2_points(out_xy.reshape(1, -1), out_inf)[0]

    def commit_g2(self, g2_powers, polynomials):
        """The commitments in G2: sum_j c_j [tau^j] G2 for every polynomial, one kzg_g2_lincomb call each.  g2_powers:
        the G2 section of a setup (a list of G2 point tuples, or (xy, inf) arrays).  Polynomials, their canonical
        coefficients and the degree rule are commit's."""
        xy, inf = self._g2_arrays(g2_powers, "commit_g2")
        max_degree = xy.shape[0] - 1
        coeffs = [self._coeffs(p) for p in polynomials]
        for c in coeffs:
            if len(c) - 1 > max_degree:
                raise ValueError(
                    f"Polynomial degree {len(c) - 1} exceeds maximum allowed degree {max_degree}")   # kzg.py:103-106
        ctx = self._context()
        out = []
        for c in coeffs:
            rows = c if isinstance(c, np.ndarray) else self._scalar_rows(c, len(c), "commit_g2")
            with _bad_input_is_value_error():
                out_xy, out_inf = ctx.g2_lincomb(xy[:len(c)], None if inf is None else inf[:len(c)], rows)
            out.append(_native.limbs_to_g2_points(out_xy.reshape(1, -1), out_inf)[0])
        return out

    @staticmethod
    def _g2_chain(g2_chain, who):
        if g2_chain not in ("links", "fold"):
            raise ValueError(f"{who}: g2_chain must be \"links\" or \"fold\", not {g2_chain!r}")
        return g2_chain

    def _below_order(self, v, who, name, least=0):
        v = int(v)
        if not least <= v < self.curve_order:
            raise ValueError(f"{who}: {name} must be in [{least}, r)")
        return v

    def scale_key(self, ck, s, c0=1):
        """The CommitmentKey whose point i is [c0 * s^i mod r] ck[i], computed on the device from key handle to key
        handle (kzg_srs_mul_powers): what a contribution s does to a monomial key.  ck may be a LagrangeKey (its
        points are scaled all the same); the result is a plain key.  s, c0: ints in [0, r)."""
        s, c0 = self._below_order(s, "scale_key", "s"), self._below_order(c0, "scale_key", "c0")
        key = self._key(ck)
        with _bad_input_is_value_error():
            return CommitmentKey(key._ctx, key._ctx.srs_mul_powers(key.srs, s, c0))

    def unit_setup(self, n, n_g2):
        """The TrustedSetup of tau = 1, where a ceremony starts: n copies of the G1 generator (n a power of two, at
        least 2), n_g2 >= 2 copies of the G2 generator, the Lagrange key of the monomial one."""
        n, n_g2 = int(n), int(n_g2)
        if n < 2 or n & (n - 1) or n_g2 < 2:
            raise ValueError("unit_setup: n must be a power of two >= 2 and n_g2 >= 2")
        ctx = self._context()
        xy, inf = _native.points_to_limbs([self.G1] * n, ctx.fp_limbs)
        mono = CommitmentKey(ctx, ctx.srs_load_g1(xy, inf))
        try:
            return TrustedSetup(mono, self._lagrange_of(mono), [self.G2] * n_g2)
        except Exception:
            mono.srs.close()
            raise

    def contribute(self, setup, secret=None):
        """One participant's step of a powers-of-tau ceremony: (new TrustedSetup, Contribution) with every power of
        the old tau multiplied by the same power of a secret s, 1 <= s < r -- drawn from `secrets` when not given, and
        not kept.  Monomial key: scale_key(setup.monomial, s); G2 powers: multiply_each_g2 by s^j; Lagrange key:
        kzg_srs_lagrange of the new monomial key.  Contribution.pubkey = [s] G2 and .tau_g1 = the new [tau] G1 are what
        verify_contribution needs besides the two setups."""
        order = self.curve_order
        s = secrets.randbelow(order - 1) + 1 if secret is None else self._below_order(secret, "contribute", "secret", 1)
        if len(setup.monomial) < 2 or len(setup.g2) < 2:
            raise ValueError("contribute: the setup needs [tau] G1 and [tau] G2 (two points of each group)")
        opened = []
        try:
            mono = self.scale_key(setup.monomial, s)
            opened.append(mono.srs)
            powers, t = [], 1
            for _ in setup.g2:
                powers.append(t)
                t = t * s % order
            g2 = self.multiply_each_g2(list(setup.g2) + [self.G2], powers + [s])
            lag = self._lagrange_of(mono)
            opened.append(lag.srs)
            return TrustedSetup(mono, lag, g2[:-1]), Contribution(g2[-1], mono[1])
        except Exception:
            for h in opened:
                h.close()
            raise

    def verify_contribution(self, before, after, contribution, r=None, pairing="device", g2_chain="links"):
        """Did one contribution turn `before` into `after`?  True iff pubkey and tau_g1 are finite points of their
        prime-order subgroups, tau_g1 is after.monomial[1], e(tau_g1, G2) = e(before.monomial[1], pubkey) (the new tau
        is the old one times the secret behind pubkey), `after` has the section lengths of `before`, and
        check_key(after.monomial, after.g2, after.lagrange, r) passes (the sections of `after` describe ONE tau).
        g2_chain: check_key's."""
        self._g2_chain(g2_chain, "verify_contribution")
        if len(before.monomial) < 2:
            raise ValueError("verify_contribution: the setup needs [tau] G1")
        pub, tau_g1 = self._g2.normalize(contribution.pubkey), self._g1.normalize(contribution.tau_g1)
        if self._g2.is_inf(pub) or self._g1.is_inf(tau_g1):
            return False
        if not (self.in_subgroup_g2([pub])[0] and self.in_subgroup([tau_g1])[0]):
            return False
        if (len(after.monomial), len(after.g2), after.lagrange.n) != (len(before.monomial), len(before.g2), before.lagrange.n):
            return False
        if not self.eq(tau_g1, after.monomial[1]):
            return False
        if not self._verdict(tau_g1, before.monomial[1], pub, pairing, "verify_contribution"):
            return False
        return self.check_key(after.monomial, after.g2, after.lagrange, r, g2_chain=g2_chain)

    def verify_contributions(self, first_tau_g1, contributions, pairing="device", g2_chain="links"):
        """A coordinator's replay of a transcript: link i holds iff e(c_i.tau_g1, G2) = e(c_(i-1).tau_g1, c_i.pubkey),
        c_(-1).tau_g1 = first_tau_g1 ([tau] G1 of the setup the chain starts from).  Returns the list of verdicts; with
        pairing="device" all links are ONE kzg_pairing_check call, one equation per link.  A link with an infinite
        point is False (its equation would hold for any partner).  Membership in the subgroups is verify_contribution's
        business, or the loader's.  g2_chain is check_key's keyword, taken (and checked) so that a coordinator passes one
        set of options to every call of a replay; the links themselves hold no chain of G2 powers."""
        self._g2_chain(g2_chain, "verify_contributions")
        if pairing not in ("device", "host"):
            raise ValueError(f"verify_contributions: pairing must be \"device\" or \"host\", not {pairing!r}")
        links, prev = [], self._g1.normalize(first_tau_g1)
        for c in contributions:
            links.append((self._g1.normalize(c.tau_g1), prev, self._g2.normalize(c.pubkey)))
            prev = links[-1][0]
        if not links:
            return []
        finite = [not (self._g1.is_inf(t) or self._g1.is_inf(p) or self._g2.is_inf(q)) for t, p, q in links]
        if pairing == "device":
            holds = self.pairing_check([[(t, self.G2), (self.neg(p), q)] for t, p, q in links])
        else:
            holds = [self.pairing(self.G2, t) == self.pairing(q, p) for t, p, q in links]
        return [bool(f and h) for f, h in zip(finite, holds)]

    def save_trusted_setup(self, path, ck, g2_points, lagrange_order="natural"):
        """Writes a trusted-setup text file (parse_trusted_setup's layout) from a monomial key of power-of-two length
        and a list of G2 points.  The Lagrange section is kzg_srs_lagrange of the key; every point is compressed on
        the device.  lagrange_order="bit_reversed" writes the Lagrange section in bit-reversed order."""
        if lagrange_order not in ("natural", "bit_reversed"):
            raise ValueError(f"lagrange_order must be \"natural\" or \"bit_reversed\", not {lagrange_order!r}")
        self._monomial_key(ck, "save_trusted_setup")
        key = self._key(ck)
        g2_points = list(g2_points)
        if not g2_points:
            raise ValueError("save_trusted_setup: at least one G2 point (the generator) is needed")
        lag = self._lagrange_of(key)
        try:
            lag_blobs = lag.srs.export_compressed()
        finally:
            lag.srs.close()
        if lagrange_order == "bit_reversed":
            lag_blobs = bit_reverse_rows(lag_blobs)
        text = format_trusted_setup(lag_blobs, self.compress_g2(g2_points), key.srs.export_compressed())
        with open(path, "w") as f:
            f.write(text)

    def load_trusted_setup(self, path, check=True, check_subgroup=True, lagrange_order="natural", r=None,
                           g2_chain="links"):
        """Reads a trusted-setup text file -> TrustedSetup.  The G1 sections are decompressed and expanded on the
        device (kzg_srs_load_g1_compressed), the G2 section by kzg_g2_decompress; check_subgroup tests every point for
        membership in its prime-order subgroup.  A point that fails raises ValueError naming the section, the index
        and the status.  check: the three sections must describe ONE tau (check_key; r fixes its randomness),
        else ValueError naming the part that failed.  lagrange_order="bit_reversed": the file's Lagrange section is
        in bit-reversed order and is un-permuted on load.  g2_chain: check_key's."""
        if lagrange_order not in ("natural", "bit_reversed"):
            raise ValueError(f"lagrange_order must be \"natural\" or \"bit_reversed\", not {lagrange_order!r}")
        self._g2_chain(g2_chain, "load_trusted_setup")
        ctx = self._context()
        with open(path) as f:
            n1, n2, lag_blobs, g2_blobs, mono_blobs = parse_trusted_setup(f.read(), ctx.g1_bytes, ctx.g2_bytes)
        if lagrange_order == "bit_reversed":
            lag_blobs = bit_reverse_rows(lag_blobs)
        log_n, w = self._domain(n1, None)
        srs = []
        try:
            for name, blobs in (("G1 monomial", mono_blobs), ("G1 Lagrange", lag_blobs)):
                try:
                    srs.append(ctx.srs_load_g1_compressed(blobs, check_subgroup))
                except _native.NativeError as e:
                    if e.code != -1:
                        raise
                    raise ValueError(f"trusted setup, {name} section: {e}") from e
            xy, inf, status = ctx.g2_decompress(g2_blobs, check_subgroup)
            bad = np.flatnonzero(status)
            if bad.size:
                i = int(bad[0])
                raise ValueError(f"trusted setup, G2 section: point {i} has status {int(status[i])} "
                                 f"({_curve.G2_STATUS_TEXT[int(status[i])]})")
            setup = TrustedSetup(CommitmentKey(ctx, srs[0]), LagrangeKey(ctx, srs[1], n1, w),
                                 _native.limbs_to_g2_points(xy, inf))
            if check:
                part = self._key_fault(setup.monomial, setup.g2, setup.lagrange, r, g2_chain)
                if part is not None:
                    raise ValueError(f"trusted setup: the sections do not describe one tau: {part}")
        except Exception:
            for h in srs:
                h.close()
            raise
        return setup

    _CHECK_KEY_PAIRS = 16

    def check_key(self, ck, g2_points, lagrange=None, r=None, g2_chain="links"):
        """Do the pieces describe ONE tau -- ck = [tau^i G1], g2_points = [tau^j G2], lagrange (optional) the Lagrange
        form of ck?  True iff (1) ck[0] and g2_points[0] are the generators, (2) G1 chain: for a random rho,
        e(sum_{i<n-1} rho^i S_i, T_1) = e(sum_{i<n-1} rho^i S_{i+1}, G2) -- one commit of two polynomials against the
        key and one device pairing check, (3) G2 chain: e([rho^j] S_1, T_j) = e([rho^j] G1, T_{j+1}) for every j, in
        equations of at most 16 pairs with their own rho each, all in one kzg_pairing_check call, (4) the Lagrange key
        equals kzg_srs_lagrange(ck) point by point.  rho: 128 random bits unless r fixes it.  Membership of the points
        in their subgroups is the loader's business (check_subgroup), not this call's.
        g2_chain="fold" replaces (3) by the G2 image of (2): for one rho, e(S_1, sum_{j<m-1} rho^j T_j) =
        e(G1, sum_{j<m-1} rho^j T_{j+1}), the two sums by kzg_g2_lincomb_powers on the device and the equation in the
        same kzg_pairing_check call as (2)'s -- no host multiplication and two equations whatever m is.  The verdict
        and the name of a failing condition are those of "links"."""
        return self._key_fault(ck, g2_points, lagrange, r, g2_chain) is None

    def _key_fault(self, ck, g2_points, lagrange, r, g2_chain="links"):
        """None, or the name of the first of check_key's four conditions that fails"""
        self._g2_chain(g2_chain, "check_key")
        self._monomial_key(ck, "check_key")
        key = self._key(ck)
        ctx = self._context()
        order = self.curve_order
        g2 = [self._g2.normalize(pt) for pt in g2_points]
        n, m = len(key), len(g2)
        if m < 1:
            raise ValueError("check_key: at least one G2 point is needed")
        if (n > 1 or m > 1) and (n < 2 or m < 2):
            raise ValueError("check_key: chaining the powers needs [tau] G1 and [tau] G2 (two points of each group)")

        def fresh(e):
            return (secrets.randbits(128) if r is None else (int(r) + e)) % order or 1

        # (1) the generators
        if not self.eq(key[0], self.G1):
            return "the first G1 power is not the generator"
        if not self._g2.eq(g2[0], self.G2):
            return "the first G2 power is not the generator"
        if n == 1:
            return None
        # (2) the G1 chain: the powers of rho on the device, two commitments, one pairing equation
        rho = fresh(0)
        import torch
        d_ones = self._upload(ctx, np.tile(_native.int_to_words(1), (n - 1, 1)))
        d_pows = torch.empty_like(d_ones)
        ctx.vec_mul_powers(n - 1, d_ones.data_ptr(), rho, 1, d_pows.data_ptr())
        ctx.synchronize()
        pows = d_pows.cpu().numpy().view(np.uint64)
        lo, hi = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
        lo[:n - 1], hi[1:] = pows, pows
        c_lo, c_hi = self.commit(key, [lo, hi])
        equations = [[(c_lo, g2[1]), (self.neg(c_hi), self.G2)]]
        # (3) the G2 chain, 8 links (16 pairs) per equation; pairs of infinities (skipped by the device) fill the rest
        s1 = key[1]
        links = self._CHECK_KEY_PAIRS // 2
        if g2_chain == "fold":
            # both sums on the device, one equation; a G2 power that is no point of the twist fails the chain, as the
            # pairing check of "links" would say
            xy, inf = self._g2_arrays(g2, "check_key")
            rho_1 = fresh(1)
            try:
                lo_hi = [ctx.g2_lincomb_powers(xy[a:a + m - 1], inf[a:a + m - 1], rho_1, 1) for a in (0, 1)]
            except _native.NativeError as e:
                if e.code != -1:
                    raise
                return "the G2 powers are not a chain of powers of the tau of [tau] G1"
            a_pt, b_pt = (_native.limbs_to_g2_points(o_xy.reshape(1, -1), o_inf)[0] for o_xy, o_inf in lo_hi)
            equations.append([(s1, a_pt), (self.neg(self.G1), b_pt)])
        for e, start in enumerate(range(0, m - 1, links) if g2_chain == "links" else (), 1):
            rho_e, wgt, eq = fresh(e), 1, []
            for j in range(start, min(start + links, m - 1)):
                eq += [(self.multiply(s1, wgt), g2[j]), (self.neg(self.multiply(self.G1, wgt)), g2[j + 1])]
                wgt = wgt * rho_e % order
            equations.append(eq)
        k = max(len(eq) for eq in equations)
        equations = [eq + [(self.Z1, self.G2)] * (k - len(eq)) for eq in equations]
        verdicts = self.pairing_check(equations)
        if not verdicts[0]:
            return "the G1 powers are not a chain of powers of the tau of [tau] G2"
        if not all(verdicts[1:]):
            return "the G2 powers are not a chain of powers of the tau of [tau] G1"
        # (4) the Lagrange key
        if lagrange is not None:
            if not isinstance(lagrange, LagrangeKey):
                raise TypeError("check_key: lagrange must be a LagrangeKey")
            if lagrange.n != n:
                return "the Lagrange key has another length than the monomial key"
            mine = self._lagrange_of(key)
            try:
                if mine.w != lagrange.w:
                    return "the Lagrange key is over another root of unity"
                (xa, ia), (xb, ib) = mine.srs.export(), lagrange.srs.export()
                if not (np.array_equal(ia, ib) and np.array_equal(xa, xb)):
                    return "the Lagrange points are not the Lagrange form of the G1 powers"
            finally:
                mine.srs.close()
        return None

    def commit(self, ck, polynomials):
        """kzg.py:80-120."""
        key = self._key(ck)
        max_degree = len(key) - 1
        coeffs = [self._coeffs(p) for p in polynomials]
        for c in coeffs:
            if len(c) - 1 > max_degree:
                raise ValueError(
                    f"Polynomial degree {len(c) - 1} exceeds maximum allowed degree {max_degree}")   # kzg.py:103-106
        if not coeffs:
            return []
        arr, lens, stride = self._pack(coeffs)
        xy, inf = self._context().commit(key.srs, arr, lens, stride)
        return self._points(xy, inf)

    def open(self, ck, polynomials, z, xi):
        """kzg.py:122-159."""
        key = self._key(ck)
        coeffs = [self._coeffs(p) for p in polynomials]
        z, xi = self._canon(z), self._canon(xi)                                       # kzg.py:144-145
        arr, lens, stride = self._pack(coeffs)
        try:
            xy, inf, _ = self._context().open(key.srs, arr, lens, stride, _native.int_to_words(z),
                                              _native.int_to_words(xi))
        except _native.NativeError as e:
            if e.code == _native.KZG_ERR_DEGREE:
                raise ValueError(
                    f"Polynomial degree exceeds maximum allowed degree {len(key) - 1}") from e   # via kzg.py:157 -> :103
            raise
        return self._points(xy, inf)[0]

    # ---- Shplonk (Boneh-Drake-Fisch-Gabizon 2020, second scheme): any polynomials at any point sets, one proof of two
    #      G1 points, two pairings.  With T the union of the sets S_i and Z_S = prod_(z in S) (X - z):
    #        W  = commit( q ),  q = sum_i gamma^(i+1) (f_i - r_i) / Z_(S_i)        r_i: the interpolant of f_i on S_i
    #        W' = commit( L / (X - zeta) ),  L = sum_i gamma^(i+1) Z_(T\S_i)(zeta) (f_i - r_i(zeta)) - Z_T(zeta) q
    #      and the verifier checks e(F + zeta W', G2) = e(W', tau G2) for the commitment F of L.
    _MULTI_MAX = 63                # polynomials (the second proof point takes q as one more) and points per opening

    def evaluate_each(self, polynomials, points):
        """values[i][j] = polynomials[i](points[j]) on the device: one kzg_fr_poly_eval_batch, one synchronisation.
        At most 64 polynomials and 64 points."""
        coeffs = [self._coeffs(p) for p in polynomials]
        pts = [self._canon(z) for z in points]
        if len(coeffs) > 64 or len(pts) > 64:
            raise ValueError("evaluate_each: at most 64 polynomials and 64 points")
        if not coeffs or not pts:
            return [[] for _ in coeffs]
        ctx = self._context()
        arr, lens, stride = self._pack(coeffs)
        d = self._upload(ctx, arr)
        return ctx.poly_eval_batch(d.data_ptr(), lens, stride, pts)

    def _point_sets(self, point_sets, k, who):
        """-> (the sets as canonical ints, their de-duplicated union T in order of first appearance)"""
        sets = [[self._canon(z) for z in S] for S in point_sets]
        if len(sets) != k:
            raise ValueError(f"{who}: {len(sets)} point sets for {k} polynomials")
        for i, S in enumerate(sets):
            if not S:
                raise ValueError(f"{who}: point set {i} is empty")
            if len(set(S)) != len(S):
                raise ValueError(f"{who}: point set {i} repeats a point")
        T = list(dict.fromkeys(z for S in sets for z in S))
        if k > self._MULTI_MAX or len(T) > self._MULTI_MAX:
            raise ValueError(f"{who}: at most {self._MULTI_MAX} polynomials and {self._MULTI_MAX} distinct points")
        return sets, T

    def _vanishing_at(self, points, x):
        """prod_(z in points) (x - z)"""
        acc = 1
        for z in points:
            acc = acc * (x - z) % self.curve_order
        return acc

    def open_multi(self, ck, polynomials, point_sets, gamma, zeta):
        """One proof that polynomials[i] takes its values at every point of point_sets[i] (non-empty, no point twice).
        zeta: a callable W -> challenge (Fiat-Shamir: zeta must depend on W), or a fixed value (tests).  Returns
        OpenMulti(W, W2, zeta, evaluations) with evaluations[i][j] = polynomials[i](point_sets[i][j]).  The weights are
        gamma^(i+1), as open's xi^(i+1): when every set is [z], W equals open(ck, polynomials, z, gamma)."""
        r = self.curve_order
        key = self._key(ck)
        coeffs = [self._coeffs(p) for p in polynomials]
        k = len(coeffs)
        sets, T = self._point_sets(point_sets, k, "open_multi")
        gamma = self._canon(gamma)
        if k == 0:
            return OpenMulti(self.Z1, self.Z1, self._canon(zeta(self.Z1) if callable(zeta) else zeta), [])
        ctx = self._context()
        arr, lens, stride = self._pack(coeffs)
        rows = np.zeros((k + 1, stride, 4), dtype=np.uint64)         # row k: the quotient q, left there by the first call
        rows[:k] = arr
        d = self._upload(ctx, rows)
        d_q = d.data_ptr() + k * stride * 32
        values = ctx.poly_eval_batch(d.data_ptr(), lens, stride, T)
        col = {z: j for j, z in enumerate(T)}
        evaluations = [[values[i][col[z]] for z in S] for i, S in enumerate(sets)]
        # W: sum over z in T of Q_z[ sum_i w_iz f_i ],  w_iz = gamma^(i+1) / prod_(m in S_i, m != z) (z - m)
        weights, g, gpow = [[0] * len(T) for _ in range(k)], 1, []
        for i, S in enumerate(sets):
            g = g * gamma % r
            gpow.append(g)
            for z in S:
                weights[i][col[z]] = g * pow(self._vanishing_at([m for m in S if m != z], z), -1, r) % r
        try:
            xy, inf = ctx.open_points(key.srs, d.data_ptr(), lens, stride, T, weights, d_quot=d_q, device=True)
            W = self._points(xy, inf)[0]
            zeta = self._canon(zeta(W) if callable(zeta) else zeta)
            # W': one single-point quotient at zeta over the k polynomials and q; it does not depend on the constant
            # term of L, so the r_i(zeta) are the verifier's alone
            w2 = [[gpow[i] * self._vanishing_at([z for z in T if z not in S], zeta) % r] for i, S in enumerate(sets)]
            w2.append([-self._vanishing_at(T, zeta) % r])
            xy, inf = ctx.open_points(key.srs, d.data_ptr(), list(lens) + [max(max(lens) - 1, 0)], stride, [zeta], w2,
                                      device=True)
        except _native.NativeError as e:
            if e.code == _native.KZG_ERR_DEGREE:
                raise ValueError(f"Polynomial degree exceeds maximum allowed degree {len(key) - 1}") from e
            raise
        return OpenMulti(W, self._points(xy, inf)[0], zeta, evaluations)

    def _multi_claim(self, commitments, sets, T, evaluations, W, gamma, zeta):
        """F = sum_i gamma^(i+1) Z_(T\\S_i)(zeta) (C_i - r_i(zeta) G1) - Z_T(zeta) W, r_i the interpolant of the claimed
        values on S_i (Lagrange's formula)"""
        r = self.curve_order
        parts, const, g = [], 0, 1
        for C, S, vals in zip(commitments, sets, evaluations):
            g = g * gamma % r
            r_i = 0
            for z, v in zip(S, vals):
                others = [m for m in S if m != z]
                r_i += int(v) * self._vanishing_at(others, zeta) * pow(self._vanishing_at(others, z), -1, r)
            scale = g * self._vanishing_at([z for z in T if z not in S], zeta) % r
            parts.append(self.multiply(C, scale))
            const = (const + scale * r_i) % r
        parts.append(self.multiply(self.G1, -const % r))
        parts.append(self.multiply(W, -self._vanishing_at(T, zeta) % r))
        return self._sum_g1(parts)

    def check_multi(self, rk, commitments, point_sets, evaluations, proof, gamma, zeta, pairing="device"):
        """Does `proof` -- open_multi's result, or the pair (W, W') -- show that the polynomial of commitments[i] takes
        evaluations[i][j] at point_sets[i][j]?  e(F + zeta W', G2) == e(W', rk), rk = tau G2: two pairings whatever the
        number of polynomials and points.  zeta: the challenge the prover used (re-derived from W by a Fiat-Shamir
        caller).  A point off the curve: False.  pairing: as in verify_points."""
        if pairing not in ("device", "host"):
            raise ValueError(f"check_multi: pairing must be \"device\" or \"host\", not {pairing!r}")
        commitments = list(commitments)
        sets, T = self._point_sets(point_sets, len(commitments), "check_multi")
        evaluations = [[self._canon(v) for v in vals] for vals in evaluations]
        if len(evaluations) != len(sets) or any(len(v) != len(S) for v, S in zip(evaluations, sets)):
            raise ValueError("check_multi: evaluations must follow point_sets")
        W, W2 = (proof.W, proof.W2) if hasattr(proof, "W2") else proof
        points = []
        for pt in [*commitments, W, W2]:
            pt = self._g1.normalize(tuple(int(c) for c in pt))
            if not (0 <= pt[0] < self._cv.p and 0 <= pt[1] < self._cv.p and _curve.on_curve_g1(pt, self._cv)):
                return False
            points.append(pt)
        *commitments, W, W2 = points
        gamma, zeta = self._canon(gamma), self._canon(zeta)
        F = self._multi_claim(commitments, sets, T, evaluations, W, gamma, zeta)
        return self._verdict(self.add(F, self.multiply(W2, zeta)), W2, rk, pairing, "check_multi")

    # ---- verification (host).  Both checks rest on one folded claim per opening:
    #      F = sum_i xi^(i+1) (C_i - v_i G1) commits to sum_i xi^(i+1) (p_i - v_i), which (X - z) divides iff the v_i are
    #      the values at z; the proof pi commits to the quotient, so  e(F, G2) = e(pi, (tau - z) G2).
    def _sum_g1(self, points):
        try:
            return _native.g1_sum(self.curve_type, points)            # the library's host group law
        except _native.NativeUnavailable:
            total = self.Z1
            for pt in points:
                total = self.add(total, pt)
            return total

    def _folded_claim(self, commitments, evaluations, xi):
        """F above.  Weights are xi^(i+1) by position in EACH list, as the reference's two loops have it
        (kzg.py:187-194; its batch form indexes the evaluations by the commitments' positions, kzg.py:262-266)."""
        weight, parts = xi, []
        for C in commitments:
            parts.append(self.multiply(C, int(weight)))
            weight *= xi
        weight, value = xi, self.Fq(0)
        for v in evaluations:
            value += weight * self.Fq(v)
            weight *= xi
        parts.append(self.multiply(self.G1, int(-value)))
        return self._sum_g1(parts)

    def check(self, rk, commitments, z, evaluations, proof, xi):
        """kzg.py:161-211: two pairings, e(F, G2) against e(pi, tau G2 - z G2)."""
        z, xi = self.Fq(z), self.Fq(xi)
        F = self._folded_claim(commitments, evaluations, xi)
        shifted_key = self.add(rk, self.neg(self.multiply(self.G2, int(z))))
        return self.pairing(self.G2, F) == self.pairing(shifted_key, proof)

    def batch_check(self, rk, commitments_list, z_list, evaluations_list, proof_list, xi_list, r=None):
        """kzg.py:213-288: the openings' equations e(F_i + z_i pi_i, G2) = e(pi_i, tau G2) added up with weights
        rho^(i+1) (rho = `r`, sampled when not given: kzg.py:244-245) -- two pairings for any number of openings."""
        rho = self.Fq(self.Fq.random_element() if r is None else r)
        weight, lhs, rhs = rho, [], []
        for commitments, z, evaluations, proof, xi in zip(commitments_list, z_list, evaluations_list, proof_list,
                                                          xi_list):
            evaluations = list(evaluations)
            if len(evaluations) < len(commitments):
                raise IndexError("list index out of range")              # kzg.py:266 reads evaluations[j] per commitment
            F = self._folded_claim(commitments, evaluations[:len(commitments)], self.Fq(xi))
            lhs.append(self.multiply(self.add(F, self.multiply(proof, int(self.Fq(z)))), int(weight)))
            rhs.append(self.multiply(proof, int(weight)))
            weight *= rho
        return self.pairing(self.G2, self._sum_g1(lhs)) == self.pairing(rk, self._sum_g1(rhs))

    # ---- evaluation form (Lagrange-basis keys): commit to and open value vectors f[i] = p(w^i) -------------------
    def _domain(self, n, w):
        """Validate (n, w) on the host: n a power of two >= 2, w a primitive n-th root (w^(n/2) = -1).  -> (log_n, w)."""
        n = int(n)
        if n < 2 or n & (n - 1):
            raise ValueError(f"domain size {n} is not a power of two >= 2")
        r = self.curve_order
        if (r - 1) % n:
            raise ValueError(f"the scalar field has no {n}-th roots of unity")
        w = int(self.Fq.root_of_unity(n)) if w is None else int(w) % r
        if pow(w, n // 2, r) != r - 1:
            raise ValueError(f"w is not a primitive {n}-th root of unity")
        return n.bit_length() - 1, w

    def _value_lists(self, value_lists, n):
        out = []
        for v in value_lists:
            m = len(v) if hasattr(v, "__len__") else len(v.list())
            if m > n:
                raise ValueError(f"{m} values exceed the domain size {n}")
            c = self._coeffs(v)          # canonical ints (or a uint64[m, 4] buffer); trailing zero values dropped
            if len(c) > n:
                raise ValueError(f"{len(c)} values exceed the domain size {n}")
            out.append(c)
        return out

    def setup_lagrange(self, n, tau=None, w=None):
        """setup() in the Lagrange basis of {w^i}, i < n: (LagrangeKey [L_i(tau) G1], tau G2).  w defaults to
        Fq.root_of_unity(n), the root of plonk/encoder.py:49."""
        log_n, w = self._domain(n, w)
        tau = self._tau(tau)
        ctx = self._context()
        srs = ctx.srs_generate_lagrange(_native.int_to_words(tau), log_n, w)
        return LagrangeKey(ctx, srs, 1 << log_n, w), self.multiply(self.G2, tau)

    def lagrange_key(self, ck, n, w=None):
        """The Lagrange key of the first n points of a monomial key (CommitmentKey or list of points): an inverse
        NTT over G1 on the device, no tau needed."""
        log_n, w = self._domain(n, w)
        if len(ck) < (1 << log_n):
            raise ValueError(f"commitment key of {len(ck)} points is shorter than the domain ({1 << log_n})")
        key = self._key(ck)
        ctx = self._context()
        return LagrangeKey(ctx, ctx.srs_lagrange(key.srs, log_n, w), 1 << log_n, w)

    def commit_evaluations(self, lk, value_lists):
        """Commitments to value vectors: equal to commit(ck, [interpolant]) for the same tau."""
        if not isinstance(lk, LagrangeKey):
            raise TypeError("commit_evaluations needs a LagrangeKey (setup_lagrange / lagrange_key)")
        vals = self._value_lists(value_lists, lk.n)
        if not vals:
            return []
        arr, lens, stride = self._pack(vals)
        xy, inf = self._context().commit(lk.srs, arr, lens, stride)
        return self._points(xy, inf)

    def open_evaluations(self, lk, value_lists, z, xi):
        """open() from value vectors: the same proof as open(ck, [interpolants], z, xi), z in the domain included."""
        if not isinstance(lk, LagrangeKey):
            raise TypeError("open_evaluations needs a LagrangeKey (setup_lagrange / lagrange_key)")
        vals = self._value_lists(value_lists, lk.n)
        z, xi = self._canon(z), self._canon(xi)
        arr, lens, stride = self._pack(vals)
        xy, inf, _ = self._context().open_evals(lk.srs, arr, lens, stride, _native.int_to_words(z),
                                                _native.int_to_words(xi))
        return self._points(xy, inf)[0]

    def _eval_domain(self, lk_or_w):
        """(log_n, w) of a LagrangeKey, or of the root w itself (the domain size is its multiplicative order)"""
        if isinstance(lk_or_w, LagrangeKey):
            return lk_or_w.log_n, lk_or_w.w
        r = self.curve_order
        w = int(lk_or_w) % r
        n, x = 1, w
        while x != 1 and n < (1 << 40):
            x = x * x % r
            n *= 2
        if x != 1:
            raise ValueError("w is not a root of unity of power-of-two order")
        return self._domain(n, w)

    def evaluate_evaluations(self, lk_or_w, values, z):
        """p(z) for the interpolant of values over {w^i} (barycentric, on the device; z in the domain included).
        lk_or_w: a LagrangeKey, or the root w itself (the domain size is then its multiplicative order)."""
        log_n, w = self._eval_domain(lk_or_w)
        vals = self._value_lists([values], 1 << log_n)[0]
        z = self._canon(z)
        if not len(vals):
            return self.Fq(0)
        ctx = self._context()
        d = self._upload(ctx, vals if isinstance(vals, np.ndarray) else _native.ints_to_limbs(vals))
        return self.Fq(ctx.eval_lagrange(log_n, w, len(vals), d.data_ptr(), z))

    def evaluate_evaluations_each(self, lk_or_w, value_lists, z_list):
        """[p_j(z_j)]: evaluate_evaluations for every vector of value_lists at its own point, in one batch on the
        device (kzg_fr_eval_lagrange_batch: a fixed number of launches whatever the count)."""
        log_n, w = self._eval_domain(lk_or_w)
        vals = self._value_lists(value_lists, 1 << log_n)
        zs = [self._canon(z) for z in z_list]
        if len(zs) != len(vals):
            raise ValueError(f"{len(vals)} value vectors but {len(zs)} points")
        if not vals:
            return []
        arr, lens, stride = self._pack(vals)
        out = self._context().eval_lagrange_batch(log_n, w, arr, lens, stride, _native.ints_to_limbs(zs))
        return [self.Fq(v) for v in _native.limbs_to_ints(out)]

    # ---- every proof on a domain at once (FK20: Feist-Khovratovich, "Fast amortized KZG proofs", 2020) -------------
    _DOMAIN_MAX = 1 << 20

    def _domain_size(self, n):
        n = int(n)
        if n < 2 or n & (n - 1) or n > self._DOMAIN_MAX:
            raise ValueError(f"domain size {n} is not a power of two in [2, 2^20]")
        return n

    @staticmethod
    def _monomial_key(ck, who):
        if isinstance(ck, (LagrangeKey, DomainTable)):
            raise TypeError(f"{who} needs a monomial key (setup / load_key / a list of points)")

    @staticmethod
    def _table_n(table, n, l=None):
        """a given domain size n (None: not given) and coset size l (None: not asked) against a table's: its n"""
        if n is not None and int(n) != table.n:
            raise ValueError(f"n = {n} differs from the table's domain size {table.n}")
        if l is not None and l != table.l:
            raise ValueError(f"l = {l} differs from the table's coset size {table.l}")
        return table.n

    def domain_table(self, ck, n):
        """The FK20 table of the first n points of a monomial key (CommitmentKey or list of points) for domain size n
        (a power of two, 2 <= n <= 2^20).  Built on the device; tables of a CommitmentKey are cached per (key, n)."""
        self._monomial_key(ck, "domain_table")
        n = self._domain_size(n)
        if len(ck) < n:
            raise ValueError(f"commitment key of {len(ck)} points is shorter than the domain ({n})")
        key = self._key(ck)
        ctx = self._context()
        return self._table_cached(key, (id(key), n), lambda: DomainTable(
            ctx, ctx.domain_table(key.srs, n.bit_length() - 1), n))

    def _table_cached(self, key, cache_key, make):
        return _lru_get(self._tables, cache_key, self._TABLE_CACHE, lambda e: e[0] is key, lambda: (key, make()),
                        lambda e: e[1].table.close())[1]

    def _fk20_call(self, who, ck_or_table, polynomials, n, w, l=None, N=None):
        """Host-side checks of open_domain* (l is None) and open_cosets*, `who` in the messages, before any device
        work: -> (coefficient lists, n, l, log_N, w).  n defaults to the smallest power of two >= the longest
        polynomial (setup_lagrange's rule; at least 2l for cosets), N to n."""
        cosets = l is not None
        if isinstance(ck_or_table, LagrangeKey):
            raise TypeError(f"{who} needs a monomial key or a {'coset table' if cosets else 'DomainTable'}, "
                            "not a LagrangeKey")
        if cosets:
            l = 1 << self._log2_exact(l, "coset size")
        coeffs = [self._coeffs(p) for p in polynomials]
        longest = max((len(c) for c in coeffs), default=0)
        if isinstance(ck_or_table, DomainTable):
            n = self._table_n(ck_or_table, n, l)
        elif n is None:
            n = max(2, 2 * l) if cosets else 2
            while n < longest:
                n *= 2
        n = self._domain_size(n)
        if cosets and l > n // 2:
            raise ValueError(f"coset size {l} exceeds n/2 = {n // 2}")
        if longest > n:
            raise ValueError(f"polynomial of {longest} coefficients exceeds the domain size {n}")
        if not isinstance(ck_or_table, DomainTable) and len(ck_or_table) < n:
            raise ValueError(f"commitment key of {len(ck_or_table)} points is shorter than the domain ({n})")
        N = n if N is None else int(N)
        if N < n or N & (N - 1) or N > min(4 * n, 2 * self._DOMAIN_MAX):
            raise ValueError(f"N = {N} is not a power of two in [n, min(4n, 2^21)]")
        log_N, w = self._domain(N, w)
        return coeffs, n, l, log_N, w

    def _combine_on_device(self, ctx, coeffs, xi):
        """sum_j xi^(j+1) coeffs[j] on the device (as in open): -> (device tensor of canonical words, its length)"""
        r = self.curve_order
        arr, lens, stride = self._pack(coeffs)
        length = max(max(lens, default=0), 1)
        import torch
        d_comb = torch.zeros((length, 4), dtype=torch.int64, device=f"cuda:{ctx.device}")
        d_in = self._upload(ctx, arr)                     # its synchronise covers the zero fill above as well
        ptrs = [d_in.data_ptr() + j * stride * 32 for j in range(len(coeffs))]
        scalars, x = [], xi
        for _ in coeffs:
            scalars.append(x)                                                  # xi^(j+1): kzg.py:148-150
            x = x * xi % r
        ctx.vec_lincomb(length, ptrs, lens, scalars, d_comb.data_ptr())
        return d_comb, length

    def open_domain(self, ck_or_table, polynomials, xi, n=None, w=None):
        """open(ck, polynomials, w^i, xi) for every i < n at once: a list of n proofs.  The xi^(j+1) combination runs
        on the device (as in open), then FK20 on the combined polynomial.  w defaults to Fq.root_of_unity(n)."""
        coeffs, n, _, _, w = self._fk20_call("open_domain", ck_or_table, polynomials, n, w)
        xi = self._canon(xi)
        table = ck_or_table if isinstance(ck_or_table, DomainTable) else self.domain_table(ck_or_table, n)
        ctx = self._context()
        d_comb, length = self._combine_on_device(ctx, coeffs, xi)
        xy, inf, _ = ctx.open_domain(table.table, d_comb.data_ptr(), [length], length, w, device=True, evals=False)
        return self._points(xy[0], inf[0])

    def open_domain_each(self, ck_or_table, polynomials, n=None, w=None):
        """All n proofs of each polynomial on its own: result[j][i] == open(ck, [polynomials[j]], w^i, 1)."""
        coeffs, n, _, _, w = self._fk20_call("open_domain", ck_or_table, polynomials, n, w)
        if not coeffs:
            return []
        table = ck_or_table if isinstance(ck_or_table, DomainTable) else self.domain_table(ck_or_table, n)
        arr, lens, stride = self._pack(coeffs)
        xy, inf, _ = self._context().open_domain(table.table, np.ascontiguousarray(arr), lens, stride, w, evals=False)
        return [self._points(xy[j], inf[j]) for j in range(len(coeffs))]

    # ---- coset openings: the values at l = 2^log_l points h zeta^k with ONE proof (FK20's multi-reveal) -------------
    #      Z = X^l - a, a = h^l; rho = p mod Z; pi = [(p - rho)/Z (tau)] G1; check e(C - [rho(tau)], G2) = e(pi, [tau^l] G2 - a G2).
    _COSET_MAX_LOG_L = 12          # kzg_open_coset

    @staticmethod
    def _log2_exact(v, what):
        v = int(v)
        if v < 1 or v & (v - 1):
            raise ValueError(f"{what} {v} is not a power of two")
        return v.bit_length() - 1

    def coset_table(self, ck, n, l):
        """The coset table of the first n points of a monomial key for cosets of l points (powers of two, 2 <= n <=
        2^20, l <= n/2).  Built on the device; cached per (key, n, l) beside domain_table's tables."""
        self._monomial_key(ck, "coset_table")
        n = self._domain_size(n)
        log_l = self._log2_exact(l, "coset size")
        if (1 << log_l) > n // 2:
            raise ValueError(f"coset size {l} exceeds n/2 = {n // 2}")
        if len(ck) < n:
            raise ValueError(f"commitment key of {len(ck)} points is shorter than the domain ({n})")
        key = self._key(ck)
        ctx = self._context()
        return self._table_cached(key, (id(key), n, 1 << log_l), lambda: DomainTable(
            ctx, ctx.coset_table(key.srs, n.bit_length() - 1, log_l), n, 1 << log_l))

    def _coset_table_for(self, ck_or_table, n, l):
        return ck_or_table if isinstance(ck_or_table, DomainTable) else self.coset_table(ck_or_table, n, l)

    def open_cosets(self, ck_or_table, polynomials, xi, l, n=None, w=None, N=None):
        """One proof per coset of l points of the domain {w^t, t < N}: coset i is {w^(i + k N/l), k < l}, a list of
        N/l proofs of the xi^(j+1) combination (combined on the device, as in open_domain).  w defaults to
        Fq.root_of_unity(N), N to n."""
        coeffs, n, l, log_N, w = self._fk20_call("open_cosets", ck_or_table, polynomials, n, w, l, N)
        xi = self._canon(xi)
        table = self._coset_table_for(ck_or_table, n, l)
        ctx = self._context()
        d_comb, length = self._combine_on_device(ctx, coeffs, xi)
        xy, inf, _ = ctx.open_cosets(table.table, d_comb.data_ptr(), [length], length, log_N, w, device=True,
                                     evals=False)
        return self._points(xy[0], inf[0])

    def open_cosets_each(self, ck_or_table, polynomials, l, n=None, w=None, N=None, with_values=False):
        """Every coset proof of each polynomial on its own: result[j][i] == open_coset(ck, [polynomials[j]], w^i, l,
        1, w^(N/l)).  with_values: (proofs, values), values[j][i][k] = p_j(w^(i + k N/l))."""
        coeffs, n, l, log_N, w = self._fk20_call("open_cosets", ck_or_table, polynomials, n, w, l, N)
        if not coeffs:
            return ([], []) if with_values else []
        table = self._coset_table_for(ck_or_table, n, l)
        arr, lens, stride = self._pack(coeffs)
        xy, inf, ev = self._context().open_cosets(table.table, np.ascontiguousarray(arr), lens, stride, log_N, w,
                                                  evals=with_values)
        proofs = [self._points(xy[j], inf[j]) for j in range(len(coeffs))]
        if not with_values:
            return proofs
        return proofs, self._cell_values(ev, len(coeffs), (1 << log_N) // l, l)

    @staticmethod
    def _cell_values(ev, b, cosets, l):
        """uint64[b, cosets, l, 4] words -> values[j][i][k], ints"""
        ints = _native.limbs_to_ints(np.ascontiguousarray(ev).reshape(-1, 4))
        return [[[ints[(j * cosets + i) * l + k] for k in range(l)] for i in range(cosets)] for j in range(b)]

    # ---- coset recovery: the polynomial back from any n/l of its N/l cosets (recover_cells_and_kzg_proofs of EIP-7594)
    def _recover_call(self, coset_indices, values, l, n, N, w):
        """Host-side checks of recover_cosets*, before any device work: -> (uint32 indices, uint64[b, K, l, 4] values,
        b, log_n, log_N, log_l, w)."""
        log_l = self._log2_exact(l, "coset size")
        l = 1 << log_l
        if log_l > self._COSET_MAX_LOG_L:
            raise ValueError(f"coset size {l} exceeds 2^{self._COSET_MAX_LOG_L}")
        log_n = self._log2_exact(n, "degree bound n")
        n = 1 << log_n
        N = 2 * n if N is None else int(N)
        if N < n or N < 2 or N & (N - 1) or N > 2 * self._DOMAIN_MAX:
            raise ValueError(f"N = {N} is not a power of two in [max(n, 2), 2^21]")
        if l > n or l >= N:
            raise ValueError(f"coset size {l} exceeds n = {n} or is not below N = {N}")
        log_N, w = self._domain(N, w)
        cosets = N // l
        idx = [int(i) for i in coset_indices]
        K = len(idx)
        if K * l < n:
            raise ValueError(f"{K} cosets of {l} values cannot determine a polynomial of degree < {n}")
        if any(i < 0 or i >= cosets for i in idx):
            raise ValueError(f"a coset index is outside [0, {cosets})")
        if len(set(idx)) != K:
            raise ValueError("a coset index is repeated")
        b = len(values)
        if b < 1:
            raise ValueError("recover_cosets needs at least one polynomial")
        r = self.curve_order
        flat = []
        for j, cells in enumerate(values):
            if len(cells) != K:
                raise ValueError(f"polynomial {j} has {len(cells)} cells for {K} coset indices")
            for cell in cells:
                if len(cell) != l:
                    raise ValueError(f"a cell of polynomial {j} has {len(cell)} values, not l = {l}")
                flat.extend(int(v) % r for v in cell)
        arr = _native.ints_to_limbs(flat).reshape(b, K, l, 4)
        return np.asarray(idx, dtype=np.uint32), arr, b, log_n, log_N, log_l, w

    @staticmethod
    def _first_inconsistent(ok, n):
        bad = [j for j, f in enumerate(ok) if not f]
        if bad:
            raise ValueError(f"recover_cosets: the values of polynomial {bad[0]} lie on no polynomial of degree < {n}")

    def recover_cosets(self, coset_indices, values, l, n, N=None, w=None):
        """The b polynomials of degree < n whose values on the cosets coset_indices[k] of {w^t, t < N} (open_cosets'
        numbering: coset i is {w^(i + k N/l), k < l}) are values[j][k], any K >= n/l distinct cosets in any order:
        b coefficient lists of length n.  ValueError names the first polynomial whose values lie on no polynomial of
        degree < n.  N defaults to 2n, w to Fq.root_of_unity(N)."""
        idx, arr, b, log_n, log_N, log_l, w = self._recover_call(coset_indices, values, l, n, N, w)
        coeffs, ok = self._context().recover_cosets(log_n, log_N, log_l, w, idx, arr, b)
        self._first_inconsistent(ok, 1 << log_n)
        ints = _native.limbs_to_ints(np.ascontiguousarray(coeffs).reshape(-1, 4))
        n = 1 << log_n
        return [ints[j * n:(j + 1) * n] for j in range(b)]

    def recover_cosets_and_open(self, ck_or_table, coset_indices, values, l, n=None, w=None, N=None):
        """recover_cosets followed by open_cosets_each(..., with_values=True) on the recovered polynomials, whose
        coefficients never leave the device: (proofs, values) of all N/l cosets of each polynomial.  n defaults to
        the table's domain size, else to N/2 (N given) or K l."""
        if isinstance(ck_or_table, LagrangeKey):
            raise TypeError("recover_cosets_and_open needs a monomial key or a coset table, not a LagrangeKey")
        if isinstance(ck_or_table, DomainTable):
            n = self._table_n(ck_or_table, n)
        elif n is None:
            n = int(N) // 2 if N is not None else len(coset_indices) * int(l)
        idx, arr, b, log_n, log_N, log_l, w = self._recover_call(coset_indices, values, l, n, N, w)
        n, l = 1 << log_n, 1 << log_l
        # what open_cosets asks on top (_fk20_call runs again, on the sizes alone)
        self._fk20_call("recover_cosets_and_open", ck_or_table, [], n, w, l, 1 << log_N)
        table = self._coset_table_for(ck_or_table, n, l)
        ctx = self._context()
        import torch
        d_coeffs = torch.empty((b, n, 4), dtype=torch.int64, device=f"cuda:{ctx.device}")
        d_vals = self._upload(ctx, arr)
        _, ok = ctx.recover_cosets(log_n, log_N, log_l, w, idx, d_vals.data_ptr(), b, d_coeffs=d_coeffs.data_ptr())
        self._first_inconsistent(ok, n)
        xy, inf, ev = ctx.open_cosets(table.table, d_coeffs.data_ptr(), [n] * b, n, log_N, w, device=True, evals=True)
        return [self._points(xy[j], inf[j]) for j in range(b)], self._cell_values(ev, b, (1 << log_N) // l, l)

    def _coset_root(self, l, zeta):
        """zeta for cosets of l points: Fq.root_of_unity(l) by default; a given one must be a primitive l-th root."""
        r = self.curve_order
        log_l = self._log2_exact(l, "coset size")
        if (r - 1) % (1 << log_l):
            raise ValueError(f"the scalar field has no {l}-th roots of unity")
        zeta = int(self.Fq.root_of_unity(1 << log_l)) if zeta is None else int(zeta) % r
        if log_l == 0:
            if zeta != 1:
                raise ValueError("zeta must be 1 for l = 1")
        elif pow(zeta, (1 << log_l) // 2, r) != r - 1:
            raise ValueError(f"zeta is not a primitive {l}-th root of unity")
        return log_l, zeta

    def open_coset(self, ck, polynomials, h, l, xi, zeta=None, with_values=False):
        """ONE proof for the values of the xi^(j+1) combination at the l points h zeta^k (zeta defaults to
        Fq.root_of_unity(l)): the commitment of (p - rho) / (X^l - h^l), rho = p mod (X^l - h^l).  l = 1 is open() at
        z = h.  with_values: (proof, [combined(h zeta^k) for k < l])."""
        self._monomial_key(ck, "open_coset")
        log_l, zeta = self._coset_root(l, zeta)
        if log_l > self._COSET_MAX_LOG_L:
            raise ValueError(f"coset size {l} exceeds 2^{self._COSET_MAX_LOG_L}")
        h = self._canon(h)
        if h == 0:
            raise ValueError("h must be non-zero")
        xi = self._canon(xi)
        coeffs = [self._coeffs(p) for p in polynomials]
        if len(coeffs) > 64:
            raise ValueError("at most 64 polynomials per opening")
        longest = max((len(c) for c in coeffs), default=0)
        if longest > len(ck):
            raise ValueError(f"Polynomial degree {longest - 1} exceeds maximum allowed degree {len(ck) - 1}")
        key = self._key(ck)
        arr, lens, stride = self._pack(coeffs)
        xy, inf, ev = self._context().open_coset(key.srs, arr, lens, stride, log_l, h, zeta, xi)
        proof = self._points(xy, inf)[0]
        if not with_values:
            return proof
        return proof, [int(v) for v in _native.limbs_to_ints(np.ascontiguousarray(ev).reshape(-1, 4))]

    # ---- coset verification (host) ---------------------------------------------------------------------------------
    def coset_verification_key(self, l, tau):
        """[tau^l] G2, the verifier's key for cosets of l points (l = 1: setup's tau G2)."""
        self._log2_exact(l, "coset size")
        return self.multiply(self.G2, pow(int(tau) % self.curve_order, int(l), self.curve_order))

    def _coset_remainder(self, h, values, zeta):
        """rho_j = h^-j l^-1 sum_k y_k zeta^(-jk): the coefficients of the remainder from its values at h zeta^k."""
        r, l = self.curve_order, len(values)
        h, zinv = int(self.Fq(h)), pow(zeta, -1, r)
        lin, hinv = pow(l, -1, r), pow(h, -1, r)
        ys = [int(self.Fq(v)) for v in values]
        out, hp = [], lin
        for j in range(l):
            zj = pow(zinv, j, r)
            acc, zp = 0, 1
            for y in ys:
                acc += y * zp
                zp = zp * zj % r
            out.append(acc % r * hp % r)
            hp = hp * hinv % r
        return out

    def _folded_cosets(self, commitments, evaluations, xi, l):
        """(sum_j xi^(j+1) C_j as a list of terms, sum_j xi^(j+1) y_j[k] for k < l) -- _folded_claim per value"""
        r = self.curve_order
        if len(evaluations) < len(commitments):
            raise IndexError("list index out of range")
        weight, parts, folded = xi, [], [0] * l
        for j, C in enumerate(commitments):
            ys = list(evaluations[j])
            if len(ys) != l:
                raise ValueError(f"{len(ys)} values for a coset of {l} points")
            parts.append(self.multiply(C, weight))
            folded = [(f + weight * int(self.Fq(y))) % r for f, y in zip(folded, ys)]
            weight = weight * xi % r
        return parts, folded

    def _rho_commitment_terms(self, ck, rho):
        return [self.multiply(ck[j], c) for j, c in enumerate(rho) if c]

    def check_coset(self, ck, rk_l, commitments, h, evaluations, proof, xi, zeta=None):
        """Two pairings: e(F - [rho(tau)], G2) = e(pi, rk_l - h^l G2), F = sum_j xi^(j+1) C_j, rho the remainder of the
        folded values; evaluations[j] holds the l values of polynomial j at h zeta^k."""
        evaluations = [list(e) for e in evaluations]
        l = len(evaluations[0]) if evaluations else 1
        _, zeta = self._coset_root(l, zeta)
        r = self.curve_order
        h, xi = int(self.Fq(h)), int(self.Fq(xi))
        if h == 0 or len(ck) < l:
            return False
        parts, folded = self._folded_cosets(commitments, evaluations, xi, l)
        rho = self._coset_remainder(h, folded, zeta)
        parts += [self.neg(p) for p in self._rho_commitment_terms(ck, rho)]
        shifted = self.add(rk_l, self.neg(self.multiply(self.G2, pow(h, l, r))))
        return self.pairing(self.G2, self._sum_g1(parts)) == self.pairing(shifted, proof)

    def batch_check_cosets(self, ck, rk_l, commitments_list, h_list, evaluations_list, proof_list, xi_list, zeta=None,
                           r=None):
        """Every claim e(F_i - [rho_i(tau)] + a_i pi_i, G2) = e(pi_i, rk_l), a_i = h_i^l, weighted rho^(i+1) as in
        batch_check: two pairings in all, and the weighted remainders fold into ONE polynomial of degree < l, so the
        interpolants cost one l-term sum."""
        order = self.curve_order
        claims = list(zip(commitments_list, h_list, evaluations_list, proof_list, xi_list))
        if not claims:
            return True
        l = len(list(claims[0][2])[0]) if len(list(claims[0][2])) else 1
        _, zeta = self._coset_root(l, zeta)
        if len(ck) < l:
            return False
        rho_w = int(self.Fq(self.Fq.random_element() if r is None else r))
        weight, lhs, rhs, rho_sum = rho_w, [], [], [0] * l
        for commitments, h, evaluations, proof, xi in claims:
            evaluations = [list(e) for e in evaluations]
            h = int(self.Fq(h))
            if h == 0:
                return False
            parts, folded = self._folded_cosets(commitments, evaluations, int(self.Fq(xi)), l)
            rho = self._coset_remainder(h, folded, zeta)
            rho_sum = [(s + weight * c) % order for s, c in zip(rho_sum, rho)]
            F = self._sum_g1(parts + [self.multiply(proof, pow(h, l, order))])
            lhs.append(self.multiply(F, weight))
            rhs.append(self.multiply(proof, weight))
            weight = weight * rho_w % order
        lhs += [self.neg(p) for p in self._rho_commitment_terms(ck, rho_sum)]
        return self.pairing(self.G2, self._sum_g1(lhs)) == self.pairing(rk_l, self._sum_g1(rhs))

    # ---- pairing-product checks on the device (kzg_pairing_check / kzg_pairing_product) ----------------
    _PAIRING_MAX_PAIRS = 16

    def _pairing_arrays(self, pairs, who):
        """one equation [(G1 point, G2 point), ...] or a list of equations -> (single, g1 xy, g1 inf, g2 xy, g2 inf, k)
        in the C layout; every equation of a call has the same number k of pairs, 1 <= k <= 16"""
        pairs = list(pairs)
        single = bool(pairs) and len(pairs[0]) == 2 and len(pairs[0][0]) == 3 and not isinstance(pairs[0][0][0], (tuple, list))
        eqs = [pairs] if single else [list(e) for e in pairs]
        if not eqs:
            return single, None, None, None, None, 0
        k = len(eqs[0])
        if not 1 <= k <= self._PAIRING_MAX_PAIRS:
            raise ValueError(f"{who}: an equation has between 1 and {self._PAIRING_MAX_PAIRS} pairs, not {k}")
        if any(len(e) != k for e in eqs) or any(len(pr) != 2 for e in eqs for pr in e):
            raise ValueError(f"{who}: every equation of a call needs the same number of (G1, G2) pairs")
        L = (self._cv.p.bit_length() + 63) // 64
        g1_xy, g1_inf = _native.points_to_limbs([pr[0] for e in eqs for pr in e], L, self._g1.normalize)
        g2_xy, g2_inf = _native.g2_points_to_limbs([self._g2.normalize(pr[1]) for e in eqs for pr in e], L)
        return single, g1_xy, g1_inf, g2_xy, g2_inf, k

    def _pairing_subgroups(self, g1_xy, g1_inf, g2_xy, g2_inf, k, who):
        """check_subgroup=True of pairing_check / pairing_product: every G2 point through kzg_g2_check_subgroup and, on
        bls12_381 (bn254's G1 has cofactor 1), every G1 point through kzg_g1_check_subgroup.  A point outside its
        subgroup raises ValueError naming the equation and the pair; a malformed point is left to the pairing."""
        ctx = self._context()
        checks = [("G2", ctx.g2_check_subgroup(g2_xy, g2_inf))]
        if self.curve_type == "bls12_381":
            checks.append(("G1", ctx.g1_check_subgroup(g1_xy, g1_inf)))
        for group, status in checks:
            bad = np.flatnonzero(status == 3)
            if bad.size:
                i = int(bad[0])
                raise ValueError(f"{who}: equation {i // k}, pair {i % k}: the {group} point is outside the "
                                 f"prime-order subgroup")

    def pairing_check(self, pairs, check_subgroup=False):
        """Is the product of e(P_i, Q_i) over the pairs (P_i in G1, Q_i in G2) of an equation one?  pairs: one equation
        as a list of (G1_point, G2_point) -> bool, or a list of equations (the same number of pairs each, at most 16)
        -> a list of bools, one wave of the device per equation.  A malformed point (a coordinate >= p, off its curve
        or twist) gives False.  Membership in the prime-order subgroups is tested only with check_subgroup=True: a point
        outside its subgroup then raises ValueError naming the equation and the pair (a pairing check against such a
        point proves nothing)."""
        single, g1_xy, g1_inf, g2_xy, g2_inf, k = self._pairing_arrays(pairs, "pairing_check")
        if k == 0:
            return []
        if check_subgroup:
            self._pairing_subgroups(g1_xy, g1_inf, g2_xy, g2_inf, k, "pairing_check")
        status = self._context().pairing_check(g1_xy, g1_inf, g2_xy, g2_inf, k)
        out = [int(st) == 0 for st in status]
        return out[0] if single else out

    def pairing_product(self, pairs, check_subgroup=False):
        """The value of the product: the 12-tuple pairing() returns, raised to c = _native.PAIRING_GT_MULTIPLE[curve] (1 on
        BN254, 3 on BLS12-381) -- for one equation, or a list of them for a list of equations.  ValueError for a
        malformed point; with check_subgroup=True also for a point outside its prime-order subgroup."""
        single, g1_xy, g1_inf, g2_xy, g2_inf, k = self._pairing_arrays(pairs, "pairing_product")
        if k == 0:
            return []
        if check_subgroup:
            self._pairing_subgroups(g1_xy, g1_inf, g2_xy, g2_inf, k, "pairing_product")
        gt, status = self._context().pairing_product(g1_xy, g1_inf, g2_xy, g2_inf, k)
        if (status == 2).any():
            raise ValueError(f"pairing_product: equation {int(np.flatnonzero(status == 2)[0])} has a malformed point")
        out = [_native.gt_to_tuple(row, self.curve_type) for row in gt]
        return out[0] if single else out

    def _verdict(self, L_pt, R_pt, g2_right, pairing, who):
        """e(L, G2) == e(R, g2_right): pairing = "device": one kzg_pairing_check on [(L, G2), (-R, g2_right)];
        "host": the two pure-Python pairings of pairing.py.  The verdicts are the same."""
        if pairing == "device":
            return self.pairing_check([(L_pt, self.G2), (self.neg(R_pt), g2_right)])
        if pairing == "host":
            return self.pairing(self.G2, L_pt) == self.pairing(g2_right, R_pt)
        raise ValueError(f"{who}: pairing must be \"device\" or \"host\", not {pairing!r}")

    # ---- bulk verification (device): K claims folded into the two G1 points of one pairing equation -----------------
    _VERIFY_MAX_N = 1 << 21

    def _g1_arrays(self, points, what):
        """points: a list of point tuples, or (xy uint64[n, 2L], inf uint8[n] | None) in the C layout -> (xy, inf)."""
        L = (self._cv.p.bit_length() + 63) // 64                  # uint64 limbs per coordinate (kzg_fp_limbs)
        if isinstance(points, tuple) and len(points) == 2 and isinstance(points[0], np.ndarray):
            xy = np.ascontiguousarray(points[0], dtype=np.uint64).reshape(-1, 2 * L)
            inf = None if points[1] is None else np.ascontiguousarray(points[1], dtype=np.uint8).reshape(-1)
            if inf is not None and inf.size != xy.shape[0]:
                raise ValueError(f"{what}: {inf.size} infinity flags for {xy.shape[0]} points")
            return xy, inf
        return _native.points_to_limbs(points, L, self._g1.normalize)

    def verify_cosets(self, ck, rk_l, commitments, commitment_indices, coset_indices, values, proofs, l, N, w=None,
                      r=None, check_subgroup=False, pairing="device"):
        """Cell k claims: the polynomial of commitments[commitment_indices[k]] takes the l values values[k][t] at
        w^(coset_indices[k] + t N/l), t < l, with proof proofs[k] -- open_cosets' numbering; l = 1: single points.
        All claims are combined with weights r^(k+1) (r sampled when not given, as in batch_check) into two G1 points
        on the device, then pairing(G2, L) == pairing(rk_l, R) with rk_l = [tau^l] G2 (coset_verification_key).
        proofs / commitments: lists of point tuples or (xy, inf) arrays in the C layout (what Context.open_cosets
        returns); values: nested lists or a uint64[K, l, 4] array.  A point off the curve: False.  No claims: True.
        check_subgroup=True first runs commitments and proofs through kzg_g1_check_subgroup on the device and returns
        False when one lies outside the prime-order subgroup: for a point T of the cofactor torsion pi + T satisfies
        the pairing equation whenever pi does, so a verifier of untrusted proofs wants it.  The default skips the
        test (as check / batch_check do).  pairing: "device" ends with one kzg_pairing_check on [(L, G2), (-R, rk_l)],
        "host" with the two Python pairings; the verdict is the same."""
        if pairing not in ("device", "host"):
            raise ValueError(f"verify_cosets: pairing must be \"device\" or \"host\", not {pairing!r}")
        self._monomial_key(ck, "verify_cosets")
        l = 1 << self._log2_exact(l, "coset size")
        N = int(N)
        if N < 2 or N & (N - 1) or N > self._VERIFY_MAX_N:
            raise ValueError(f"N = {N} is not a power of two in [2, 2^21]")
        if l > N // 2:
            raise ValueError(f"coset size {l} exceeds N/2 = {N // 2}")
        if l > (1 << self._COSET_MAX_LOG_L):
            raise ValueError(f"coset size {l} exceeds 2^{self._COSET_MAX_LOG_L}")
        log_N, w = self._domain(N, w)
        if len(ck) < l:
            raise ValueError(f"commitment key of {len(ck)} points is shorter than the coset size {l}")
        comm_idx = np.ascontiguousarray(commitment_indices, dtype=np.int64).reshape(-1)
        coset_idx = np.ascontiguousarray(coset_indices, dtype=np.int64).reshape(-1)
        K = comm_idx.size
        pxy, pinf = self._g1_arrays(proofs, "proofs")
        cxy, cinf = self._g1_arrays(commitments, "commitments")
        if isinstance(values, np.ndarray) and values.dtype == np.uint64:
            vals = np.ascontiguousarray(values)
        else:
            order = self.curve_order
            rows = [list(v) for v in values]
            if any(len(v) != l for v in rows):
                raise ValueError(f"every cell needs {l} values")
            flat = [int(y) % order for v in rows for y in v]
            vals = _native.ints_to_limbs(flat) if flat else np.zeros((0, 4), dtype=np.uint64)
        if coset_idx.size != K or pxy.shape[0] != K or vals.size != K * l * 4:
            raise ValueError("commitment_indices, coset_indices, values and proofs must describe the same number of "
                             f"cells of {l} values")
        if K > (1 << 21) or K * l > (1 << 24):
            raise ValueError("at most 2^21 cells and 2^24 values per call")
        if not 1 <= cxy.shape[0] <= (1 << 16):
            raise ValueError("between 1 and 2^16 commitments per call")
        if K and (comm_idx.min() < 0 or comm_idx.max() >= cxy.shape[0]):
            raise ValueError("commitment index out of range")
        if K and (coset_idx.min() < 0 or coset_idx.max() >= N // l):
            raise ValueError(f"coset index out of range [0, {N // l})")
        rho = int(self.Fq(self.Fq.random_element() if r is None else r))
        if K == 0:
            return True
        key = self._key(ck)
        if check_subgroup:
            ctx = self._context()
            if ctx.g1_check_subgroup(cxy, cinf).any() or ctx.g1_check_subgroup(pxy, pinf).any():
                return False
        try:
            xy, inf = self._context().verify_cosets(key.srs, log_N, l.bit_length() - 1, w, cxy, cinf,
                                                    comm_idx.astype(np.uint32), coset_idx.astype(np.uint32),
                                                    vals.reshape(K, l, 4), pxy, pinf, rho)
        except _native.NativeError as e:
            if e.code == -1 and "not on the curve" in str(e):
                return False
            raise
        L_pt, R_pt = self._points(xy, inf)
        return self._verdict(L_pt, R_pt, rk_l, pairing, "verify_cosets")

    def verify_domain(self, ck, rk, commitment, values, proofs, N=None, w=None, r=None, check_subgroup=False,
                      pairing="device"):
        """The whole output of open_domain at once: proofs[i] opens `commitment` to values[i] at w^i, i < N (N defaults
        to the number of proofs); rk is setup's tau G2.  verify_cosets with l = 1 (check_subgroup: as there)."""
        if isinstance(values, np.ndarray) and values.dtype == np.uint64:
            count = values.size // 4
        else:
            values = [[v] for v in values]
            count = len(values)
        N = count if N is None else int(N)
        return self.verify_cosets(ck, rk, [commitment], np.zeros(count, dtype=np.int64),
                                  np.arange(count, dtype=np.int64), values, proofs, 1, N, w=w, r=r,
                                  check_subgroup=check_subgroup, pairing=pairing)

    # ---- bulk verification at arbitrary points (device): blob batches into the two G1 points of one pairing equation --
    @staticmethod
    def _verification_key(rk, who):
        if not (isinstance(rk, (tuple, list)) and len(rk) == 3 and isinstance(rk[0], tuple)):
            raise TypeError(f"{who}: rk must be a G2 point (setup's tau G2)")

    def verify_points(self, rk, commitments, commitment_indices, z_list, evaluations, proofs, r=None,
                      check_subgroup=False, pairing="device"):
        """Claim k: the polynomial of commitments[commitment_indices[k]] takes the value evaluations[k] at z_list[k]
        -- any field element, the output of open / open_evaluations with xi = 1 or an EIP-4844 blob proof -- with proof
        proofs[k].  All claims are combined with weights r^(k+1) (r sampled when not given, as in batch_check) into two
        G1 points on the device (kzg_verify_points), then pairing(G2, L) == pairing(rk, R) with rk = tau G2.
        proofs / commitments: lists of point tuples or (xy, inf) arrays in the C layout.  A point off the curve: False.
        No claims: True.  check_subgroup, pairing: as in verify_cosets."""
        if pairing not in ("device", "host"):
            raise ValueError(f"verify_points: pairing must be \"device\" or \"host\", not {pairing!r}")
        self._verification_key(rk, "verify_points")
        order = self.curve_order
        comm_idx = np.ascontiguousarray(commitment_indices, dtype=np.int64).reshape(-1)
        K = comm_idx.size
        pxy, pinf = self._g1_arrays(proofs, "proofs")
        cxy, cinf = self._g1_arrays(commitments, "commitments")
        zs = [int(v) % order for v in z_list]
        ys = [int(v) % order for v in evaluations]
        if len(zs) != K or len(ys) != K or pxy.shape[0] != K:
            raise ValueError("commitment_indices, z_list, evaluations and proofs must describe the same number of claims")
        if K > (1 << 21):
            raise ValueError("at most 2^21 claims per call")
        if not 1 <= cxy.shape[0] <= (1 << 16):
            raise ValueError("between 1 and 2^16 commitments per call")
        if K and (comm_idx.min() < 0 or comm_idx.max() >= cxy.shape[0]):
            raise ValueError("commitment index out of range")
        rho = int(self.Fq(self.Fq.random_element() if r is None else r))
        if K == 0:
            return True
        ctx = self._context()
        if check_subgroup and (ctx.g1_check_subgroup(cxy, cinf).any() or ctx.g1_check_subgroup(pxy, pinf).any()):
            return False
        try:
            xy, inf = ctx.verify_points(cxy, cinf, comm_idx.astype(np.uint32), _native.ints_to_limbs(zs),
                                        _native.ints_to_limbs(ys), pxy, pinf, rho)
        except _native.NativeError as e:
            if e.code == -1 and "not on the curve" in str(e):
                return False
            raise
        L_pt, R_pt = self._points(xy, inf)
        return self._verdict(L_pt, R_pt, rk, pairing, "verify_points")

    def verify_blobs(self, lk_or_w, rk, commitments, value_lists, z_list, proofs, r=None, check_subgroup=False,
                     pairing="device"):
        """A batch of blobs: value_lists[j] (values over the domain of lk_or_w) against commitments[j] at the challenge
        z_list[j] with proof proofs[j] -- verify_blob_kzg_proof_batch of EIP-4844 with the challenges given (the hash
        that derives them is the protocol's).  The claimed values are computed on the device
        (evaluate_evaluations_each), then verify_points."""
        self._verification_key(rk, "verify_blobs")
        value_lists, z_list = list(value_lists), list(z_list)
        commitments = self._g1_arrays(commitments, "commitments")          # converted once: verify_points takes (xy, inf)
        proofs = self._g1_arrays(proofs, "proofs")
        if not (len(value_lists) == len(z_list) == commitments[0].shape[0] == proofs[0].shape[0]):
            raise ValueError("commitments, value_lists, z_list and proofs must describe the same number of blobs")
        if not value_lists:
            return True
        ys = self.evaluate_evaluations_each(lk_or_w, value_lists, z_list)
        return self.verify_points(rk, commitments, np.arange(len(ys), dtype=np.int64), z_list, [int(v) for v in ys],
                                  proofs, r=r, check_subgroup=check_subgroup, pairing=pairing)

    # ---- EIP-4844 blobs as bytes (device intake, SHA-256 challenges on the device): the spec's calls by name ------------
    #      A blob is n elements of 32 big-endian bytes in bit-reversed order over the domain; commitments and proofs are
    #      compressed points (compress_g1's formats).  blobs: a list of bytes objects or a uint8[b, 32 n] array;
    #      commitments / proofs: lists of bytes objects or uint8[b, G] arrays.
    _FS_DOMAIN = b"FSBLOBVERIFY_V1_"               # the domain of the blob challenge (hashed on the device)
    _RHO_DOMAIN = b"RCKZGBATCH___V1_"              # the domain of the batch's weight base (hashed here)

    @staticmethod
    def _byte_rows(rows, size, what):
        """a list of bytes objects or a uint8[b, size] array -> uint8[b, size]; ValueError names the first row of another
        size"""
        if isinstance(rows, np.ndarray):
            arr = np.ascontiguousarray(rows, dtype=np.uint8)
            if arr.ndim != 2 or arr.shape[1] != size:
                raise ValueError(f"{what}: an array of shape {arr.shape}, expected (b, {size})")
            return arr if arr.flags.writeable else arr.copy()          # torch uploads writable arrays only
        rows = [bytes(x) for x in rows]
        for i, x in enumerate(rows):
            if len(x) != size:
                raise ValueError(f"{what} {i}: {len(x)} bytes, expected {size}")
        return np.frombuffer(bytearray(b"".join(rows)), dtype=np.uint8).reshape(len(rows), size)     # writable

    def _blob_size(self, n):
        """log_n of a blob of n elements: a power of two in [2, 2^24]"""
        n = int(n)
        if n < 2 or n & (n - 1) or n > (1 << 24):
            raise ValueError(f"blob size {n} is not a power of two in [2, 2^24]")
        return n.bit_length() - 1

    def _first_bad_element(self, blob_row, j):
        """the ValueError of a blob whose status is 1: its first element >= r, found on the host"""
        r, raw = self.curve_order, blob_row.tobytes()
        i = next(i for i in range(len(raw) // 32) if int.from_bytes(raw[32 * i:32 * i + 32], "big") >= r)
        return ValueError(f"blob {j}: element {i} is not below the field modulus")

    def blob_to_values(self, blobs, n, bit_reversed=True, strict=True):
        """The field elements of b blobs of n elements: a uint64[b, n, 4] array of canonical limbs, in natural domain
        order when the blobs are bit-reversed (EIP-4844's order; bit_reversed=False keeps the order of the bytes) --
        the form commit_evaluations / open_evaluations take.  Checked and permuted on the device (kzg_blob_to_fr).
        strict: the first blob holding an element >= r raises ValueError naming the blob and its first such element;
        strict=False returns (values, status), status uint8[b] with 1 for such a blob (its elements >= r read as 0)."""
        log_n = self._blob_size(n)
        arr = self._byte_rows(blobs, 32 << log_n, "blob")
        with _bad_input_is_value_error():
            vals, status = self._context().blob_to_fr(arr, log_n, bit_reversed)
        if not strict:
            return vals, status
        bad = np.flatnonzero(status)
        if bad.size:
            raise self._first_bad_element(arr[int(bad[0])], int(bad[0]))
        return vals

    def blob_challenges(self, blobs, commitments, n):
        """[z_j]: SHA-256("FSBLOBVERIFY_V1_" | n as 16 bytes | blob_j | commitment_j) mod r, compute_challenge of
        EIP-4844, one lane per blob on the device (kzg_blob_challenges).  The bytes are hashed as given."""
        log_n = self._blob_size(n)
        ctx = self._context()
        arr = self._byte_rows(blobs, 32 << log_n, "blob")
        comm = self._byte_rows(commitments, ctx.g1_bytes, "commitment")
        if comm.shape[0] != arr.shape[0]:
            raise ValueError(f"{arr.shape[0]} blobs but {comm.shape[0]} commitments")
        if not arr.shape[0]:
            return []
        with _bad_input_is_value_error():
            z = ctx.blob_challenges(arr, comm, log_n)
        return [self.Fq(v) for v in _native.limbs_to_ints(z)]

    @staticmethod
    def _lagrange_key(lk, who):
        if not isinstance(lk, LagrangeKey):
            raise TypeError(f"{who} needs a LagrangeKey (setup_lagrange / lagrange_key)")

    def blob_to_kzg_commitment(self, lk, blobs):
        """blob_to_kzg_commitment of EIP-4844 for every blob: a list of compressed commitments (bytes).  Intake on the
        device, the commit pipeline on the Lagrange key, compression on the device.  A blob with an element >= r
        raises ValueError."""
        self._lagrange_key(lk, "blob_to_kzg_commitment")
        vals = self.blob_to_values(blobs, lk.n)
        b = vals.shape[0]
        if not b:
            return []
        ctx = self._context()
        xy, inf = ctx.commit(lk.srs, vals, [lk.n] * b, lk.n)
        return [row.tobytes() for row in ctx.g1_compress(xy, inf)]

    def compute_blob_kzg_proof(self, lk, blobs, commitments):
        """compute_blob_kzg_proof of EIP-4844 for every blob: a list of compressed proofs (bytes).  The blobs are
        uploaded once; challenges z_j and values come from the device (kzg_blob_challenges_device, kzg_blob_to_fr_device),
        then one evaluation-form opening per blob at z_j with xi = 1, queued through the commit pipeline
        (kzg_open_evals_device_async).  A blob with an element >= r raises ValueError."""
        self._lagrange_key(lk, "compute_blob_kzg_proof")
        n, log_n = lk.n, self._blob_size(lk.n)
        ctx = self._context()
        arr = self._byte_rows(blobs, 32 * n, "blob")
        comm = self._byte_rows(commitments, ctx.g1_bytes, "commitment")
        b = arr.shape[0]
        if comm.shape[0] != b:
            raise ValueError(f"{b} blobs but {comm.shape[0]} commitments")
        if not b:
            return []
        import torch
        dev = f"cuda:{ctx.device}"
        d_vals = torch.empty((b, n, 4), dtype=torch.int64, device=dev)
        d_z = torch.empty((b, 4), dtype=torch.int64, device=dev)
        d_status = torch.empty(b, dtype=torch.uint8, device=dev)
        d_blobs, d_comm = self._upload(ctx, arr), self._upload(ctx, comm)
        with _bad_input_is_value_error():
            ctx.blob_to_fr_device(d_blobs.data_ptr(), log_n, b, True, d_vals.data_ptr(), d_status.data_ptr())
            ctx.blob_challenges_device(d_blobs.data_ptr(), d_comm.data_ptr(), log_n, b, d_z.data_ptr())
        ctx.synchronize()
        bad = np.flatnonzero(d_status.cpu().numpy())
        if bad.size:
            raise self._first_bad_element(arr[int(bad[0])], int(bad[0]))
        z = np.ascontiguousarray(d_z.cpu().numpy().view(np.uint64))
        one = _native.int_to_words(1)
        out = [_native.result_buffers(ctx.fp_limbs, evals=4) for _ in range(b)]
        try:
            for j in range(b):
                ctx.open_evals_device_async(lk.srs, d_vals.data_ptr() + j * n * 32, [n], n, z[j], one, *out[j])
        finally:
            ctx.commit_flush()
        xy = np.stack([o[0] for o in out])
        inf = np.concatenate([o[1] for o in out])
        return [row.tobytes() for row in ctx.g1_compress(xy, inf)]

    def _blob_batch_rho(self, n, commitments, zs, ys, proofs):
        """SHA-256("RCKZGBATCH___V1_" | n as 8 bytes | b as 8 bytes | per blob: commitment | z | y | proof) mod r --
        160 b bytes, on the host.  commitments / proofs: rows of bytes; zs, ys: ints."""
        import hashlib
        h = hashlib.sha256(self._RHO_DOMAIN + int(n).to_bytes(8, "big") + len(zs).to_bytes(8, "big"))
        for c, z, y, p in zip(commitments, zs, ys, proofs):
            h.update(bytes(c) + int(z).to_bytes(32, "big") + int(y).to_bytes(32, "big") + bytes(p))
        return int.from_bytes(h.digest(), "big") % self.curve_order

    def verify_blob_kzg_proof_batch(self, lk_or_w, rk, blobs, commitments, proofs, pairing="device"):
        """verify_blob_kzg_proof_batch of EIP-4844: do proofs[j] open commitments[j] to the value of blobs[j] at its
        challenge, for every j?  lk_or_w: a LagrangeKey or the domain's root w (as in verify_blobs); rk: setup's tau G2.
        The blobs are uploaded once and stay on the device: intake, challenges and the values y_j = p_j(z_j)
        (kzg_blob_to_fr_device, kzg_blob_challenges_device, kzg_fr_eval_lagrange_batch_device); only z and y come back.
        Commitments and proofs are decompressed with the subgroup test on the device.  The claims are folded by
        kzg_verify_points with the weights rho^(k+1), rho = SHA-256("RCKZGBATCH___V1_" | n | b | per blob:
        commitment | z | y | proof) mod r: the protocol fixes the verdict, not the weights (the specification's
        rho^k differ by the common factor rho).  Two pairings: on the device in one kzg_pairing_check
        (pairing="device"), or pairing.py's on the host ("host"); the verdict is the same.
        False, not an exception: an element >= r, a malformed point, a point off the curve or outside the subgroup, a
        wrong proof.  ValueError: mismatched counts or sizes.  No blobs: True."""
        if pairing not in ("device", "host"):
            raise ValueError(f"verify_blob_kzg_proof_batch: pairing must be \"device\" or \"host\", not {pairing!r}")
        self._verification_key(rk, "verify_blob_kzg_proof_batch")
        log_n, w = self._eval_domain(lk_or_w)
        n = 1 << log_n
        self._blob_size(n)
        ctx = self._context()
        G = ctx.g1_bytes
        arr = self._byte_rows(blobs, 32 * n, "blob")
        comm = self._byte_rows(commitments, G, "commitment")
        prf = self._byte_rows(proofs, G, "proof")
        b = arr.shape[0]
        if comm.shape[0] != b or prf.shape[0] != b:
            raise ValueError("blobs, commitments and proofs must describe the same number of blobs")
        if not b:
            return True
        import torch
        dev = f"cuda:{ctx.device}"
        d_vals = torch.empty((b, n, 4), dtype=torch.int64, device=dev)
        d_zy = torch.empty((2, b, 4), dtype=torch.int64, device=dev)
        d_status = torch.empty(b, dtype=torch.uint8, device=dev)
        d_blobs, d_comm = self._upload(ctx, arr), self._upload(ctx, comm)
        d_z, d_y = d_zy.data_ptr(), d_zy.data_ptr() + b * 32
        with _bad_input_is_value_error():
            ctx.blob_to_fr_device(d_blobs.data_ptr(), log_n, b, True, d_vals.data_ptr(), d_status.data_ptr())
            ctx.blob_challenges_device(d_blobs.data_ptr(), d_comm.data_ptr(), log_n, b, d_z)
            ctx.eval_lagrange_batch(log_n, w, d_vals.data_ptr(), [n] * b, n, d_z, d_out=d_y)
        ctx.synchronize()
        if d_status.cpu().numpy().any():
            return False
        zy = np.ascontiguousarray(d_zy.cpu().numpy().view(np.uint64))
        xy, inf, status = ctx.g1_decompress(np.concatenate([comm, prf]), check_subgroup=True)
        if status.any():
            return False
        zs, ys = _native.limbs_to_ints(zy[0]), _native.limbs_to_ints(zy[1])
        rho = self._blob_batch_rho(n, comm, zs, ys, prf)
        out_xy, out_inf = ctx.verify_points(xy[:b], inf[:b], np.arange(b, dtype=np.uint32), zy[0], zy[1], xy[b:],
                                            inf[b:], rho)
        L_pt, R_pt = self._points(out_xy, out_inf)
        return self._verdict(L_pt, R_pt, rk, pairing, "verify_blob_kzg_proof_batch")

    # ---- EIP-7594 cells as bytes: the spec's calls by name --------------------------------------------
    #      The extended blob is ext[m] = p(w^(brp_N(m))), m < N; cell c is ext[l c .. l c + l), 32 big-endian bytes per
    #      element.  brp_N(l c + t) = brp_l(t) C + brp_C(c), C = N/l: cell c is open_cosets' coset brp_C(c), element t
    #      of a cell that coset's value brp_l(t).  The blob's own domain has the root w^(N/n).
    _CELL_RHO_DOMAIN = b"RCKZGCBATCH__V1_"         # the domain of the cell batch's weight base (hashed here)

    @staticmethod
    def _brp(i, bits):
        """i < 2^bits with its bits reversed"""
        return int(format(i, f"0{bits}b")[::-1], 2) if bits else 0

    def values_to_blob(self, values, n, bit_reversed=True):
        """The inverse of blob_to_values: uint64[b, n, 4] canonical limbs (or b lists of n ints) -> b blobs (bytes) of
        n elements of 32 big-endian bytes, element i the value bitrev(i) when bit_reversed (natural domain order in,
        EIP-4844's order out).  Encoded and permuted on the device (kzg_fr_to_blob).  A value >= r raises ValueError
        naming its row."""
        log_n = self._blob_size(n)
        if isinstance(values, np.ndarray) and values.dtype == np.uint64:
            vals = np.ascontiguousarray(values)
            if vals.size % (4 << log_n):
                raise ValueError(f"values: {vals.size // 4} elements are no rows of {n}")
            vals = vals.reshape(-1, 1 << log_n, 4)
        else:
            rows = [list(v) for v in values]
            if any(len(v) != 1 << log_n for v in rows):
                raise ValueError(f"every row needs {n} values")
            flat = [int(y) for v in rows for y in v]
            if any(y < 0 or y >> 256 for y in flat):
                raise ValueError("a value does not fit 256 bits")
            vals = (_native.ints_to_limbs(flat) if flat else np.zeros((0, 4), dtype=np.uint64)).reshape(-1, 1 << log_n, 4)
        if not vals.shape[0]:
            return []
        with _bad_input_is_value_error():
            out, status = self._context().fr_to_blob(vals, log_n, bit_reversed)
        bad = np.flatnonzero(status)
        if bad.size:
            raise ValueError(f"row {int(bad[0])}: a value is not below the field modulus")
        return [row.tobytes() for row in out]

    def _cell_sizes(self, who, l, n, N, w):
        """Host-side size checks of the cell calls: -> (n, l, N, log_N, w, w_n), w_n = w^(N/n) the blob's root.  N
        defaults to 2n; the ranges are open_cosets' (l <= n/2, n <= N <= 4n)."""
        l = 1 << self._log2_exact(l, "cell size")
        if l < 2:
            raise ValueError(f"{who}: a cell holds at least two elements")
        n = self._domain_size(n)
        if l > n // 2:
            raise ValueError(f"{who}: cell size {l} exceeds n/2 = {n // 2}")
        if l > (1 << self._COSET_MAX_LOG_L):
            raise ValueError(f"{who}: cell size {l} exceeds 2^{self._COSET_MAX_LOG_L}")
        N = 2 * n if N is None else int(N)
        if N < n or N & (N - 1) or N > min(4 * n, 2 * self._DOMAIN_MAX):
            raise ValueError(f"{who}: N = {N} is not a power of two in [n, min(4n, 2^21)]")
        log_N, w = self._domain(N, w)
        return n, l, N, log_N, w, pow(w, N // n, self.curve_order)

    def _cells_key_n(self, who, ck_or_table, n, l):
        """n of a call that takes a key or a coset table: the table's (a given n and l must agree), else the given one"""
        if isinstance(ck_or_table, LagrangeKey):
            raise TypeError(f"{who} needs a monomial key or a coset table, not a LagrangeKey")
        if isinstance(ck_or_table, DomainTable):
            return self._table_n(ck_or_table, n, 1 << self._log2_exact(l, "cell size"))
        if n is None:
            raise ValueError(f"{who}: n is needed with a key (a coset table carries its own)")
        if len(ck_or_table) < int(n):
            raise ValueError(f"commitment key of {len(ck_or_table)} points is shorter than the domain ({n})")
        return n

    def _blobs_to_coeffs(self, ctx, arr, n, w_n):
        """b blobs (uint8[b, 32 n]) -> their coefficients, a device tensor int64[b, n, 4]: the intake and the inverse
        transform over the blob's domain, on the device.  A blob with an element >= r raises ValueError."""
        import torch
        b, log_n = arr.shape[0], n.bit_length() - 1
        dev = f"cuda:{ctx.device}"
        d_coeffs = torch.empty((b, n, 4), dtype=torch.int64, device=dev)
        d_status = torch.empty(b, dtype=torch.uint8, device=dev)
        d_blobs = self._upload(ctx, arr)
        with _bad_input_is_value_error():
            ctx.blob_to_fr_device(d_blobs.data_ptr(), log_n, b, True, d_coeffs.data_ptr(), d_status.data_ptr())
            ctx.ntt_device(d_coeffs.data_ptr(), log_n, _native.int_to_words(w_n), True, b)
        ctx.synchronize()
        bad = np.flatnonzero(d_status.cpu().numpy())
        if bad.size:
            raise self._first_bad_element(arr[int(bad[0])], int(bad[0]))
        return d_coeffs

    def _cells_of_coeffs(self, ctx, d_coeffs, b, n, l, N, w):
        """The C = N/l cells of b resident coefficient vectors (the engine is idle: the caller has synchronised):
        cells[j][c], bytes.  Zero-padded to N, one forward transform, then kzg_fr_to_blob_device with the
        bit-reversed order: row j is cell 0 .. C - 1 of blob j one after the other."""
        import torch
        log_N = N.bit_length() - 1
        dev = f"cuda:{ctx.device}"
        d_ext = torch.zeros((b, N, 4), dtype=torch.int64, device=dev)
        d_ext[:, :n] = d_coeffs
        d_out = torch.empty((b, 32 * N), dtype=torch.uint8, device=dev)
        d_status = torch.empty(b, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(ctx.device)              # the pad ran on torch's stream, the engine has its own
        with _bad_input_is_value_error():
            ctx.ntt_device(d_ext.data_ptr(), log_N, _native.int_to_words(w), False, b)
            ctx.fr_to_blob_device(d_ext.data_ptr(), log_N, b, True, d_out.data_ptr(), d_status.data_ptr())
        ctx.synchronize()
        if d_status.cpu().numpy().any():
            raise RuntimeError("a transform left a value that is not below the field modulus")
        out = d_out.cpu().numpy()
        size = 32 * l
        return [[row[c * size:(c + 1) * size].tobytes() for c in range(N // l)] for row in out]

    def _cell_proofs_of_coeffs(self, ctx, table, d_coeffs, b, n, l, log_N, w):
        """proofs[j][c], compressed: the proof of cell c is open_cosets' proof of coset brp_C(c)"""
        C = (1 << log_N) // l
        xy, inf, _ = ctx.open_cosets(table.table, d_coeffs.data_ptr(), [n] * b, n, log_N, w, device=True, evals=False)
        comp = ctx.g1_compress(xy.reshape(b * C, -1), inf.reshape(-1))
        bits = C.bit_length() - 1
        perm = [self._brp(c, bits) for c in range(C)]
        return [[comp[j * C + i].tobytes() for i in perm] for j in range(b)]

    def compute_cells(self, blobs, n, l, N=None, w=None):
        """compute_cells of EIP-7594 for every blob: cells[j][c], C = N/l cells of 32 l bytes each (N defaults to 2n,
        w to Fq.root_of_unity(N); a blob lives on the domain of w^(N/n)).  Every step stays on the device: intake,
        inverse transform of size n, zero pad, forward transform of size N, kzg_fr_to_blob_device.  A blob with an
        element >= r raises ValueError."""
        n, l, N, _, w, w_n = self._cell_sizes("compute_cells", l, n, N, w)
        arr = self._byte_rows(blobs, 32 * n, "blob")
        if not arr.shape[0]:
            return []
        ctx = self._context()
        d_coeffs = self._blobs_to_coeffs(ctx, arr, n, w_n)
        return self._cells_of_coeffs(ctx, d_coeffs, arr.shape[0], n, l, N, w)

    def compute_cells_and_kzg_proofs(self, ck_or_table, blobs, l, n=None, N=None, w=None):
        """compute_cells_and_kzg_proofs of EIP-7594 for every blob: (cells, proofs), proofs[j][c] the compressed proof
        of cell c.  compute_cells' chain, then kzg_open_cosets_device on the same resident coefficients (its values
        are not requested) and kzg_g1_compress.  ck_or_table: a monomial key (n is then needed) or a coset table."""
        who = "compute_cells_and_kzg_proofs"
        n = self._cells_key_n(who, ck_or_table, n, l)
        n, l, N, log_N, w, w_n = self._cell_sizes(who, l, n, N, w)
        arr = self._byte_rows(blobs, 32 * n, "blob")
        b = arr.shape[0]
        if not b:
            return [], []
        table = self._coset_table_for(ck_or_table, n, l)
        ctx = self._context()
        d_coeffs = self._blobs_to_coeffs(ctx, arr, n, w_n)
        cells = self._cells_of_coeffs(ctx, d_coeffs, b, n, l, N, w)
        return cells, self._cell_proofs_of_coeffs(ctx, table, d_coeffs, b, n, l, log_N, w)

    def _cell_indices(self, cell_indices, C, who):
        idx = [int(i) for i in cell_indices]
        if any(i < 0 or i >= C for i in idx):
            raise ValueError(f"{who}: a cell index is outside [0, {C})")
        return idx

    def recover_cells_and_kzg_proofs(self, ck_or_table, cell_indices, cells, l, n=None, N=None, w=None):
        """recover_cells_and_kzg_proofs of EIP-7594 for a batch: cells[j][k] (32 l bytes) is cell cell_indices[k] of
        blob j, any K >= n/l distinct cells in any order, one index set for the batch -> (cells, proofs), all C cells
        and all C proofs of each blob.  The bytes go through the device intake (log_n = log_l), then
        kzg_recover_cosets_device, kzg_open_cosets_device, and the transform and kzg_fr_to_blob_device of
        compute_cells.  ValueError: an element >= r (naming blob and cell), sizes, an index out of range or repeated,
        fewer than n/l cells, and recover_cosets' for cells that lie on no polynomial of degree < n."""
        who = "recover_cells_and_kzg_proofs"
        n = self._cells_key_n(who, ck_or_table, n, l)
        n, l, N, log_N, w, _ = self._cell_sizes(who, l, n, N, w)
        C, log_l, log_n = N // l, l.bit_length() - 1, n.bit_length() - 1
        idx = self._cell_indices(cell_indices, C, who)
        K = len(idx)
        if len(set(idx)) != K:
            raise ValueError(f"{who}: a cell index is repeated")
        if K * l < n:
            raise ValueError(f"{who}: {K} cells of {l} values cannot determine a polynomial of degree < {n}")
        b = len(cells)
        if b < 1:
            raise ValueError(f"{who} needs at least one blob")
        rows = []
        for j, blob_cells in enumerate(cells):
            if len(blob_cells) != K:
                raise ValueError(f"blob {j} has {len(blob_cells)} cells for {K} cell indices")
            rows.append(self._byte_rows(blob_cells, 32 * l, f"blob {j}: cell"))
        arr = np.ascontiguousarray(np.stack(rows)).reshape(b * K, 32 * l)
        table = self._coset_table_for(ck_or_table, n, l)
        ctx = self._context()
        import torch
        dev = f"cuda:{ctx.device}"
        d_vals = torch.empty((b * K, l, 4), dtype=torch.int64, device=dev)
        d_status = torch.empty(b * K, dtype=torch.uint8, device=dev)
        d_coeffs = torch.empty((b, n, 4), dtype=torch.int64, device=dev)
        d_cells = self._upload(ctx, arr)
        with _bad_input_is_value_error():
            ctx.blob_to_fr_device(d_cells.data_ptr(), log_l, b * K, True, d_vals.data_ptr(), d_status.data_ptr())
        ctx.synchronize()
        bad = np.flatnonzero(d_status.cpu().numpy())
        if bad.size:
            q = int(bad[0])
            raise ValueError(f"blob {q // K}: cell {idx[q % K]} holds an element that is not below the field modulus")
        bits = C.bit_length() - 1
        coset_idx = np.asarray([self._brp(i, bits) for i in idx], dtype=np.uint32)
        with _bad_input_is_value_error():
            _, ok = ctx.recover_cosets(log_n, log_N, log_l, w, coset_idx, d_vals.data_ptr(), b,
                                       d_coeffs=d_coeffs.data_ptr())
        self._first_inconsistent(ok, n)
        out = self._cells_of_coeffs(ctx, d_coeffs, b, n, l, N, w)
        return out, self._cell_proofs_of_coeffs(ctx, table, d_coeffs, b, n, l, log_N, w)

    def _cell_batch_rho(self, n, l, commitments, commitment_indices, cell_indices, cells, proofs):
        """SHA-256("RCKZGCBATCH__V1_" | n | l | number of distinct commitments | K (8 bytes big-endian each) | the
        distinct commitments | per cell: commitment index (8 bytes) | cell index (8 bytes) | the cell's 32 l bytes |
        proof) mod r, on the host: one Merkle-Damgard chain has no parallel form.  Rows of bytes; indices: ints."""
        import hashlib
        h = hashlib.sha256(self._CELL_RHO_DOMAIN + int(n).to_bytes(8, "big") + int(l).to_bytes(8, "big")
                           + len(commitments).to_bytes(8, "big") + len(cells).to_bytes(8, "big"))
        for c in commitments:
            h.update(bytes(c))
        for ci, ki, cell, p in zip(commitment_indices, cell_indices, cells, proofs):
            h.update(int(ci).to_bytes(8, "big") + int(ki).to_bytes(8, "big"))
            h.update(cell)
            h.update(bytes(p))
        return int.from_bytes(h.digest(), "big") % self.curve_order

    def verify_cell_kzg_proof_batch(self, ck, rk_l, commitments, cell_indices, cells, proofs, l, N, w=None,
                                    pairing="device", n=None):
        """verify_cell_kzg_proof_batch of EIP-7594: is cells[k] (32 l bytes) cell cell_indices[k] of the blob of
        commitments[k], with proof proofs[k], for every k?  One compressed commitment per cell, deduplicated here in
        order of first appearance; rk_l = [tau^l] G2 (coset_verification_key); n (the blob's size, part of the
        challenge) defaults to N/2.  Commitments and proofs are decompressed with the subgroup test on the device
        (enqueued before the batch challenge is hashed on the host, awaited after it); the cells go to
        kzg_verify_cosets_bytes as bytes, which folds the claims with the weights rho^(k+1); two pairings as in
        verify_cosets.  False, not an exception: an element >= r, a malformed point, a point off the curve or outside
        the subgroup, a wrong proof.  ValueError: mismatched counts or sizes, an index out of range.  No cells: True."""
        who = "verify_cell_kzg_proof_batch"
        if pairing not in ("device", "host"):
            raise ValueError(f"{who}: pairing must be \"device\" or \"host\", not {pairing!r}")
        self._monomial_key(ck, who)
        l = 1 << self._log2_exact(l, "cell size")
        N = int(N)
        if N < 2 or N & (N - 1) or N > self._VERIFY_MAX_N:
            raise ValueError(f"N = {N} is not a power of two in [2, 2^21]")
        if l > N // 2:
            raise ValueError(f"cell size {l} exceeds N/2 = {N // 2}")
        if l > (1 << self._COSET_MAX_LOG_L):
            raise ValueError(f"cell size {l} exceeds 2^{self._COSET_MAX_LOG_L}")
        n = N // 2 if n is None else int(n)
        if n < l or n > N or n & (n - 1):
            raise ValueError(f"n = {n} is not a power of two in [l, N]")
        log_N, w = self._domain(N, w)
        if len(ck) < l:
            raise ValueError(f"commitment key of {len(ck)} points is shorter than the cell size {l}")
        ctx = self._context()
        G, C = ctx.g1_bytes, N // l
        comm = self._byte_rows(commitments, G, "commitment")
        prf = self._byte_rows(proofs, G, "proof")
        arr = self._byte_rows(cells, 32 * l, "cell")
        idx = self._cell_indices(cell_indices, C, who)
        K = len(idx)
        if comm.shape[0] != K or prf.shape[0] != K or arr.shape[0] != K:
            raise ValueError("commitments, cell_indices, cells and proofs must describe the same number of cells")
        if K > (1 << 21) or K * l > (1 << 24):
            raise ValueError("at most 2^21 cells and 2^24 values per call")
        if K == 0:
            return True
        first, comm_idx = {}, []
        for row in comm:
            comm_idx.append(first.setdefault(row.tobytes(), len(first)))
        distinct = list(first)
        if len(distinct) > (1 << 16):
            raise ValueError("at most 2^16 distinct commitments per call")
        n_comm = len(distinct)
        points = np.concatenate([np.frombuffer(b"".join(distinct), dtype=np.uint8).reshape(n_comm, G), prf])
        import torch
        dev = f"cuda:{ctx.device}"
        P = 2 * ctx.fp_limbs
        d_xy = torch.empty((n_comm + K, P), dtype=torch.int64, device=dev)
        d_inf = torch.empty(n_comm + K, dtype=torch.uint8, device=dev)
        d_status = torch.empty(n_comm + K, dtype=torch.uint8, device=dev)
        d_points = self._upload(ctx, points)
        ctx.g1_decompress_device(d_points.data_ptr(), n_comm + K, True, d_xy.data_ptr(), d_inf.data_ptr(),
                                 d_status.data_ptr())
        rho = self._cell_batch_rho(n, l, distinct, comm_idx, idx, arr, prf)          # the device works meanwhile
        ctx.synchronize()
        if d_status.cpu().numpy().any():
            return False
        xy = np.ascontiguousarray(d_xy.cpu().numpy().view(np.uint64))
        inf = d_inf.cpu().numpy()
        bits = C.bit_length() - 1
        coset_idx = np.asarray([self._brp(i, bits) for i in idx], dtype=np.uint32)
        key = self._key(ck)
        out_xy, out_inf, status = ctx.verify_cosets_bytes(key.srs, log_N, l.bit_length() - 1, w, xy[:n_comm],
                                                          inf[:n_comm], np.asarray(comm_idx, dtype=np.uint32),
                                                          coset_idx, arr, xy[n_comm:], inf[n_comm:], rho,
                                                          bit_reversed=True)
        if status:
            return False
        L_pt, R_pt = self._points(out_xy, out_inf)
        return self._verdict(L_pt, R_pt, rk_l, pairing, who)
