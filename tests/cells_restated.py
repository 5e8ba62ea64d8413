"""EIP-7594 cells as bytes, restated from the conventions of DESIGN.md 4.13 with hashlib and Python integers: the
reference of tests/test_cells_host.py and tests/test_cells_gpu.py.  Nothing here imports the package under test.

The domain is {w^t, t < N}; cells hold l elements and there are C = N/l of them.  The extended blob is
ext[m] = p(w^(brp_N(m))), cell c is ext[l c .. l c + l), every element 32 big-endian bytes.  In the library's numbering
coset i is {w^(i + k C), k < l} and value k of it is p(w^(i + k C))."""
import hashlib

from blob_restated import R, G_BYTES  # noqa: F401  (the moduli and point sizes are stated once)

CELL_RHO_DOMAIN = b"RCKZGCBATCH__V1_"          # RANDOM_CHALLENGE_KZG_CELL_BATCH_DOMAIN


def brp(i, bits):
    """i < 2^bits with its bits reversed"""
    out = 0
    for _ in range(bits):
        out, i = (out << 1) | (i & 1), i >> 1
    return out


def log2(v):
    assert v >= 1 and v & (v - 1) == 0
    return v.bit_length() - 1


def coset_of_cell(c, C):
    """cell c is the library's coset brp_C(c)"""
    return brp(c, log2(C))


def value_of_element(t, l):
    """element t of a cell is the library's value brp_l(t) of that coset"""
    return brp(t, log2(l))


def be32(v):
    return int(v).to_bytes(32, "big")


def fr_to_blob(rows, curve, bit_reversed=True):
    """rows of n ints -> ([bytes of 32 n], [status]): element i is value brp(i) when bit_reversed; a value >= r is
    written as zeros and sets the row's status"""
    r = R[curve]
    out, status = [], []
    for row in rows:
        bits = log2(len(row))
        picked = [row[brp(i, bits) if bit_reversed else i] for i in range(len(row))]
        status.append(1 if any(v >= r for v in picked) else 0)
        out.append(b"".join(be32(v if v < r else 0) for v in picked))
    return out, status


def cells_of_coset_values(values, l):
    """values[i][k] = p(w^(i + k C)), i < C (what open_cosets_each(with_values=True) returns for one polynomial) ->
    the C cells as bytes"""
    C = len(values)
    return [b"".join(be32(values[coset_of_cell(c, C)][value_of_element(t, l)]) for t in range(l)) for c in range(C)]


def coset_values_of_cell(cell, l):
    """the inverse for one cell: its l values in the library's order (value k at position k)"""
    vals = [0] * l
    for t in range(l):
        vals[value_of_element(t, l)] = int.from_bytes(cell[32 * t:32 * t + 32], "big")
    return vals


def rho_preimage(n, l, commitments, commitment_indices, cell_indices, cells, proofs):
    """domain | n | l | number of distinct commitments | K (8 bytes big-endian each) | the distinct commitments |
    per cell: commitment index (8 B) | cell index (8 B) | the cell's 32 l bytes | proof"""
    K = len(cells)
    assert len(commitment_indices) == len(cell_indices) == len(proofs) == K
    data = CELL_RHO_DOMAIN + n.to_bytes(8, "big") + l.to_bytes(8, "big") + len(commitments).to_bytes(8, "big") \
        + K.to_bytes(8, "big")
    data += b"".join(bytes(c) for c in commitments)
    for ci, ki, cell, p in zip(commitment_indices, cell_indices, cells, proofs):
        assert len(cell) == 32 * l
        data += int(ci).to_bytes(8, "big") + int(ki).to_bytes(8, "big") + bytes(cell) + bytes(p)
    return data


def rho(n, l, commitments, commitment_indices, cell_indices, cells, proofs, curve):
    data = rho_preimage(n, l, commitments, commitment_indices, cell_indices, cells, proofs)
    return int.from_bytes(hashlib.sha256(data).digest(), "big") % R[curve]


def dedup(rows):
    """(distinct rows in order of first appearance, index of every row among them)"""
    first, idx = {}, []
    for row in rows:
        idx.append(first.setdefault(bytes(row), len(first)))
    return list(first), idx
