"""EIP-7594 cells as bytes on the CPU: the restatement (tests/cells_restated.py) against the
conventions, the output element of csrc/blob.h -- the text blob_output_kernel compiles -- built for the host
(tests/shim/cells_shim.cpp) against int.to_bytes, the new symbols of the library, and the argument checks of the
facade that need no device.  The shim runs plain and with -DKZG_AUDIT, and once as a program of its own under the
address and undefined-behaviour sanitizers."""
import ctypes
import hashlib
import os
import random
import subprocess

import pytest

import cells_restated as CR

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_DIR = os.path.join(HERE, "shim")
SRC = os.path.join(SHIM_DIR, "cells_shim.cpp")
CURVE_IDS = {"bn254": 0, "bls12_381": 1}
CURVES = ["bls12_381", "bn254"]
U64x4 = ctypes.c_uint64 * 4
DISTINCT = int.from_bytes(bytes(range(1, 33)), "big")          # 0x0102..20: every byte differs, below both moduli


# ---- the restatement --------------------------------------------------------------------------------------------

def test_restated_brp_and_the_domain_constant():
    assert [CR.brp(i, 3) for i in range(8)] == [0, 4, 2, 6, 1, 5, 3, 7]
    assert CR.brp(0, 0) == 0 and CR.brp(1, 1) == 1 and CR.brp(1, 13) == 1 << 12
    assert all(CR.brp(CR.brp(i, 7), 7) == i for i in range(128))
    assert CR.CELL_RHO_DOMAIN == b"RCKZGCBATCH__V1_" and len(CR.CELL_RHO_DOMAIN) == 16
    assert DISTINCT < min(CR.R.values())


@pytest.mark.parametrize("N,l", [(16, 2), (128, 4)])
def test_index_identity_for_every_cell_and_element(N, l):
    """brp_N(l c + t) = brp_l(t) C + brp_C(c): cell c is coset brp_C(c), element t its value brp_l(t)"""
    C = N // l
    log_N, log_l, log_C = CR.log2(N), CR.log2(l), CR.log2(C)
    seen = set()
    for c in range(C):
        for t in range(l):
            e = CR.brp(l * c + t, log_N)
            assert e == CR.brp(t, log_l) * C + CR.brp(c, log_C)
            assert e == CR.value_of_element(t, l) * C + CR.coset_of_cell(c, C)      # the exponent i + k C of coset i
            seen.add(e)
    assert seen == set(range(N))


def test_restated_cells_from_a_polynomial_evaluated_by_hand():
    """p over the domain of N = 8 with l = 2: the cells are the extended blob cut in pieces"""
    curve = "bn254"
    r, N, l = CR.R[curve], 8, 2
    C = N // l
    w = pow(5, (r - 1) // N, r)
    assert pow(w, N // 2, r) == r - 1
    p = [3, 1, 4, 1]
    ev = [sum(a * pow(w, t * k, r) for k, a in enumerate(p)) % r for t in range(N)]
    ext = [ev[CR.brp(m, 3)] for m in range(N)]
    values = [[ev[i + k * C] for k in range(l)] for i in range(C)]               # the library's cosets
    cells = CR.cells_of_coset_values(values, l)
    assert b"".join(cells) == b"".join(v.to_bytes(32, "big") for v in ext)
    assert b"".join(cells) == CR.fr_to_blob([ev], curve)[0][0]
    for c in range(C):
        assert CR.coset_values_of_cell(cells[c], l) == values[CR.coset_of_cell(c, C)]


def test_restated_fr_to_blob_marks_a_row_and_writes_zeros():
    r = CR.R["bn254"]
    rows = [[5, r - 1, 7, 9], [5, r, 7, 9]]
    out, status = CR.fr_to_blob(rows, "bn254", bit_reversed=True)
    assert status == [0, 1]
    assert out[0] == b"".join(v.to_bytes(32, "big") for v in [5, 7, r - 1, 9])
    assert out[1] == b"".join(v.to_bytes(32, "big") for v in [5, 7, 0, 9])
    assert CR.fr_to_blob(rows[:1], "bn254", bit_reversed=False)[0][0][32:64] == (r - 1).to_bytes(32, "big")


@pytest.mark.parametrize("curve", CURVES)
def test_rho_against_a_byte_string_concatenated_by_hand(curve):
    from kzg_snark_amd.kzg import KZG
    kzg = KZG(curve)
    G, r, n, l = CR.G_BYTES[curve], CR.R[curve], 4096, 64
    rng = random.Random(G)
    comms = [bytes(rng.randrange(256) for _ in range(G)) for _ in range(2)]
    per_cell = [comms[1], comms[0], comms[1]]
    distinct, comm_idx = CR.dedup(per_cell)
    assert distinct == [comms[1], comms[0]] and comm_idx == [0, 1, 0]            # order of first appearance
    cell_idx = [127, 0, 5]
    cells = [bytes(rng.randrange(256) for _ in range(32 * l)) for _ in range(3)]
    proofs = [bytes(rng.randrange(256) for _ in range(G)) for _ in range(3)]
    data = b"RCKZGCBATCH__V1_" + b"\x00" * 6 + b"\x10\x00" + b"\x00" * 7 + b"\x40" + b"\x00" * 7 + b"\x02" \
        + b"\x00" * 7 + b"\x03" + comms[1] + comms[0]
    for k in range(3):
        data += b"\x00" * 7 + bytes([comm_idx[k]]) + b"\x00" * 7 + bytes([cell_idx[k]]) + cells[k] + proofs[k]
    assert len(data) == 48 + 2 * G + 3 * (16 + 32 * l + G)
    assert CR.rho_preimage(n, l, distinct, comm_idx, cell_idx, cells, proofs) == data
    want = int.from_bytes(hashlib.sha256(data).digest(), "big") % r
    assert CR.rho(n, l, distinct, comm_idx, cell_idx, cells, proofs, curve) == want
    assert kzg._cell_batch_rho(n, l, distinct, comm_idx, cell_idx, cells, proofs) == want
    assert [kzg._brp(i, 7) for i in range(128)] == [CR.brp(i, 7) for i in range(128)] and kzg._brp(0, 0) == 0


# ---- blob.h's output element on the host ---------------------------------------------------------------------------

def build_shim(audit):
    kind = "audit" if audit else "plain"
    so = os.path.join(SHIM_DIR, f"libcells_shim_{kind}.so")
    subprocess.run(["g++", "-O0" if audit else "-O1", "-std=c++17", *(["-DKZG_AUDIT"] if audit else []), "-shared",
                    "-fPIC", SRC, "-o", so], check=True)
    return ctypes.CDLL(so)


@pytest.fixture(scope="module", params=["plain", "audit"])
def shim(request):
    lib = build_shim(request.param == "audit")
    lib.audited = request.param == "audit"
    if lib.audited:
        lib.cs_audit_count.restype = ctypes.c_ulonglong
    return lib


def limbs_of(v):
    return U64x4(*[(v >> (64 * j)) & 0xffffffffffffffff for j in range(4)])


@pytest.mark.parametrize("curve", CURVES)
def test_output_element_against_int_to_bytes(shim, curve):
    r, cid = CR.R[curve], CURVE_IDS[curve]
    rng = random.Random(5)
    for v in [0, 1, r - 1, r, (1 << 256) - 1, DISTINCT, r + 1, 1 << 255, r - (1 << 224)] + \
             [rng.randrange(1 << 256) for _ in range(16)]:
        out = (ctypes.c_uint8 * 32)()
        ok = shim.cs_output_element(cid, limbs_of(v), out)
        assert ok == (1 if v < r else 0), hex(v)
        assert bytes(out) == (v if v < r else 0).to_bytes(32, "big"), hex(v)
    if shim.audited:
        assert shim.cs_audit_count() == 0


@pytest.mark.parametrize("curve", CURVES)
def test_output_element_undoes_the_intake_element(shim, curve):
    r, cid = CR.R[curve], CURVE_IDS[curve]
    rng = random.Random(6)
    for v in [0, 1, r - 1, DISTINCT] + [rng.randrange(r) for _ in range(16)]:
        out = (ctypes.c_uint8 * 32)()
        assert shim.cs_round_trip(cid, v.to_bytes(32, "big"), out) == 1
        assert bytes(out) == v.to_bytes(32, "big")
    out = (ctypes.c_uint8 * 32)()
    assert shim.cs_round_trip(cid, r.to_bytes(32, "big"), out) == 0 and bytes(out) == bytes(32)


def test_shim_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """cells_shim.cpp with its own main(): the chosen values in buffers of their exact size, on both curves; built with
    -DKZG_AUDIT and -fsanitize=address,undefined (no recovery, static runtimes) and run as a program of its own."""
    exe = str(tmp_path / "cells_shim_san")
    subprocess.run(["g++", "-O0", "-g", "-std=c++17", "-DKZG_AUDIT", "-DCELLS_SHIM_MAIN",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    SRC, "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    assert "no violations" in res.stdout


# ---- the library and the facade, without a device --------------------------------------------------------------------

def test_new_symbols_resolve_and_the_abi_version_stays():
    from kzg_snark_amd import _native, build
    build.build(verbose=False)
    L = _native.lib()
    for name in ("kzg_fr_to_blob", "kzg_fr_to_blob_device", "kzg_verify_cosets_bytes"):
        assert name in _native.SIGNATURES and getattr(L, name) is not None
    assert _native.MISSING == []
    assert L.kzg_abi_version() == 1


def test_facade_refuses_sizes_before_any_device_work():
    from kzg_snark_amd.kzg import KZG
    kzg = KZG("bls12_381")
    blob = b"\x00" * (32 * 8)
    with pytest.raises(ValueError):
        kzg.compute_cells([blob], 8, 3)                                 # l is not a power of two
    with pytest.raises(ValueError):
        kzg.compute_cells([blob], 8, 8)                                 # l above n/2
    with pytest.raises(ValueError):
        kzg.compute_cells([blob], 8, 2, N=4)                            # N below n
    with pytest.raises(ValueError):
        kzg.compute_cells([blob], 8, 2, N=64)                           # N above 4n
    with pytest.raises(ValueError):
        kzg.compute_cells([blob[:-1]], 8, 2)                            # a blob of another size
    with pytest.raises(ValueError):
        kzg.compute_cells([blob], 8, 2, w=3)                            # not a primitive N-th root
    assert kzg.compute_cells([], 8, 2) == []
    with pytest.raises(ValueError):
        kzg.values_to_blob([[1, 2, 3]], 4)                              # a short row
    with pytest.raises(ValueError):
        kzg.values_to_blob([[1, 2, 3, 1 << 256]], 4)                    # no 256-bit number
    assert kzg.values_to_blob([], 4) == []
