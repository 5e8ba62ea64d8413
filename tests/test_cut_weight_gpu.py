"""The multiply-add of a column cut (csrc/field.h: Field::unpeel) carries its weight 2^(32-L) as an inline constant of
one asm statement -- or, with -DKZG_CUT_WEIGHT_CONST, reads it from a word of constant memory that every translation
unit's code object carries for itself.  A wrong weight (or a word that a code object had not initialised) would make
every BLS12-381 base-field product of that unit wrong.  So one entry point of each unit that instantiates such
products is run at a small size against FROZEN values (tests/golden/cut_weight_vectors.json, written by the
pure-Python oracle: make_cut_weight_golden.py):

  msm.hip      a commitment of 64 coefficients (key generation and window tables, accumulate, the reduce stage)
  domain.hip   every FK20 proof on the domains of 2 and 8 points (table construction, the G1 transforms and the
               Hadamard stage)

lagrange.hip and verify.hip instantiate them too; tests/test_lagrange_gpu.py and tests/test_verify_gpu.py run those
on BLS12-381 against the oracle."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "cut_weight_vectors.json")


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def kzg(gold):
    from kzg_snark_amd.kzg import KZG
    return KZG(gold["curve"])


def pt_of(entry):
    return (1, 1, 0) if entry is None else (int(entry[0], 16), int(entry[1], 16), 1)


def test_commit_of_64_points(gold, kzg):
    v = gold["commit"]
    coeffs = [int(c, 16) for c in v["coeffs"]]
    ck, _ = kzg.setup(len(coeffs) - 1, tau=int(gold["tau"], 16))
    assert kzg.commit(ck, [coeffs]) == [pt_of(v["commitment"])]


def test_every_proof_on_a_small_domain(gold, kzg, native):
    ctx = kzg._context()
    L = ctx.fp_limbs
    for v in gold["open_domain"]:
        log_n, n = v["log_n"], 1 << v["log_n"]
        coeffs = [int(c, 16) for c in v["coeffs"]]
        ck, _ = kzg.setup(n - 1, tau=int(gold["tau"], 16))
        table = ctx.domain_table(ck.srs, log_n)
        arr = native.ints_to_limbs(coeffs).reshape(1, n, 4)
        xy, inf, _ = ctx.open_domain(table, np.ascontiguousarray(arr), [n], n, int(v["w"], 16), evals=False)
        ints = native.limbs_to_ints(np.ascontiguousarray(xy).reshape(-1, L))
        got = [(1, 1, 0) if inf[0, i] else (ints[2 * i], ints[2 * i + 1], 1) for i in range(n)]
        assert got == [pt_of(p) for p in v["proofs"]], log_n
        table.close()
