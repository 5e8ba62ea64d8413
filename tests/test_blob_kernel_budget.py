"""The two kernels of csrc/blob.hip stay in registers: one lane of blob_challenge_kernel walks a whole
blob, 2,050 compressions at n = 4096, so a message window or the state spilled to scratch, or staged through LDS,
would be paid 2,050 times.  Budget of the challenge kernel: eight state words, 16 + 16 message words (the block being
compressed and the one being loaded) and temporaries -- at most 96 VGPRs, no scratch, no LDS.  Read from the built
code object (no GPU needed), as tests/test_kernel_budget.py does."""
import os
import sys

import pytest

from restated import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "kzg_snark_amd", "lib", "libkzg_mi355x.so")


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LIB):
        sys.path.insert(0, ROOT)
        from kzg_snark_amd import build
        build.build(verbose=False)
    out, listing = kernel_resources(LIB)
    rows = [(name, vgpr, lds, scratch) for name, vgpr, _, _, lds, scratch in listing]
    assert rows, out
    return rows


def test_challenge_kernel_is_register_only(kernels):
    rows = [k for k in kernels if "blob_challenge_kernel" in k[0]]
    assert len(rows) == 2, rows                                   # one per curve
    for _, vgpr, lds, scratch in rows:
        assert vgpr <= 96 and lds == 0 and scratch == 0


def test_intake_kernel_is_small(kernels):
    rows = [k for k in kernels if "blob_intake_kernel" in k[0]]
    assert len(rows) == 2, rows                                   # one per scalar field
    for _, vgpr, lds, scratch in rows:
        assert vgpr <= 64 and lds == 0 and scratch == 0           # 16 words in flight: eight waves per SIMD
