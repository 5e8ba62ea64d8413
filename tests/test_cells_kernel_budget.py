"""blob_output_kernel of csrc/blob.hip is the intake kernel run backwards -- two 16-byte loads, the
comparison with r, eight byte swaps, two 16-byte stores -- and keeps the intake kernel's budget for the same 16 words
in flight: at most 64 VGPRs, no scratch, no LDS.  Read from the built code object (no GPU needed), as
tests/test_blob_kernel_budget.py does."""
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


def test_output_kernel_is_small(kernels):
    rows = [k for k in kernels if "blob_output_kernel" in k[0]]
    assert len(rows) == 2, rows                                   # one per scalar field
    for _, vgpr, lds, scratch in rows:
        assert vgpr <= 64 and lds == 0 and scratch == 0           # 16 words in flight: eight waves per SIMD
