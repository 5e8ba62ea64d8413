"""The pairing kernel of csrc/pairing.hip calls no function and spills nothing: one instance per curve
behind both entry points (kzg_pairing_check and kzg_pairing_product launch the same kernel, with and without a value
buffer), no scratch memory -- a gfx950 kernel that calls functions keeps callee-saved registers there, which is why
fp_tower.h runs one inlined interpreter -- and a static LDS block (the slots the lanes of a wave exchange through) within
the 64 KiB a workgroup may declare.  Read from the built code object (no GPU needed), as
tests/test_blob_kernel_budget.py does; the VGPR and LDS figures themselves are in DESIGN.md's table."""
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


def test_one_pairing_kernel_per_curve_without_scratch(kernels):
    rows = [k for k in kernels if "pairing_kernel" in k[0]]
    assert len(rows) == 2, rows                                   # one per curve
    assert len({lds for _, _, lds, _ in rows}) == 2                # 9-limb and 13-limb slots
    for _, vgpr, lds, scratch in rows:
        assert scratch == 0
        assert 0 < lds <= 65536
