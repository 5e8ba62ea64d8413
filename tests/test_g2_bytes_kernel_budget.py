"""The kernels of csrc/g2_bytes.hip stay in registers: a lane holds a G2 point's accumulator and one
operand as Fp2 values, twice what a G1 lane holds, and G2 counts are small, so the kernels run one wave per workgroup
with the whole register file and must not touch scratch memory.  The VGPR bounds are the figures of DESIGN 4.14's kernel
table.  Read from the built code object (no GPU needed), as tests/test_blob_kernel_budget.py does."""
import os
import sys

import pytest

from restated import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "kzg_snark_amd", "lib", "libkzg_mi355x.so")
# kernel -> the VGPR counts DESIGN.md 4.14 states, (bn254, bls12_381): the smaller and the larger of the two instances
BUDGET = {"g2_decompress_kernel": (118, 173), "g2_subgroup_kernel": (269, 285), "g2_compress_kernel": (110, 168)}


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LIB):
        sys.path.insert(0, ROOT)
        from kzg_snark_amd import build
        build.build(verbose=False)
    out, listing = kernel_resources(LIB)
    assert listing, out
    return listing


def test_design_states_the_budget():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("### 4.14"):]
    for kernel, (bn, bls) in BUDGET.items():
        for curve, vgpr in (("BN254", bn), ("BLS12-381", bls)):
            assert f"| `{kernel}` | {curve} | {vgpr} |" in section, (kernel, curve)


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_once_per_curve_no_scratch_and_within_the_stated_registers(kernels, kernel):
    rows = sorted((vgpr, agpr, lds, scratch) for name, vgpr, agpr, _, lds, scratch in kernels if name == kernel)
    assert len(rows) == 2, rows                                   # one per curve
    for (vgpr, agpr, lds, scratch), budget in zip(rows, BUDGET[kernel]):
        assert scratch == 0 and lds == 0
        assert vgpr <= budget and vgpr <= 512
