"""The kernels of csrc/g_mul.hip stay in registers: a lane holds the accumulator, one table entry and
the temporaries of one addition, keeps its table of multiples in global memory and must not touch scratch memory -- the
G2 kernel runs one wave per workgroup with the whole register file for that.  The VGPR bounds are the figures of
DESIGN 4.16's kernel table.  Read from the built code object (no GPU needed), as tests/test_g2_bytes_kernel_budget.py
does."""
import os
import sys

import pytest

from restated import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "kzg_snark_amd", "lib", "libkzg_mi355x.so")
# kernel -> the VGPR counts DESIGN.md 4.16 states per curve, and the workgroup size
BUDGET = {"g1_mul_each_kernel": ({"BN254": 142, "BLS12-381": 198}, 256),
          "g2_mul_each_kernel": ({"BN254": 506, "BLS12-381": 371}, 64)}


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LIB):
        sys.path.insert(0, ROOT)
        from kzg_snark_amd import build
        build.build(verbose=False)
    out, listing = kernel_resources(LIB)
    assert listing, out
    return out, listing


def test_design_states_the_budget():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("### 4.16"):]
    for kernel, (per_curve, _) in BUDGET.items():
        for curve, vgpr in per_curve.items():
            assert f"| `{kernel}` | {curve} | {vgpr} |" in section, (kernel, curve)


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_once_per_curve_no_scratch_and_within_the_stated_registers(kernels, kernel):
    out, listing = kernels
    rows = sorted((vgpr, agpr, lds, scratch) for name, vgpr, agpr, _, lds, scratch in listing if name == kernel)
    assert len(rows) == 2, rows                                   # one per curve
    per_curve, wg = BUDGET[kernel]
    for (vgpr, agpr, lds, scratch), budget in zip(rows, sorted(per_curve.values())):
        assert scratch == 0 and lds == 0
        assert vgpr <= budget and vgpr <= 512
    lines = [ln for ln in out.splitlines() if ln.startswith(kernel + " ")]
    assert len(lines) == 2 and all(ln.split()[-2:] == ["wg", str(wg)] for ln in lines)
    # the workgroup sizes the Python layer states are the kernels'
    from kzg_snark_amd import _native
    assert (_native.Context.G1_MUL_LANES, _native.Context.G2_MUL_LANES) == (256, 64)
    assert (_native.Context.G1_MUL_LAUNCH_LANES, _native.Context.G2_MUL_LAUNCH_LANES) == (131072, 16384)
