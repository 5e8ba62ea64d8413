"""The kernels of csrc/g2_lincomb.hip stay in registers: a lane holds the ladder of g_mul.h and, after
it, the full addition of the wave sum, keeps its table of multiples in global memory and must not touch scratch memory;
one wave per workgroup with the whole register file.  The VGPR bounds and the LDS sizes are the figures of DESIGN 4.17's
kernel table.  Read from the built code object (no GPU needed), as tests/test_g_mul_kernel_budget.py does."""
import os
import sys

import pytest

from restated import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "kzg_snark_amd", "lib", "libkzg_mi355x.so")
# kernel -> {curve: (VGPRs, LDS bytes)} as DESIGN.md 4.17 states them, and the workgroup size
BUDGET = {"g2_lincomb_kernel": ({"BN254": (499, 6912), "BLS12-381": (389, 9984)}, 64),
          "g2_lincomb_fold_kernel": ({"BN254": (226, 6912), "BLS12-381": (365, 9984)}, 64)}
# the rows of DESIGN.md 4.16 that this unit must leave alone
G2_MUL_EACH = {"BN254": 506, "BLS12-381": 371}


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
    section = text[text.index("### 4.17"):]
    for kernel, (per_curve, wg) in BUDGET.items():
        for curve, (vgpr, lds) in per_curve.items():
            assert f"| `{kernel}` | {curve} | {vgpr} | {lds} | {wg} |" in section, (kernel, curve)


def test_the_lds_is_half_a_wave_of_jacobian_points():
    # 6 N limbs of 4 bytes for 32 parked lanes; an Fp element is N = 9 (BN254) or 13 (BLS12-381) limbs
    for per_curve, _ in BUDGET.values():
        assert per_curve["BN254"][1] == 6 * 9 * 4 * 32 and per_curve["BLS12-381"][1] == 6 * 13 * 4 * 32


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_once_per_curve_no_scratch_and_within_the_stated_registers(kernels, kernel):
    out, listing = kernels
    rows = sorted((lds, vgpr, agpr, scratch) for name, vgpr, agpr, _, lds, scratch in listing if name == kernel)
    assert len(rows) == 2, rows                                   # one per curve: the LDS size tells them apart
    per_curve, wg = BUDGET[kernel]
    for (lds, vgpr, agpr, scratch), (budget, want_lds) in zip(rows, sorted(per_curve.values(), key=lambda v: v[1])):
        assert scratch == 0
        assert lds == want_lds
        assert vgpr <= budget and vgpr <= 512
    lines = [ln for ln in out.splitlines() if ln.startswith(kernel + " ")]
    assert len(lines) == 2 and all(ln.split()[-2:] == ["wg", str(wg)] for ln in lines)
    from kzg_snark_amd import _native
    assert (_native.Context.G2_LINCOMB_LANES, _native.Context.G2_LINCOMB_FOLD_LANES) == (64, 64)
    assert _native.Context.G2_LINCOMB_LAUNCH_LANES == 1024 * 64


def test_g2_mul_each_kernel_keeps_its_rows(kernels):
    out, listing = kernels
    rows = sorted((vgpr, lds, scratch) for name, vgpr, _, _, lds, scratch in listing if name == "g2_mul_each_kernel")
    assert rows == sorted((v, 0, 0) for v in G2_MUL_EACH.values())
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    for curve, vgpr in G2_MUL_EACH.items():
        assert f"| `g2_mul_each_kernel` | {curve} | {vgpr} |" in text
