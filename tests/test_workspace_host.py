"""csrc/devmem.h and csrc/ver_layout.h without a GPU (tests/shim/workspace_shim.cpp, a program of its own over a counting
hipMalloc / hipFree): the scoped owners free on every exit, the carve measures and assigns alike, the counting sort
groups as the bulk verifications expect -- and the two workspaces kzg_prof_read reports on come out byte for byte as
the running sum of 256-byte-rounded segments that verify.hip and verify_points.hip used to write out by hand, which
is restated here.  The sizes that come from device headers (point and record bytes, the power table, the thread
counts) are arguments of the layouts: the test passes the same numbers to the shim and to the restatement."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "shim", "workspace_shim.cpp")
ROCM_INCLUDES = [os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "/opt/rocm/include"]
POW_TAB = 3073                                                        # an argument of the layouts: any number would do

pytestmark = pytest.mark.skipif(
    shutil.which("g++") is None or not any(os.path.exists(os.path.join(d, "hip", "hip_runtime_api.h")) for d in ROCM_INCLUDES),
    reason="needs g++ and the ROCm headers")


def compile_shim(exe, *extra):
    inc = next(d for d in ROCM_INCLUDES if os.path.exists(os.path.join(d, "hip", "hip_runtime_api.h")))
    subprocess.run(["g++", "-O0", "-g", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__",
                    "-I" + inc, *extra, SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return compile_shim(str(tmp_path_factory.mktemp("ws") / "workspace_shim"))


def test_owners_carve_and_counting_sort(shim):
    """three temporaries with a failure injected at allocation 0, 1, 2 and none: nothing stays alive; release() hands
    over exactly one; a zero-byte or absent take_if is null and moves nothing; both passes agree on the total;
    comm_idx = [2, 0, 2, 1, 0] sorts to off = [0, 2, 3, 5], perm = [1, 4, 3, 0, 2]; an index equal to n_comm is
    reported at its position (the assertions are in the shim's check_* functions)"""
    res = subprocess.run([shim], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-2000:])
    assert "no violations" in res.stdout


def test_the_same_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the program itself carries the sanitizers' static runtimes; the leak checker confirms the counts"""
    exe = compile_shim(str(tmp_path / "workspace_shim_san"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                       "-static-libasan", "-static-libubsan")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    assert "no violations" in res.stdout


def running_sum(segments):
    """what the drivers wrote by hand: o = total; total += ceil(bytes / 256) * 256, segment after segment; an optional
    array that is absent took a zero-byte segment and a null pointer"""
    offsets, total = {}, 0
    for name, size in segments:
        offsets[name] = -1 if size is None else total
        total += -(-(size or 0) // 256) * 256
    return offsets, total


def shim_layout(shim, *args):
    res = subprocess.run([shim, *map(str, args)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-2000:])
    rows = dict(line.split() for line in res.stdout.splitlines())
    return {k: int(v) for k, v in rows.items() if k != "total"}, int(rows["total"])


# (K, n_comm, log_l, proof flags?, commitment flags?)
CASES = [(1, 1, 0, False, False), (5, 3, 3, True, False), (257, 2, 12, True, True)]
SIZES = [(64, 64), (96, 104)]                                         # (bytes of an affine point, of a key record)


@pytest.mark.parametrize("pt,rb", SIZES)
@pytest.mark.parametrize("K,n_comm,log_l,pf,cf", CASES)
def test_verify_cosets_workspace(shim, K, n_comm, log_l, pf, cf, pt, rb):
    l = 1 << log_l
    M = K * l
    sum_threads = max(l, 1 << 15)
    nsp = 1 if n_comm >= 64 else 64
    want = running_sum([
        ("pxy", K * pt), ("pinf", K if pf else None), ("cxy", n_comm * pt), ("cinf", n_comm if cf else None),
        ("recs", K * rb), ("vals", M * 32), ("r", K * 32), ("s", K * 32), ("slice", K * 32), ("cidx", K * 4),
        ("perm", K * 4), ("off", (n_comm + 1) * 4), ("wtab", POW_TAB * 32), ("rtab", POW_TAB * 32),
        ("part", sum_threads * 32), ("cpart", n_comm * nsp * 32), ("T", l * 32), ("coef", n_comm * 32), ("bad", 4)])
    got = shim_layout(shim, "verify", K, n_comm, l, int(pf), int(cf), pt, rb, POW_TAB, sum_threads, nsp)
    assert got == want
    assert all(o % 256 == 0 for o in got[0].values() if o >= 0) and got[1] % 256 == 0


@pytest.mark.parametrize("pt,rb", SIZES)
@pytest.mark.parametrize("K,n_comm,log_l,pf,cf", CASES)
def test_verify_points_workspace(shim, K, n_comm, log_l, pf, cf, pt, rb):
    tb, launch_max, weight_threads, table, xyzz = 256, 512, 1 << 14, 8, 2 * pt
    n_short = n_comm + 1
    nsp = 1 if n_comm >= 64 else 64
    nb, nc = -(-K // tb), -(-n_short // tb)
    blocks = 2 * nb + nc
    launches = -(-blocks // launch_max)
    launch_blocks = -(-blocks // launches)
    tab_bytes = table * xyzz * launch_blocks * tb
    want = running_sum([
        ("pxy", K * pt), ("pinf", K if pf else None), ("cxy", n_short * pt), ("cinf", n_short if cf else None),
        ("precs", K * rb), ("crecs", n_short * rb), ("z", K * 32), ("y", K * 32), ("r", K * 32), ("s", K * 32),
        ("perm", K * 4), ("off", (n_comm + 1) * 4), ("rtab", POW_TAB * 32), ("ypart", weight_threads * 32),
        ("cpart", n_comm * nsp * 32), ("coef", n_short * 32), ("partial", blocks * xyzz), ("out", 3 * xyzz), ("bad", 4),
        ("tab", tab_bytes)])
    got = shim_layout(shim, "points", K, n_comm, int(pf), int(cf), pt, rb, POW_TAB, weight_threads, nsp, blocks, xyzz,
                      tab_bytes)
    assert got == want
