"""bench.py's plain run and --dump-outputs DIR.

CPU: arguments the headline loop cannot honour are refused before anything starts.
GPU: at 2^12 (B = 4) the dumped sample is every coefficient of the last step, so the dumped commitments can be
checked against the trapdoor identity commit(ck, p) = p(tau) G1 on the host; two runs with the same arguments
dump the same arrays, and the plain line carries the headline keys."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
TAU = 0x6b7a675f736e61726b7a675f736e6172          # bench.py's TAU: the key is [tau^i] G1
NAMES = ["coefficients_sample.npy", "coefficients_sample_index.npy", "commitments_infinity.npy",
         "commitments_xy.npy"]


def run(args, timeout=600):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    return subprocess.run([sys.executable, BENCH, *args], capture_output=True, text=True, timeout=timeout, env=e)


@pytest.mark.parametrize("args", [["--steps", "0"], ["--warmup", "-1"], ["--mode", "range", "--dump-outputs", "x"]])
def test_arguments_the_headline_loop_cannot_honour_are_refused(args):
    p = run(args)
    assert p.returncode == 2 and "error" in p.stderr
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]


def words_to_ints(words):
    """float64 [..., k] little-endian 32-bit words -> Python ints."""
    w = words.astype(np.uint64)
    return [sum(int(v) << (32 * j) for j, v in enumerate(row)) for row in w.reshape(-1, w.shape[-1])]


@pytest.mark.gpu
def test_dump_outputs_are_the_last_steps_commitments(tmp_path):
    from oracle import py_oracle as O
    log_n, B = 12, 4
    lines = {}
    for tag in ("a", "b"):
        p = run(["--gpus", "1", "--steps", "3", "--warmup", "2", "--log-n", str(log_n), "--batch", str(B),
                 "--dump-outputs", str(tmp_path / tag)])
        assert p.returncode == 0, p.stderr[-4000:]
        js = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert len(js) == 1, p.stdout
        lines[tag] = json.loads(js[0])
    out = lines["a"]
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in out, key
    assert out["steps"] == 3 and out["warmup"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0
    assert "verified" not in out and "open" not in out and "cpu_baseline" not in out      # --full only

    assert sorted(os.listdir(tmp_path / "a")) == NAMES
    got = {name: np.load(tmp_path / "a" / name) for name in NAMES}
    for name in NAMES:
        assert got[name].dtype == np.float64, name
        assert np.array_equal(got[name], np.load(tmp_path / "b" / name)), name

    n = 1 << log_n
    cv = O.curve("bls12_381")
    assert np.array_equal(got["coefficients_sample_index.npy"], np.arange(B * n))
    coeffs = words_to_ints(got["coefficients_sample.npy"])
    assert all(c < cv.r for c in coeffs)
    xy = words_to_ints(got["commitments_xy.npy"])                     # x0, y0, x1, y1, ...
    assert got["commitments_xy.npy"].shape == (B, 2, 12)
    assert not got["commitments_infinity.npy"].any()
    for p in range(B):
        want = O.normalize(O.commit_trapdoor(coeffs[p * n:(p + 1) * n], TAU % cv.r, cv), cv)
        assert (xy[2 * p], xy[2 * p + 1]) == want, p
