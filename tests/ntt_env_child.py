"""Bodies of the child processes that test_ntt_plans_gpu.py starts for the paths csrc/ntt.hip selects from the
environment (KZG_NTT_TWIST_TABLE, KZG_NTT_TILE_LOG): the library reads both once, into statics, so each runs in a fresh
interpreter that has the variable set from the start.  A failed assertion ends the child with a non-zero status."""
import os

import numpy as np

from kzg_snark_amd import _native as native
from oracle import c_oracle as CO
from oracle import py_oracle as O
from ntt_helpers import assert_same, edge_vector, transform_on_device

CURVES = ["bls12_381", "bn254"]
KZG_ERR_ARG = -1


def twist_table():
    """KZG_NTT_TWIST_TABLE=1: pass 1 multiplies by one entry of the full [N1][N2] table (EPI_TABLE).
      * whole transforms at 2^13 (odd split) and 2^14, forward and inverse, against the C oracle;
      * kzg_ntt_columns_device at 2^13 on 16 columns whose first is global column 0 or 16 (EPI_TABLE with
        PLAIN = false; the table's column is col_base + tile * C + line), against OracleNttOps.columns -- the columns
        of the whole transform's first pass; like every pass that ends with the twist it hands on weakly normalised
        words: below 2r, the restatement's residue;
      * kzg_ntt_rows_twist_device needs the factor tables the full table replaced: KZG_ERR_ARG, and the context goes
        on working."""
    import torch
    import oracle_backends as OB
    assert os.environ.get("KZG_NTT_TWIST_TABLE") == "1"
    native.lib()
    for ci, curve in enumerate(CURVES):
        cv = O.curve(curve)
        ctx = native.Context(curve)
        wants = {}
        for log_n in (13, 14):
            w = cv.root_of_unity(1 << log_n)
            raw = edge_vector(np.random.RandomState(310 + log_n + ci), 1 << log_n, cv.r, native)
            for inverse in (False, True):
                want = CO.fft(curve, raw.copy(), w, inverse=inverse)
                assert_same(transform_on_device(native, ctx, raw, log_n, w, inverse), want, (curve, log_n, inverse))
                wants[log_n, inverse] = (raw, want)
        log_n, n_cols = 13, 16
        N1 = 1 << ((log_n + 1) // 2)
        w = cv.root_of_unity(1 << log_n)
        ww = native.int_to_words(w)
        rs = np.random.RandomState(330 + ci)
        for inverse in (False, True):
            spec = OB.OracleNttOps(log_n, w, cv.r, inverse)
            for col_base in (0, 16):
                raw = edge_vector(rs, N1 * n_cols, cv.r, native)
                host = torch.from_numpy(raw.view(np.int64).copy()).view(N1, n_cols, 4)
                dev = host.to("cuda:0")
                torch.cuda.synchronize()     # torch's stream wrote it; the context runs on a stream of its own
                ctx.ntt_columns_device(dev.data_ptr(), log_n, ww, inverse, n_cols, col_base)
                ctx.synchronize()
                spec.columns(host, col_base)
                got = native.limbs_to_ints(dev.cpu().numpy().view(np.uint64).reshape(-1, 4))
                exp = native.limbs_to_ints(host.numpy().view(np.uint64).reshape(-1, 4))
                what = (curve, "columns", inverse, col_base)
                assert all(v < 2 * cv.r for v in got), what
                bad = [i for i, (g, e) in enumerate(zip(got, exp)) if g % cv.r != e]
                assert not bad, what + (len(bad), bad[:8])
        rows = torch.zeros((16, (1 << log_n) // N1, 4), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        try:
            ctx.ntt_rows_twist_device(rows.data_ptr(), log_n, ww, False, 16, 0)
        except native.NativeError as e:
            assert e.code == KZG_ERR_ARG, e
        else:
            raise AssertionError("kzg_ntt_rows_twist_device ran without the factor tables")
        raw, want = wants[13, True]
        assert_same(transform_on_device(native, ctx, raw, 13, w, True), want, (curve, "after the refusal"))
        ctx.close()
    print("twist_table ok")


def tile_log_9():
    """KZG_NTT_TILE_LOG=9: what an untuned context takes (kzg_prof_read reports it); set_tuning("ntt_tile_log", 12)
    goes first, tuning 0 gives the variable its say back.  2^14, forward and inverse, equal to the C oracle in each
    of the three states."""
    assert os.environ.get("KZG_NTT_TILE_LOG") == "9"
    native.lib()
    log_n = 14
    for ci, curve in enumerate(CURVES):
        cv = O.curve(curve)
        ctx = native.Context(curve)
        w = cv.root_of_unity(1 << log_n)
        raw = edge_vector(np.random.RandomState(350 + ci), 1 << log_n, cv.r, native)
        wants = {inverse: CO.fft(curve, raw.copy(), w, inverse=inverse) for inverse in (False, True)}
        for tuning, took in ((None, 9), (12, 12), (0, 9)):
            if tuning is not None:
                ctx.set_tuning("ntt_tile_log", tuning)
            for inverse in (False, True):
                got = transform_on_device(native, ctx, raw, log_n, w, inverse)
                assert ctx.prof_read("ntt_tile_log")[0] == took, (curve, tuning, ctx.prof_read("ntt_tile_log"))
                assert_same(got, wants[inverse], (curve, "tuning", tuning, inverse))
        ctx.close()
    print("tile_log_9 ok")
