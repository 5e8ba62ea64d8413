"""ctypes binding of libkzg_mi355x.so (include/kzg_mi355x.h).

There is no CPU fallback: if the shared library is missing, or no gfx950 device
is visible, the first call raises NativeUnavailable -- loudly, by design."""
import ctypes
import os
from operator import methodcaller as _methodcaller

# HIP multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues per stream priority (default 4) and streams that share
# a queue serialise.  The commit pipeline no longer depends on this (csrc/msm.hip: two internal streams, the long kernel
# on a queue of the high-priority pool; measured equal at 4 and 8, EXPERIMENTS E3), and the line has no effect where
# the variable is already set or the HIP runtime already runs: it only spreads the CALLER's streams over more queues.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np  # noqa: E402

_HERE = os.path.dirname(os.path.abspath(__file__))
# KZG_MI355X_LIB: load another build of the library (A/B timing of kernel variants)
LIB_PATH = os.environ.get("KZG_MI355X_LIB") or os.path.join(_HERE, "lib", "libkzg_mi355x.so")

KZG_CURVE_BN254 = 0
KZG_CURVE_BLS12_381 = 1
CURVE_IDS = {"bn254": KZG_CURVE_BN254, "bls12_381": KZG_CURVE_BLS12_381}

HIP_STREAM_LEGACY = 1          # hipStreamLegacy: the explicit handle of HIP's null stream (hip_runtime_api.h)
KZG_ERR_DEGREE = -4
KZG_ERR_NODEV = -3

# every symbol include/kzg_mi355x.h declares (tests/test_abi.py checks the .so exports them all)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_vp = ctypes.c_void_p
SIGNATURES = {
    "kzg_abi_version": (ctypes.c_int, []),
    "kzg_fp_limbs": (ctypes.c_int, [ctypes.c_int]),
    "kzg_ctx_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(_vp)]),
    "kzg_ctx_destroy": (None, [_vp]),
    "kzg_last_error": (ctypes.c_char_p, [_vp]),
    "kzg_ctx_set_stream": (ctypes.c_int, [_vp, _vp]),
    "kzg_fft_ff_any": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_int]),
    "kzg_fft_ff_any_device": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_int]),
    "kzg_ctx_synchronize": (ctypes.c_int, [_vp]),
    "kzg_ctx_set_tuning": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_int64]),
    "kzg_ntt": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, _vp, ctypes.c_int]),
    "kzg_ntt_device": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, _vp, ctypes.c_int, ctypes.c_uint32]),
    "kzg_ntt_columns_device": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, _vp, ctypes.c_int, ctypes.c_uint64,
                                              ctypes.c_uint64]),
    "kzg_ntt_rows_device": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, _vp, ctypes.c_int, ctypes.c_uint64]),
    "kzg_ntt_rows_twist_device": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, _vp, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64]),
    "kzg_ntt_columns_plain_device": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, _vp, ctypes.c_int, ctypes.c_uint64]),
    "kzg_ntt_rows_exchange_device": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp, ctypes.c_int, ctypes.c_uint64,
                                                    ctypes.c_uint32, ctypes.c_int]),
    "kzg_srs_generate_strided": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                                ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "kzg_srs_load_g1": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "kzg_srs_free": (None, [_vp]),
    "kzg_srs_size": (ctypes.c_size_t, [_vp]),
    "kzg_srs_generate": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "kzg_srs_generate_range": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "kzg_srs_export": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp, _vp]),
    "kzg_commit": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp, _vp]),
    "kzg_commit_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp, _vp]),
    "kzg_commit_device_async": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp, _vp]),
    "kzg_commit_flush": (ctypes.c_int, [_vp]),
    "kzg_open": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp, _vp, _vp, _vp, _vp]),
    "kzg_open_shard_begin": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp, _vp, _vp]),
    "kzg_open_shard_finish": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int, _vp, _vp, _vp]),
    "kzg_fr_vec_op": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_size_t, _vp, _vp, _vp]),
    "kzg_fr_vec_lincomb": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_size_t, _vp, _vp, _vp, _vp]),
    "kzg_fr_vec_mul_powers": (ctypes.c_int, [_vp, ctypes.c_size_t, _vp, _vp, _vp, _vp]),
    "kzg_fr_vec_inverse": (ctypes.c_int, [_vp, ctypes.c_size_t, _vp, _vp]),
    "kzg_fr_vec_prefix_product": (ctypes.c_int, [_vp, ctypes.c_size_t, _vp, _vp]),
    "kzg_fr_poly_eval": (ctypes.c_int, [_vp, ctypes.c_size_t, _vp, _vp, _vp]),
    "kzg_fr_poly_eval_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp, ctypes.c_size_t,
                                              _vp]),
    "kzg_open_points_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp, ctypes.c_size_t,
                                              _vp, _vp, _vp, _vp]),
    "kzg_open_points": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp, ctypes.c_size_t,
                                       _vp, _vp, _vp, _vp]),
    "kzg_prof_enable": (ctypes.c_int, [_vp, ctypes.c_int]),
    "kzg_prof_reset": (ctypes.c_int, [_vp]),
    "kzg_prof_read": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double),
                                     ctypes.POINTER(ctypes.c_uint64)]),
    "kzg_open_device_async": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp, _vp, _vp, _vp, _vp]),
    "kzg_g1_sum": (ctypes.c_int, [ctypes.c_int, _vp, _vp, ctypes.c_size_t, _vp, _vp]),
    "kzg_open_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp, _vp, _vp, _vp, _vp]),
    "kzg_srs_generate_lagrange": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, _vp, ctypes.POINTER(_vp)]),
    "kzg_srs_lagrange": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, _vp, ctypes.POINTER(_vp)]),
    "kzg_open_evals": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp, _vp, _vp, _vp, _vp]),
    "kzg_open_evals_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp, _vp, _vp, _vp,
                                             _vp]),
    "kzg_open_evals_device_async": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp, _vp, _vp,
                                                   _vp, _vp]),
    "kzg_fr_eval_lagrange": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, ctypes.c_size_t, _vp, _vp, _vp]),
    "kzg_domain_table_create": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, ctypes.POINTER(_vp)]),
    "kzg_domain_table_size": (ctypes.c_size_t, [_vp]),
    "kzg_domain_table_free": (None, [_vp]),
    "kzg_open_domain": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp, _vp, _vp, _vp]),
    "kzg_open_domain_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp, _vp, _vp,
                                              _vp]),
    "kzg_coset_table_create": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_vp)]),
    "kzg_open_cosets": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, _vp, _vp,
                                       _vp, _vp]),
    "kzg_open_cosets_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32,
                                              _vp, _vp, _vp, _vp]),
    "kzg_open_coset": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, _vp, _vp,
                                      _vp, _vp, _vp, _vp]),
    "kzg_open_coset_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32,
                                             _vp, _vp, _vp, _vp, _vp, _vp]),
    "kzg_verify_cosets": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_size_t,
                                         _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp, _vp, _vp]),
    "kzg_verify_points": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp,
                                         _vp, _vp]),
    "kzg_fr_eval_lagrange_batch": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_size_t,
                                                  ctypes.c_size_t, _vp, _vp]),
    "kzg_fr_eval_lagrange_batch_device": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_size_t,
                                                         ctypes.c_size_t, _vp, _vp]),
    "kzg_recover_cosets": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp,
                                          ctypes.c_size_t, _vp, ctypes.c_size_t, _vp, _vp]),
    "kzg_g1_compress": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "kzg_g1_decompress": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_int, _vp, _vp, _vp]),
    "kzg_g1_decompress_device": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_int, _vp, _vp, _vp]),
    "kzg_g1_check_subgroup": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "kzg_g2_compress": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "kzg_g2_decompress": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_int, _vp, _vp, _vp]),
    "kzg_g2_decompress_device": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_int, _vp, _vp, _vp]),
    "kzg_g2_check_subgroup": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "kzg_g1_mul_each": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp, _vp, _vp]),
    "kzg_g1_mul_each_device": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp, _vp, _vp]),
    "kzg_g1_mul_powers": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp, _vp, _vp, _vp]),
    "kzg_srs_mul_powers": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.POINTER(_vp)]),
    "kzg_g2_mul_each": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp, _vp, _vp]),
    "kzg_g2_mul_powers": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp, _vp, _vp, _vp]),
    "kzg_g2_lincomb": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp, _vp, _vp]),
    "kzg_g2_lincomb_powers": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp, _vp, _vp, _vp]),
    "kzg_srs_load_g1_compressed": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(_vp)]),
    "kzg_srs_export_compressed": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp]),
    "kzg_recover_cosets_device": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp,
                                                 ctypes.c_size_t, _vp, ctypes.c_size_t, _vp, _vp]),
    "kzg_pairing_check": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp]),
    "kzg_pairing_product": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp, _vp]),
    "kzg_pairing_gt_multiple": (ctypes.c_int, [ctypes.c_int]),
    "kzg_blob_to_fr": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, ctypes.c_size_t, ctypes.c_int, _vp, _vp]),
    "kzg_blob_to_fr_device": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, ctypes.c_size_t, ctypes.c_int, _vp, _vp]),
    "kzg_fr_to_blob": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, ctypes.c_size_t, ctypes.c_int, _vp, _vp]),
    "kzg_fr_to_blob_device": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, ctypes.c_size_t, ctypes.c_int, _vp, _vp]),
    "kzg_verify_cosets_bytes": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _vp,
                                               ctypes.c_size_t, _vp, _vp, _vp, ctypes.c_int, _vp, _vp, ctypes.c_size_t,
                                               _vp, _vp, _vp, _vp]),
    "kzg_blob_challenges": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, _vp, ctypes.c_size_t, _vp]),
    "kzg_blob_challenges_device": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, _vp, ctypes.c_size_t, _vp]),
}


class NativeUnavailable(RuntimeError):
    pass


class NativeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libkzg_mi355x error {code}: {msg}")
        self.code = code


_lib = None
MISSING = []


def _preload_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's).  If this
    library were loaded first it would bind the system runtime and a later `import torch` would
    start a SECOND HIP runtime in the process (torch then reports "No HIP GPUs are available", and
    stream handles could not be shared).  Loading torch's copy first -- by path, without importing
    torch -- makes both sides resolve to one runtime whatever the import order."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    """Load the shared library (no GPU needed for loading; needed for contexts)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeUnavailable(
                f"{LIB_PATH} not built: run `python -m kzg_snark_amd.build` (no CPU fallback exists)")
        _preload_torch_hip_runtime()
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name, None)
            if fn is None:          # tests/test_abi.py requires MISSING to stay empty
                MISSING.append(name)
                continue
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check_out(a, dtype, size, what):
    """An output of a pipelined call is written later through a raw pointer: it must be a writable, contiguous numpy
    array of the right size (a temporary or a list would be gone, or never seen, by then)."""
    if a is None and what == "eval_out":
        return
    if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.flags.c_contiguous and a.flags.writeable
            and a.size >= size):
        raise TypeError(f"{what}: need a writable C-contiguous numpy {np.dtype(dtype).name} array of >= {size} elements")


def _as_vp(a):
    """numpy array / int device pointer / ctypes array -> c_void_p."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(ctypes.c_void_p)
    if isinstance(a, int):
        return ctypes.c_void_p(a)
    return ctypes.cast(a, ctypes.c_void_p)


def _fr(v):
    """one Fr scalar (anything int() takes) -> pointer to its 4 canonical words"""
    return _as_vp(int_to_words(int(v)))


def _inf_arg(inf, n, who):
    """infinity flags beside n points: None, or contiguous uint8[n]; `who` names the call and the pair in the message"""
    if inf is None:
        return None
    inf = np.ascontiguousarray(inf, dtype=np.uint8).reshape(-1)
    if inf.size != n:
        raise ValueError(f"{who} differ in length")
    return inf


def result_buffers(limbs, shape=(), evals=None):
    """Zeroed host arrays an entry point writes its results into: (xy uint64[*shape, 2*limbs], inf uint8[*shape],
    ev uint64[*evals] or None).  shape () is one point: xy uint64[2*limbs], inf uint8[1]."""
    shape = tuple(shape)
    return (np.zeros(shape + (2 * limbs,), dtype=np.uint64), np.zeros(shape or 1, dtype=np.uint8),
            None if evals is None else np.zeros(evals, dtype=np.uint64))


class Context:
    """One engine context: one curve, one GPU, one stream (kzg_ctx)."""

    def __init__(self, curve_type="bls12_381", device=0):
        if curve_type not in CURVE_IDS:
            raise ValueError(f"Unsupported curve type: {curve_type}")    # kzg.py:37
        self.curve_type = curve_type
        self.device = int(device)
        self.curve_id = CURVE_IDS[curve_type]
        self.fp_limbs = lib().kzg_fp_limbs(self.curve_id)
        h = ctypes.c_void_p()
        rc = lib().kzg_ctx_create(self.curve_id, int(device), ctypes.byref(h))
        if rc == KZG_ERR_NODEV:
            raise NativeUnavailable(
                "kzg_ctx_create: no gfx950 (MI355X) device visible; this engine has no CPU fallback")
        if rc != 0:
            raise NativeError(rc, "kzg_ctx_create failed")
        self._h = h
        # host arrays (and keys) the library still holds raw pointers to: the outputs of the pipelined entry points
        # are written when their slot is retired -- by a later commit or by commit_flush() -- so the context keeps
        # them alive until the flush, whatever the caller does with its own references
        self._inflight = []

    def close(self):
        if getattr(self, "_h", None):
            lib().kzg_ctx_destroy(self._h)       # waits for the device; pending results are dropped, not written
            self._h = None
            self._inflight = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            msg = lib().kzg_last_error(self._h)
            raise NativeError(rc, msg.decode() if msg else "")

    def _handle(self, fn, *args):
        """fn(ctx, *args, &handle), checked: the new handle"""
        h = ctypes.c_void_p()
        self._check(fn(self._h, *args, ctypes.byref(h)))
        return h

    def set_stream(self, stream_ptr):
        self._check(lib().kzg_ctx_set_stream(self._h, ctypes.c_void_p(stream_ptr or 0)))

    def bind_torch_stream(self, stream=None):
        """Run this context's work on a torch stream (default: torch's CURRENT stream on the
        context's device) so that tensors produced or consumed by torch ops are ordered with the
        engine's kernels without explicit synchronisation.  A fresh context owns a private
        non-blocking stream: a torch producer on another stream then needs torch.cuda.synchronize()
        (or an event) before the engine reads its output -- INTEGRATION.md, "stream ordering".
        Returns the torch stream that was bound."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        # torch's default stream is HIP's null stream (handle 0), and a NULL handle means "back to the
        # context's own stream" in kzg_ctx_set_stream: name the null stream explicitly instead
        self.set_stream(stream.cuda_stream or HIP_STREAM_LEGACY)
        self._torch_stream = stream            # keep the handle alive as long as it is bound
        return stream

    def synchronize(self):
        self._check(lib().kzg_ctx_synchronize(self._h))

    def set_tuning(self, key, value):
        """Fix a choice the library otherwise makes from what is resident ("ntt_tile_log", "open_tile_threads",
        "open_direct_tiles", "open_cosets_group", the "*_chunk" keys; 0 = the library's choice).  Results never depend
        on it."""
        self._check(lib().kzg_ctx_set_tuning(self._h, key.encode(), int(value)))

    # ---- measurement hooks
    def prof_enable(self, on=True):
        self._check(lib().kzg_prof_enable(self._h, int(bool(on))))

    def prof_reset(self):
        self._check(lib().kzg_prof_reset(self._h))

    def prof_read(self, name):
        """(total milliseconds, launches) of one span since the last reset."""
        ms, cnt = ctypes.c_double(0), ctypes.c_uint64(0)
        self._check(lib().kzg_prof_read(self._h, name.encode(), ctypes.byref(ms), ctypes.byref(cnt)))
        return ms.value, cnt.value

    # ---- NTT
    def ntt(self, data, log_n, w_words, inverse):
        """data: C-contiguous uint64[n,4] numpy array, transformed in place."""
        assert data.dtype == np.uint64 and data.flags.c_contiguous and data.size == 4 << log_n
        self._check(lib().kzg_ntt(self._h, _as_vp(data), log_n, _as_vp(w_words), int(bool(inverse))))

    def fft_ff_any(self, data, w_words, inverse):
        """fft_ff / ifft_ff of a list of ANY length >= 1 (reference recursion semantics), in place."""
        assert data.dtype == np.uint64 and data.flags.c_contiguous and data.ndim == 2 and data.shape[1] == 4
        self._check(lib().kzg_fft_ff_any(self._h, _as_vp(data), data.shape[0], _as_vp(w_words), int(bool(inverse))))

    def ntt_device(self, d_ptr, log_n, w_words, inverse, batch=1):
        self._check(lib().kzg_ntt_device(self._h, _as_vp(d_ptr), log_n, _as_vp(w_words),
                                         int(bool(inverse)), batch))

    def ntt_columns_device(self, d_ptr, log_n, w_words, inverse, n_cols, col_base):
        self._check(lib().kzg_ntt_columns_device(self._h, _as_vp(d_ptr), log_n, _as_vp(w_words),
                                                 int(bool(inverse)), n_cols, col_base))

    def ntt_rows_device(self, d_ptr, log_n, w_words, inverse, n_rows):
        self._check(lib().kzg_ntt_rows_device(self._h, _as_vp(d_ptr), log_n, _as_vp(w_words),
                                              int(bool(inverse)), n_rows))

    def ntt_rows_twist_device(self, d_ptr, log_n, w_words, inverse, n_rows, row_base):
        self._check(lib().kzg_ntt_rows_twist_device(self._h, _as_vp(d_ptr), log_n, _as_vp(w_words),
                                                    int(bool(inverse)), n_rows, row_base))

    def ntt_columns_plain_device(self, d_ptr, log_n, w_words, inverse, n_cols):
        self._check(lib().kzg_ntt_columns_plain_device(self._h, _as_vp(d_ptr), log_n, _as_vp(w_words),
                                                       int(bool(inverse)), n_cols))

    def ntt_rows_exchange_device(self, d_src, d_dst, log_n, w_words, inverse, n_rows, world, blocked_out):
        self._check(lib().kzg_ntt_rows_exchange_device(self._h, _as_vp(d_src), _as_vp(d_dst), log_n, _as_vp(w_words),
                                                       int(bool(inverse)), n_rows, world, int(bool(blocked_out))))

    # ---- SRS
    def srs_load_g1(self, xy, inf=None):
        """xy: uint64[n, 2*fp_limbs] affine canonical; inf: uint8[n] flags or None."""
        n = xy.shape[0]
        assert xy.dtype == np.uint64 and xy.flags.c_contiguous and xy.shape[1] == 2 * self.fp_limbs
        if inf is not None:
            assert inf.dtype == np.uint8 and inf.size == n and inf.flags.c_contiguous
        return Srs(self, self._handle(lib().kzg_srs_load_g1, _as_vp(xy), _as_vp(inf), n), n)

    def srs_load_g1_compressed(self, blobs, check_subgroup=True):
        """blobs: uint8[n, g1_bytes] compressed points (include/kzg_mi355x.h: the byte formats); decompressed and
        expanded on the device.  A point that does not decompress (or, with check_subgroup, lies outside the
        subgroup) raises NativeError naming the first such index."""
        blobs = np.ascontiguousarray(blobs, dtype=np.uint8).reshape(-1, self.g1_bytes)
        return Srs(self, self._handle(lib().kzg_srs_load_g1_compressed, _as_vp(blobs), blobs.shape[0],
                                      int(bool(check_subgroup))), blobs.shape[0])

    # ---- compressed points and subgroup membership
    @property
    def g1_bytes(self):
        """bytes of a compressed G1 point: 48 (bls12_381) or 32 (bn254)"""
        return 8 * self.fp_limbs

    def g1_compress(self, xy, inf=None):
        """affine points (uint64[n, 2*fp_limbs], uint8[n] flags or None) -> uint8[n, g1_bytes]"""
        xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1, 2 * self.fp_limbs)
        n = xy.shape[0]
        inf = _inf_arg(inf, n, "g1_compress: inf and xy")
        out = np.zeros((n, self.g1_bytes), dtype=np.uint8)
        self._check(lib().kzg_g1_compress(self._h, _as_vp(xy), _as_vp(inf), n, _as_vp(out)))
        return out

    def g1_decompress(self, blobs, check_subgroup=True):
        """uint8[n, g1_bytes] -> (xy uint64[n, 2*fp_limbs], inf uint8[n], status uint8[n]); status 0 ok, 1 bad
        encoding, 2 no such point, 3 outside the subgroup.  A failed point is all zeros."""
        blobs = np.ascontiguousarray(blobs, dtype=np.uint8).reshape(-1, self.g1_bytes)
        n = blobs.shape[0]
        xy = np.zeros((n, 2 * self.fp_limbs), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.uint8)
        status = np.zeros(n, dtype=np.uint8)
        self._check(lib().kzg_g1_decompress(self._h, _as_vp(blobs), n, int(bool(check_subgroup)), _as_vp(xy),
                                            _as_vp(inf), _as_vp(status)))
        return xy, inf, status

    def g1_decompress_device(self, d_bytes, n, check_subgroup, d_xy, d_inf, d_status):
        """The same on device pointers, enqueued on the context's stream (no synchronisation)."""
        self._check(lib().kzg_g1_decompress_device(self._h, _as_vp(d_bytes), int(n), int(bool(check_subgroup)),
                                                   _as_vp(d_xy), _as_vp(d_inf), _as_vp(d_status)))

    def g1_check_subgroup(self, xy, inf=None):
        """status uint8[n] of affine points: 0 in the subgroup (infinity included), 2 a coordinate >= p or off the
        curve, 3 on the curve but outside the subgroup"""
        xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1, 2 * self.fp_limbs)
        n = xy.shape[0]
        inf = _inf_arg(inf, n, "g1_check_subgroup: inf and xy")
        status = np.zeros(n, dtype=np.uint8)
        self._check(lib().kzg_g1_check_subgroup(self._h, _as_vp(xy), _as_vp(inf), n, _as_vp(status)))
        return status

    # ---- the G2 forms: points are uint64[n, 4*fp_limbs], x.c0 | x.c1 | y.c0 | y.c1 (pairing_check's layout)
    @property
    def g2_bytes(self):
        """bytes of a compressed G2 point: 96 (bls12_381) or 64 (bn254)"""
        return 16 * self.fp_limbs

    def g2_compress(self, xy, inf=None):
        """affine points (uint64[n, 4*fp_limbs], uint8[n] flags or None) -> uint8[n, g2_bytes]"""
        xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1, 4 * self.fp_limbs)
        n = xy.shape[0]
        inf = _inf_arg(inf, n, "g2_compress: inf and xy")
        out = np.zeros((n, self.g2_bytes), dtype=np.uint8)
        self._check(lib().kzg_g2_compress(self._h, _as_vp(xy), _as_vp(inf), n, _as_vp(out)))
        return out

    def g2_decompress(self, blobs, check_subgroup=True):
        """uint8[n, g2_bytes] -> (xy uint64[n, 4*fp_limbs], inf uint8[n], status uint8[n]); status 0 ok, 1 bad
        encoding, 2 no such point, 3 outside the subgroup.  A failed point is all zeros."""
        blobs = np.ascontiguousarray(blobs, dtype=np.uint8).reshape(-1, self.g2_bytes)
        n = blobs.shape[0]
        xy = np.zeros((n, 4 * self.fp_limbs), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.uint8)
        status = np.zeros(n, dtype=np.uint8)
        self._check(lib().kzg_g2_decompress(self._h, _as_vp(blobs), n, int(bool(check_subgroup)), _as_vp(xy),
                                            _as_vp(inf), _as_vp(status)))
        return xy, inf, status

    def g2_decompress_device(self, d_bytes, n, check_subgroup, d_xy, d_inf, d_status):
        """The same on device pointers, enqueued on the context's stream (no synchronisation)."""
        self._check(lib().kzg_g2_decompress_device(self._h, _as_vp(d_bytes), int(n), int(bool(check_subgroup)),
                                                   _as_vp(d_xy), _as_vp(d_inf), _as_vp(d_status)))

    def g2_check_subgroup(self, xy, inf=None):
        """status uint8[n] of affine points: 0 in the subgroup (infinity included), 2 a coordinate >= p or off the
        twist, 3 on the twist but outside the subgroup"""
        xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1, 4 * self.fp_limbs)
        n = xy.shape[0]
        inf = _inf_arg(inf, n, "g2_check_subgroup: inf and xy")
        status = np.zeros(n, dtype=np.uint8)
        self._check(lib().kzg_g2_check_subgroup(self._h, _as_vp(xy), _as_vp(inf), n, _as_vp(status)))
        return status

    # ---- per-point scalar multiplication: out[i] = [k_i] P_i, the products kept apart
    G1_MUL_LANES = 256          # lanes per workgroup of g1_mul_each_kernel / g2_mul_each_kernel (csrc/g_mul.hip)
    G2_MUL_LANES = 64
    G1_MUL_LAUNCH_LANES = 512 * 256     # lanes of one launch at the most (GM_LAUNCH_LANES1 / 2, csrc/g_mul.h): a longer
    G2_MUL_LAUNCH_LANES = 256 * 64      # call is split evenly over the fewest launches, all over one table

    def _mul_each(self, group, xy, inf, scalars, s, c0):
        """group 1 | 2; scalars uint64[n, 4] (each the 256-bit integer as it stands), or None for the power form
        c0 * s^i mod r -> (xy, inf) of the products"""
        width = 2 * group * self.fp_limbs
        name = "g%d_mul_%s" % (group, "powers" if scalars is None else "each")
        xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1, width)
        n = xy.shape[0]
        inf = _inf_arg(inf, n, f"{name}: inf and xy")
        out_xy, out_inf = np.zeros((n, width), dtype=np.uint64), np.zeros(n, dtype=np.uint8)
        if scalars is None:
            self._check(getattr(lib(), "kzg_" + name)(self._h, _as_vp(xy), _as_vp(inf), n, _fr(s), _fr(c0),
                                                      _as_vp(out_xy), _as_vp(out_inf)))
        else:
            scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
            if scalars.shape[0] != n:
                raise ValueError(f"{name}: {scalars.shape[0]} scalars for {n} points")
            self._check(getattr(lib(), "kzg_" + name)(self._h, _as_vp(xy), _as_vp(inf), n, _as_vp(scalars),
                                                      _as_vp(out_xy), _as_vp(out_inf)))
        return out_xy, out_inf

    def g1_mul_each(self, xy, inf, scalars):
        """affine points (uint64[n, 2*fp_limbs], uint8[n] flags or None) and scalars uint64[n, 4] -> (xy, inf)"""
        return self._mul_each(1, xy, inf, scalars, None, None)

    def g1_mul_powers(self, xy, inf, s, c0=1):
        """point i times c0 * s^i mod r (s, c0 ints below r), the scalars formed on the device"""
        return self._mul_each(1, xy, inf, None, s, c0)

    def g2_mul_each(self, xy, inf, scalars):
        """the same for points of the twist, uint64[n, 4*fp_limbs] (x.c0 | x.c1 | y.c0 | y.c1)"""
        return self._mul_each(2, xy, inf, scalars, None, None)

    def g2_mul_powers(self, xy, inf, s, c0=1):
        return self._mul_each(2, xy, inf, None, s, c0)

    # ---- linear combinations in G2: sum_i [k_i] Q_i as one point
    G2_LINCOMB_LANES = 64               # lanes per workgroup of g2_lincomb_kernel (GL_TB, csrc/g2_lincomb.h): one wave
    G2_LINCOMB_LAUNCH_LANES = 1024 * 64     # lanes of one launch at the most (GL_LAUNCH_LANES), all over one table
    G2_LINCOMB_FOLD_LANES = 64          # lanes per workgroup of g2_lincomb_fold_kernel (GL_FOLD_TB)
    G2_LINCOMB_FOLD_SPAN = 256          # points one workgroup of the fold adds (GL_FOLD_SPAN)

    def _g2_lincomb(self, xy, inf, scalars, s, c0):
        width = 4 * self.fp_limbs
        name = "g2_lincomb" if s is None else "g2_lincomb_powers"
        xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1, width)
        n = xy.shape[0]
        inf = _inf_arg(inf, n, f"{name}: inf and xy")
        out_xy, out_inf = np.zeros(width, dtype=np.uint64), np.zeros(1, dtype=np.uint8)
        if s is None:
            scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
            if scalars.shape[0] != n:
                raise ValueError(f"{name}: {scalars.shape[0]} scalars for {n} points")
            self._check(lib().kzg_g2_lincomb(self._h, _as_vp(xy), _as_vp(inf), n, _as_vp(scalars), _as_vp(out_xy),
                                             _as_vp(out_inf)))
        else:
            self._check(lib().kzg_g2_lincomb_powers(self._h, _as_vp(xy), _as_vp(inf), n, _fr(s), _fr(c0),
                                                    _as_vp(out_xy), _as_vp(out_inf)))
        return out_xy, out_inf

    def g2_lincomb(self, xy, inf, scalars):
        """points of the twist (uint64[n, 4*fp_limbs], uint8[n] flags or None) and scalars uint64[n, 4], each the 256-bit
        integer as it stands -> (xy uint64[4*fp_limbs], inf uint8[1]) of the ONE point sum_i [k_i] Q_i; n = 0: infinity"""
        return self._g2_lincomb(xy, inf, scalars, None, None)

    def g2_lincomb_powers(self, xy, inf, s, c0=1):
        """the same with the scalars c0 * s^i mod r (s, c0 ints below r), formed on the device"""
        return self._g2_lincomb(xy, inf, None, s, c0)

    def g1_mul_each_device(self, d_xy, d_inf, n, d_scalars, d_out_xy, d_out_inf):
        """The same on device pointers (d_inf may be None), enqueued on the context's stream (no synchronisation); a
        point that is refused leaves zeros and the flag 2."""
        self._check(lib().kzg_g1_mul_each_device(self._h, _as_vp(d_xy), _as_vp(d_inf), int(n), _as_vp(d_scalars),
                                                 _as_vp(d_out_xy), _as_vp(d_out_inf)))

    def srs_mul_powers(self, srs, s, c0=1):
        """key handle -> new key handle: point i of `srs` (monomial or Lagrange) times c0 * s^i mod r; a plain key"""
        return Srs(self, self._handle(lib().kzg_srs_mul_powers, srs._h, _fr(s), _fr(c0)), srs.n)

    # ---- pairing-product checks
    def _pairing_args(self, g1_xy, g1_inf, g2_xy, g2_inf, k, who):
        L = self.fp_limbs
        k = int(k)
        g1_xy = np.ascontiguousarray(g1_xy, dtype=np.uint64).reshape(-1, 2 * L)
        g2_xy = np.ascontiguousarray(g2_xy, dtype=np.uint64).reshape(-1, 4 * L)
        n = g1_xy.shape[0]
        if g2_xy.shape[0] != n or k < 1 or n % k:
            raise ValueError(f"{who}: {n} G1 points and {g2_xy.shape[0]} G2 points do not make equations of {k} pairs")
        g1_inf = _inf_arg(g1_inf, n, f"{who}: g1_inf and g1_xy")
        g2_inf = _inf_arg(g2_inf, n, f"{who}: g2_inf and g2_xy")
        return g1_xy, g1_inf, g2_xy, g2_inf, n // k, k

    def pairing_check(self, g1_xy, g1_inf, g2_xy, g2_inf, k):
        """m equations of k pairs, row-major: g1_xy uint64[m * k, 2*fp_limbs] (x | y), g2_xy uint64[m * k, 4*fp_limbs]
        (x.c0 | x.c1 | y.c0 | y.c1), flags uint8[m * k] or None -> status uint8[m]: 0 the product of the k pairings is
        one, 1 it is not, 2 a malformed point.  Pending pipeline results stay pending."""
        g1_xy, g1_inf, g2_xy, g2_inf, m, k = self._pairing_args(g1_xy, g1_inf, g2_xy, g2_inf, k, "pairing_check")
        status = np.zeros(m, dtype=np.uint8)
        self._check(lib().kzg_pairing_check(self._h, _as_vp(g1_xy), _as_vp(g1_inf), _as_vp(g2_xy), _as_vp(g2_inf), m, k,
                                            _as_vp(status)))
        return status

    def pairing_product(self, g1_xy, g1_inf, g2_xy, g2_inf, k):
        """The same with the values: (gt uint64[m, 12, fp_limbs], status uint8[m]); gt[e] is the product of equation e
        to the power PAIRING_GT_MULTIPLE[curve], six Fp2 tower coefficients c0 | c1, zeros where the status is 2."""
        g1_xy, g1_inf, g2_xy, g2_inf, m, k = self._pairing_args(g1_xy, g1_inf, g2_xy, g2_inf, k, "pairing_product")
        status = np.zeros(m, dtype=np.uint8)
        gt = np.zeros((m, 12, self.fp_limbs), dtype=np.uint64)
        self._check(lib().kzg_pairing_product(self._h, _as_vp(g1_xy), _as_vp(g1_inf), _as_vp(g2_xy), _as_vp(g2_inf), m,
                                              k, _as_vp(gt), _as_vp(status)))
        return gt, status

    # ---- EIP-4844 blobs as bytes
    def blob_to_fr(self, blobs, log_n, bit_reversed=True):
        """uint8[b, 32 << log_n] big-endian elements -> (values uint64[b, n, 4] canonical limbs, status uint8[b]);
        bit_reversed: element i lands at bitrev(i) (a blob in EIP-4844's order comes out in natural domain order).
        status 1: some element of the blob is >= r (written as zeros)."""
        size = 32 << int(log_n)
        blobs = np.ascontiguousarray(blobs, dtype=np.uint8).reshape(-1, size)
        b = blobs.shape[0]
        vals = np.zeros((b, 1 << int(log_n), 4), dtype=np.uint64)
        status = np.zeros(b, dtype=np.uint8)
        self._check(lib().kzg_blob_to_fr(self._h, int(log_n), _as_vp(blobs), b, int(bool(bit_reversed)), _as_vp(vals),
                                         _as_vp(status)))
        return vals, status

    def blob_to_fr_device(self, d_blobs, log_n, b, bit_reversed, d_vals, d_status):
        """The same on device pointers, enqueued on the context's stream (no synchronisation)."""
        self._check(lib().kzg_blob_to_fr_device(self._h, int(log_n), _as_vp(d_blobs), int(b), int(bool(bit_reversed)),
                                                _as_vp(d_vals), _as_vp(d_status)))

    def fr_to_blob(self, vals, log_n, bit_reversed=True):
        """The inverse of blob_to_fr: uint64[b, n, 4] canonical limbs -> (uint8[b, 32 << log_n] big-endian elements,
        status uint8[b]); bit_reversed: byte element i is value bitrev(i).  status 1: some element of the row is >= r
        (its bytes are zeros)."""
        n = 1 << int(log_n)
        vals = np.ascontiguousarray(vals, dtype=np.uint64).reshape(-1, n, 4)
        b = vals.shape[0]
        out = np.zeros((b, 32 * n), dtype=np.uint8)
        status = np.zeros(b, dtype=np.uint8)
        self._check(lib().kzg_fr_to_blob(self._h, int(log_n), _as_vp(vals), b, int(bool(bit_reversed)), _as_vp(out),
                                         _as_vp(status)))
        return out, status

    def fr_to_blob_device(self, d_vals, log_n, b, bit_reversed, d_bytes, d_status):
        """The same on device pointers, enqueued on the context's stream (no synchronisation)."""
        self._check(lib().kzg_fr_to_blob_device(self._h, int(log_n), _as_vp(d_vals), int(b), int(bool(bit_reversed)),
                                                _as_vp(d_bytes), _as_vp(d_status)))

    def blob_challenges(self, blobs, commitments, log_n):
        """uint8[b, 32 << log_n] blobs and uint8[b, g1_bytes] commitments -> uint64[b, 4]: the challenges
        SHA-256("FSBLOBVERIFY_V1_" | n | blob | commitment) mod r, hashed on the device, one lane per blob."""
        blobs = np.ascontiguousarray(blobs, dtype=np.uint8).reshape(-1, 32 << int(log_n))
        commitments = np.ascontiguousarray(commitments, dtype=np.uint8).reshape(-1, self.g1_bytes)
        b = blobs.shape[0]
        if commitments.shape[0] != b:
            raise ValueError("blob_challenges: blobs and commitments differ in number")
        z = np.zeros((b, 4), dtype=np.uint64)
        self._check(lib().kzg_blob_challenges(self._h, int(log_n), _as_vp(blobs), _as_vp(commitments), b, _as_vp(z)))
        return z

    def blob_challenges_device(self, d_blobs, d_commitments, log_n, b, d_z):
        """The same on device pointers, enqueued on the context's stream (no synchronisation)."""
        self._check(lib().kzg_blob_challenges_device(self._h, int(log_n), _as_vp(d_blobs), _as_vp(d_commitments),
                                                     int(b), _as_vp(d_z)))

    def srs_generate(self, tau_words, n, start=0):
        return Srs(self, self._handle(lib().kzg_srs_generate_range, _as_vp(tau_words), start, n), n)

    def srs_generate_strided(self, tau_words, start, n, run_len, inner_stride, outer_stride):
        """point i = tau^(start + (i // run_len) * outer_stride + (i % run_len) * inner_stride) * G1"""
        return Srs(self, self._handle(lib().kzg_srs_generate_strided, _as_vp(tau_words), start, n, run_len,
                                      inner_stride, outer_stride), n)

    # ---- evaluation form (Lagrange keys over the domain {w^i}, n = 2^log_n)
    def srs_generate_lagrange(self, tau_words, log_n, w):
        """[L_i(tau) G1], i < 2^log_n: the Lagrange key from the secret."""
        h = self._handle(lib().kzg_srs_generate_lagrange, _as_vp(tau_words), int(log_n), _fr(w))
        return Srs(self, h, 1 << int(log_n), basis=(int(log_n), int(w)))

    def srs_lagrange(self, monomial, log_n, w):
        """The Lagrange key from the first 2^log_n points of a monomial key (inverse NTT over G1)."""
        h = self._handle(lib().kzg_srs_lagrange, monomial._h, int(log_n), _fr(w))
        return Srs(self, h, 1 << int(log_n), basis=(int(log_n), int(w)))

    def open_evals(self, srs, vals, lens, stride, z_words, xi_words, device=False):
        """Opening from value vectors (uint64[k, stride, 4] host array, or a device pointer with device=True)
        against a Lagrange key: (out_xy, out_inf, eval)."""
        return self._open("kzg_open_evals", srs, vals, lens, stride, z_words, xi_words, device)

    def open_evals_device_async(self, srs, d_vals, lens, stride, z_words, xi_words, out_xy, out_inf, eval_out):
        """Pipelined opening from values: the outputs (numpy arrays the caller keeps alive) are filled by the time
        commit_flush() returns -- the slot rules of open_device_async."""
        self._open_async(lib().kzg_open_evals_device_async, srs, d_vals, lens, stride, z_words, xi_words, out_xy,
                         out_inf, eval_out)

    def eval_lagrange(self, log_n, w, n, d_vals, z):
        """p(z) of the interpolant of n device-resident values over {w^i} (barycentric, z in the domain included)."""
        out = np.zeros(4, dtype=np.uint64)
        self._check(lib().kzg_fr_eval_lagrange(self._h, int(log_n), _fr(w), n, _as_vp(d_vals), _fr(z), _as_vp(out)))
        return int.from_bytes(out.tobytes(), "little")

    def eval_lagrange_batch(self, log_n, w, vals, lens, stride, z, d_out=None):
        """p_j(z_j) of the interpolants of len(lens) value vectors over {w^i}, vector j at its own point.  Host form
        (d_out None): vals uint64[b, stride, 4], z uint64[b, 4] -> uint64[b, 4].  Device form: vals, z and d_out are
        device pointers (32-byte aligned); enqueued on the context's stream without waiting for the call's own work
        (the host may wait for the previous call's copy of its lengths), returns None."""
        lens_a = np.ascontiguousarray(lens, dtype=np.uint64).reshape(-1)
        b = lens_a.size
        if d_out is not None:
            self._check(lib().kzg_fr_eval_lagrange_batch_device(self._h, int(log_n), _fr(w), _as_vp(vals),
                                                                _as_vp(lens_a), b, int(stride), _as_vp(z),
                                                                _as_vp(d_out)))
            return None
        vals = np.ascontiguousarray(vals, dtype=np.uint64)
        z = np.ascontiguousarray(z, dtype=np.uint64)
        if vals.size != b * int(stride) * 4 or z.size != b * 4:
            raise ValueError("eval_lagrange_batch: vals is not [b][stride][4] or z is not [b][4]")
        out = np.zeros((b, 4), dtype=np.uint64)
        self._check(lib().kzg_fr_eval_lagrange_batch(self._h, int(log_n), _fr(w), _as_vp(vals), _as_vp(lens_a), b,
                                                     int(stride), _as_vp(z), _as_vp(out)))
        return out

    # ---- every proof on a domain (FK20)
    def domain_table(self, monomial, log_n):
        """The FK20 table of the first 2^log_n points of a monomial key."""
        return DomainTable(self, self._handle(lib().kzg_domain_table_create, monomial._h, int(log_n)),
                           1 << int(log_n))

    def open_domain(self, table, polys, lens, stride, w, device=False, evals=True):
        """All n proofs of each of len(lens) coefficient vectors (uint64[b, stride, 4] host array, or a device pointer
        with device=True) at w^i: (out_xy uint64[b, n, 2*fp_limbs], out_inf uint8[b, n], evals uint64[b, n, 4] or
        None)."""
        b, n = len(lens), table.n
        lens_a = np.asarray(lens, dtype=np.uint64)
        out = result_buffers(self.fp_limbs, (b, n), (b, n, 4) if evals else None)
        fn = lib().kzg_open_domain_device if device else lib().kzg_open_domain
        self._check(fn(self._h, table._h, _as_vp(polys), _as_vp(lens_a), b, stride, _fr(w), *map(_as_vp, out)))
        return out

    # ---- coset openings (FK20 multi-reveal, and one coset by division)
    def coset_table(self, monomial, log_n, log_l):
        """The coset table of the first 2^log_n points of a monomial key for cosets of 2^log_l points."""
        return DomainTable(self, self._handle(lib().kzg_coset_table_create, monomial._h, int(log_n), int(log_l)),
                           1 << int(log_n), 1 << int(log_l))

    def open_cosets(self, table, polys, lens, stride, log_N, w, device=False, evals=True):
        """The N/l coset proofs of each of len(lens) coefficient vectors (uint64[b, stride, 4] host array, or a device
        pointer with device=True) on the domain {w^t, t < N = 2^log_N}: (out_xy uint64[b, N/l, 2*fp_limbs],
        out_inf uint8[b, N/l], evals uint64[b, N/l, l, 4] or None)."""
        b, l = len(lens), table.l
        cosets = (1 << int(log_N)) // l
        lens_a = np.asarray(lens, dtype=np.uint64)
        out = result_buffers(self.fp_limbs, (b, cosets), (b, cosets, l, 4) if evals else None)
        fn = lib().kzg_open_cosets_device if device else lib().kzg_open_cosets
        self._check(fn(self._h, table._h, _as_vp(polys), _as_vp(lens_a), b, stride, int(log_N), _fr(w),
                       *map(_as_vp, out)))
        return out

    def open_coset(self, srs, polys, lens, stride, log_l, h, zeta, xi, device=False):
        """One coset proof of the xi-combination of len(lens) polynomials at h * zeta^k, k < 2^log_l:
        (out_xy uint64[2*fp_limbs], out_inf uint8[1], values uint64[l, 4])."""
        k = len(lens)
        lens_a = np.asarray(lens, dtype=np.uint64)
        out = result_buffers(self.fp_limbs, evals=(1 << int(log_l), 4))
        fn = lib().kzg_open_coset_device if device else lib().kzg_open_coset
        self._check(fn(self._h, srs._h, _as_vp(polys), _as_vp(lens_a), k, stride, int(log_l), _fr(h), _fr(zeta),
                       _fr(xi), *map(_as_vp, out)))
        return out

    # ---- bulk verification
    def verify_cosets(self, srs, log_N, log_l, w, comm_xy, comm_inf, comm_idx, coset_idx, values, proof_xy, proof_inf,
                      rho):
        """The two G1 points (L, R) of the rho-weighted combination of K coset claims: (xy uint64[2, 2*fp_limbs],
        inf uint8[2]); the claims hold iff e(L, G2) = e(R, [tau^l] G2).  comm_xy uint64[n_comm, 2*fp_limbs] with
        comm_inf uint8[n_comm] or None; comm_idx / coset_idx uint32[K]; values uint64[K, l, 4]; proof_xy
        uint64[K, 2*fp_limbs] with proof_inf uint8[K] or None -- the layouts open_cosets / open_domain return."""
        P = 2 * self.fp_limbs
        comm_idx = np.ascontiguousarray(comm_idx, dtype=np.uint32).reshape(-1)
        coset_idx = np.ascontiguousarray(coset_idx, dtype=np.uint32).reshape(-1)
        K, l = comm_idx.size, 1 << int(log_l)
        comm_xy = np.ascontiguousarray(comm_xy, dtype=np.uint64).reshape(-1, P)
        proof_xy = np.ascontiguousarray(proof_xy, dtype=np.uint64).reshape(-1, P)
        values = np.ascontiguousarray(values, dtype=np.uint64)
        if coset_idx.size != K or proof_xy.shape[0] != K or values.size != K * l * 4:
            raise ValueError("verify_cosets: comm_idx, coset_idx, values and proofs describe different numbers of cells")
        comm_inf = _inf_arg(comm_inf, comm_xy.shape[0], "verify_cosets: comm_inf and comm_xy")
        proof_inf = _inf_arg(proof_inf, K, "verify_cosets: proof_inf and proof_xy")
        out_xy, out_inf, _ = result_buffers(self.fp_limbs, (2,))
        self._check(lib().kzg_verify_cosets(self._h, srs._h, int(log_N), int(log_l), _fr(w), _as_vp(comm_xy),
                                            _as_vp(comm_inf), comm_xy.shape[0], _as_vp(comm_idx), _as_vp(coset_idx),
                                            _as_vp(values), _as_vp(proof_xy), _as_vp(proof_inf), K, _fr(rho),
                                            _as_vp(out_xy), _as_vp(out_inf)))
        # the library retires every pipeline slot before it returns, as kzg_commit_flush does
        self._inflight.clear()
        return out_xy, out_inf

    def verify_cosets_bytes(self, srs, log_N, log_l, w, comm_xy, comm_inf, comm_idx, coset_idx, cells, proof_xy,
                            proof_inf, rho, bit_reversed=True):
        """verify_cosets with the values as cells of 32-byte big-endian elements (uint8[K, 32 * l]; bit_reversed:
        element t of a cell is value bitrev(t) of its coset): (xy, inf, status).  status 1: some element is >= r, both
        points are then at infinity."""
        P = 2 * self.fp_limbs
        comm_idx = np.ascontiguousarray(comm_idx, dtype=np.uint32).reshape(-1)
        coset_idx = np.ascontiguousarray(coset_idx, dtype=np.uint32).reshape(-1)
        K, l = comm_idx.size, 1 << int(log_l)
        comm_xy = np.ascontiguousarray(comm_xy, dtype=np.uint64).reshape(-1, P)
        proof_xy = np.ascontiguousarray(proof_xy, dtype=np.uint64).reshape(-1, P)
        cells = np.ascontiguousarray(cells, dtype=np.uint8)
        if coset_idx.size != K or proof_xy.shape[0] != K or cells.size != K * l * 32:
            raise ValueError("verify_cosets_bytes: comm_idx, coset_idx, cells and proofs describe different numbers "
                             "of cells")
        comm_inf = _inf_arg(comm_inf, comm_xy.shape[0], "verify_cosets_bytes: comm_inf and comm_xy")
        proof_inf = _inf_arg(proof_inf, K, "verify_cosets_bytes: proof_inf and proof_xy")
        out_xy, out_inf, _ = result_buffers(self.fp_limbs, (2,))
        status = np.zeros(1, dtype=np.uint8)
        self._check(lib().kzg_verify_cosets_bytes(self._h, srs._h, int(log_N), int(log_l), _fr(w), _as_vp(comm_xy),
                                                  _as_vp(comm_inf), comm_xy.shape[0], _as_vp(comm_idx),
                                                  _as_vp(coset_idx), _as_vp(cells), int(bool(bit_reversed)),
                                                  _as_vp(proof_xy), _as_vp(proof_inf), K, _fr(rho), _as_vp(out_xy),
                                                  _as_vp(out_inf), _as_vp(status)))
        self._inflight.clear()
        return out_xy, out_inf, int(status[0])

    def verify_points(self, comm_xy, comm_inf, comm_idx, z, y, proof_xy, proof_inf, rho):
        """The two G1 points (L, R) of the rho-weighted combination of K claims at arbitrary points: (xy
        uint64[2, 2*fp_limbs], inf uint8[2]); the claims hold iff e(L, G2) = e(R, [tau] G2).  comm_xy
        uint64[n_comm, 2*fp_limbs] with comm_inf uint8[n_comm] or None; comm_idx uint32[K]; z, y uint64[K, 4];
        proof_xy uint64[K, 2*fp_limbs] with proof_inf uint8[K] or None.  Pending pipeline results stay pending."""
        P = 2 * self.fp_limbs
        comm_idx = np.ascontiguousarray(comm_idx, dtype=np.uint32).reshape(-1)
        K = comm_idx.size
        comm_xy = np.ascontiguousarray(comm_xy, dtype=np.uint64).reshape(-1, P)
        proof_xy = np.ascontiguousarray(proof_xy, dtype=np.uint64).reshape(-1, P)
        z = np.ascontiguousarray(z, dtype=np.uint64)
        y = np.ascontiguousarray(y, dtype=np.uint64)
        if proof_xy.shape[0] != K or z.size != K * 4 or y.size != K * 4:
            raise ValueError("verify_points: comm_idx, z, y and proofs describe different numbers of claims")
        comm_inf = _inf_arg(comm_inf, comm_xy.shape[0], "verify_points: comm_inf and comm_xy")
        proof_inf = _inf_arg(proof_inf, K, "verify_points: proof_inf and proof_xy")
        out_xy, out_inf, _ = result_buffers(self.fp_limbs, (2,))
        self._check(lib().kzg_verify_points(self._h, _as_vp(comm_xy), _as_vp(comm_inf), comm_xy.shape[0],
                                            _as_vp(comm_idx), _as_vp(z), _as_vp(y), _as_vp(proof_xy),
                                            _as_vp(proof_inf), K, _fr(rho), _as_vp(out_xy), _as_vp(out_inf)))
        return out_xy, out_inf

    # ---- coset recovery
    def recover_cosets(self, log_n, log_N, log_l, w, coset_idx, values, b, d_coeffs=None):
        """b coefficient vectors of 2^log_n elements from their values on the K cosets coset_idx (uint32[K]) of the
        domain {w^t, t < 2^log_N}: values uint64[b, K, l, 4] (host) -> (coeffs uint64[b, n, 4], consistent uint8[b]).
        With d_coeffs (a device pointer to b * n * 32 bytes) `values` is a device pointer as well, the coefficients
        stay on the device and coeffs is None.  consistent[j] = 0: the values of vector j lie on no polynomial of
        degree < n."""
        coset_idx = np.ascontiguousarray(coset_idx, dtype=np.uint32).reshape(-1)
        K, b = coset_idx.size, int(b)
        ok = np.zeros(max(b, 1), dtype=np.uint8)
        w_words = _fr(w)
        if d_coeffs is not None:
            self._check(lib().kzg_recover_cosets_device(self._h, int(log_n), int(log_N), int(log_l), w_words,
                                                        _as_vp(coset_idx), K, _as_vp(values), b, _as_vp(d_coeffs),
                                                        _as_vp(ok)))
            return None, ok[:b]
        values = np.ascontiguousarray(values, dtype=np.uint64)
        if values.size != b * K * (4 << int(log_l)):
            raise ValueError("recover_cosets: values is not [b][K][l][4]")
        coeffs = np.zeros((max(b, 1), 1 << int(log_n), 4), dtype=np.uint64)
        self._check(lib().kzg_recover_cosets(self._h, int(log_n), int(log_N), int(log_l), w_words, _as_vp(coset_idx),
                                             K, _as_vp(values), b, _as_vp(coeffs), _as_vp(ok)))
        return coeffs[:b], ok[:b]

    # ---- commit / open on host buffers
    def _commit(self, fn, srs, scalars, lens, stride):
        lens_a = np.asarray(lens, dtype=np.uint64)
        out_xy, out_inf, _ = result_buffers(self.fp_limbs, (len(lens),))
        self._check(fn(self._h, srs._h, _as_vp(scalars), _as_vp(lens_a), len(lens), stride, _as_vp(out_xy),
                       _as_vp(out_inf)))
        return out_xy, out_inf

    def commit(self, srs, scalars, lens, stride):
        """scalars: uint64[n_polys, stride, 4]; lens: per-polynomial coefficient counts."""
        return self._commit(lib().kzg_commit, srs, scalars, lens, stride)

    def commit_device(self, srs, d_scalars, lens, stride):
        return self._commit(lib().kzg_commit_device, srs, d_scalars, lens, stride)

    def commit_device_async(self, srs, d_scalars, lens, stride, out_xy, out_inf):
        """Pipelined commit: results land in the caller's out_xy / out_inf (numpy, kept alive by the
        caller) by the time commit_flush() returns."""
        lens_a = np.asarray(lens, dtype=np.uint64)
        _check_out(out_xy, np.uint64, len(lens) * 2 * self.fp_limbs, "out_xy")
        _check_out(out_inf, np.uint8, len(lens), "out_inf")
        # the library adopts the host pointers only once the work is queued, and every failure after that leaves
        # through a flush (commit_t in msm.hip, kzg_commit in api.hip): when a call returns non-zero, no pipeline slot
        # points at these arrays, so they are recorded after the call has returned KZG_OK
        self._check(lib().kzg_commit_device_async(self._h, srs._h, _as_vp(d_scalars), _as_vp(lens_a), len(lens),
                                                  stride, _as_vp(out_xy), _as_vp(out_inf)))
        self._inflight.append((srs, out_xy, out_inf))

    def commit_flush(self):
        """Drain the pipeline: every pending result is on the host when this returns (or raises)."""
        try:
            self._check(lib().kzg_commit_flush(self._h))
        finally:
            # the library retires every slot in kzg_commit_flush, also on error: nothing points at these any more
            self._inflight.clear()

    def _open(self, name, srs, data, lens, stride, z_words, xi_words, device):
        """kzg_open / kzg_open_evals (`name`), or its _device form: (out_xy, out_inf, eval)"""
        lens_a = np.asarray(lens, dtype=np.uint64)
        out = result_buffers(self.fp_limbs, evals=4)
        fn = getattr(lib(), name + "_device" if device else name)
        self._check(fn(self._h, srs._h, _as_vp(data), _as_vp(lens_a), len(lens), stride, _as_vp(z_words),
                       _as_vp(xi_words), *map(_as_vp, out)))
        return out

    def open(self, srs, polys, lens, stride, z_words, xi_words, device=False):
        return self._open("kzg_open", srs, polys, lens, stride, z_words, xi_words, device)

    def _open_async(self, fn, srs, d_data, lens, stride, z_words, xi_words, out_xy, out_inf, eval_out):
        lens_a = np.asarray(lens, dtype=np.uint64)
        _check_out(out_xy, np.uint64, 2 * self.fp_limbs, "out_xy")
        _check_out(out_inf, np.uint8, 1, "out_inf")
        _check_out(eval_out, np.uint64, 4, "eval_out")
        self._check(fn(self._h, srs._h, _as_vp(d_data), _as_vp(lens_a), len(lens), stride, _as_vp(z_words),
                       _as_vp(xi_words), _as_vp(out_xy), _as_vp(out_inf), _as_vp(eval_out)))
        self._inflight.append((srs, out_xy, out_inf, eval_out))          # after KZG_OK, as in commit_device_async

    def open_device_async(self, srs, d_polys, lens, stride, z_words, xi_words, out_xy, out_inf, eval_out):
        """Pipelined open: out_xy (uint64[2*fp_limbs]), out_inf (uint8[1]) and eval_out (uint64[4]) -- numpy arrays
        the caller keeps alive -- are filled by the time commit_flush() returns."""
        self._open_async(lib().kzg_open_device_async, srs, d_polys, lens, stride, z_words, xi_words, out_xy, out_inf,
                         eval_out)

    # ---- device vector / polynomial primitives (device pointers, canonical elements)
    def vec_op(self, op, n, d_a, d_b, d_out):
        self._check(lib().kzg_fr_vec_op(self._h, {"add": 0, "sub": 1, "mul": 2}[op], n, _as_vp(d_a), _as_vp(d_b),
                                        _as_vp(d_out)))

    def vec_lincomb(self, n, d_ptrs, lens, scalars, d_out):
        k = len(d_ptrs)
        ptrs = (ctypes.c_void_p * max(k, 1))(*[int(p) for p in d_ptrs])
        lens_a = np.asarray(lens, dtype=np.uint64)
        sc = np.ascontiguousarray(np.concatenate([int_to_words(int(s)) for s in scalars]) if k else np.zeros(4, np.uint64))
        self._check(lib().kzg_fr_vec_lincomb(self._h, n, k, ctypes.cast(ptrs, ctypes.c_void_p), _as_vp(lens_a),
                                             _as_vp(sc), _as_vp(d_out)))

    def vec_mul_powers(self, n, d_a, s, c0, d_out):
        self._check(lib().kzg_fr_vec_mul_powers(self._h, n, _as_vp(d_a), _fr(s), _fr(c0), _as_vp(d_out)))

    def vec_inverse(self, n, d_a, d_out):
        self._check(lib().kzg_fr_vec_inverse(self._h, n, _as_vp(d_a), _as_vp(d_out)))

    def vec_prefix_product(self, n, d_a, d_out):
        self._check(lib().kzg_fr_vec_prefix_product(self._h, n, _as_vp(d_a), _as_vp(d_out)))

    def poly_eval(self, n, d_a, z):
        out = np.zeros(4, dtype=np.uint64)
        self._check(lib().kzg_fr_poly_eval(self._h, n, _as_vp(d_a), _fr(z), _as_vp(out)))
        return int.from_bytes(out.tobytes(), "little")

    def poly_eval_batch(self, d_polys, lens, stride, points):
        """p_i(z_j) for the device polynomials (rows of d_polys) at `points`: [k][t] ints, one synchronisation"""
        k, t = len(lens), len(points)
        if k == 0 or t == 0:
            return [[0] * t for _ in range(k)]
        lens_a = np.asarray(lens, dtype=np.uint64)
        out = np.zeros((k, t, 4), dtype=np.uint64)
        self._check(lib().kzg_fr_poly_eval_batch(self._h, _as_vp(d_polys), _as_vp(lens_a), k, stride,
                                                 _as_vp(ints_to_limbs(points)), t, _as_vp(out)))
        vals = limbs_to_ints(out.reshape(k * t, 4))
        return [vals[i * t:(i + 1) * t] for i in range(k)]

    def open_points(self, srs, polys, lens, stride, points, weights, d_quot=None, device=False):
        """kzg_open_points[_device]: commit(sum_j Q_(z_j)[sum_i weights[i][j] p_i]) -> (out_xy, out_inf).  points: t
        ints; weights: k rows of t ints; d_quot: device pointer that receives the quotient's coefficients, or None."""
        k, t = len(lens), len(points)
        lens_a = np.asarray(lens, dtype=np.uint64)
        pts = ints_to_limbs(points) if t else np.zeros((1, 4), dtype=np.uint64)
        flat = [w for row in weights for w in row]
        if len(flat) != k * t:
            raise ValueError("open_points: weights must be k rows of t values")
        w = ints_to_limbs(flat) if flat else np.zeros((1, 4), dtype=np.uint64)
        out_xy, out_inf, _ = result_buffers(self.fp_limbs)
        fn = lib().kzg_open_points_device if device else lib().kzg_open_points
        self._check(fn(self._h, srs._h, _as_vp(polys), _as_vp(lens_a), k, stride, _as_vp(pts), t, _as_vp(w),
                       _as_vp(d_quot), _as_vp(out_xy), _as_vp(out_inf)))
        return out_xy, out_inf

    # ---- sharded open (device pointers)
    def open_shard_begin(self, d_polys, lens, stride, z_words, xi_words):
        lens_a = np.asarray(lens, dtype=np.uint64)
        h = np.zeros(4, dtype=np.uint64)
        self._check(lib().kzg_open_shard_begin(self._h, _as_vp(d_polys), _as_vp(lens_a), len(lens), stride,
                                               _as_vp(z_words), _as_vp(xi_words), _as_vp(h)))
        return h

    def open_shard_finish(self, srs, z_words, carry_words, first_rank):
        out = result_buffers(self.fp_limbs, evals=4)
        self._check(lib().kzg_open_shard_finish(self._h, srs._h, _as_vp(z_words), _as_vp(carry_words),
                                                int(bool(first_rank)), *map(_as_vp, out)))
        return out


class _Handle:
    """A device object of one context; `_free` names the ABI function that releases it.  Closing after the context
    has closed is a no-op (kzg_ctx_destroy has released everything the context owned)."""
    _free = None

    def close(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            getattr(lib(), self._free)(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Srs(_Handle):
    """Device-resident commitment key (kzg_srs): the reference's `ck` list.  basis: None for a monomial key
    ([tau^i] G1), (log_n, w) for a Lagrange key over the domain {w^i} ([L_i(tau)] G1)."""

    _free = "kzg_srs_free"

    def __init__(self, ctx, h, n, basis=None):
        self.ctx = ctx
        self._h = h
        self.n = n
        self.basis = basis

    def export(self, start=0, count=None):
        count = self.n - start if count is None else count
        xy = np.zeros((count, 2 * self.ctx.fp_limbs), dtype=np.uint64)
        inf = np.zeros(count, dtype=np.uint8)
        self.ctx._check(lib().kzg_srs_export(self.ctx._h, self._h, start, count, _as_vp(xy), _as_vp(inf)))
        return xy, inf

    def export_compressed(self, start=0, count=None):
        """points [start, start + count) as compressed blobs, uint8[count, g1_bytes]"""
        count = self.n - start if count is None else count
        out = np.zeros((count, self.ctx.g1_bytes), dtype=np.uint8)
        self.ctx._check(lib().kzg_srs_export_compressed(self.ctx._h, self._h, start, count, _as_vp(out)))
        return out


class DomainTable(_Handle):
    """FK20 table of one monomial key, domain size n and coset size l (kzg_domain_table; l = 1 from domain_table):
    2n affine points on the device."""

    _free = "kzg_domain_table_free"

    def __init__(self, ctx, h, n, l=1):
        self.ctx = ctx
        self._h = h
        self.n = n
        self.l = l


def g1_sum(curve_type, points):
    """Sum of G1 points given as facade tuples (x, y, 1) / (1, 1, 0), on the host in the library's C++ (kzg_g1_sum):
    microseconds per point where the pure-Python group law takes tens -- the add-up of the ranks' partial results.
    The points must be NORMALISED: the coordinates of a point whose z is neither 0 nor 1 are taken as they stand."""
    cid = CURVE_IDS[curve_type]
    L = lib().kzg_fp_limbs(cid)
    xy, inf = points_to_limbs(points, L)
    out_xy, out_inf, _ = result_buffers(L)
    rc = lib().kzg_g1_sum(cid, _as_vp(xy), _as_vp(inf), len(inf), _as_vp(out_xy), _as_vp(out_inf))
    if rc != 0:
        raise NativeError(rc, "kzg_g1_sum: a coordinate is not reduced or a point is not on the curve")
    return limbs_to_points(out_xy, out_inf)[0]


class _GtMultiple:
    """PAIRING_GT_MULTIPLE[curve name or id]: the c of kzg_pairing_product, whose values are e(P, Q)^c with e the
    pairing raised to (p^12 - 1) / r (csrc/fp_tower.h states c per curve; read from the library)."""

    def __getitem__(self, curve):
        cid = CURVE_IDS[curve] if isinstance(curve, str) else int(curve)
        c = lib().kzg_pairing_gt_multiple(cid)
        if c <= 0:
            raise KeyError(curve)
        return c


PAIRING_GT_MULTIPLE = _GtMultiple()


def g2_points_to_limbs(points, limbs):
    """G2 facade tuples ((x0, x1), (y0, y1), (1, 0)) / infinity with z = (0, 0) -> the C layout (xy uint64[n, 4*limbs]:
    x.c0 | x.c1 | y.c0 | y.c1, inf uint8[n]).  The points must be normalised."""
    points = list(points)
    inf = np.zeros(len(points), dtype=np.uint8)
    coords = []
    for i, pt in enumerate(points):
        z = pt[2]
        if z == 0 or tuple(z) == (0, 0):
            inf[i] = 1
            coords += [0, 0, 0, 0]
        else:
            if tuple(z) != (1, 0):
                raise ValueError("G2 points must be normalised")
            coords += [int(pt[0][0]), int(pt[0][1]), int(pt[1][0]), int(pt[1][1])]
    if not coords:
        return np.zeros((0, 4 * limbs), dtype=np.uint64), inf
    return np.ascontiguousarray(ints_to_limbs(coords, limbs).reshape(len(points), 4 * limbs)), inf


def limbs_to_g2_points(xy, inf):
    """affine G2 points in the C layout (x.c0 | x.c1 | y.c0 | y.c1 limbs per row, one infinity flag each) -> facade
    tuples ((x0, x1), (y0, y1), (1, 0)), infinity ((1, 0), (1, 0), (0, 0))"""
    out = []
    for row, f in zip(np.atleast_2d(xy), np.atleast_1d(inf)):
        if f:
            out.append(((1, 0), (1, 0), (0, 0)))
        else:
            v = limbs_to_ints(row.reshape(4, -1))
            out.append(((v[0], v[1]), (v[2], v[3]), (1, 0)))
    return out


def gt_to_tuple(gt_row, curve_type):
    """one value of kzg_pairing_product (uint64[12, fp_limbs]) -> the 12-tuple kzg_snark_amd/pairing.py returns:
    coefficient k of the tower value (a_k + b_k i) becomes entries k = a_k - shift b_k and k + 6 = b_k (its embed_fp2)"""
    from .pairing import _CURVES
    pc = _CURVES[curve_type]
    v = limbs_to_ints(np.ascontiguousarray(gt_row).reshape(12, -1))
    out = [0] * 12
    for k in range(6):
        a, b = v[2 * k], v[2 * k + 1]
        out[k] = (a - pc.shift * b) % pc.p
        out[k + 6] = b % pc.p
    return tuple(out)


_contexts = {}


def default_device():
    """The GPU the facade uses when none is named: KZG_MI355X_DEVICE, else torch's current device when this process
    has already initialised torch.cuda (one process per GPU: the launcher's torch.cuda.set_device(local_rank)), else 0."""
    import sys
    env = os.environ.get("KZG_MI355X_DEVICE")
    if env:
        return int(env)
    torch = sys.modules.get("torch")
    if torch is not None:
        try:
            if torch.cuda.is_available() and torch.cuda.is_initialized():
                return int(torch.cuda.current_device())
        except Exception:    # noqa: BLE001 -- a torch without a usable GPU runtime: the engine will say so itself
            pass
    return 0


def get_context(curve_type, device=None):
    device = default_device() if device is None else int(device)
    key = (curve_type, device)
    if key not in _contexts:
        _contexts[key] = Context(curve_type, device)
    return _contexts[key]


# ---- integer <-> limb marshalling -------------------------------------------------

def _load_pyconv():
    """csrc/pyconv.c built by kzg_snark_amd.build (CPython API; marshalling only).  Absent: the Python forms below."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "_kzg_pyconv.so")
    if not os.path.exists(path):
        return None
    try:
        import importlib.machinery
        import importlib.util
        loader = importlib.machinery.ExtensionFileLoader("_kzg_pyconv", path)
        spec = importlib.util.spec_from_loader("_kzg_pyconv", loader)
        mod = importlib.util.module_from_spec(spec)
        loader.exec_module(mod)
        return mod
    except Exception:   # noqa: BLE001 -- built for another interpreter, say: the Python forms still work
        return None


_pyconv = _load_pyconv()


def ints_to_limbs(values, limbs=4):
    """list of non-negative ints (< 2^(64*limbs)) -> uint64[n, limbs] (little-endian)."""
    nb = 8 * limbs
    if _pyconv is not None:
        if not isinstance(values, (list, tuple)):
            values = list(values)
        buf = _pyconv.ints_to_bytes(values, nb)          # a bytearray: wrapped, not copied
        return np.frombuffer(buf, dtype="<u8").reshape(len(values), limbs)
    try:                                   # plain ints (what every facade path passes): 1.8x the generator form
        buf = b"".join(map(_methodcaller("to_bytes", nb, "little"), values))
    except AttributeError:                 # field elements and other int()-able objects
        buf = b"".join(int(v).to_bytes(nb, "little") for v in values)
    return np.frombuffer(buf, dtype="<u8").reshape(len(values), limbs).copy()


def limbs_to_ints(arr):
    a = np.ascontiguousarray(arr, dtype="<u8")
    nb = 8 * a.shape[-1]
    if _pyconv is not None:
        return _pyconv.bytes_to_ints(a.reshape(-1).view(np.uint8), nb)
    raw = a.tobytes()
    return [int.from_bytes(raw[i:i + nb], "little") for i in range(0, len(raw), nb)]


def points_to_limbs(points, limbs, normalize=None):
    """Facade point tuples -> the C layout (xy uint64[n, 2*limbs] C-contiguous, inf uint8[n]); the one place where they
    become C arrays.  z == 0: flag 1 and zero coordinates; z == 1: the coordinates as given; any other z:
    normalize(point) when a callable is given (curve.normalize), the coordinates as given when it is None."""
    points = list(points)
    inf = np.zeros(len(points), dtype=np.uint8)
    coords = []
    for i, pt in enumerate(points):
        x, y, z = (int(c) for c in pt)
        if z == 0:
            inf[i] = 1
            x = y = 0
        elif z != 1 and normalize is not None:
            x, y, z = normalize((x, y, z))
        coords += [x, y]
    if not coords:
        return np.zeros((0, 2 * limbs), dtype=np.uint64), inf
    return np.ascontiguousarray(ints_to_limbs(coords, limbs).reshape(len(points), 2 * limbs)), inf


def limbs_to_points(xy, inf):
    """affine G1 points in the C layout (x | y limbs per row, one infinity flag each; a single row and flag too) ->
    facade tuples (x, y, 1), infinity (1, 1, 0)"""
    out = []
    for row, f in zip(np.atleast_2d(xy), np.atleast_1d(inf)):
        if f:
            out.append((1, 1, 0))
        else:
            v = limbs_to_ints(row.reshape(2, -1))
            out.append((v[0], v[1], 1))
    return out


def int_to_words(v, limbs=4):
    return np.frombuffer(int(v).to_bytes(8 * limbs, "little"), dtype="<u8").copy()
