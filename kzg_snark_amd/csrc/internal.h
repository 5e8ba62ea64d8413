// internal.h -- library-private declarations shared by the translation units of
// libkzg_mi355x.so (api.hip, ntt.hip, msm.hip, msm_prep.hip, poly.hip, lagrange.hip, domain.hip, verify.hip,
// recover.hip, g1_bytes.hip, verify_points.hip, blob.hip, pairing.hip, g2_bytes.hip, g_mul.hip): the context, error and profiling plumbing, the dispatch by curve (KZG_BY_CURVE,
// KZG_BY_FR) and the entry points of ntt.hip and poly.hip.  Shared device helpers live in fr_util.h (one Fr element,
// the power-table lookup), g1_util.h (word arrays, XYZZ points), g1_words.h (point <-> canonical words) and
// srs_rec.h (key records); devmem.h owns device temporaries and carves the scratch buffers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <vector>
#include "field.h"
#include "devmem.h"

namespace kzg {

constexpr int KZG_OK = 0;
constexpr int KZG_ERR_ARG = -1;      // bad argument
constexpr int KZG_ERR_HIP = -2;      // HIP runtime error (see kzg_last_error)
constexpr int KZG_ERR_NODEV = -3;    // no usable gfx950 device
constexpr int KZG_ERR_DEGREE = -4;   // polynomial longer than the SRS (kzg.py:103-106)
constexpr int KZG_ERR_ALLOC = -5;

// A cached evaluation domain: everything the NTT kernels need for one
// (log_n, w, direction).  Built once per distinct root (callers reuse the same
// domain for every transform of a proof: plonk/encoder.py:49).
struct NttDomain {
  uint32_t log_n = 0;
  int inverse = 0;
  uint32_t w[8] = {0};        // caller's root, canonical words
  uint32_t kmax = 0;          // stage table holds (w^(n/2^kmax))^e, e < 2^(kmax-1)
  uint32_t h = 0;             // twist exponent split e = hi*2^h + lo
  uint32_t* d_stage = nullptr;   // [2^(kmax-1)][9] Montgomery limbs
  uint32_t* d_twA = nullptr;     // [2^(log_n-h)][9]  (w^(2^h))^u  (x n^-1 when inverse)
  uint32_t* d_twB = nullptr;     // [2^h][9]          w^l
  uint32_t* d_scale = nullptr;   // [9] n^-1 for a single-pass inverse transform; null: the last pass only reduces
  uint32_t* d_twist = nullptr;   // [n][9] w^(t*v) for two-pass sizes (row t of N2 entries); only with KZG_NTT_TWIST_TABLE=1
  uint64_t last_use = 0;
};

// Optional per-kernel timing with HIP events on the context's stream (bench.py's roofline
// leg): each named span accumulates elapsed ms and a launch count.
struct ProfSpan {
  std::string name;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  double total_ms = 0;
  uint64_t count = 0;
};

// words of Ctx::clk_probe
enum : int {
  CLK_ACC_LAUNCHES = 4,     // launches of msm_accumulate that reported when their waves left
  CLK_ACC_EXIT_SUM = 5,     // sum of the exit times of all their waves
  CLK_ACC_EXIT_FIRST = 6,   // sum over the launches of the first wave's exit time
  CLK_ACC_EXIT_LAST = 7,    // ... and of the last wave's
  CLK_ACC_WAVES = 8,        // waves per launch
  CLK_WORDS = 16
};

// The shape of one two-pass tile scan (poly.hip): all that its fill and eval launches need, free of the field
// template so that a context can keep it.
struct TileShape {
  size_t n = 0;                                   // coefficients
  uint32_t tb = 0, ntiles = 0, nsuper = 0;        // nsuper = 0: every tile sums all aggregates above it
  uint32_t *G = nullptr, *H = nullptr, *A = nullptr, *zinv = nullptr, *W = nullptr;      // the carve of the scan buffer
  uint32_t z[9] = {0}, z_inv[9] = {0};            // Montgomery limbs
};
// The slice between kzg_open_shard_begin and kzg_open_shard_finish.  HELD covers the slices without tiles too
// (shape.tb = 0): the empty one (shape.n = 0) and z = 0, whose finish is a copy.
struct OpenSlice {
  enum State { NEVER, HELD, LOST } state = NEVER;   // LOST: another opening took the two buffers since
  uint32_t z_words[8] = {0};                        // begin's z, canonical: finish must be given the same
  TileShape shape;
};

struct Ctx {
  int curve = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;
  std::vector<NttDomain> domains;
  uint64_t tick = 0;
  uint32_t ntt_lds_attr_set = 0;   // per ntt_pass_kernel instantiation: hipFuncAttributeMaxDynamicSharedMemorySize applies per device
  DevBuf ntt_scratch;     // pass-1 output of two-pass transforms
  DevBuf io;              // staging for the host-pointer entry points
  DevBuf poly_tmp[4];     // open(): combined polynomial + suffix values; [1]: the point tables of kzg_open_points;
                          // [2], [3]: scratch of the vector primitives and of kzg_fr_poly_eval[_batch]
  DevBuf scan_tmp;        // open(): chunk values, tile aggregates, power tables (open_slice holds their carve)
  DevBuf lagr_tmp;        // lagrange.hip: combined values, denominators, inverses, quotient, partial sums
  DevBuf dom_tmp;         // domain.hip: G1 transform buffers and the Fr vectors of one chunk of kzg_open_domain
  DevBuf ver_tmp;         // verify.hip: staged claims, proof records, weights, power tables, partial sums
  DevBuf rec_tmp;         // recover.hip: power tables, the product tree, Z and its inverses, one chunk of vectors
  DevBuf vpt_tmp;         // verify_points.hip: staged claims, weights, power table, partial sums and partial points
  DevBuf pair_tmp;        // pairing.hip: staged points, flags, values and statuses of one kzg_pairing_* call
  DevBuf gmul_tmp;        // g_mul.hip, g2_lincomb.hip: the lanes' tables of multiples, the power table, the staged arrays of one call
  size_t ver_last_bytes = 0;             // what the last kzg_verify_cosets carved out of ver_tmp (kzg_prof_read)
  size_t vpt_last_bytes = 0;              // what the last kzg_verify_points carved out of vpt_tmp (kzg_prof_read)
  uint32_t ver_lds_attr_set = 0;          // per ver_cell_kernel instantiation, as ntt_lds_attr_set
  // kzg_fr_eval_lagrange_batch*: the vector lengths travel from this pinned array; the event marks the last copy out
  // of it, waited for before the array is rewritten (the caller's own array need not outlive the call)
  uint32_t* eval_lens_pin = nullptr;
  size_t eval_lens_cap = 0;
  hipEvent_t eval_lens_ev = nullptr;
  OpenSlice open_slice;                   // what kzg_open_shard_begin left in poly_tmp[0] and scan_tmp for _finish
  // kzg_ctx_set_tuning: 0 = the library's own choice
  int tune_ntt_tile_log = 0;              // LDS tile of the transform (8..12)
  int tune_open_tb = 0;                   // threads per tile of the opening's scan (128 | 256)
  int tune_open_direct_max = 0;           // tiles up to which every tile sums all aggregates above it
  int tune_open_domain_chunk = 0;         // vectors per chunk of kzg_open_domain
  int tune_open_cosets_chunk = 0;         // vectors per chunk of kzg_open_cosets
  int tune_open_cosets_group = 0;         // 1 + log2 of kzg_open_cosets' Straus group (1..5)
  int tune_recover_chunk = 0;             // vectors per chunk of kzg_recover_cosets
  int tune_eval_batch_chunk = 0;          // vectors per chunk of kzg_fr_eval_lagrange_batch
  int last_ntt_tile_log = 0;              // what the last transform used (kzg_prof_read "ntt_tile_log")
  void* msm_work = nullptr;               // MsmWork (msm.hip)
  bool prof_on = false;
  std::vector<ProfSpan> prof;
  // [CLK_WORDS] profiling only: shader-clock / 100 MHz ticks of one wave of msm_accumulate ([0..1]) and of ntt_pass
  // ([2..3]); from CLK_ACC_LAUNCHES on, when the waves of msm_accumulate left (100 MHz ticks, sums over every launch)
  unsigned long long* clk_probe = nullptr;
  std::vector<hipStream_t> aux_streams;   // commit pipeline
  std::vector<hipEvent_t> aux_events;
};

int set_err(Ctx* c, int code, const char* what, hipError_t e = hipSuccess);
// RAII span: records an event pair around the launches issued while it is alive (no-op when profiling is off)
struct ProfScope {
  Ctx* c;
  ProfSpan* span = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipStream_t st = nullptr;
  ProfScope(Ctx* ctx, const char* name, hipStream_t stream = nullptr);
  ~ProfScope();
};

#define KZG_HIP(c, call)                                         \
  do {                                                           \
    hipError_t e__ = (call);                                     \
    if (e__ != hipSuccess) return set_err((c), KZG_ERR_HIP, #call, e__); \
  } while (0)
// the same as a value, KZG_OK or the recorded error, for a function that has to reach its own exit
#define KZG_HIP_RC(c, call) hip_rc((c), (call), #call)
inline int hip_rc(Ctx* c, hipError_t e, const char* what) { return e == hipSuccess ? KZG_OK : set_err(c, KZG_ERR_HIP, what, e); }

// Call-through by the context's curve: fn<Bn254 | Bls12_381>(args) for code over the curve, fn<BnFr | BlsFr>(args) for
// code over the scalar field alone.
#define KZG_BY_CURVE(c, fn, ...) ((c)->curve == 0 ? fn<Bn254>(__VA_ARGS__) : fn<Bls12_381>(__VA_ARGS__))
#define KZG_BY_FR(c, fn, ...) ((c)->curve == 0 ? fn<BnFr>(__VA_ARGS__) : fn<BlsFr>(__VA_ARGS__))

// msm.hip: is an accumulate kernel of the commit pipeline queued or running?
bool msm_accumulate_in_flight(Ctx* c);

// ntt.hip
int ntt_run_device(Ctx* c, uint32_t* d_data, uint32_t log_n, const uint32_t* w_words, int inverse,
                   uint32_t batch);
int ntt_partial_device(Ctx* c, uint32_t* d_data, uint32_t log_n, const uint32_t* w_words, int inverse, int rows_pass,
                       uint64_t count, uint64_t col_base);
int ntt_rows_exchange_device(Ctx* c, const uint32_t* d_src, uint32_t* d_dst, uint32_t log_n, const uint32_t* w_words,
                             int inverse, uint64_t n_rows, uint32_t world, int blocked_out);
int fft_ragged_device(Ctx* c, uint32_t* d_data, uint64_t n, const uint32_t* w_words, int inverse);
void ntt_free_domains(Ctx* c);

// poly.hip: device vector / polynomial primitives over Fr
int fr_vec_binary(Ctx* c, int op, size_t n, const uint32_t* a, const uint32_t* b, uint32_t* out);
int fr_vec_lincomb(Ctx* c, size_t n, size_t k, const uint32_t* const* ptrs, const size_t* lens, const uint32_t* scalars,
                   uint32_t* out);
int fr_vec_mul_powers(Ctx* c, size_t n, const uint32_t* a, const uint32_t* s, const uint32_t* cc, uint32_t* out);
int fr_vec_inverse(Ctx* c, size_t n, const uint32_t* a, uint32_t* out);
int fr_vec_prefix_product(Ctx* c, size_t n, const uint32_t* a, uint32_t* out);
int fr_poly_eval(Ctx* c, size_t n, const uint32_t* a, const uint32_t* z, uint64_t* out);
int fr_poly_eval_batch(Ctx* c, const uint32_t* d_polys, const size_t* lens, size_t k, size_t stride,
                       const uint32_t* points, size_t t, uint64_t* out);

// lagrange.hip (beside its table of w^i; not poly.hip, whose multiplier is built without field.h's chain pin):
// d_tab <- the two-level power table of `base` (Montgomery form), POW_TAB entries of 32 bytes, read by fr_pow_lookup
// (fr_util.h).  Enqueues one launch of fr_pow_table_kernel.
struct FrArg;   // fr_util.h
__attribute__((visibility("hidden")))   // library-private: not in the exported symbol list
int fr_pow_table(Ctx* c, const FrArg& base, uint32_t* d_tab);

}  // namespace kzg
