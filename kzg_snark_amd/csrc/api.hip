// api.hip -- the extern "C" surface of libkzg_mi355x.so (include/kzg_mi355x.h).
#include "internal.h"
#include "g1_words.h"
#include "msm.h"
#include "../../include/kzg_mi355x.h"
#include <cstdio>
#include <cstring>
#include <new>

struct kzg_ctx {
  kzg::Ctx c;
};
struct kzg_srs {
  kzg::Srs* s;
};
struct kzg_domain_table {
  kzg::DomainTable* t;
};

namespace kzg {
int device_any_nonzero(Ctx* c, const uint32_t* d_words, size_t from, size_t to, bool* out);   // poly.hip
}

namespace kzg {

int set_err(Ctx* c, int code, const char* what, hipError_t e) {
  if (c) {
    c->err = what ? what : "";
    if (e != hipSuccess) {
      c->err += ": ";
      c->err += hipGetErrorString(e);
    }
  }
  return code;
}

ProfScope::ProfScope(Ctx* ctx, const char* name, hipStream_t stream) : c(ctx) {
  if (!c->prof_on) return;
  st = stream ? stream : c->stream;
  for (auto& sp : c->prof)
    if (sp.name == name) { span = &sp; break; }
  if (!span) {
    c->prof.reserve(64);   // spans are referenced by pointer while alive
    c->prof.push_back(ProfSpan{name, {}, 0, 0});
    span = &c->prof.back();
  }
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { span = nullptr; return; }
  hipEventRecord(e0, st);
}
ProfScope::~ProfScope() {
  if (!span) return;
  hipEventRecord(e1, st);
  span->pending.emplace_back(e0, e1);
}

int ensure_buf(Ctx* c, DevBuf& b, size_t bytes) {
  if (b.cap >= bytes) return KZG_OK;
  if (b.p) {
    KZG_HIP(c, hipStreamSynchronize(c->stream));
    KZG_HIP(c, hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
  }
  hipError_t e = hipMalloc(&b.p, bytes);
  if (e != hipSuccess) {
    b.p = nullptr;
    return set_err(c, KZG_ERR_ALLOC, "hipMalloc", e);
  }
  b.cap = bytes;
  return KZG_OK;
}

}  // namespace kzg

namespace kzg {
// sum of n affine points on the HOST (XYZZ accumulator, mixed additions of ec.h -- exact for O, P + P, P - P --, one
// inversion at the end): the "reduce" of partial MSM results that RCCL has no operator for
template <class C>
static int g1_sum_t(const uint64_t* xy, const uint8_t* inf, size_t n, uint64_t* out_xy, uint8_t* out_inf) {
  using F = typename C::Fp;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(xy);
  XYZZ<C> acc = Ec<C>::infinity();
  for (size_t i = 0; i < n; ++i) {
    if (inf && inf[i]) continue;
    Fe<F> x, y;   // coordinates must be canonical field elements of a point on the curve
    if (!import_affine<C>(w + i * 2 * F::NW, w + i * 2 * F::NW + F::NW, x, y)) return KZG_ERR_ARG;
    acc = Ec<C>::madd(acc, x, y);
  }
  *out_inf = affine_to_words<C>(Ec<C>::to_affine(acc), reinterpret_cast<uint32_t*>(out_xy));
  return KZG_OK;
}
}  // namespace kzg

using namespace kzg;

// The prologue of every entry point that takes a context: `bad` (the null checks of its arguments) is KZG_ERR_ARG,
// then `c` is the context and its device the current one.
#define KZG_ENTER(bad)                           \
  if (!ctx || (bad)) return KZG_ERR_ARG;         \
  Ctx* c = &ctx->c;                              \
  KZG_HIP(c, hipSetDevice(c->device))

// the epilogue of the key constructors: a key that was built becomes the caller's handle
static int adopt_srs(int rc, Srs* s, kzg_srs** out) {
  if (rc == KZG_OK) *out = new kzg_srs{s};
  return rc;
}

// the host-pointer entry points: `bytes` of host memory into the context's staging buffer, in stream order
static int stage_host(Ctx* c, const void* src, size_t bytes, void** d) {
  int rc = ensure_buf(c, c->io, bytes ? bytes : 32);
  if (rc) return rc;
  if (bytes) KZG_HIP(c, hipMemcpyAsync(c->io.p, src, bytes, hipMemcpyHostToDevice, c->stream));
  *d = c->io.p;
  return KZG_OK;
}

extern "C" {

int kzg_g1_sum(int curve_id, const uint64_t* xy, const uint8_t* inf, size_t n, uint64_t* out_xy, uint8_t* out_inf) {
  if ((n && !xy) || !out_xy || !out_inf) return KZG_ERR_ARG;
  if (curve_id == KZG_CURVE_BN254) return g1_sum_t<Bn254>(xy, inf, n, out_xy, out_inf);
  if (curve_id == KZG_CURVE_BLS12_381) return g1_sum_t<Bls12_381>(xy, inf, n, out_xy, out_inf);
  return KZG_ERR_ARG;
}

int kzg_abi_version(void) { return 1; }

int kzg_fp_limbs(int curve_id) {
  if (curve_id == KZG_CURVE_BN254) return 4;
  if (curve_id == KZG_CURVE_BLS12_381) return 6;
  return 0;
}

int kzg_ctx_create(int curve_id, int device_id, kzg_ctx** out) {
  if (!out) return KZG_ERR_ARG;
  *out = nullptr;
  if (curve_id != KZG_CURVE_BN254 && curve_id != KZG_CURVE_BLS12_381) return KZG_ERR_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev)
    return KZG_ERR_NODEV;   // no CPU fallback by design
  if (hipSetDevice(device_id) != hipSuccess) return KZG_ERR_NODEV;
  kzg_ctx* h = new (std::nothrow) kzg_ctx();
  if (!h) return KZG_ERR_ALLOC;
  h->c.curve = curve_id;
  h->c.device = device_id;
  if (hipStreamCreateWithFlags(&h->c.stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return KZG_ERR_HIP;
  }
  h->c.own_stream = true;
  *out = h;
  return KZG_OK;
}

void kzg_ctx_destroy(kzg_ctx* ctx) {
  if (!ctx) return;
  Ctx* c = &ctx->c;
  hipSetDevice(c->device);
  hipDeviceSynchronize();
  ntt_free_domains(c);
  msm_free_work(c);
  for (DevBuf* b : {&c->ntt_scratch, &c->io, &c->scan_tmp, &c->lagr_tmp, &c->dom_tmp, &c->ver_tmp, &c->rec_tmp,
                    &c->vpt_tmp, &c->pair_tmp, &c->gmul_tmp,
                    &c->poly_tmp[0], &c->poly_tmp[1], &c->poly_tmp[2], &c->poly_tmp[3]})
    hipFree(b->p);
  hipFree(c->clk_probe);
  if (c->eval_lens_pin) hipHostFree(c->eval_lens_pin);
  if (c->eval_lens_ev) hipEventDestroy(c->eval_lens_ev);
  for (auto s : c->aux_streams) hipStreamDestroy(s);
  for (auto e : c->aux_events) hipEventDestroy(e);
  if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
  delete ctx;
}

const char* kzg_last_error(const kzg_ctx* ctx) { return ctx ? ctx->c.err.c_str() : "null context"; }

int kzg_ctx_set_stream(kzg_ctx* ctx, void* hip_stream) {
  KZG_ENTER(false);
  if (hip_stream) {
    // HIP offers no validation of a stream handle: every entry point, hipStreamQuery included, dereferences it (a
    // readable buffer that is no stream crashed the process on ROCm 7.2, profiles/r03_stream_query_crash.log, and a
    // query on a capturing stream would invalidate the capture).  So nothing is asked of the runtime here: the two
    // documented aliases (hipStreamLegacy, hipStreamPerThread) are taken as such, any other small integer or
    // misaligned value cannot be a runtime object and is refused, and for everything else the caller guarantees a
    // live hipStream_t of this process.
    const uintptr_t hv = reinterpret_cast<uintptr_t>(hip_stream);
    const bool alias = hip_stream == static_cast<void*>(hipStreamLegacy) || hip_stream == static_cast<void*>(hipStreamPerThread);
    if (!alias && (hv < 65536 || (hv & 7)))
      return set_err(c, KZG_ERR_ARG, "kzg_ctx_set_stream: not a stream handle (small integer or misaligned value)");
    if (c->own_stream && c->stream) {
      KZG_HIP(c, hipStreamSynchronize(c->stream));
      KZG_HIP(c, hipStreamDestroy(c->stream));
    }
    // hipStreamLegacy names HIP's null stream (torch's default stream).  Internally that is the plain
    // null handle, which every runtime entry point accepts (event record / wait on the alias do not).
    c->stream = hip_stream == static_cast<void*>(hipStreamLegacy) ? nullptr : static_cast<hipStream_t>(hip_stream);
    c->own_stream = false;
  } else if (!c->own_stream) {
    KZG_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->own_stream = true;
  }
  return KZG_OK;
}

int kzg_ctx_set_tuning(kzg_ctx* ctx, const char* key, int64_t value) {
  if (!ctx || !key) return KZG_ERR_ARG;
  Ctx* c = &ctx->c;
  const std::string k(key);
  if (k == "ntt_tile_log") {
    if (value != 0 && (value < 8 || value > 12)) return set_err(c, KZG_ERR_ARG, "ntt_tile_log: 0 or 8..12");
    c->tune_ntt_tile_log = (int)value;
  } else if (k == "open_tile_threads") {
    if (value != 0 && value != 128 && value != 256) return set_err(c, KZG_ERR_ARG, "open_tile_threads: 0, 128 or 256");
    c->tune_open_tb = (int)value;
  } else if (k == "open_direct_tiles") {
    if (value < 0 || value > (1 << 20)) return set_err(c, KZG_ERR_ARG, "open_direct_tiles: 0 .. 2^20");
    c->tune_open_direct_max = (int)value;
  } else if (k == "open_domain_chunk") {
    if (value < 0 || value > 1024) return set_err(c, KZG_ERR_ARG, "open_domain_chunk: 0 .. 1024");
    c->tune_open_domain_chunk = (int)value;
  } else if (k == "open_cosets_chunk") {
    if (value < 0 || value > 1024) return set_err(c, KZG_ERR_ARG, "open_cosets_chunk: 0 .. 1024");
    c->tune_open_cosets_chunk = (int)value;
  } else if (k == "open_cosets_group") {
    if (value < 0 || value > 5) return set_err(c, KZG_ERR_ARG, "open_cosets_group: 0 .. 5");
    c->tune_open_cosets_group = (int)value;
  } else if (k == "recover_chunk") {
    if (value < 0 || value > 1024) return set_err(c, KZG_ERR_ARG, "recover_chunk: 0 .. 1024");
    c->tune_recover_chunk = (int)value;
  } else if (k == "eval_batch_chunk") {
    if (value < 0 || value > 65535) return set_err(c, KZG_ERR_ARG, "eval_batch_chunk: 0 .. 65535");
    c->tune_eval_batch_chunk = (int)value;
  } else {
    return set_err(c, KZG_ERR_ARG, "kzg_ctx_set_tuning: unknown key");
  }
  return KZG_OK;
}

int kzg_ctx_synchronize(kzg_ctx* ctx) {
  if (!ctx) return KZG_ERR_ARG;
  Ctx* c = &ctx->c;
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  return KZG_OK;
}

int kzg_ntt_device(kzg_ctx* ctx, void* d_data, uint32_t log_n, const uint64_t w[4], int inverse,
                   uint32_t batch) {
  KZG_ENTER(!d_data || !w);
  return ntt_run_device(c, static_cast<uint32_t*>(d_data), log_n, reinterpret_cast<const uint32_t*>(w),
                        inverse ? 1 : 0, batch);
}

int kzg_ntt_columns_device(kzg_ctx* ctx, void* d_data, uint32_t log_n, const uint64_t w[4], int inverse,
                           uint64_t n_cols, uint64_t col_base) {
  KZG_ENTER(!d_data || !w);
  return ntt_partial_device(c, static_cast<uint32_t*>(d_data), log_n, reinterpret_cast<const uint32_t*>(w),
                            inverse ? 1 : 0, 0, n_cols, col_base);
}

int kzg_ntt_rows_device(kzg_ctx* ctx, void* d_data, uint32_t log_n, const uint64_t w[4], int inverse,
                        uint64_t n_rows) {
  KZG_ENTER(!d_data || !w);
  return ntt_partial_device(c, static_cast<uint32_t*>(d_data), log_n, reinterpret_cast<const uint32_t*>(w),
                            inverse ? 1 : 0, 1, n_rows, 0);
}

int kzg_ntt_rows_twist_device(kzg_ctx* ctx, void* d_data, uint32_t log_n, const uint64_t w[4], int inverse,
                              uint64_t n_rows, uint64_t row_base) {
  KZG_ENTER(!d_data || !w);
  return ntt_partial_device(c, static_cast<uint32_t*>(d_data), log_n, reinterpret_cast<const uint32_t*>(w),
                            inverse ? 1 : 0, 2, n_rows, row_base);
}

int kzg_ntt_columns_plain_device(kzg_ctx* ctx, void* d_data, uint32_t log_n, const uint64_t w[4], int inverse,
                                 uint64_t n_cols) {
  KZG_ENTER(!d_data || !w);
  return ntt_partial_device(c, static_cast<uint32_t*>(d_data), log_n, reinterpret_cast<const uint32_t*>(w),
                            inverse ? 1 : 0, 3, n_cols, 0);
}

int kzg_ntt_rows_exchange_device(kzg_ctx* ctx, const void* d_src, void* d_dst, uint32_t log_n, const uint64_t w[4],
                                 int inverse, uint64_t n_rows, uint32_t world, int blocked_out) {
  KZG_ENTER(!d_src || !d_dst || !w);
  return ntt_rows_exchange_device(c, static_cast<const uint32_t*>(d_src), static_cast<uint32_t*>(d_dst), log_n,
                                  reinterpret_cast<const uint32_t*>(w), inverse ? 1 : 0, n_rows, world, blocked_out);
}

int kzg_ntt(kzg_ctx* ctx, uint64_t* data, uint32_t log_n, const uint64_t w[4], int inverse) {
  KZG_ENTER(!data || !w);
  if (log_n > 24) return set_err(c, KZG_ERR_ARG, "kzg_ntt: log_n > 24 not supported");
  const size_t bytes = (size_t)32 << log_n;
  void* d = nullptr;
  int rc = stage_host(c, data, bytes, &d);
  if (rc) return rc;
  rc = ntt_run_device(c, static_cast<uint32_t*>(d), log_n, reinterpret_cast<const uint32_t*>(w), inverse ? 1 : 0, 1);
  if (rc) return rc;
  KZG_HIP(c, hipMemcpyAsync(data, d, bytes, hipMemcpyDeviceToHost, c->stream));
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  return KZG_OK;
}

int kzg_fft_ff_any_device(kzg_ctx* ctx, void* d_data, size_t n, const uint64_t w[4], int inverse) {
  KZG_ENTER(!d_data || !w);
  if (n && !(n & (n - 1))) {   // power of two: the tiled kernels compute the same recursion
    uint32_t log_n = 0;
    while ((1ull << log_n) < n) ++log_n;
    return ntt_run_device(c, static_cast<uint32_t*>(d_data), log_n, reinterpret_cast<const uint32_t*>(w),
                          inverse ? 1 : 0, 1);
  }
  return fft_ragged_device(c, static_cast<uint32_t*>(d_data), n, reinterpret_cast<const uint32_t*>(w), inverse ? 1 : 0);
}

int kzg_fft_ff_any(kzg_ctx* ctx, uint64_t* data, size_t n, const uint64_t w[4], int inverse) {
  KZG_ENTER(!data || !w);
  if (n == 0 || n > ((size_t)1 << 24)) return set_err(c, KZG_ERR_ARG, "kzg_fft_ff_any: length must be in [1, 2^24]");
  const size_t bytes = n * 32;
  void* d = nullptr;
  int rc = stage_host(c, data, bytes, &d);
  if (rc) return rc;
  rc = kzg_fft_ff_any_device(ctx, d, n, w, inverse);
  if (rc) return rc;
  KZG_HIP(c, hipMemcpyAsync(data, d, bytes, hipMemcpyDeviceToHost, c->stream));
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  return KZG_OK;
}

int kzg_srs_load_g1(kzg_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, kzg_srs** out) {
  KZG_ENTER(!xy || !out);
  *out = nullptr;
  Srs* s = nullptr;
  const int rc = srs_load(c, xy, inf, n, &s);
  return adopt_srs(rc, s, out);
}

int kzg_srs_generate_range(kzg_ctx* ctx, const uint64_t tau[4], size_t start, size_t n, kzg_srs** out) {
  KZG_ENTER(!tau || !out);
  *out = nullptr;
  Srs* s = nullptr;
  const int rc = srs_generate(c, tau, start, n, &s);
  return adopt_srs(rc, s, out);
}

int kzg_srs_generate_strided(kzg_ctx* ctx, const uint64_t tau[4], size_t start, size_t n, size_t run_len,
                             size_t inner_stride, size_t outer_stride, kzg_srs** out) {
  KZG_ENTER(!tau || !out || run_len == 0);
  *out = nullptr;
  Srs* s = nullptr;
  const int rc = srs_generate(c, tau, start, n, &s, run_len, inner_stride, outer_stride);
  return adopt_srs(rc, s, out);
}

int kzg_srs_generate(kzg_ctx* ctx, const uint64_t tau[4], size_t n, kzg_srs** out) {
  return kzg_srs_generate_range(ctx, tau, 0, n, out);
}

int kzg_srs_export(kzg_ctx* ctx, const kzg_srs* srs, size_t start, size_t count, uint64_t* xy, uint8_t* inf) {
  KZG_ENTER(!srs || !xy || !inf);
  return srs_export(c, srs->s, start, count, xy, inf);
}

int kzg_srs_load_g1_compressed(kzg_ctx* ctx, const uint8_t* bytes, size_t n, int check_subgroup, kzg_srs** out) {
  KZG_ENTER(!bytes || !out);
  *out = nullptr;
  Srs* s = nullptr;
  const int rc = srs_load_g1_compressed(c, bytes, n, check_subgroup, &s);
  return adopt_srs(rc, s, out);
}

int kzg_srs_export_compressed(kzg_ctx* ctx, const kzg_srs* srs, size_t start, size_t count, uint8_t* out_bytes) {
  KZG_ENTER(!srs || (count && !out_bytes));
  if (srs->s->curve != c->curve) return set_err(c, KZG_ERR_ARG, "SRS belongs to another curve");
  return srs_export_compressed(c, srs->s, start, count, out_bytes);
}

int kzg_g1_compress(kzg_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out_bytes) {
  KZG_ENTER(n && (!xy || !out_bytes));
  return g1_compress(c, xy, inf, n, out_bytes);
}

int kzg_g1_decompress(kzg_ctx* ctx, const uint8_t* bytes, size_t n, int check_subgroup, uint64_t* out_xy,
                      uint8_t* out_inf, uint8_t* out_status) {
  KZG_ENTER(n && (!bytes || !out_xy || !out_inf || !out_status));
  return g1_decompress(c, bytes, n, check_subgroup, out_xy, out_inf, out_status);
}

int kzg_g1_decompress_device(kzg_ctx* ctx, const void* d_bytes, size_t n, int check_subgroup, void* d_xy, void* d_inf,
                             void* d_status) {
  KZG_ENTER(n && (!d_bytes || !d_xy || !d_inf || !d_status));
  return g1_decompress_device(c, d_bytes, n, check_subgroup, d_xy, d_inf, d_status);
}

int kzg_g1_check_subgroup(kzg_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out_status) {
  KZG_ENTER(n && (!xy || !out_status));
  return g1_check_subgroup(c, xy, inf, n, out_status);
}

int kzg_g2_compress(kzg_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out_bytes) {
  KZG_ENTER(n && (!xy || !out_bytes));
  return g2_compress(c, xy, inf, n, out_bytes);
}

int kzg_g2_decompress(kzg_ctx* ctx, const uint8_t* bytes, size_t n, int check_subgroup, uint64_t* out_xy,
                      uint8_t* out_inf, uint8_t* out_status) {
  KZG_ENTER(n && (!bytes || !out_xy || !out_inf || !out_status));
  return g2_decompress(c, bytes, n, check_subgroup, out_xy, out_inf, out_status);
}

int kzg_g2_decompress_device(kzg_ctx* ctx, const void* d_bytes, size_t n, int check_subgroup, void* d_xy, void* d_inf,
                             void* d_status) {
  KZG_ENTER(n && (!d_bytes || !d_xy || !d_inf || !d_status));
  return g2_decompress_device(c, d_bytes, n, check_subgroup, d_xy, d_inf, d_status);
}

int kzg_g2_check_subgroup(kzg_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out_status) {
  KZG_ENTER(n && (!xy || !out_status));
  return g2_check_subgroup(c, xy, inf, n, out_status);
}

int kzg_g1_mul_each(kzg_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, const uint64_t* scalars,
                    uint64_t* out_xy, uint8_t* out_inf) {
  KZG_ENTER(n && (!xy || !scalars || !out_xy || !out_inf));
  return g1_mul_each(c, xy, inf, n, reinterpret_cast<const uint32_t*>(scalars), nullptr, nullptr, out_xy, out_inf);
}

int kzg_g1_mul_each_device(kzg_ctx* ctx, const void* d_xy, const void* d_inf, size_t n, const void* d_scalars,
                           void* d_out_xy, void* d_out_inf) {
  KZG_ENTER(n && (!d_xy || !d_scalars || !d_out_xy || !d_out_inf));
  return g1_mul_each_device(c, d_xy, d_inf, n, d_scalars, d_out_xy, d_out_inf);
}

int kzg_g1_mul_powers(kzg_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, const uint64_t s[4],
                      const uint64_t c0[4], uint64_t* out_xy, uint8_t* out_inf) {
  KZG_ENTER(!s || !c0 || (n && (!xy || !out_xy || !out_inf)));
  return g1_mul_each(c, xy, inf, n, nullptr, reinterpret_cast<const uint32_t*>(s), reinterpret_cast<const uint32_t*>(c0),
                     out_xy, out_inf);
}

int kzg_srs_mul_powers(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t s[4], const uint64_t c0[4], kzg_srs** out) {
  KZG_ENTER(!srs || !s || !c0 || !out);
  *out = nullptr;
  if (srs->s->curve != c->curve) return set_err(c, KZG_ERR_ARG, "SRS belongs to another curve");
  Srs* key = nullptr;
  const int rc = srs_mul_powers(c, srs->s, reinterpret_cast<const uint32_t*>(s), reinterpret_cast<const uint32_t*>(c0), &key);
  return adopt_srs(rc, key, out);
}

int kzg_g2_mul_each(kzg_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, const uint64_t* scalars,
                    uint64_t* out_xy, uint8_t* out_inf) {
  KZG_ENTER(n && (!xy || !scalars || !out_xy || !out_inf));
  return g2_mul_each(c, xy, inf, n, reinterpret_cast<const uint32_t*>(scalars), nullptr, nullptr, out_xy, out_inf);
}

int kzg_g2_mul_powers(kzg_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, const uint64_t s[4],
                      const uint64_t c0[4], uint64_t* out_xy, uint8_t* out_inf) {
  KZG_ENTER(!s || !c0 || (n && (!xy || !out_xy || !out_inf)));
  return g2_mul_each(c, xy, inf, n, nullptr, reinterpret_cast<const uint32_t*>(s), reinterpret_cast<const uint32_t*>(c0),
                     out_xy, out_inf);
}

int kzg_g2_lincomb(kzg_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, const uint64_t* scalars,
                   uint64_t* out_xy, uint8_t* out_inf) {
  KZG_ENTER(!out_xy || !out_inf || (n && (!xy || !scalars)));
  return g2_lincomb(c, xy, inf, n, reinterpret_cast<const uint32_t*>(scalars), nullptr, nullptr, out_xy, out_inf);
}

int kzg_g2_lincomb_powers(kzg_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, const uint64_t s[4],
                          const uint64_t c0[4], uint64_t* out_xy, uint8_t* out_inf) {
  KZG_ENTER(!s || !c0 || !out_xy || !out_inf || (n && !xy));
  return g2_lincomb(c, xy, inf, n, nullptr, reinterpret_cast<const uint32_t*>(s), reinterpret_cast<const uint32_t*>(c0),
                    out_xy, out_inf);
}

int kzg_pairing_check(kzg_ctx* ctx, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy,
                      const uint8_t* g2_inf, size_t m, size_t k, uint8_t* out_status) {
  KZG_ENTER(m && (!g1_xy || !g2_xy || !out_status));
  return pairing_product(c, g1_xy, g1_inf, g2_xy, g2_inf, m, k, nullptr, out_status);
}

int kzg_pairing_product(kzg_ctx* ctx, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy,
                        const uint8_t* g2_inf, size_t m, size_t k, uint64_t* out_gt, uint8_t* out_status) {
  KZG_ENTER(m && (!g1_xy || !g2_xy || !out_gt || !out_status));
  return pairing_product(c, g1_xy, g1_inf, g2_xy, g2_inf, m, k, out_gt, out_status);
}

int kzg_pairing_gt_multiple(int curve) { return pairing_gt_multiple(curve); }

int kzg_blob_to_fr(kzg_ctx* ctx, uint32_t log_n, const uint8_t* blobs, size_t b, int bit_reversed, uint64_t* out_vals,
                   uint8_t* out_status) {
  KZG_ENTER(b && (!blobs || !out_vals || !out_status));
  return blob_to_fr(c, log_n, blobs, b, bit_reversed, out_vals, out_status);
}

int kzg_blob_to_fr_device(kzg_ctx* ctx, uint32_t log_n, const void* d_blobs, size_t b, int bit_reversed, void* d_vals,
                          void* d_status) {
  KZG_ENTER(b && (!d_blobs || !d_vals || !d_status));
  return blob_to_fr_device(c, log_n, d_blobs, b, bit_reversed, d_vals, d_status);
}

int kzg_fr_to_blob(kzg_ctx* ctx, uint32_t log_n, const uint64_t* vals, size_t b, int bit_reversed, uint8_t* out_bytes,
                   uint8_t* out_status) {
  KZG_ENTER(b && (!vals || !out_bytes || !out_status));
  return fr_to_blob(c, log_n, vals, b, bit_reversed, out_bytes, out_status);
}

int kzg_fr_to_blob_device(kzg_ctx* ctx, uint32_t log_n, const void* d_vals, size_t b, int bit_reversed, void* d_bytes,
                          void* d_status) {
  KZG_ENTER(b && (!d_vals || !d_bytes || !d_status));
  return fr_to_blob_device(c, log_n, d_vals, b, bit_reversed, d_bytes, d_status);
}

int kzg_blob_challenges(kzg_ctx* ctx, uint32_t log_n, const uint8_t* blobs, const uint8_t* commitments, size_t b,
                        uint64_t* out_z) {
  KZG_ENTER(b && (!blobs || !commitments || !out_z));
  return blob_challenges(c, log_n, blobs, commitments, b, out_z);
}

int kzg_blob_challenges_device(kzg_ctx* ctx, uint32_t log_n, const void* d_blobs, const void* d_commitments, size_t b,
                               void* d_z) {
  KZG_ENTER(b && (!d_blobs || !d_commitments || !d_z));
  return blob_challenges_device(c, log_n, d_blobs, d_commitments, b, d_z);
}

size_t kzg_srs_size(const kzg_srs* srs) { return srs ? srs->s->n : 0; }

void kzg_srs_free(kzg_srs* srs) {
  if (!srs) return;
  srs_free(srs->s);
  delete srs;
}

int kzg_commit_device(kzg_ctx* ctx, const kzg_srs* srs, const void* d_scalars, const size_t* lens, size_t n_polys,
                      size_t stride, uint64_t* out_xy, uint8_t* out_inf) {
  KZG_ENTER(!srs || !lens || !out_xy || !out_inf || (n_polys && !d_scalars));
  return commit_device(c, srs->s, static_cast<const uint32_t*>(d_scalars), lens, n_polys, stride, out_xy, out_inf);
}

int kzg_commit_device_async(kzg_ctx* ctx, const kzg_srs* srs, const void* d_scalars, const size_t* lens,
                            size_t n_polys, size_t stride, uint64_t* out_xy, uint8_t* out_inf) {
  KZG_ENTER(!srs || !lens || !out_xy || !out_inf || (n_polys && !d_scalars));
  return commit_device(c, srs->s, static_cast<const uint32_t*>(d_scalars), lens, n_polys, stride, out_xy, out_inf,
                       false);
}

int kzg_commit_flush(kzg_ctx* ctx) {
  KZG_ENTER(false);
  return commit_flush(c);
}

int kzg_commit(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* scalars, const size_t* lens, size_t n_polys,
               size_t stride, uint64_t* out_xy, uint8_t* out_inf) {
  KZG_ENTER(!srs || !lens || !out_xy || !out_inf || (n_polys && stride && !scalars));
  const size_t bytes = n_polys * stride * 32;
  int rc = ensure_buf(c, c->io, bytes ? bytes : 32);
  if (rc) return rc;
  // One polynomial at a time: the copy of polynomial p + 1 is ordered on the context's stream behind the prep of
  // polynomial p (which is all that reads p's scalars) and so travels while p is being accumulated.
  const size_t fpw = (c->curve == 0 ? Bn254::Fp::NW : Bls12_381::Fp::NW) / 2;   // 64-bit words per coordinate
  auto* io = static_cast<uint32_t*>(c->io.p);
  for (size_t p = 0; p < n_polys; ++p) {   // all arguments are checked before any work is queued
    if (lens[p] > srs->s->n) return set_err(c, KZG_ERR_DEGREE, "polynomial longer than the commitment key");
    if (lens[p] > stride) return set_err(c, KZG_ERR_ARG, "kzg_commit: lens[p] > stride");
  }
  for (size_t p = 0; p < n_polys && rc == KZG_OK; ++p) {
    if (lens[p])
      rc = KZG_HIP_RC(c, hipMemcpyAsync(io + p * stride * 8, scalars + p * stride * 4, lens[p] * 32,
                                        hipMemcpyHostToDevice, c->stream));
    if (rc == KZG_OK)
      rc = commit_device(c, srs->s, io + p * stride * 8, lens + p, 1, stride, out_xy + p * 2 * fpw, out_inf + p, false);
  }
  const int rc2 = commit_flush(c);                     // also on an error: nothing may point at out_xy / out_inf afterwards
  return rc ? rc : rc2;
}

int kzg_open_device(kzg_ctx* ctx, const kzg_srs* srs, const void* d_polys, const size_t* lens, size_t k,
                    size_t stride, const uint64_t z[4], const uint64_t xi[4], uint64_t* out_xy, uint8_t* out_inf,
                    uint64_t* eval_out) {
  KZG_ENTER(!srs || !z || !xi || !out_xy || !out_inf || (k && (!lens || !d_polys)));
  uint32_t* d_quot = nullptr;
  size_t qlen = 0;
  uint64_t ev[4];
  int rc = open_quotient_device(c, static_cast<const uint32_t*>(d_polys), lens, k, stride,
                                reinterpret_cast<const uint32_t*>(z), reinterpret_cast<const uint32_t*>(xi), &d_quot,
                                &qlen, ev);
  if (rc) return rc;
  if (eval_out) memcpy(eval_out, ev, 32);
  const size_t srs_n = srs->s->n;
  if (qlen > srs_n) {
    // The reference checks the DEGREE of the witness (kzg.py:103 via :157): coefficients
    // beyond the key are fine as long as they are zero.
    bool nz = false;
    rc = device_any_nonzero(c, d_quot, srs_n, qlen, &nz);
    if (rc) return rc;
    if (nz) return set_err(c, KZG_ERR_DEGREE, "witness polynomial longer than the commitment key");
    qlen = srs_n;
  }
  return commit_device(c, srs->s, d_quot, &qlen, 1, qlen ? qlen : 1, out_xy, out_inf);
}

int kzg_open_device_async(kzg_ctx* ctx, const kzg_srs* srs, const void* d_polys, const size_t* lens, size_t k,
                          size_t stride, const uint64_t z[4], const uint64_t xi[4], uint64_t* out_xy, uint8_t* out_inf,
                          uint64_t* eval_out) {
  KZG_ENTER(!srs || !z || !xi || !out_xy || !out_inf || !eval_out || (k && (!lens || !d_polys)));
  uint32_t* d_quot = nullptr;
  size_t qlen = 0;
  int rc = open_quotient_device(c, static_cast<const uint32_t*>(d_polys), lens, k, stride,
                                reinterpret_cast<const uint32_t*>(z), reinterpret_cast<const uint32_t*>(xi), &d_quot,
                                &qlen, eval_out, /*sync=*/false);
  if (rc) return rc;
  if (!d_quot) {   // every polynomial empty: witness 0, evaluation 0 (already in eval_out)
    memset(out_xy, 0, (size_t)kzg_fp_limbs(c->curve) * 16);
    *out_inf = 1;
    memset(eval_out, 0, 32);
    return KZG_OK;
  }
  const size_t srs_n = srs->s->n;
  if (qlen > srs_n) {   // rare: the degree check of kzg.py:103 needs the coefficients beyond the key, which synchronises
    bool nz = false;
    rc = device_any_nonzero(c, d_quot, srs_n, qlen, &nz);
    if (rc) return rc;
    if (nz) return set_err(c, KZG_ERR_DEGREE, "witness polynomial longer than the commitment key");
    qlen = srs_n;
  }
  // S_0 = combined(z) sits right below the quotient in the scan's buffer (poly.hip layout)
  return commit_device(c, srs->s, d_quot, &qlen, 1, qlen ? qlen : 1, out_xy, out_inf, /*drain=*/false, d_quot - 8,
                       eval_out);
}

int kzg_open(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* polys, const size_t* lens, size_t k, size_t stride,
             const uint64_t z[4], const uint64_t xi[4], uint64_t* out_xy, uint8_t* out_inf, uint64_t* eval_out) {
  KZG_ENTER(!srs || !z || !xi || !out_xy || !out_inf || (k && (!lens || !polys)));
  void* d = nullptr;
  if (int rc = stage_host(c, polys, k * stride * 32, &d)) return rc;
  return kzg_open_device(ctx, srs, d, lens, k, stride, z, xi, out_xy, out_inf, eval_out);
}

int kzg_open_points_device(kzg_ctx* ctx, const kzg_srs* srs, const void* d_polys, const size_t* lens, size_t k,
                           size_t stride, const uint64_t* points, size_t t, const uint64_t* weights, void* d_quot,
                           uint64_t* out_xy, uint8_t* out_inf) {
  KZG_ENTER(!srs || !out_xy || !out_inf || (k && (!lens || !d_polys)) || (t && !points) || (k && t && !weights));
  uint32_t* d_q = nullptr;
  size_t qlen = 0;
  int rc = open_points_quotient_device(c, static_cast<const uint32_t*>(d_polys), lens, k, stride,
                                       reinterpret_cast<const uint32_t*>(points), t,
                                       reinterpret_cast<const uint32_t*>(weights), &d_q, &qlen);
  if (rc) return rc;
  if (!d_q) {   // nothing but constants or empty polynomials: Q = 0
    memset(out_xy, 0, (size_t)kzg_fp_limbs(c->curve) * 16);
    *out_inf = 1;
    return KZG_OK;
  }
  if (d_quot) KZG_HIP(c, hipMemcpyAsync(d_quot, d_q, qlen * 32, hipMemcpyDeviceToDevice, c->stream));
  const size_t srs_n = srs->s->n;
  if (qlen > srs_n) {   // the degree of Q decides, as in kzg_open_device
    bool nz = false;
    rc = device_any_nonzero(c, d_q, srs_n, qlen, &nz);
    if (rc) return rc;
    if (nz) return set_err(c, KZG_ERR_DEGREE, "witness polynomial longer than the commitment key");
    qlen = srs_n;
  }
  return commit_device(c, srs->s, d_q, &qlen, 1, qlen ? qlen : 1, out_xy, out_inf);
}

int kzg_open_points(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* polys, const size_t* lens, size_t k,
                    size_t stride, const uint64_t* points, size_t t, const uint64_t* weights, void* d_quot,
                    uint64_t* out_xy, uint8_t* out_inf) {
  KZG_ENTER(!srs || !out_xy || !out_inf || (k && (!lens || !polys)));
  void* d = nullptr;
  if (int rc = stage_host(c, polys, k * stride * 32, &d)) return rc;
  return kzg_open_points_device(ctx, srs, d, lens, k, stride, points, t, weights, d_quot, out_xy, out_inf);
}

int kzg_open_shard_begin(kzg_ctx* ctx, const void* d_polys, const size_t* lens, size_t k, size_t stride,
                         const uint64_t z[4], const uint64_t xi[4], uint64_t* chunk_eval_out) {
  KZG_ENTER(!z || !xi || !chunk_eval_out || (k && (!lens || !d_polys)));
  return open_shard_begin_device(c, static_cast<const uint32_t*>(d_polys), lens, k, stride,
                                 reinterpret_cast<const uint32_t*>(z), reinterpret_cast<const uint32_t*>(xi),
                                 chunk_eval_out);
}

int kzg_open_shard_finish(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t z[4], const uint64_t carry[4],
                          int first_rank, uint64_t* out_xy, uint8_t* out_inf, uint64_t* eval_out) {
  KZG_ENTER(!srs || !z || !carry || !out_xy || !out_inf);
  uint32_t* d_vec = nullptr;
  size_t len = 0;
  uint64_t ev[4];
  int rc = open_shard_finish_device(c, reinterpret_cast<const uint32_t*>(z), reinterpret_cast<const uint32_t*>(carry),
                                    first_rank, &d_vec, &len, ev);
  if (rc) return rc;
  if (eval_out) memcpy(eval_out, ev, 32);
  if (len > srs->s->n) return set_err(c, KZG_ERR_DEGREE, "quotient slice longer than the key shard");
  return commit_device(c, srs->s, d_vec, &len, 1, len ? len : 1, out_xy, out_inf);
}

int kzg_srs_generate_lagrange(kzg_ctx* ctx, const uint64_t tau[4], uint32_t log_n, const uint64_t w[4],
                              kzg_srs** out) {
  KZG_ENTER(!tau || !w || !out);
  *out = nullptr;
  Srs* s = nullptr;
  const int rc = srs_generate_lagrange(c, reinterpret_cast<const uint32_t*>(tau), log_n, reinterpret_cast<const uint32_t*>(w),
                                 &s);
  return adopt_srs(rc, s, out);
}

int kzg_srs_lagrange(kzg_ctx* ctx, const kzg_srs* monomial, uint32_t log_n, const uint64_t w[4], kzg_srs** out) {
  KZG_ENTER(!monomial || !w || !out);
  *out = nullptr;
  Srs* s = nullptr;
  const int rc = srs_lagrange(c, monomial->s, log_n, reinterpret_cast<const uint32_t*>(w), &s);
  return adopt_srs(rc, s, out);
}

int kzg_open_evals_device(kzg_ctx* ctx, const kzg_srs* srs, const void* d_vals, const size_t* lens, size_t k,
                          size_t stride, const uint64_t z[4], const uint64_t xi[4], uint64_t* out_xy, uint8_t* out_inf,
                          uint64_t* eval_out) {
  KZG_ENTER(!srs || !z || !xi || !out_xy || !out_inf || (k && (!lens || !d_vals)));
  return open_evals_device(c, srs->s, static_cast<const uint32_t*>(d_vals), lens, k, stride,
                           reinterpret_cast<const uint32_t*>(z), reinterpret_cast<const uint32_t*>(xi), out_xy, out_inf,
                           eval_out, /*sync=*/true);
}

int kzg_open_evals_device_async(kzg_ctx* ctx, const kzg_srs* srs, const void* d_vals, const size_t* lens, size_t k,
                                size_t stride, const uint64_t z[4], const uint64_t xi[4], uint64_t* out_xy,
                                uint8_t* out_inf, uint64_t* eval_out) {
  KZG_ENTER(!srs || !z || !xi || !out_xy || !out_inf || !eval_out || (k && (!lens || !d_vals)));
  return open_evals_device(c, srs->s, static_cast<const uint32_t*>(d_vals), lens, k, stride,
                           reinterpret_cast<const uint32_t*>(z), reinterpret_cast<const uint32_t*>(xi), out_xy, out_inf,
                           eval_out, /*sync=*/false);
}

int kzg_open_evals(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* vals, const size_t* lens, size_t k, size_t stride,
                   const uint64_t z[4], const uint64_t xi[4], uint64_t* out_xy, uint8_t* out_inf, uint64_t* eval_out) {
  KZG_ENTER(!srs || !z || !xi || !out_xy || !out_inf || (k && (!lens || !vals)));
  void* d = nullptr;
  if (int rc = stage_host(c, vals, k * stride * 32, &d)) return rc;
  return kzg_open_evals_device(ctx, srs, d, lens, k, stride, z, xi, out_xy, out_inf, eval_out);
}

int kzg_domain_table_create(kzg_ctx* ctx, const kzg_srs* monomial, uint32_t log_n, kzg_domain_table** out) {
  KZG_ENTER(!monomial || !out);
  *out = nullptr;
  DomainTable* t = nullptr;
  int rc = domain_table_create(c, monomial->s, log_n, &t);
  if (rc) return rc;
  *out = new kzg_domain_table{t};
  return KZG_OK;
}

size_t kzg_domain_table_size(const kzg_domain_table* t) { return t ? domain_table_size(t->t) : 0; }

void kzg_domain_table_free(kzg_domain_table* t) {
  if (!t) return;
  domain_table_free(t->t);
  delete t;
}

int kzg_open_domain_device(kzg_ctx* ctx, const kzg_domain_table* t, const void* d_polys, const size_t* lens, size_t b,
                           size_t stride, const uint64_t w[4], uint64_t* out_xy, uint8_t* out_inf,
                           uint64_t* eval_out) {
  KZG_ENTER(!t || !w || (b && (!lens || !d_polys || !out_xy || !out_inf)));
  return open_domain(c, t->t, static_cast<const uint32_t*>(d_polys), /*host_polys=*/false, lens, b, stride,
                     reinterpret_cast<const uint32_t*>(w), out_xy, out_inf, eval_out);
}

int kzg_open_domain(kzg_ctx* ctx, const kzg_domain_table* t, const uint64_t* polys, const size_t* lens, size_t b,
                    size_t stride, const uint64_t w[4], uint64_t* out_xy, uint8_t* out_inf, uint64_t* eval_out) {
  KZG_ENTER(!t || !w || (b && (!lens || !polys || !out_xy || !out_inf)));
  return open_domain(c, t->t, reinterpret_cast<const uint32_t*>(polys), /*host_polys=*/true, lens, b, stride,
                     reinterpret_cast<const uint32_t*>(w), out_xy, out_inf, eval_out);
}

int kzg_coset_table_create(kzg_ctx* ctx, const kzg_srs* monomial, uint32_t log_n, uint32_t log_l,
                           kzg_domain_table** out) {
  KZG_ENTER(!monomial || !out);
  *out = nullptr;
  DomainTable* t = nullptr;
  int rc = coset_table_create(c, monomial->s, log_n, log_l, &t);
  if (rc) return rc;
  *out = new kzg_domain_table{t};
  return KZG_OK;
}

int kzg_open_cosets_device(kzg_ctx* ctx, const kzg_domain_table* t, const void* d_polys, const size_t* lens, size_t b,
                           size_t stride, uint32_t log_N, const uint64_t w[4], uint64_t* out_xy, uint8_t* out_inf,
                           uint64_t* eval_out) {
  KZG_ENTER(!t || !w || (b && (!lens || !d_polys || !out_xy || !out_inf)));
  return open_cosets(c, t->t, static_cast<const uint32_t*>(d_polys), /*host_polys=*/false, lens, b, stride, log_N,
                     reinterpret_cast<const uint32_t*>(w), out_xy, out_inf, eval_out);
}

int kzg_open_cosets(kzg_ctx* ctx, const kzg_domain_table* t, const uint64_t* polys, const size_t* lens, size_t b,
                    size_t stride, uint32_t log_N, const uint64_t w[4], uint64_t* out_xy, uint8_t* out_inf,
                    uint64_t* eval_out) {
  KZG_ENTER(!t || !w || (b && (!lens || !polys || !out_xy || !out_inf)));
  return open_cosets(c, t->t, reinterpret_cast<const uint32_t*>(polys), /*host_polys=*/true, lens, b, stride, log_N,
                     reinterpret_cast<const uint32_t*>(w), out_xy, out_inf, eval_out);
}

int kzg_open_coset_device(kzg_ctx* ctx, const kzg_srs* srs, const void* d_polys, const size_t* lens, size_t k,
                          size_t stride, uint32_t log_l, const uint64_t h[4], const uint64_t zeta[4],
                          const uint64_t xi[4], uint64_t* out_xy, uint8_t* out_inf, uint64_t* eval_out) {
  KZG_ENTER(!srs || !h || !zeta || !xi || !out_xy || !out_inf || (k && (!lens || !d_polys)));
  if (srs->s->curve != c->curve) return set_err(c, KZG_ERR_ARG, "SRS belongs to another curve");
  if (srs->s->basis != SRS_MONOMIAL) return set_err(c, KZG_ERR_ARG, "kzg_open_coset: the key must be monomial");
  uint32_t* d_quot = nullptr;
  size_t qlen = 0;
  int rc = open_coset_quotient_device(c, static_cast<const uint32_t*>(d_polys), lens, k, stride, log_l,
                                      reinterpret_cast<const uint32_t*>(h), reinterpret_cast<const uint32_t*>(zeta),
                                      reinterpret_cast<const uint32_t*>(xi), srs->s->n, &d_quot, &qlen, eval_out);
  if (rc) return rc;
  return commit_device(c, srs->s, d_quot, &qlen, 1, qlen ? qlen : 1, out_xy, out_inf);
}

int kzg_open_coset(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* polys, const size_t* lens, size_t k,
                   size_t stride, uint32_t log_l, const uint64_t h[4], const uint64_t zeta[4], const uint64_t xi[4],
                   uint64_t* out_xy, uint8_t* out_inf, uint64_t* eval_out) {
  KZG_ENTER(!srs || !h || !zeta || !xi || !out_xy || !out_inf || (k && (!lens || !polys)));
  if (srs->s->curve != c->curve) return set_err(c, KZG_ERR_ARG, "SRS belongs to another curve");
  if (srs->s->basis != SRS_MONOMIAL) return set_err(c, KZG_ERR_ARG, "kzg_open_coset: the key must be monomial");
  int rc = open_coset_check(c, lens, k, stride, log_l, reinterpret_cast<const uint32_t*>(h),
                            reinterpret_cast<const uint32_t*>(zeta), srs->s->n);     // before anything is queued
  if (rc) return rc;
  void* d = nullptr;
  if ((rc = stage_host(c, polys, k * stride * 32, &d))) return rc;
  return kzg_open_coset_device(ctx, srs, d, lens, k, stride, log_l, h, zeta, xi, out_xy, out_inf, eval_out);
}

int kzg_verify_cosets(kzg_ctx* ctx, const kzg_srs* monomial, uint32_t log_N, uint32_t log_l, const uint64_t w[4],
                      const uint64_t* comm_xy, const uint8_t* comm_inf, size_t n_comm, const uint32_t* comm_idx,
                      const uint32_t* coset_idx, const uint64_t* values, const uint64_t* proof_xy,
                      const uint8_t* proof_inf, size_t K, const uint64_t rho[4], uint64_t* out_xy, uint8_t* out_inf) {
  KZG_ENTER(!monomial || !w || !rho || !out_xy || !out_inf || !comm_xy || (K && (!comm_idx || !coset_idx ||
            !values || !proof_xy)));
  return verify_cosets(c, monomial->s, log_N, log_l, reinterpret_cast<const uint32_t*>(w), comm_xy, comm_inf, n_comm,
                       comm_idx, coset_idx, values, proof_xy, proof_inf, K, reinterpret_cast<const uint32_t*>(rho),
                       out_xy, out_inf);
}

int kzg_verify_cosets_bytes(kzg_ctx* ctx, const kzg_srs* monomial, uint32_t log_N, uint32_t log_l, const uint64_t w[4],
                            const uint64_t* comm_xy, const uint8_t* comm_inf, size_t n_comm, const uint32_t* comm_idx,
                            const uint32_t* coset_idx, const uint8_t* cells, int bit_reversed, const uint64_t* proof_xy,
                            const uint8_t* proof_inf, size_t K, const uint64_t rho[4], uint64_t* out_xy,
                            uint8_t* out_inf, uint8_t* out_status) {
  KZG_ENTER(!monomial || !w || !rho || !out_xy || !out_inf || !out_status || !comm_xy || (K && (!comm_idx ||
            !coset_idx || !cells || !proof_xy)));
  return verify_cosets_bytes(c, monomial->s, log_N, log_l, reinterpret_cast<const uint32_t*>(w), comm_xy, comm_inf,
                             n_comm, comm_idx, coset_idx, cells, bit_reversed, proof_xy, proof_inf, K,
                             reinterpret_cast<const uint32_t*>(rho), out_xy, out_inf, out_status);
}

int kzg_verify_points(kzg_ctx* ctx, const uint64_t* comm_xy, const uint8_t* comm_inf, size_t n_comm,
                      const uint32_t* comm_idx, const uint64_t* z, const uint64_t* y, const uint64_t* proof_xy,
                      const uint8_t* proof_inf, size_t K, const uint64_t rho[4], uint64_t* out_xy, uint8_t* out_inf) {
  KZG_ENTER(!rho || !out_xy || !out_inf || !comm_xy || (K && (!comm_idx || !z || !y || !proof_xy)));
  return verify_points(c, comm_xy, comm_inf, n_comm, comm_idx, z, y, proof_xy, proof_inf, K,
                       reinterpret_cast<const uint32_t*>(rho), out_xy, out_inf);
}

int kzg_recover_cosets(kzg_ctx* ctx, uint32_t log_n, uint32_t log_N, uint32_t log_l, const uint64_t w[4],
                       const uint32_t* coset_idx, size_t K, const uint64_t* values, size_t b, uint64_t* out_coeffs,
                       uint8_t* out_consistent) {
  KZG_ENTER(!w || !coset_idx || !values || !out_coeffs || !out_consistent);
  return recover_cosets(c, log_n, log_N, log_l, reinterpret_cast<const uint32_t*>(w), coset_idx, K,
                        reinterpret_cast<const uint32_t*>(values), /*host_ptrs=*/true, b,
                        reinterpret_cast<uint32_t*>(out_coeffs), out_consistent);
}

int kzg_recover_cosets_device(kzg_ctx* ctx, uint32_t log_n, uint32_t log_N, uint32_t log_l, const uint64_t w[4],
                              const uint32_t* coset_idx, size_t K, const void* d_values, size_t b, void* d_coeffs,
                              uint8_t* out_consistent) {
  KZG_ENTER(!w || !coset_idx || !d_values || !d_coeffs || !out_consistent);
  return recover_cosets(c, log_n, log_N, log_l, reinterpret_cast<const uint32_t*>(w), coset_idx, K,
                        static_cast<const uint32_t*>(d_values), /*host_ptrs=*/false, b,
                        static_cast<uint32_t*>(d_coeffs), out_consistent);
}

// The vector primitives select the device first and check their arguments then.
int kzg_fr_vec_op(kzg_ctx* ctx, int op, size_t n, const void* d_a, const void* d_b, void* d_out) {
  KZG_ENTER(false);
  if (op < 0 || op > 2 || (n && (!d_a || !d_b || !d_out))) return KZG_ERR_ARG;
  return fr_vec_binary(c, op, n, static_cast<const uint32_t*>(d_a), static_cast<const uint32_t*>(d_b),
                       static_cast<uint32_t*>(d_out));
}

int kzg_fr_vec_lincomb(kzg_ctx* ctx, size_t n, size_t k, const void* const* d_ptrs, const size_t* lens,
                       const uint64_t* scalars, void* d_out) {
  KZG_ENTER(false);
  if (k && (!d_ptrs || !lens || !scalars)) return KZG_ERR_ARG;
  if (n && !d_out) return KZG_ERR_ARG;
  return fr_vec_lincomb(c, n, k, reinterpret_cast<const uint32_t* const*>(d_ptrs), lens,
                        reinterpret_cast<const uint32_t*>(scalars), static_cast<uint32_t*>(d_out));
}

int kzg_fr_vec_mul_powers(kzg_ctx* ctx, size_t n, const void* d_a, const uint64_t s[4], const uint64_t c0[4],
                          void* d_out) {
  KZG_ENTER(false);
  if (!s || !c0 || (n && (!d_a || !d_out))) return KZG_ERR_ARG;
  return fr_vec_mul_powers(c, n, static_cast<const uint32_t*>(d_a), reinterpret_cast<const uint32_t*>(s),
                           reinterpret_cast<const uint32_t*>(c0), static_cast<uint32_t*>(d_out));
}

int kzg_fr_vec_inverse(kzg_ctx* ctx, size_t n, const void* d_a, void* d_out) {
  KZG_ENTER(false);
  if (n && (!d_a || !d_out)) return KZG_ERR_ARG;
  return fr_vec_inverse(c, n, static_cast<const uint32_t*>(d_a), static_cast<uint32_t*>(d_out));
}

int kzg_fr_vec_prefix_product(kzg_ctx* ctx, size_t n, const void* d_a, void* d_out) {
  KZG_ENTER(false);
  if (n && (!d_a || !d_out)) return KZG_ERR_ARG;
  return fr_vec_prefix_product(c, n, static_cast<const uint32_t*>(d_a), static_cast<uint32_t*>(d_out));
}

int kzg_fr_poly_eval(kzg_ctx* ctx, size_t n, const void* d_a, const uint64_t z[4], uint64_t out[4]) {
  KZG_ENTER(false);
  if (!z || !out || (n && !d_a)) return KZG_ERR_ARG;
  return fr_poly_eval(c, n, static_cast<const uint32_t*>(d_a), reinterpret_cast<const uint32_t*>(z), out);
}

int kzg_fr_poly_eval_batch(kzg_ctx* ctx, const void* d_polys, const size_t* lens, size_t k, size_t stride,
                           const uint64_t* points, size_t t, uint64_t* out) {
  KZG_ENTER(false);
  if (k && t && (!d_polys || !lens || !points || !out)) return KZG_ERR_ARG;
  return fr_poly_eval_batch(c, static_cast<const uint32_t*>(d_polys), lens, k, stride,
                            reinterpret_cast<const uint32_t*>(points), t, out);
}

int kzg_fr_eval_lagrange(kzg_ctx* ctx, uint32_t log_n, const uint64_t w[4], size_t len, const void* d_vals,
                         const uint64_t z[4], uint64_t out[4]) {
  KZG_ENTER(false);
  if (!w || !z || !out || (len && !d_vals)) return KZG_ERR_ARG;
  return fr_eval_lagrange(c, log_n, reinterpret_cast<const uint32_t*>(w), len, static_cast<const uint32_t*>(d_vals),
                          reinterpret_cast<const uint32_t*>(z), out);
}

int kzg_fr_eval_lagrange_batch_device(kzg_ctx* ctx, uint32_t log_n, const uint64_t w[4], const void* d_vals,
                                      const size_t* lens, size_t b, size_t stride, const void* d_z, void* d_out) {
  KZG_ENTER(false);
  if (!w || (b && (!d_vals || !lens || !d_z || !d_out))) return KZG_ERR_ARG;
  return fr_eval_lagrange_batch(c, log_n, reinterpret_cast<const uint32_t*>(w), static_cast<const uint32_t*>(d_vals),
                                lens, b, stride, static_cast<const uint32_t*>(d_z), static_cast<uint32_t*>(d_out));
}

int kzg_fr_eval_lagrange_batch(kzg_ctx* ctx, uint32_t log_n, const uint64_t w[4], const uint64_t* vals,
                               const size_t* lens, size_t b, size_t stride, const uint64_t* z, uint64_t* out) {
  KZG_ENTER(false);
  if (!w || (b && (!vals || !lens || !z || !out))) return KZG_ERR_ARG;
  if (b == 0) return KZG_OK;
  if (stride == 0 || b > ((size_t)1 << 40) / stride) return set_err(c, KZG_ERR_ARG, "kzg_fr_eval_lagrange_batch: b * stride too large");
  // staged as [values | points | results]
  const size_t vb = b * stride * 32, zb = b * 32;
  int rc = ensure_buf(c, c->io, vb + 2 * zb);
  if (rc) return rc;
  char* d = static_cast<char*>(c->io.p);
  KZG_HIP(c, hipMemcpyAsync(d, vals, vb, hipMemcpyHostToDevice, c->stream));
  KZG_HIP(c, hipMemcpyAsync(d + vb, z, zb, hipMemcpyHostToDevice, c->stream));
  rc = kzg_fr_eval_lagrange_batch_device(ctx, log_n, w, d, lens, b, stride, d + vb, d + vb + zb);
  if (rc) return rc;
  KZG_HIP(c, hipMemcpyAsync(out, d + vb + zb, zb, hipMemcpyDeviceToHost, c->stream));
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  return KZG_OK;
}

int kzg_prof_enable(kzg_ctx* ctx, int on) {
  if (!ctx) return KZG_ERR_ARG;
  Ctx* c = &ctx->c;
  if (on && !c->clk_probe) {
    KZG_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->clk_probe), CLK_WORDS * 8));
    KZG_HIP(c, hipMemset(c->clk_probe, 0, CLK_WORDS * 8));
  }
  c->prof_on = on != 0;
  return KZG_OK;
}

int kzg_prof_reset(kzg_ctx* ctx) {
  if (!ctx) return KZG_ERR_ARG;
  Ctx* c = &ctx->c;
  KZG_HIP(c, hipDeviceSynchronize());
  for (auto& sp : c->prof) {
    for (auto& pr : sp.pending) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
    sp.pending.clear();
    sp.total_ms = 0;
    sp.count = 0;
  }
  if (c->clk_probe) KZG_HIP(c, hipMemset(c->clk_probe, 0, CLK_WORDS * 8));
  return KZG_OK;
}

int kzg_prof_read(kzg_ctx* ctx, const char* name, double* total_ms, uint64_t* count) {
  if (!ctx || !name || !total_ms || !count) return KZG_ERR_ARG;
  Ctx* c = &ctx->c;
  KZG_HIP(c, hipDeviceSynchronize());
  *total_ms = 0;
  *count = 0;
  const bool acc_clk = std::string(name) == "msm_accumulate_shader_mhz", ntt_clk = std::string(name) == "ntt_pass_shader_mhz";
  if (std::string(name) == "verify_device_bytes") {   // not a span: device memory the last kzg_verify_cosets asked for
    *total_ms = (double)c->ver_last_bytes;
    *count = c->ver_last_bytes ? 1 : 0;
    return KZG_OK;
  }
  if (std::string(name) == "verify_points_device_bytes") {   // not a span: what the last kzg_verify_points carved out
    *total_ms = (double)c->vpt_last_bytes;
    *count = c->vpt_last_bytes ? 1 : 0;
    return KZG_OK;
  }
  if (std::string(name) == "recover_leaf") {   // not a span: linear factors per leaf of kzg_recover_cosets' product tree
    *total_ms = (double)recover_leaf_width();
    *count = 1;
    return KZG_OK;
  }
  if (std::string(name) == "ntt_tile_log") {   // not a span: log2 of the LDS tile the last transform took
    *total_ms = (double)c->last_ntt_tile_log;
    *count = c->last_ntt_tile_log ? 1 : 0;
    return KZG_OK;
  }
  const bool acc_tail = std::string(name) == "msm_accumulate_tail_us", acc_spread = std::string(name) == "msm_accumulate_exit_spread_us";
  if (acc_tail || acc_spread) {   // not a span: when the waves of msm_accumulate left, microseconds per launch
    unsigned long long t[CLK_WORDS] = {0};
    if (c->clk_probe) KZG_HIP(c, hipMemcpy(t, c->clk_probe, sizeof(t), hipMemcpyDeviceToHost));
    const unsigned long long waves = t[CLK_ACC_WAVES], launches = t[CLK_ACC_LAUNCHES];
    if (launches && waves) {                                    // launches of one grid size
      // sums of 100 MHz ticks, formed modulo 2^64: the differences are small and exact
      const unsigned long long ticks = acc_tail ? (waves * t[CLK_ACC_EXIT_LAST] - t[CLK_ACC_EXIT_SUM]) / waves   // last - mean
                                                : t[CLK_ACC_EXIT_LAST] - t[CLK_ACC_EXIT_FIRST];                  // last - first
      *total_ms = (double)ticks / 100.0 / (double)launches;
      *count = launches;
    }
    return KZG_OK;
  }
  if (acc_clk || ntt_clk) {   // not a span: the shader clock (MHz) the kernel's probing wave ran at
    unsigned long long t[4] = {0, 0, 0, 0};
    if (c->clk_probe) KZG_HIP(c, hipMemcpy(t, c->clk_probe, 32, hipMemcpyDeviceToHost));
    const unsigned long long* q = t + (ntt_clk ? 2 : 0);
    if (q[1]) { *total_ms = 100.0 * (double)q[0] / (double)q[1]; *count = 1; }
    return KZG_OK;
  }
  for (auto& sp : c->prof) {
    if (sp.name != name) continue;
    for (auto& pr : sp.pending) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) { sp.total_ms += ms; sp.count += 1; }
      hipEventDestroy(pr.first);
      hipEventDestroy(pr.second);
    }
    sp.pending.clear();
    *total_ms = sp.total_ms;
    *count = sp.count;
    return KZG_OK;
  }
  return KZG_OK;
}

}  // extern "C"
