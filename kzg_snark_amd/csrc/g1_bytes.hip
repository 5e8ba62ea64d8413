// g1_bytes.hip -- compressed G1 points and subgroup checks on the device: three kernels, one lane per
// point, around the single-point functions of g1_bytes.h, and the host drivers behind kzg_g1_compress,
// kzg_g1_decompress*, kzg_g1_check_subgroup, kzg_srs_load_g1_compressed and kzg_srs_export_compressed.
//
// Every lane of a kernel runs the same fixed exponent ((p+1)/4) or the same fixed scalar (|u|, twice), so the loops
// are uniform; lanes differ only where a point is infinity, malformed or outside the subgroup.  Points move as 16-byte
// vector accesses (a blob is 3 or 2 of them, an affine point 6 or 4), statuses and flags as per-lane byte stores.
#include "internal.h"
#include "msm.h"
#include "g1_util.h"
#include "srs_rec.h"
#include "g1_bytes.h"
#include <string>
#include <vector>

namespace kzg {

namespace {

constexpr size_t G1_MAX_POINTS = (size_t)1 << 24;

// blobs -> canonical affine words, infinity flags, statuses 0 / 1 / 2 (the subgroup is g1_subgroup_kernel's)
template <class C>
__global__ __launch_bounds__(256) void g1_decompress_kernel(const uint32_t* bytes, size_t n, uint32_t* xy, uint8_t* inf,
                                                            uint8_t* status) {
  using G = G1Bytes<C>;
  constexpr int NW = G::NW;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t raw[NW], w[2 * NW];
  ld_words<NW>(bytes + i * NW, raw);
  bool is_inf = false;
  const int st = G::decode(raw, false, w, w + NW, is_inf);
  st_words<2 * NW>(xy + i * 2 * NW, w);
  inf[i] = is_inf ? 1 : 0;
  status[i] = (uint8_t)st;
}

// affine points -> statuses.  after_decode = 0: every finite point is validated (a coordinate >= p or off the curve:
// 2) and tested (3).  after_decode != 0: the second half of a checked decompression -- only lanes whose status is
// still 0 are tested, and a point that fails is wiped (zeros) as every failed decompression is.
template <class C>
__global__ __launch_bounds__(256) void g1_subgroup_kernel(uint32_t* xy, const uint8_t* inf, size_t n, uint8_t* status,
                                                          int after_decode) {
  using G = G1Bytes<C>;
  constexpr int NW = G::NW;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (after_decode && status[i] != 0) return;
  const bool is_inf = inf && inf[i];
  int st = G1_OK;
  if (!is_inf) {
    uint32_t w[2 * NW];
    ld_words<2 * NW>(xy + i * 2 * NW, w);
    st = G::check_affine(w, w + NW, false);
  }
  status[i] = (uint8_t)st;
  if (after_decode && st != G1_OK) {
    uint32_t z[2 * NW];
#pragma unroll
    for (int k = 0; k < 2 * NW; ++k) z[k] = 0;
    st_words<2 * NW>(xy + i * 2 * NW, z);
  }
}

// affine points -> blobs.  recs == nullptr: canonical words (xy, inf), validated by g1_words.h's import_affine (a
// coordinate >= p or a point off the curve is counted in *bad).  Otherwise the window-0 records start .. start + n - 1
// of a key (Montgomery form, canonical; nothing to validate).
template <class C>
__global__ __launch_bounds__(256) void g1_compress_kernel(const uint32_t* xy, const uint8_t* inf, const uint32_t* recs,
                                                          size_t start, size_t n, uint32_t* bytes, uint32_t* bad) {
  using G = G1Bytes<C>;
  constexpr int NW = G::NW;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[2 * NW], raw[NW];
  bool is_inf;
  Affine<C> a;
  if (recs) {
    a.inf = load_rec<C>(recs, start + i, a.x, a.y) & 1u;
    is_inf = affine_to_words<C>(a, w);
  } else {
    is_inf = inf && inf[i];
    ld_words<2 * NW>(xy + i * 2 * NW, w);
    if (!is_inf && !import_affine<C>(w, w + NW, a.x, a.y)) atomicAdd(bad, 1u);
  }
  G::encode(w, w + NW, is_inf, raw);
  st_words<NW>(bytes + i * NW, raw);
}

inline uint32_t blocks_of(size_t n) { return (uint32_t)((n + 255) / 256); }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

const char* status_text(int st) {
  return st == G1_BAD_ENCODING ? "bad encoding" : st == G1_NOT_ON_CURVE ? "x^3 + b is not a square" :
         st == G1_NOT_IN_SUBGROUP ? "outside the prime-order subgroup" : "ok";
}

// the two launches of a decompression on device buffers; enqueue only
template <class C>
int decompress_launch(Ctx* c, const uint32_t* d_bytes, size_t n, int check_subgroup, uint32_t* d_xy, uint8_t* d_inf,
                      uint8_t* d_status) {
  hipLaunchKernelGGL(g1_decompress_kernel<C>, dim3(blocks_of(n)), dim3(256), 0, c->stream, d_bytes, n, d_xy, d_inf,
                     d_status);
  KZG_HIP(c, hipGetLastError());
  if (check_subgroup && G1Bytes<C>::ZCASH) {        // BN254: cofactor 1, a decoded point is in the subgroup
    hipLaunchKernelGGL(g1_subgroup_kernel<C>, dim3(blocks_of(n)), dim3(256), 0, c->stream, d_xy, d_inf, n, d_status, 1);
    KZG_HIP(c, hipGetLastError());
  }
  return KZG_OK;
}

// the staging buffer of the host-pointer entry points, carved: blobs | affine words | flags | statuses
struct Stage {
  uint32_t* bytes; uint32_t* xy; uint8_t* inf; uint8_t* status; uint32_t* bad;
};
template <class C>
int stage(Ctx* c, size_t n, Stage* s) {
  constexpr size_t SIZE = G1Bytes<C>::SIZE;
  return carve(c, c->io, [&](Carve& ws) {
    s->bytes = ws.take(n * SIZE);
    s->xy = ws.take(n * 2 * SIZE);
    s->inf = ws.take<uint8_t>(n);
    s->status = ws.take<uint8_t>(n);
    s->bad = ws.take(4);
  });
}

template <class C>
int compress_t(Ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out) {
  constexpr size_t SIZE = G1Bytes<C>::SIZE;
  Stage s;
  int rc = stage<C>(c, n, &s);
  if (rc) return rc;
  KZG_HIP(c, hipMemcpyAsync(s.xy, xy, n * 2 * SIZE, hipMemcpyHostToDevice, c->stream));
  if (inf) KZG_HIP(c, hipMemcpyAsync(s.inf, inf, n, hipMemcpyHostToDevice, c->stream));
  KZG_HIP(c, hipMemsetAsync(s.bad, 0, 4, c->stream));
  hipLaunchKernelGGL(g1_compress_kernel<C>, dim3(blocks_of(n)), dim3(256), 0, c->stream, s.xy,
                     inf ? s.inf : (const uint8_t*)nullptr, (const uint32_t*)nullptr, (size_t)0, n, s.bytes, s.bad);
  KZG_HIP(c, hipGetLastError());
  uint32_t bad = 0;
  KZG_HIP(c, hipMemcpyAsync(&bad, s.bad, 4, hipMemcpyDeviceToHost, c->stream));
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  if (bad) return set_err(c, KZG_ERR_ARG, "kzg_g1_compress: a coordinate >= p or a point not on the curve");
  KZG_HIP(c, hipMemcpyAsync(out, s.bytes, n * SIZE, hipMemcpyDeviceToHost, c->stream));
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  return KZG_OK;
}

template <class C>
int decompress_t(Ctx* c, const uint8_t* bytes, size_t n, int check_subgroup, uint64_t* out_xy, uint8_t* out_inf,
                 uint8_t* out_status) {
  constexpr size_t SIZE = G1Bytes<C>::SIZE;
  Stage s;
  int rc = stage<C>(c, n, &s);
  if (rc) return rc;
  {
    ProfScope span(c, "g1_decompress");
    KZG_HIP(c, hipMemcpyAsync(s.bytes, bytes, n * SIZE, hipMemcpyHostToDevice, c->stream));
    if ((rc = decompress_launch<C>(c, s.bytes, n, check_subgroup, s.xy, s.inf, s.status))) return rc;
    KZG_HIP(c, hipMemcpyAsync(out_xy, s.xy, n * 2 * SIZE, hipMemcpyDeviceToHost, c->stream));
    KZG_HIP(c, hipMemcpyAsync(out_inf, s.inf, n, hipMemcpyDeviceToHost, c->stream));
    KZG_HIP(c, hipMemcpyAsync(out_status, s.status, n, hipMemcpyDeviceToHost, c->stream));
  }
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  return KZG_OK;
}

template <class C>
int check_subgroup_t(Ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out_status) {
  constexpr size_t SIZE = G1Bytes<C>::SIZE;
  Stage s;
  int rc = stage<C>(c, n, &s);
  if (rc) return rc;
  {
    ProfScope span(c, "g1_subgroup");
    KZG_HIP(c, hipMemcpyAsync(s.xy, xy, n * 2 * SIZE, hipMemcpyHostToDevice, c->stream));
    if (inf) KZG_HIP(c, hipMemcpyAsync(s.inf, inf, n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(g1_subgroup_kernel<C>, dim3(blocks_of(n)), dim3(256), 0, c->stream, s.xy,
                       inf ? s.inf : (const uint8_t*)nullptr, n, s.status, 0);
    KZG_HIP(c, hipGetLastError());
    KZG_HIP(c, hipMemcpyAsync(out_status, s.status, n, hipMemcpyDeviceToHost, c->stream));
  }
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  return KZG_OK;
}

template <class C>
int load_compressed_t(Ctx* c, const uint8_t* bytes, size_t n, int check_subgroup, Srs** out) {
  constexpr size_t SIZE = G1Bytes<C>::SIZE;
  Stage s;
  int rc = stage<C>(c, n, &s);
  if (rc) return rc;
  std::vector<uint8_t> status(n);
  {
    ProfScope span(c, "g1_decompress");
    KZG_HIP(c, hipMemcpyAsync(s.bytes, bytes, n * SIZE, hipMemcpyHostToDevice, c->stream));
    if ((rc = decompress_launch<C>(c, s.bytes, n, check_subgroup, s.xy, s.inf, s.status))) return rc;
    KZG_HIP(c, hipMemcpyAsync(status.data(), s.status, n, hipMemcpyDeviceToHost, c->stream));
  }
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < n; ++i) {
    if (status[i] == G1_OK) continue;
    const std::string msg = "kzg_srs_load_g1_compressed: point " + std::to_string(i) + " has status " +
                            std::to_string((int)status[i]) + " (" + status_text(status[i]) + ")";
    return set_err(c, KZG_ERR_ARG, msg.c_str());
  }
  // the decoded points stay where they are: the key's expansion reads them from the staging buffer
  return srs_load_device(c, s.xy, s.inf, n, out);
}

template <class C>
int export_compressed_t(Ctx* c, const Srs* s, size_t start, size_t count, uint8_t* out) {
  constexpr size_t SIZE = G1Bytes<C>::SIZE;
  Stage st;
  int rc = stage<C>(c, count, &st);
  if (rc) return rc;
  hipLaunchKernelGGL(g1_compress_kernel<C>, dim3(blocks_of(count)), dim3(256), 0, c->stream, (const uint32_t*)nullptr,
                     (const uint8_t*)nullptr, (const uint32_t*)s->recs, start, count, st.bytes, (uint32_t*)nullptr);
  KZG_HIP(c, hipGetLastError());
  KZG_HIP(c, hipMemcpyAsync(out, st.bytes, count * SIZE, hipMemcpyDeviceToHost, c->stream));
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  return KZG_OK;
}

}  // namespace

static int size_check(Ctx* c, size_t n, const char* who) {
  if (n > G1_MAX_POINTS) {
    const std::string msg = std::string(who) + ": more than 2^24 points";
    return set_err(c, KZG_ERR_ARG, msg.c_str());
  }
  return KZG_OK;
}

int g1_compress(Ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out_bytes) {
  if (n == 0) return KZG_OK;
  if (int rc = size_check(c, n, "kzg_g1_compress")) return rc;
  return KZG_BY_CURVE(c, compress_t, c, xy, inf, n, out_bytes);
}
int g1_decompress(Ctx* c, const uint8_t* bytes, size_t n, int check_subgroup, uint64_t* out_xy, uint8_t* out_inf,
                  uint8_t* out_status) {
  if (n == 0) return KZG_OK;
  if (int rc = size_check(c, n, "kzg_g1_decompress")) return rc;
  return KZG_BY_CURVE(c, decompress_t, c, bytes, n, check_subgroup, out_xy, out_inf, out_status);
}
int g1_decompress_device(Ctx* c, const void* d_bytes, size_t n, int check_subgroup, void* d_xy, void* d_inf,
                         void* d_status) {
  if (n == 0) return KZG_OK;
  if (int rc = size_check(c, n, "kzg_g1_decompress_device")) return rc;
  if (!aligned16(d_bytes) || !aligned16(d_xy))
    return set_err(c, KZG_ERR_ARG, "kzg_g1_decompress_device: misaligned device pointer");
  ProfScope span(c, "g1_decompress");
  return KZG_BY_CURVE(c, decompress_launch, c, static_cast<const uint32_t*>(d_bytes), n, check_subgroup,
                     static_cast<uint32_t*>(d_xy), static_cast<uint8_t*>(d_inf), static_cast<uint8_t*>(d_status));
}
int g1_check_subgroup(Ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out_status) {
  if (n == 0) return KZG_OK;
  if (int rc = size_check(c, n, "kzg_g1_check_subgroup")) return rc;
  return KZG_BY_CURVE(c, check_subgroup_t, c, xy, inf, n, out_status);
}
int srs_load_g1_compressed(Ctx* c, const uint8_t* bytes, size_t n, int check_subgroup, Srs** out) {
  if (n == 0) return set_err(c, KZG_ERR_ARG, "kzg_srs_load_g1_compressed: bad size");
  if (int rc = size_check(c, n, "kzg_srs_load_g1_compressed")) return rc;
  return KZG_BY_CURVE(c, load_compressed_t, c, bytes, n, check_subgroup, out);
}
int srs_export_compressed(Ctx* c, const Srs* s, size_t start, size_t count, uint8_t* out_bytes) {
  if (start > s->n || count > s->n - start) return set_err(c, KZG_ERR_ARG, "kzg_srs_export_compressed: range");
  if (count == 0) return KZG_OK;
  if (int rc = size_check(c, count, "kzg_srs_export_compressed")) return rc;
  return KZG_BY_CURVE(c, export_compressed_t, c, s, start, count, out_bytes);
}

}  // namespace kzg
