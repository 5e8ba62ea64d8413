// g2_bytes.hip -- compressed G2 points and subgroup checks on the device: three kernels, one lane per
// point, around the single-point functions of g2_bytes.h, and the host drivers behind kzg_g2_compress,
// kzg_g2_decompress* and kzg_g2_check_subgroup.
//
// Every lane runs the same fixed exponents (the three powers of the square root in Fp2) or the same fixed scalar (|u|,
// then the closing additions of the subgroup test), so the loops are uniform; lanes differ only where a point is
// infinity, malformed, of small order or outside the subgroup.  G2 counts are small (tens to thousands: verification
// keys, the G2 powers of a trusted setup), so the kernels are laid out for registers, not occupancy: a workgroup is one
// wave, every kernel may use the whole register file (512 VGPRs and AGPRs per lane) and none touches scratch memory.
// Points move as 16-byte vector accesses (a blob is 6 or 4 of them, an affine point 12 or 8), statuses and flags as
// per-lane byte stores.
#include "internal.h"
#include "msm.h"
#include "g1_util.h"
#include "g2_bytes.h"
#include <string>

namespace kzg {

namespace {

constexpr size_t G2_MAX_POINTS = (size_t)1 << 24;
constexpr int G2_LANES = 64;

// blobs -> canonical affine words, infinity flags, statuses 0 / 1 / 2 (the subgroup is g2_subgroup_kernel's)
template <class C>
__global__ __launch_bounds__(G2_LANES) void g2_decompress_kernel(const uint32_t* bytes, size_t n, uint32_t* xy,
                                                                 uint8_t* inf, uint8_t* status) {
  using G = G2Bytes<C>;
  constexpr int NW = G::NW;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t raw[2 * NW], w[4 * NW];
  ld_words<2 * NW>(bytes + i * 2 * NW, raw);
  bool is_inf = false;
  const int st = G::decode(raw, false, w, is_inf);
  st_words<4 * NW>(xy + i * 4 * NW, w);
  inf[i] = is_inf ? 1 : 0;
  status[i] = (uint8_t)st;
}

// affine points -> statuses.  after_decode = 0: every finite point is validated (a coordinate >= p or off the twist:
// 2) and tested (3).  after_decode != 0: the second half of a checked decompression -- only lanes whose status is
// still 0 are tested, and a point that fails is wiped (zeros) as every failed decompression is.  The affine point stays
// in memory: the lane keeps its Montgomery form and the accumulator, nothing else.
template <class C>
__global__ __launch_bounds__(G2_LANES) void g2_subgroup_kernel(uint32_t* xy, const uint8_t* inf, size_t n,
                                                               uint8_t* status, int after_decode) {
  using G = G2Bytes<C>;
  constexpr int NW = G::NW;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (after_decode && status[i] != 0) return;
  const bool is_inf = inf && inf[i];
  int st = G2_OK;
  if (!is_inf) {
    st = G::check_affine(xy + i * 4 * NW, false);
  }
  status[i] = (uint8_t)st;
  if (after_decode && st != G2_OK) {
    uint32_t z[4 * NW];
#pragma unroll
    for (int k = 0; k < 4 * NW; ++k) z[k] = 0;
    st_words<4 * NW>(xy + i * 4 * NW, z);
  }
}

// affine points -> blobs; a coordinate >= p or a point off the twist (fp_tower.h's import_g2) is counted in *bad
template <class C>
__global__ __launch_bounds__(G2_LANES) void g2_compress_kernel(const uint32_t* xy, const uint8_t* inf, size_t n,
                                                               uint32_t* bytes, uint32_t* bad) {
  using G = G2Bytes<C>;
  constexpr int NW = G::NW;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[4 * NW], raw[2 * NW];
  const bool is_inf = inf && inf[i];
  ld_words<4 * NW>(xy + i * 4 * NW, w);
  Fp2<C> x, y;
  if (!is_inf && !Tower<C>::import_g2(w, x, y)) atomicAdd(bad, 1u);
  G::encode(w, is_inf, raw);
  st_words<2 * NW>(bytes + i * 2 * NW, raw);
}

inline uint32_t blocks_of(size_t n) { return (uint32_t)((n + G2_LANES - 1) / G2_LANES); }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the launches of a decompression on device buffers; enqueue only
template <class C>
int decompress_launch(Ctx* c, const uint32_t* d_bytes, size_t n, int check_subgroup, uint32_t* d_xy, uint8_t* d_inf,
                      uint8_t* d_status) {
  hipLaunchKernelGGL(g2_decompress_kernel<C>, dim3(blocks_of(n)), dim3(G2_LANES), 0, c->stream, d_bytes, n, d_xy, d_inf,
                     d_status);
  KZG_HIP(c, hipGetLastError());
  if (check_subgroup) {
    hipLaunchKernelGGL(g2_subgroup_kernel<C>, dim3(blocks_of(n)), dim3(G2_LANES), 0, c->stream, d_xy, d_inf, n, d_status, 1);
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
  constexpr size_t SIZE = G2Bytes<C>::SIZE;
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
  constexpr size_t SIZE = G2Bytes<C>::SIZE;
  Stage s;
  int rc = stage<C>(c, n, &s);
  if (rc) return rc;
  KZG_HIP(c, hipMemcpyAsync(s.xy, xy, n * 2 * SIZE, hipMemcpyHostToDevice, c->stream));
  if (inf) KZG_HIP(c, hipMemcpyAsync(s.inf, inf, n, hipMemcpyHostToDevice, c->stream));
  KZG_HIP(c, hipMemsetAsync(s.bad, 0, 4, c->stream));
  hipLaunchKernelGGL(g2_compress_kernel<C>, dim3(blocks_of(n)), dim3(G2_LANES), 0, c->stream, s.xy,
                     inf ? s.inf : (const uint8_t*)nullptr, n, s.bytes, s.bad);
  KZG_HIP(c, hipGetLastError());
  uint32_t bad = 0;
  KZG_HIP(c, hipMemcpyAsync(&bad, s.bad, 4, hipMemcpyDeviceToHost, c->stream));
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  if (bad) return set_err(c, KZG_ERR_ARG, "kzg_g2_compress: a coordinate >= p or a point not on the twist");
  KZG_HIP(c, hipMemcpyAsync(out, s.bytes, n * SIZE, hipMemcpyDeviceToHost, c->stream));
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  return KZG_OK;
}

template <class C>
int decompress_t(Ctx* c, const uint8_t* bytes, size_t n, int check_subgroup, uint64_t* out_xy, uint8_t* out_inf,
                 uint8_t* out_status) {
  constexpr size_t SIZE = G2Bytes<C>::SIZE;
  Stage s;
  int rc = stage<C>(c, n, &s);
  if (rc) return rc;
  {
    ProfScope span(c, "g2_decompress");
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
  constexpr size_t SIZE = G2Bytes<C>::SIZE;
  Stage s;
  int rc = stage<C>(c, n, &s);
  if (rc) return rc;
  {
    ProfScope span(c, "g2_subgroup");
    KZG_HIP(c, hipMemcpyAsync(s.xy, xy, n * 2 * SIZE, hipMemcpyHostToDevice, c->stream));
    if (inf) KZG_HIP(c, hipMemcpyAsync(s.inf, inf, n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(g2_subgroup_kernel<C>, dim3(blocks_of(n)), dim3(G2_LANES), 0, c->stream, s.xy,
                       inf ? s.inf : (const uint8_t*)nullptr, n, s.status, 0);
    KZG_HIP(c, hipGetLastError());
    KZG_HIP(c, hipMemcpyAsync(out_status, s.status, n, hipMemcpyDeviceToHost, c->stream));
  }
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  return KZG_OK;
}

int size_check(Ctx* c, size_t n, const char* who) {
  if (n > G2_MAX_POINTS) {
    const std::string msg = std::string(who) + ": more than 2^24 points";
    return set_err(c, KZG_ERR_ARG, msg.c_str());
  }
  return KZG_OK;
}

}  // namespace

int g2_compress(Ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out_bytes) {
  if (n == 0) return KZG_OK;
  if (int rc = size_check(c, n, "kzg_g2_compress")) return rc;
  return KZG_BY_CURVE(c, compress_t, c, xy, inf, n, out_bytes);
}
int g2_decompress(Ctx* c, const uint8_t* bytes, size_t n, int check_subgroup, uint64_t* out_xy, uint8_t* out_inf,
                  uint8_t* out_status) {
  if (n == 0) return KZG_OK;
  if (int rc = size_check(c, n, "kzg_g2_decompress")) return rc;
  return KZG_BY_CURVE(c, decompress_t, c, bytes, n, check_subgroup, out_xy, out_inf, out_status);
}
int g2_decompress_device(Ctx* c, const void* d_bytes, size_t n, int check_subgroup, void* d_xy, void* d_inf,
                         void* d_status) {
  if (n == 0) return KZG_OK;
  if (int rc = size_check(c, n, "kzg_g2_decompress_device")) return rc;
  if (!aligned16(d_bytes) || !aligned16(d_xy))
    return set_err(c, KZG_ERR_ARG, "kzg_g2_decompress_device: misaligned device pointer");
  ProfScope span(c, "g2_decompress");
  return KZG_BY_CURVE(c, decompress_launch, c, static_cast<const uint32_t*>(d_bytes), n, check_subgroup,
                     static_cast<uint32_t*>(d_xy), static_cast<uint8_t*>(d_inf), static_cast<uint8_t*>(d_status));
}
int g2_check_subgroup(Ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out_status) {
  if (n == 0) return KZG_OK;
  if (int rc = size_check(c, n, "kzg_g2_check_subgroup")) return rc;
  return KZG_BY_CURVE(c, check_subgroup_t, c, xy, inf, n, out_status);
}

}  // namespace kzg
