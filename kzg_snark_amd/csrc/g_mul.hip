// g_mul.hip -- per-point scalar multiplication on gfx950: out[i] = [k_i] P_i for n points of G1's curve
// or of the twist, the products kept APART (a commit is their sum).  Two kernels, one lane per point, around the
// single-point ladders of g_mul.h, and the host drivers behind kzg_g1_mul_each*, kzg_g1_mul_powers, kzg_srs_mul_powers,
// kzg_g2_mul_each and kzg_g2_mul_powers.
//
//   points   canonical affine words and an infinity flag (G1: x | y, G2: x.c0 | x.c1 | y.c0 | y.c1), validated by the
//            rule of every import (a coordinate >= p or a point off its curve is refused), or -- G1 -- the window-0
//            records of a key, which need no validation
//   scalars  n x 8 words, taken as the 256-bit integers they are, or the geometric sequence c0 s^i mod r, formed in
//            the kernel from the two-level power table of fr_util.h (one product and one more by c0 per lane)
//   table    a lane writes 1P .. 8P into its column of a table in the context's scratch buffer, [multiple][piece][lane]
//            (verify_points.hip's layout: the loads of a wave's lanes with equal digits fall into the same lines);
//            launches cover at most GM_LAUNCH_LANES lanes each over one table, which bounds it
//   output   canonical affine words and a flag (one inversion per lane, as domain.hip ends), or key records
// G2 counts are small and a lane holds twice a G1 lane's registers: one wave per workgroup and the whole register file,
// as in g2_bytes.hip.
#include <algorithm>
#include <string>
#include "internal.h"
#include "fr_util.h"
#include "g1_util.h"
#include "msm.h"
#include "srs_rec.h"
#include "g_mul.h"
#include "g_mul_dev.h"

namespace kzg {

// the scalars of a launch (GmScalars), a lane's column of the table (G1Tab / G2Tab) and the argument checks of a call:
// g_mul_dev.h, shared with g2_lincomb.hip
namespace {

// out[i] = [k_i] P_i, i = first + the lane's index in the launch, i < n.  Points: recs (window-0 records) or xy / inf
// (inf may be null).  Output: out_recs (records) or out_xy / out_inf.  A point that is refused leaves zeros, the flag
// GM_FLAG_BAD and its index in *bad (the smallest wins).  tab: gridDim.x * GM_TB1 columns.
template <class C>
__global__ __launch_bounds__(GM_TB1) void g1_mul_each_kernel(uint32_t n, uint32_t first, const uint32_t* xy,
                                                             const uint8_t* inf, const uint32_t* recs, GmScalars sc,
                                                             uint4* tab, uint32_t* out_xy, uint8_t* out_inf,
                                                             uint32_t* out_recs, uint32_t* bad) {
  using Fd = Field<typename C::Fp>;
  constexpr int NW = C::Fp::NW;
  const uint32_t slot = blockIdx.x * GM_TB1 + threadIdx.x, i = first + slot;
  if (i >= n) return;
  Affine<C> a;
  bool ok = true;
  if (recs) {
    a.inf = load_rec<C>(recs, i, a.x, a.y) & 1u;
  } else {
    uint32_t w[2 * NW];
    ld_words<2 * NW>(xy + (size_t)i * 2 * NW, w);
    a = affine_from_words<C>(w, true);
    if (!(inf && inf[i])) {
      a.inf = false;
      ok = import_affine<C>(w, w + NW, a.x, a.y);
    }
  }
  uint32_t w[2 * NW];
  bool flag = true;
  if (ok) {
    uint32_t k[8];
    gm_scalar<C>(sc, i, k);
    G1Tab<C> column;
    column.tab = tab; column.slots = gridDim.x * GM_TB1; column.slot = slot;
    a = Ec<C>::to_affine(g1_mul<C>(a, k, column));
    if (out_recs) {
      store_rec<C>(out_recs, i, Fd::reduce(a.x), Fd::reduce(a.y), a.inf);
      return;
    }
    flag = affine_to_words<C>(a, w);
  } else {
    atomicMin(bad, i);
    if (out_recs) return;                                  // records come from records: never refused
#pragma unroll
    for (int j = 0; j < 2 * NW; ++j) w[j] = 0;
  }
  st_words<2 * NW>(out_xy + (size_t)i * 2 * NW, w);
  out_inf[i] = ok ? (flag ? 1 : 0) : GM_FLAG_BAD;
}

// the same on the twist: points of 4 NW words, one wave per workgroup; tab: gridDim.x * GM_TB2 columns
template <class C>
__global__ __launch_bounds__(GM_TB2) void g2_mul_each_kernel(uint32_t n, uint32_t first, const uint32_t* xy,
                                                             const uint8_t* inf, GmScalars sc, uint2* tab,
                                                             uint32_t* out_xy, uint8_t* out_inf, uint32_t* bad) {
  constexpr int NW = C::Fp::NW;
  const uint32_t slot = blockIdx.x * GM_TB2 + threadIdx.x, i = first + slot;
  if (i >= n) return;
  uint32_t w[4 * NW];
  ld_words<4 * NW>(xy + (size_t)i * 4 * NW, w);
  const bool is_inf = inf && inf[i];
  Fp2<C> x = Tower<C>::zero2(), y = Tower<C>::zero2();
  const bool ok = is_inf || Tower<C>::import_g2(w, x, y);
  bool flag = true;
  if (ok) {
    uint32_t k[8];
    gm_scalar<C>(sc, i, k);
    G2Tab<C> column;
    column.tab = tab; column.slots = gridDim.x * GM_TB2; column.slot = slot;
    flag = g2_to_words<C>(g2_mul<C>(x, y, is_inf, k, column), w);
  } else {
    atomicMin(bad, i);
#pragma unroll
    for (int j = 0; j < 4 * NW; ++j) w[j] = 0;
  }
  st_words<4 * NW>(out_xy + (size_t)i * 4 * NW, w);
  out_inf[i] = ok ? (flag ? 1 : 0) : GM_FLAG_BAD;
}

// ---- host side --------------------------------------------------------------------------------------

// what a call keeps in the context's buffer: the table, the first refused index and -- power form -- the power table
// and -- host-pointer forms -- the staged arrays
struct GmWs {
  void* tab; uint32_t* bad; uint32_t* ptab; uint32_t* xy; uint8_t* inf; uint32_t* k; uint32_t* out_xy; uint8_t* out_inf;
  void layout(Carve& ws, size_t table_bytes, bool powers, size_t stage_n, size_t point_bytes, bool has_inf, bool has_k) {
    tab = ws.take<void>(table_bytes);
    bad = ws.take(4);
    ptab = ws.take_if<uint32_t>(powers, (size_t)POW_TAB * 32);
    xy = ws.take_if<uint32_t>(stage_n != 0, stage_n * point_bytes);
    inf = ws.take_if<uint8_t>(has_inf, stage_n);
    k = ws.take_if<uint32_t>(has_k, stage_n * 32);
    out_xy = ws.take_if<uint32_t>(stage_n != 0, stage_n * point_bytes);
    out_inf = ws.take_if<uint8_t>(true, stage_n);
  }
};

template <class C>
int g1_launches(Ctx* c, size_t n, const GmPlan& plan, const uint32_t* d_xy, const uint8_t* d_inf, const uint32_t* recs,
                const GmScalars& sc, void* d_tab, uint32_t* d_out_xy, uint8_t* d_out_inf, uint32_t* d_out_recs,
                uint32_t* d_bad) {
  KZG_HIP(c, hipMemsetAsync(d_bad, 0xff, 4, c->stream));
  for (uint32_t b0 = 0; b0 < plan.blocks; b0 += plan.launch_blocks) {
    hipLaunchKernelGGL(g1_mul_each_kernel<C>, dim3(std::min(plan.launch_blocks, plan.blocks - b0)), dim3(GM_TB1), 0,
                       c->stream, (uint32_t)n, b0 * GM_TB1, d_xy, d_inf, recs, sc, static_cast<uint4*>(d_tab), d_out_xy,
                       d_out_inf, d_out_recs, d_bad);
    KZG_HIP(c, hipGetLastError());
  }
  return KZG_OK;
}
template <class C>
int g2_launches(Ctx* c, size_t n, const GmPlan& plan, const uint32_t* d_xy, const uint8_t* d_inf, const GmScalars& sc,
                void* d_tab, uint32_t* d_out_xy, uint8_t* d_out_inf, uint32_t* d_bad) {
  KZG_HIP(c, hipMemsetAsync(d_bad, 0xff, 4, c->stream));
  for (uint32_t b0 = 0; b0 < plan.blocks; b0 += plan.launch_blocks) {
    hipLaunchKernelGGL(g2_mul_each_kernel<C>, dim3(std::min(plan.launch_blocks, plan.blocks - b0)), dim3(GM_TB2), 0,
                       c->stream, (uint32_t)n, b0 * GM_TB2, d_xy, d_inf, sc, static_cast<uint2*>(d_tab), d_out_xy,
                       d_out_inf, d_bad);
    KZG_HIP(c, hipGetLastError());
  }
  return KZG_OK;
}

// the host-pointer forms of both groups: stage, launch, wait, report or copy out.  k: n x 8 words, or null with s, c0
template <class C, int GROUP>
int mul_host_t(Ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, const uint32_t* k, const uint32_t* s,
               const uint32_t* c0, uint64_t* out_xy, uint8_t* out_inf, const char* who) {
  constexpr size_t PT_BYTES = (GROUP == 1 ? 2 : 4) * C::Fp::NW * 4;
  const GmPlan plan(n, GROUP == 1 ? GM_TB1 : GM_TB2, GROUP == 1 ? GM_LAUNCH_LANES1 : GM_LAUNCH_LANES2);
  const size_t table = (GROUP == 1 ? g1_column_bytes<C>() * GM_TB1 : g2_column_bytes<C>() * GM_TB2) * plan.launch_blocks;
  GmWs d;
  int rc = carve(c, c->gmul_tmp, [&](Carve& ws) { d.layout(ws, table, !k, n, PT_BYTES, inf != nullptr, k != nullptr); });
  if (rc) return rc;
  GmScalars sc;
  if ((rc = scalars_of<C>(c, d.k, s, c0, d.ptab, who, &sc))) return rc;
  ProfScope ps(c, GROUP == 1 ? "g1_mul_each" : "g2_mul_each");
  hipStream_t st = c->stream;
  KZG_HIP(c, hipMemcpyAsync(d.xy, xy, n * PT_BYTES, hipMemcpyHostToDevice, st));
  if (inf) KZG_HIP(c, hipMemcpyAsync(d.inf, inf, n, hipMemcpyHostToDevice, st));
  if (k) KZG_HIP(c, hipMemcpyAsync(d.k, k, n * 32, hipMemcpyHostToDevice, st));
  if constexpr (GROUP == 1)
    rc = g1_launches<C>(c, n, plan, d.xy, d.inf, nullptr, sc, d.tab, d.out_xy, d.out_inf, nullptr, d.bad);
  else
    rc = g2_launches<C>(c, n, plan, d.xy, d.inf, sc, d.tab, d.out_xy, d.out_inf, d.bad);
  if (rc) return rc;
  uint32_t bad = GM_NONE;
  KZG_HIP(c, hipMemcpyAsync(&bad, d.bad, 4, hipMemcpyDeviceToHost, st));
  KZG_HIP(c, hipStreamSynchronize(st));
  if (bad != GM_NONE) return refuse(c, who, bad, GROUP == 1 ? "curve" : "twist");
  KZG_HIP(c, hipMemcpyAsync(out_xy, d.out_xy, n * PT_BYTES, hipMemcpyDeviceToHost, st));
  KZG_HIP(c, hipMemcpyAsync(out_inf, d.out_inf, n, hipMemcpyDeviceToHost, st));
  KZG_HIP(c, hipStreamSynchronize(st));
  return KZG_OK;
}

template <class C>
int g1_mul_each_device_t(Ctx* c, const uint32_t* d_xy, const uint8_t* d_inf, size_t n, const uint32_t* d_k,
                         uint32_t* d_out_xy, uint8_t* d_out_inf) {
  const GmPlan plan(n, GM_TB1, GM_LAUNCH_LANES1);
  GmWs d;
  int rc = carve(c, c->gmul_tmp, [&](Carve& ws) {
    d.layout(ws, g1_column_bytes<C>() * GM_TB1 * plan.launch_blocks, false, 0, 0, false, false);
  });
  if (rc) return rc;
  GmScalars sc;
  if ((rc = scalars_of<C>(c, d_k, nullptr, nullptr, nullptr, "kzg_g1_mul_each_device", &sc))) return rc;
  ProfScope ps(c, "g1_mul_each");
  return g1_launches<C>(c, n, plan, d_xy, d_inf, nullptr, sc, d.tab, d_out_xy, d_out_inf, nullptr, d.bad);
}

template <class C>
int srs_mul_powers_t(Ctx* c, const Srs* in, const uint32_t* s, const uint32_t* c0, Srs** out) {
  const size_t n = in->n;
  const GmPlan plan(n, GM_TB1, GM_LAUNCH_LANES1);
  GmWs d;
  int rc = carve(c, c->gmul_tmp, [&](Carve& ws) {
    d.layout(ws, g1_column_bytes<C>() * GM_TB1 * plan.launch_blocks, true, 0, 0, false, false);
  });
  if (rc) return rc;
  GmScalars sc;
  if ((rc = scalars_of<C>(c, nullptr, s, c0, d.ptab, "kzg_srs_mul_powers", &sc))) return rc;
  SrsPtr key;
  if ((rc = srs_create(c, n, &key))) return rc;
  {
    ProfScope ps(c, "g1_mul_each");
    if ((rc = g1_launches<C>(c, n, plan, nullptr, nullptr, in->recs, sc, d.tab, nullptr, nullptr, key->recs, d.bad)))
      return rc;
  }
  if ((rc = srs_finish_windows(c, key.get()))) return rc;        // synchronises
  *out = key.release();
  return KZG_OK;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <class C> int g1_host(Ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, const uint32_t* k, const uint32_t* s,
                               const uint32_t* c0, uint64_t* out_xy, uint8_t* out_inf, const char* who) {
  return mul_host_t<C, 1>(c, xy, inf, n, k, s, c0, out_xy, out_inf, who);
}
template <class C> int g2_host(Ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, const uint32_t* k, const uint32_t* s,
                               const uint32_t* c0, uint64_t* out_xy, uint8_t* out_inf, const char* who) {
  return mul_host_t<C, 2>(c, xy, inf, n, k, s, c0, out_xy, out_inf, who);
}

}  // namespace

int g1_mul_each(Ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, const uint32_t* k, const uint32_t* s,
                const uint32_t* c0, uint64_t* out_xy, uint8_t* out_inf) {
  const char* who = k ? "kzg_g1_mul_each" : "kzg_g1_mul_powers";
  if (n == 0) return KZG_OK;
  if (int rc = size_check(c, n, who)) return rc;
  return KZG_BY_CURVE(c, g1_host, c, xy, inf, n, k, s, c0, out_xy, out_inf, who);
}
int g2_mul_each(Ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, const uint32_t* k, const uint32_t* s,
                const uint32_t* c0, uint64_t* out_xy, uint8_t* out_inf) {
  const char* who = k ? "kzg_g2_mul_each" : "kzg_g2_mul_powers";
  if (n == 0) return KZG_OK;
  if (int rc = size_check(c, n, who)) return rc;
  return KZG_BY_CURVE(c, g2_host, c, xy, inf, n, k, s, c0, out_xy, out_inf, who);
}
int g1_mul_each_device(Ctx* c, const void* d_xy, const void* d_inf, size_t n, const void* d_k, void* d_out_xy,
                       void* d_out_inf) {
  if (n == 0) return KZG_OK;
  if (int rc = size_check(c, n, "kzg_g1_mul_each_device")) return rc;
  if (!aligned16(d_xy) || !aligned16(d_k) || !aligned16(d_out_xy))
    return set_err(c, KZG_ERR_ARG, "kzg_g1_mul_each_device: misaligned device pointer");
  return KZG_BY_CURVE(c, g1_mul_each_device_t, c, static_cast<const uint32_t*>(d_xy), static_cast<const uint8_t*>(d_inf), n,
                      static_cast<const uint32_t*>(d_k), static_cast<uint32_t*>(d_out_xy), static_cast<uint8_t*>(d_out_inf));
}
int srs_mul_powers(Ctx* c, const Srs* in, const uint32_t* s, const uint32_t* c0, Srs** out) {
  if (int rc = size_check(c, in->n, "kzg_srs_mul_powers")) return rc;
  return KZG_BY_CURVE(c, srs_mul_powers_t, c, in, s, c0, out);
}

}  // namespace kzg
