// pairing.hip -- pairing-product checks on the device: one kernel around fp_tower.h's equation(), one
// wave per equation, and the host driver behind kzg_pairing_check and kzg_pairing_product.
//
// Layout: a workgroup is ONE wave of 64 lanes and takes ONE equation (PAIRING_EQUATIONS_PER_WORKGROUP); the grid is m
// workgroups, no grid-stride loop (m <= 2^20).  The lanes cooperate as fp_tower.h describes: in a product phase every
// lane forms one Fp2 product (36 for an Fp12 multiplication, up to 6 per pair for a point step), in a linear phase 6
// or k lanes combine them.  What crosses lanes lives in one PairingShared<C> in LDS.  The exchange (WaveLanes) is
// "lane t runs body(t), body(t + 64), ..., then the workgroup meets": with one wave per workgroup the barrier is the
// wave's own, and the decisions that differ between equations (a skipped pair, a malformed point) are taken by a whole
// wave, so no barrier is ever waited on by part of a workgroup.  The kernel calls no function: fp_tower.h's interpreter
// is inlined, with one copy of the Fp2 multiplier.
#include "internal.h"
#include "msm.h"
#include "fp_tower.h"

namespace kzg {

namespace {

constexpr size_t PAIRING_MAX_EQUATIONS = (size_t)1 << 20;
constexpr int PAIRING_EQUATIONS_PER_WORKGROUP = 1;
constexpr int PAIRING_LANES = 64;

struct WaveLanes {
  template <class Fn>
  __device__ __forceinline__ void each(int n, Fn fn) {
    for (int t = (int)threadIdx.x; t < n; t += PAIRING_LANES) fn(t);
    __syncthreads();
  }
  static __device__ __forceinline__ uint32_t uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
};

// out_gt == nullptr: statuses only
template <class C>
__global__ __launch_bounds__(PAIRING_LANES) void pairing_kernel(const uint32_t* g1, const uint8_t* g1_inf,
                                                                const uint32_t* g2, const uint8_t* g2_inf, uint32_t m,
                                                                int k, uint32_t* out_gt, uint8_t* out_status) {
  constexpr int NW = C::Fp::NW;
  __shared__ PairingShared<C> sh;
  const size_t e = blockIdx.x;
  if (e >= m) return;
  WaveLanes x;
  const int st = Tower<C>::equation(x, &sh, g1 + e * k * 2 * NW, g1_inf ? g1_inf + e * k : nullptr, g2 + e * k * 4 * NW,
                                    g2_inf ? g2_inf + e * k : nullptr, k, out_gt ? out_gt + e * 12 * NW : nullptr);
  if (threadIdx.x == 0) out_status[e] = (uint8_t)st;
}

template <class C>
int pairing_t(Ctx* c, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf,
              size_t m, size_t k, uint64_t* out_gt, uint8_t* out_status) {
  constexpr size_t FB = C::Fp::NW * 4;                  // bytes of a coordinate
  const size_t n = m * k;
  uint32_t *d_g1, *d_g2, *d_gt;
  uint8_t *d_f1, *d_f2, *d_st;
  // its own buffer: the staging buffer and the pipeline's slots are not touched
  int rc = carve(c, c->pair_tmp, [&](Carve& ws) {
    d_g1 = ws.take(n * 2 * FB);  d_g2 = ws.take(n * 4 * FB);
    d_f1 = ws.take<uint8_t>(n);  d_f2 = ws.take<uint8_t>(n);
    d_gt = ws.take_if<uint32_t>(out_gt != nullptr, m * 12 * FB);  d_st = ws.take<uint8_t>(m);
  });
  if (rc) return rc;
  {
    ProfScope span(c, "pairing");
    KZG_HIP(c, hipMemcpyAsync(d_g1, g1_xy, n * 2 * FB, hipMemcpyHostToDevice, c->stream));
    KZG_HIP(c, hipMemcpyAsync(d_g2, g2_xy, n * 4 * FB, hipMemcpyHostToDevice, c->stream));
    if (g1_inf) KZG_HIP(c, hipMemcpyAsync(d_f1, g1_inf, n, hipMemcpyHostToDevice, c->stream));
    if (g2_inf) KZG_HIP(c, hipMemcpyAsync(d_f2, g2_inf, n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(pairing_kernel<C>, dim3((uint32_t)(m / PAIRING_EQUATIONS_PER_WORKGROUP)), dim3(PAIRING_LANES), 0,
                       c->stream, d_g1, g1_inf ? d_f1 : (const uint8_t*)nullptr, d_g2,
                       g2_inf ? d_f2 : (const uint8_t*)nullptr, (uint32_t)m, (int)k, d_gt, d_st);
    KZG_HIP(c, hipGetLastError());
    if (out_gt) KZG_HIP(c, hipMemcpyAsync(out_gt, d_gt, m * 12 * FB, hipMemcpyDeviceToHost, c->stream));
    KZG_HIP(c, hipMemcpyAsync(out_status, d_st, m, hipMemcpyDeviceToHost, c->stream));
  }
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  return KZG_OK;
}

}  // namespace

int pairing_product(Ctx* c, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf,
                    size_t m, size_t k, uint64_t* out_gt, uint8_t* out_status) {
  if (k < 1 || k > (size_t)PAIRING_MAX_PAIRS) return set_err(c, KZG_ERR_ARG, "kzg_pairing: between 1 and 16 pairs per equation");
  if (m > PAIRING_MAX_EQUATIONS) return set_err(c, KZG_ERR_ARG, "kzg_pairing: more than 2^20 equations");
  if (m == 0) return KZG_OK;
  return KZG_BY_CURVE(c, pairing_t, c, g1_xy, g1_inf, g2_xy, g2_inf, m, k, out_gt, out_status);
}

int pairing_gt_multiple(int curve) { return curve == 0 ? Bn254::GT_MULTIPLE : curve == 1 ? Bls12_381::GT_MULTIPLE : 0; }

}  // namespace kzg
