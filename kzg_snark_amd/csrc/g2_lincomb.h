// g2_lincomb.h -- the sum behind kzg_g2_lincomb* (DESIGN.md 4.17): the full addition of two Jacobian points of the twist,
// a point as 6 N limbs in LDS or global memory, and how a call is cut into launches, partial sums and fold levels.
// Shared by the kernels of g2_lincomb.hip and the host (tests/shim/g2_lincomb_shim.cpp compiles this text with g++):
// nothing here is device-only.
#pragma once
#include "g_mul.h"

namespace kzg {

// p <- p + q for ANY two points of the twist.  G2Bytes::add finishes an infinite operand on either side and q = -p;
// it reports "the same finite point" (equal x and y after scaling by the other's Z, so P and P at different Z count)
// and leaves p untouched, and the doubling finishes that.
template <class C>
static KZG_HD void g2_add_full(Jac2<C>& p, const Jac2<C>& q) {
  if (G2Bytes<C>::template add<false>(p, q)) p = G2Bytes<C>::dbl(p);
}

template <class C>
static KZG_HD Jac2<C> g2_infinity() {
  Jac2<C> r;
  r.x = Tower<C>::zero2(); r.y = Tower<C>::zero2(); r.z = Tower<C>::zero2();
  return r;
}

// a Jacobian point as 6 N limbs x.c0 | x.c1 | y.c0 | y.c1 | z.c0 | z.c1, limb j at p[j * stride]: stride 1 is a row of
// global memory (one partial sum), stride = lanes is the [limb][lane] layout of LDS
template <class C>
static KZG_HD void g2_put_limbs(const Jac2<C>& v, uint32_t* p, uint32_t stride) {
  constexpr int N = C::Fp::N;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    p[(uint32_t)j * stride] = v.x.c0.l[j]; p[(uint32_t)(N + j) * stride] = v.x.c1.l[j];
    p[(uint32_t)(2 * N + j) * stride] = v.y.c0.l[j]; p[(uint32_t)(3 * N + j) * stride] = v.y.c1.l[j];
    p[(uint32_t)(4 * N + j) * stride] = v.z.c0.l[j]; p[(uint32_t)(5 * N + j) * stride] = v.z.c1.l[j];
  }
}
template <class C>
static KZG_HD Jac2<C> g2_get_limbs(const uint32_t* p, uint32_t stride) {
  constexpr int N = C::Fp::N;
  Jac2<C> r;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    r.x.c0.l[j] = p[(uint32_t)j * stride]; r.x.c1.l[j] = p[(uint32_t)(N + j) * stride];
    r.y.c0.l[j] = p[(uint32_t)(2 * N + j) * stride]; r.y.c1.l[j] = p[(uint32_t)(3 * N + j) * stride];
    r.z.c0.l[j] = p[(uint32_t)(4 * N + j) * stride]; r.z.c1.l[j] = p[(uint32_t)(5 * N + j) * stride];
  }
  return r;
}
template <class C> constexpr uint32_t g2_point_limbs() { return 6 * C::Fp::N; }

// ---- the plan of a call (g2_lincomb.hip's driver; tests/test_g2_lincomb_host.py through the shim) ---------------------
constexpr uint32_t GL_TB = 64;                            // lanes per workgroup of the product stage: one wave
constexpr uint32_t GL_LAUNCH_LANES = 1024 * GL_TB;        // one wave per SIMD of 256 CUs: 512 VGPRs leave room for no more
constexpr uint32_t GL_FOLD_TB = 64;                       // lanes per workgroup of the fold
constexpr uint32_t GL_FOLD_SPAN = 4 * GL_FOLD_TB;         // points one workgroup of the fold adds: four per lane
constexpr int GL_MAX_LEVELS = 3;

// Product stage: GmPlan's launches of at most GL_LAUNCH_LANES lanes over one table, one partial sum per workgroup.
// Fold: level l turns width[l] points into width[l + 1] = ceil(width[l] / GL_FOLD_SPAN); the last level has one
// workgroup and writes the affine result.  ok: n is within GM_MAX_POINTS, the fold fits GL_MAX_LEVELS and every index
// the kernels form in 32 bits -- the table's largest (table_top) and the last limb of the last partial -- is below 2^32.
struct GlPlan {
  GmPlan mul;
  uint32_t launches, partials, levels, width[GL_MAX_LEVELS + 1], table_top;
  bool ok;
  GlPlan(size_t n, int pieces, uint32_t point_limbs) : mul(n <= GM_MAX_POINTS ? n : 0, GL_TB, GL_LAUNCH_LANES) {
    partials = mul.blocks;
    launches = mul.launch_blocks ? (mul.blocks + mul.launch_blocks - 1) / mul.launch_blocks : 0;
    levels = 0;
    for (int l = 0; l <= GL_MAX_LEVELS; ++l) width[l] = 0;
    uint32_t w = partials;
    bool fits = true;
    while (w && (levels == 0 || w > 1)) {
      if (levels == (uint32_t)GL_MAX_LEVELS) { fits = false; break; }
      width[levels++] = w;
      w = (w + GL_FOLD_SPAN - 1) / GL_FOLD_SPAN;
    }
    if (fits) width[levels] = w;
    const uint64_t slots = (uint64_t)mul.launch_blocks * GL_TB;
    const uint64_t top = slots ? (uint64_t)GMUL_TABLE * (uint64_t)pieces * slots - 1 : 0;
    const uint64_t last_limb = (uint64_t)partials * point_limbs;
    table_top = (uint32_t)top;
    ok = n <= GM_MAX_POINTS && fits && top < ((uint64_t)1 << 32) && last_limb < ((uint64_t)1 << 32);
  }
};

}  // namespace kzg
