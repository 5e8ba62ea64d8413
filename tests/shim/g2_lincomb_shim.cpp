// Host-only test shim: kzg_snark_amd/csrc/g2_lincomb.h (the text the gfx950 kernels of g2_lincomb.hip compile) behind a
// tiny C interface, so tests/test_g2_lincomb_host.py can check the full addition on the twist against curve.py's group
// law without a GPU, restate the wave sum and the fold over it, and read the plan of a call.  A Jacobian point crosses
// the interface as the 6 N limbs of g2_put_limbs (stride 1), opaque to Python.  Test infrastructure only.
#include <stdio.h>
#include <string.h>
#include "../../kzg_snark_amd/csrc/g2_lincomb.h"
using namespace kzg;

template <class C>
static int from_affine(const uint32_t* xy, int inf, uint32_t* out) {
  Jac2<C> p = g2_infinity<C>();
  if (!inf) {
    if (!Tower<C>::import_g2(xy, p.x, p.y)) return 1;
    p.z = Tower<C>::one2();
  }
  g2_put_limbs<C>(p, out, 1);
  return 0;
}
template <class C>
static void add(const uint32_t* a, const uint32_t* b, uint32_t* out) {
  Jac2<C> p = g2_get_limbs<C>(a, 1);
  g2_add_full<C>(p, g2_get_limbs<C>(b, 1));
  g2_put_limbs<C>(p, out, 1);
}
// the same point at another Z: (X l^2, Y l^3, Z l) for l in Fp (canonical words, not zero)
template <class C>
static void rescale(const uint32_t* a, const uint32_t* lambda, uint32_t* out) {
  using Fd = Field<typename C::Fp>;
  Jac2<C> p = g2_get_limbs<C>(a, 1);
  const Fe<typename C::Fp> l = Fd::to_mont(Fd::from_words(lambda)), l2 = Fd::mul(l, l), l3 = Fd::mul(l2, l);
  p.x.c0 = Fd::mul(p.x.c0, l2); p.x.c1 = Fd::mul(p.x.c1, l2);
  p.y.c0 = Fd::mul(p.y.c0, l3); p.y.c1 = Fd::mul(p.y.c1, l3);
  p.z.c0 = Fd::mul(p.z.c0, l); p.z.c1 = Fd::mul(p.z.c1, l);
  g2_put_limbs<C>(p, out, 1);
}
template <class C>
static void to_affine(const uint32_t* a, uint32_t* out, int* out_inf) {
  *out_inf = g2_to_words<C>(g2_get_limbs<C>(a, 1), out) ? 1 : 0;
}

#define BY_CURVE(fn, ...) (curve == 0 ? (fn<Bn254>(__VA_ARGS__), 0) : curve == 1 ? (fn<Bls12_381>(__VA_ARGS__), 0) : -1)

extern "C" int gl_point_limbs(int curve) {
  return curve == 0 ? (int)g2_point_limbs<Bn254>() : curve == 1 ? (int)g2_point_limbs<Bls12_381>() : -1;
}
extern "C" int gl_from_affine(int curve, const uint32_t* xy, int inf, uint32_t* out) {
  return curve == 0 ? from_affine<Bn254>(xy, inf, out) : curve == 1 ? from_affine<Bls12_381>(xy, inf, out) : -1;
}
extern "C" int gl_add(int curve, const uint32_t* a, const uint32_t* b, uint32_t* out) { return BY_CURVE(add, a, b, out); }
extern "C" int gl_rescale(int curve, const uint32_t* a, const uint32_t* lambda, uint32_t* out) {
  return BY_CURVE(rescale, a, lambda, out);
}
extern "C" int gl_to_affine(int curve, const uint32_t* a, uint32_t* out, int* out_inf) {
  return BY_CURVE(to_affine, a, out, out_inf);
}

// 0: lanes per workgroup of the product stage, 1: lanes per launch, 2: lanes per workgroup of the fold, 3: points per
// workgroup of the fold, 4: the largest n, 5: the most levels a fold may have
extern "C" uint64_t gl_const(int which) {
  const uint64_t v[] = {GL_TB, GL_LAUNCH_LANES, GL_FOLD_TB, GL_FOLD_SPAN, GM_MAX_POINTS, (uint64_t)GL_MAX_LEVELS};
  return which >= 0 && which < 6 ? v[which] : 0;
}
// the plan of a call of n points as g2_lincomb.hip's driver builds it.  out: blocks, launch_blocks, launches, partials,
// levels, width[0 .. GL_MAX_LEVELS], table_top, ok, pieces per table entry; *vectors: the 8-byte vectors the driver
// allocates for the table; *partial_limbs: the limbs it allocates for the partial sums of the product stage
template <class C>
static void plan_of(uint64_t n, uint32_t* out, uint64_t* vectors, uint64_t* partial_limbs) {
  const GlPlan plan((size_t)n, gm_g2_pieces<C>(), g2_point_limbs<C>());
  int at = 0;
  out[at++] = plan.mul.blocks; out[at++] = plan.mul.launch_blocks; out[at++] = plan.launches; out[at++] = plan.partials;
  out[at++] = plan.levels;
  for (int l = 0; l <= GL_MAX_LEVELS; ++l) out[at++] = plan.width[l];
  out[at++] = plan.table_top; out[at++] = plan.ok ? 1u : 0u; out[at++] = (uint32_t)gm_g2_pieces<C>();
  *vectors = (uint64_t)(g2_column_bytes<C>() / 8) * GL_TB * plan.mul.launch_blocks;
  *partial_limbs = (uint64_t)plan.width[0] * g2_point_limbs<C>();
}
extern "C" int gl_plan(int curve, uint64_t n, uint32_t* out, uint64_t* vectors, uint64_t* partial_limbs) {
  return BY_CURVE(plan_of, n, out, vectors, partial_limbs);
}
// the largest table index a launch of g workgroups touches, by the kernels' own 32-bit arithmetic
template <class C>
static void top_of(uint32_t g, uint32_t* top) {
  const uint32_t slots = g * GL_TB;
  const int p = gm_g2_pieces<C>();
  *top = gm_piece_index(gm_entry_index(GMUL_TABLE - 1, p, slots, slots - 1), p - 1, slots);
}
extern "C" int gl_table_top(int curve, uint32_t g, uint32_t* top) { return BY_CURVE(top_of, g, top); }
