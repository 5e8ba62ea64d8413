// fr_util.h -- what the translation units share about ONE scalar-field element: the kernel-argument form, the loads
// and stores of an element in global or shared memory, the wave shuffle, the lookup in a two-level power table
// (built by fr_pow_table, lagrange.hip) and the host-side root-of-unity helpers over Field<F>.
#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
#include "field.h"

namespace kzg {

struct FrArg {                    // one Fr element (both scalar fields: 9 x 29-bit limbs) as a kernel argument
  uint32_t l[9];
};

// 8 canonical words, two 16-byte accesses
template <class F>
__device__ __forceinline__ Fe<F> load_words(const uint32_t* p) {
  const uint4* g = reinterpret_cast<const uint4*>(p);
  const uint4 lo = g[0], hi = g[1];
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  return Field<F>::from_words(w);
}
template <class F>
__device__ __forceinline__ void store_words(uint32_t* p, const Fe<F>& v) {
  uint32_t w[8];
  Field<F>::to_words(Field<F>::reduce(v), w);
  uint4* g = reinterpret_cast<uint4*>(p);
  g[0] = make_uint4(w[0], w[1], w[2], w[3]);
  g[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
template <class F>
__device__ __forceinline__ Fe<F> load_limbs(const uint32_t* p) {
  Fe<F> r;
#pragma unroll
  for (int j = 0; j < F::N; ++j) r.l[j] = p[j];
  return r;
}
template <class F>
__device__ __forceinline__ void store_limbs(uint32_t* p, const Fe<F>& v) {
#pragma unroll
  for (int j = 0; j < F::N; ++j) p[j] = v.l[j];
}
template <class F>
__device__ __forceinline__ Fe<F> arg_fe(const FrArg& a) {
  return load_limbs<F>(a.l);
}

template <class F>
__device__ __forceinline__ Fe<F> shfl_xor_fe(const Fe<F>& v, int mask) {
  Fe<F> r;
#pragma unroll
  for (int j = 0; j < F::N; ++j) r.l[j] = __shfl_xor(v.l[j], mask);
  return r;
}

// Two-level power table of one base x: tab[i] = x^i (i < POW_TLO), tab[POW_TLO + i] = (x^POW_TLO)^i (i < POW_THI),
// Montgomery words, so x^e = lo[e & 2047] * hi[e >> 11] for every e <= 2^21 is one product.
constexpr uint32_t POW_TLOG = 11;
constexpr uint32_t POW_TLO = 1u << POW_TLOG;
constexpr uint32_t POW_THI = (1u << (21 - POW_TLOG)) + 1;       // exponents up to 2^21 inclusive
constexpr uint32_t POW_TAB = POW_TLO + POW_THI;                 // 3073 entries

template <class F>
__device__ __forceinline__ Fe<F> fr_pow_lookup(const uint32_t* tab, uint32_t e) {
  return Field<F>::mul(load_words<F>(tab + (size_t)(e & (POW_TLO - 1)) * 8),
                       load_words<F>(tab + (size_t)(POW_TLO + (e >> POW_TLOG)) * 8));
}

// ---- host side (static: the library exports no symbol of these) ---------------------------------------------------

template <class F>
static inline FrArg fr_arg(const Fe<F>& v) {
  static_assert(sizeof(v.l) == sizeof(FrArg::l), "scalar fields have 9 limbs");
  FrArg a;
  memcpy(a.l, v.l, sizeof(a.l));
  return a;
}

// canonical words -> Montgomery element
template <class F>
static inline Fe<F> mont_from_words(const uint32_t* w) {
  return Field<F>::to_mont(Field<F>::from_words(w));
}

// Montgomery element -> canonical words
template <class F>
static inline void words_from_mont(const Fe<F>& mont, uint32_t* w) {
  Field<F>::to_words(Field<F>::from_mont(mont), w);
}

// the smallest generator of the scalar field's multiplicative group (Montgomery): g^N != 1 for every N < r - 1
template <class C>
static inline Fe<typename C::Fr> fr_generator() {
  const uint32_t w[8] = {C::ID == 0 ? 5u : 7u, 0, 0, 0, 0, 0, 0, 0};
  return mont_from_words<typename C::Fr>(w);
}

// w (Montgomery) is a primitive 2^log_n-th root of unity, log_n >= 1: w^(n/2) = -1
template <class F>
static inline bool primitive_root(const Fe<F>& w_mont, uint32_t log_n) {
  using Fd = Field<F>;
  if (log_n == 0) return false;
  Fe<F> x = w_mont;
  for (uint32_t q = 1; q < log_n; ++q) x = Fd::sqr(x);
  return Fd::eq(x, Fd::neg(Fd::one()));
}

// (2^log_n)^-1, Montgomery (not reduced)
template <class F>
static inline Fe<F> inv_pow2(uint32_t log_n) {
  uint32_t nw[8] = {0};
  nw[log_n >> 5] = 1u << (log_n & 31);
  return Field<F>::inv(mont_from_words<F>(nw));
}

}  // namespace kzg
