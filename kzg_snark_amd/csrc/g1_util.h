// g1_util.h -- device helpers of the kernels that keep G1 points as XYZZ in global memory (lagrange.hip, domain.hip):
// the point's load and store, scalar times point, the bit reversal of a transform index.
#pragma once
#include <hip/hip_runtime.h>
#include "ec.h"

namespace kzg {

// point idx of an array of XYZZ points: x y zz zzz, 4 N limbs, 16-byte accesses
template <class C>
__device__ __forceinline__ XYZZ<C> ld_point(const uint32_t* base, size_t idx) {
  constexpr int N = C::Fp::N;
  const uint4* p = reinterpret_cast<const uint4*>(base + idx * 4 * N);
  uint32_t w[4 * N];
#pragma unroll
  for (int q = 0; q < N; ++q) {
    const uint4 v = p[q];
    w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
  }
  XYZZ<C> r;
#pragma unroll
  for (int j = 0; j < N; ++j) { r.x.l[j] = w[j]; r.y.l[j] = w[N + j]; r.zz.l[j] = w[2 * N + j]; r.zzz.l[j] = w[3 * N + j]; }
  return r;
}
template <class C>
__device__ __forceinline__ void st_point(uint32_t* base, size_t idx, const XYZZ<C>& v) {
  constexpr int N = C::Fp::N;
  uint32_t w[4 * N];
#pragma unroll
  for (int j = 0; j < N; ++j) { w[j] = v.x.l[j]; w[N + j] = v.y.l[j]; w[2 * N + j] = v.zz.l[j]; w[3 * N + j] = v.zzz.l[j]; }
  uint4* p = reinterpret_cast<uint4*>(base + idx * 4 * N);
#pragma unroll
  for (int q = 0; q < N; ++q) p[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
}

// e * P by double-and-add from the top bit (e: 8 canonical words).  Exact for every input (ec.h's add / dbl).
template <class C>
__device__ __forceinline__ XYZZ<C> g1_mul_words(const XYZZ<C>& p, const uint32_t* e) {
  XYZZ<C> acc = Ec<C>::infinity();
#pragma unroll 1
  for (int k = 7; k >= 0; --k) {
    const uint32_t word = e[k];
#pragma unroll 1
    for (int b = 31; b >= 0; --b) {
      acc = Ec<C>::dbl(acc);
      if ((word >> b) & 1u) acc = Ec<C>::add(acc, p);
    }
  }
  return acc;
}

__device__ __forceinline__ uint32_t bitrev(uint32_t i, uint32_t log_len) {
  return log_len ? __brev(i) >> (32 - log_len) : 0u;
}

}  // namespace kzg
