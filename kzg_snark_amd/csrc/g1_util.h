// g1_util.h -- device helpers of the kernels that move G1 points through global memory (lagrange.hip, domain.hip,
// g1_bytes.hip, srs_rec.h): the 16-byte word-array load and store, the XYZZ point's load and store, scalar times
// point, the bit reversal of a transform index.
#pragma once
#include <hip/hip_runtime.h>
#include "ec.h"

namespace kzg {

// W words (a whole number of 16-byte accesses) between 16-byte aligned memory and registers
template <int W>
__device__ __forceinline__ void ld_words(const uint32_t* p, uint32_t* w) {
  static_assert(W % 4 == 0, "whole 16-byte accesses");
  const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (int i = 0; i < W / 4; ++i) {
    const uint4 v = q[i];
    w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
  }
}
template <int W>
__device__ __forceinline__ void st_words(uint32_t* p, const uint32_t* w) {
  static_assert(W % 4 == 0, "whole 16-byte accesses");
  uint4* q = reinterpret_cast<uint4*>(p);
#pragma unroll
  for (int i = 0; i < W / 4; ++i) q[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}

// point idx of an array of XYZZ points: x y zz zzz, 4 N limbs
template <class C>
__device__ __forceinline__ XYZZ<C> ld_point(const uint32_t* base, size_t idx) {
  constexpr int N = C::Fp::N;
  uint32_t w[4 * N];
  ld_words<4 * N>(base + idx * 4 * N, w);
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
  st_words<4 * N>(base + idx * 4 * N, w);
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
