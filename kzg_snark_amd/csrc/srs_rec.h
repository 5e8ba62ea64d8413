// srs_rec.h -- the record layout of the device commitment-key table (msm.hip header comment), shared by the
// translation units that read or write window-0 records (msm.hip, lagrange.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "ec.h"
#include "g1_util.h"

namespace kzg {

template <class C> struct Rec {
  static constexpr int WORDS = C::REC_WORDS;
  static constexpr int N = C::Fp::N;
  static constexpr int FLAG = 2 * N;   // word index of the flags (bit 0: infinity)
};

// x, y and the flag word of a record (bit 0: point at infinity)
template <class C>
__device__ __forceinline__ uint32_t load_rec(const uint32_t* recs, size_t idx, Fe<typename C::Fp>& x,
                                             Fe<typename C::Fp>& y) {
  constexpr int N = C::Fp::N;
  const uint32_t* p = recs + idx * Rec<C>::WORDS;
  uint32_t flag;
  constexpr int Q = (2 * N + 3) / 4;                 // 16-byte loads covering x and y
  uint32_t w[4 * Q];
  if constexpr (4 * Q <= Rec<C>::WORDS && (Rec<C>::WORDS % 4) == 0) {
    ld_words<4 * Q>(p, w);
    if constexpr (Rec<C>::FLAG < 4 * Q) flag = w[Rec<C>::FLAG]; else flag = p[Rec<C>::FLAG];
  } else {
    const uint2* q = reinterpret_cast<const uint2*>(p);
#pragma unroll
    for (int i = 0; i < (2 * N) / 2; ++i) {
      const uint2 v = q[i];
      w[2 * i] = v.x; w[2 * i + 1] = v.y;
    }
    flag = p[Rec<C>::FLAG];
  }
#pragma unroll
  for (int j = 0; j < N; ++j) { x.l[j] = w[j]; y.l[j] = w[N + j]; }
  return flag;
}

template <class C>
__device__ __forceinline__ void store_rec(uint32_t* recs, size_t idx, const Fe<typename C::Fp>& x,
                                          const Fe<typename C::Fp>& y, bool inf) {
  constexpr int N = C::Fp::N;
  uint32_t* p = recs + idx * Rec<C>::WORDS;
#pragma unroll
  for (int j = 0; j < N; ++j) { p[j] = inf ? 0u : x.l[j]; p[N + j] = inf ? 0u : y.l[j]; }
#pragma unroll
  for (int j = 2 * N; j < Rec<C>::WORDS; ++j) p[j] = 0;
  p[Rec<C>::FLAG] = inf ? 1u : 0u;
}

}  // namespace kzg
