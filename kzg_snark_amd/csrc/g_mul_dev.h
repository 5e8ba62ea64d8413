// g_mul_dev.h -- what the kernels and drivers of g_mul.hip and g2_lincomb.hip share around the ladders of g_mul.h: the
// scalars of a launch, a lane's column of the table of multiples, and the checks and refusals of a call's arguments.
// Device code and host drivers (g_mul.h itself stays free of both: the host shims compile it).  Everything here is
// internal to the translation unit that includes it.
#pragma once
#include <string>
#include "internal.h"
#include "fr_util.h"
#include "g1_util.h"
#include "g_mul.h"

namespace kzg {

namespace {

// GM_TB1 / GM_TB2 (lanes per workgroup), GM_LAUNCH_LANES1 / 2 (lanes per launch) and GM_MAX_POINTS: g_mul.h
constexpr uint32_t GM_NONE = 0xffffffffu;                 // *bad while every point is good
constexpr uint8_t GM_FLAG_BAD = 2;                        // out_inf of a point that was refused

// the scalars of a launch: k != null: n x 8 words; else c0 s^i with s^i from the power table
struct GmScalars {
  const uint32_t* k;
  const uint32_t* ptab;
  FrArg c0;                                               // Montgomery form
};

template <class C>
__device__ __forceinline__ void gm_scalar(const GmScalars& sc, uint32_t i, uint32_t* k) {
  using Fr = typename C::Fr;
  if (sc.k) {
    ld_words<8>(sc.k + (size_t)i * 8, k);
  } else {
    const Fe<Fr> v = Field<Fr>::mul(fr_pow_lookup<Fr>(sc.ptab, i), arg_fe<Fr>(sc.c0));
    Field<Fr>::to_words(Field<Fr>::from_mont(v), k);
  }
}

// a lane's column of the table: entry e is PIECES vectors V at the indices of g_mul.h's gm_entry_index /
// gm_piece_index.  The entry's first index is hidden from the optimiser behind an empty asm: the table phase stores
// entry `it`, the loop's own counter, and strength reduction would otherwise keep one 64-bit address PER PIECE alive
// across the whole ladder, in registers the G2 lanes do not have (hundreds of bytes of scratch memory).
template <class V, int PIECES>
struct GmColumn {
  V* tab;
  uint32_t slots, slot;
  __device__ __forceinline__ uint32_t entry(int e) const {
    uint32_t idx = gm_entry_index(e, PIECES, slots, slot);
    asm volatile("" : "+v"(idx));
    return idx;
  }
  __device__ __forceinline__ V& at(uint32_t entry_idx, int q) const { return tab[gm_piece_index(entry_idx, q, slots)]; }
};
template <class C>
struct G1Tab : GmColumn<uint4, gm_g1_pieces<C>()> {
  static constexpr int N = C::Fp::N;
  __device__ __forceinline__ void store(int e, const XYZZ<C>& v) const {
    uint32_t w[4 * N];
#pragma unroll
    for (int j = 0; j < N; ++j) { w[j] = v.x.l[j]; w[N + j] = v.y.l[j]; w[2 * N + j] = v.zz.l[j]; w[3 * N + j] = v.zzz.l[j]; }
    const uint32_t at0 = this->entry(e);
#pragma unroll
    for (int q = 0; q < N; ++q) this->at(at0, q) = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  }
  __device__ __forceinline__ XYZZ<C> load(int e) const {
    uint32_t w[4 * N];
    const uint32_t at0 = this->entry(e);
#pragma unroll
    for (int q = 0; q < N; ++q) {
      const uint4 v = this->at(at0, q);
      w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
    XYZZ<C> r;
#pragma unroll
    for (int j = 0; j < N; ++j) { r.x.l[j] = w[j]; r.y.l[j] = w[N + j]; r.zz.l[j] = w[2 * N + j]; r.zzz.l[j] = w[3 * N + j]; }
    return r;
  }
};
// a Jacobian point of the twist is 6 N limbs (N is odd): 3 N pieces of 8 bytes
template <class C>
struct G2Tab : GmColumn<uint2, gm_g2_pieces<C>()> {
  static constexpr int N = C::Fp::N;
  __device__ __forceinline__ void store(int e, const Jac2<C>& v) const {
    uint32_t w[6 * N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      w[j] = v.x.c0.l[j]; w[N + j] = v.x.c1.l[j]; w[2 * N + j] = v.y.c0.l[j]; w[3 * N + j] = v.y.c1.l[j];
      w[4 * N + j] = v.z.c0.l[j]; w[5 * N + j] = v.z.c1.l[j];
    }
    const uint32_t at0 = this->entry(e);
#pragma unroll
    for (int q = 0; q < 3 * N; ++q) this->at(at0, q) = make_uint2(w[2 * q], w[2 * q + 1]);
  }
  __device__ __forceinline__ Jac2<C> load(int e) const {
    uint32_t w[6 * N];
    const uint32_t at0 = this->entry(e);
#pragma unroll
    for (int q = 0; q < 3 * N; ++q) {
      const uint2 v = this->at(at0, q);
      w[2 * q] = v.x; w[2 * q + 1] = v.y;
    }
    Jac2<C> r;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      r.x.c0.l[j] = w[j]; r.x.c1.l[j] = w[N + j]; r.y.c0.l[j] = w[2 * N + j]; r.y.c1.l[j] = w[3 * N + j];
      r.z.c0.l[j] = w[4 * N + j]; r.z.c1.l[j] = w[5 * N + j];
    }
    return r;
  }
};

// ---- host side: a call's arguments ------------------------------------------------------------------------------------

template <class C>
int check_scalar(Ctx* c, const uint32_t* v, const char* who, const char* name) {
  if (gmul_scalar_below<typename C::Fr>(v)) return KZG_OK;
  const std::string msg = std::string(who) + ": " + name + " is not below the group order r";
  return set_err(c, KZG_ERR_ARG, msg.c_str());
}

// the scalars of a launch from a call's arguments; the power form checks s and c0 and enqueues the table's launch
template <class C>
int scalars_of(Ctx* c, const uint32_t* d_k, const uint32_t* s, const uint32_t* c0, uint32_t* d_ptab, const char* who,
               GmScalars* sc) {
  using Fr = typename C::Fr;
  sc->k = d_k;
  sc->ptab = d_ptab;
  sc->c0 = FrArg{};
  if (d_k) return KZG_OK;
  if (int rc = check_scalar<C>(c, s, who, "s")) return rc;
  if (int rc = check_scalar<C>(c, c0, who, "c0")) return rc;
  sc->c0 = fr_arg<Fr>(mont_from_words<Fr>(c0));
  return fr_pow_table(c, fr_arg<Fr>(mont_from_words<Fr>(s)), d_ptab);
}

inline int refuse(Ctx* c, const char* who, uint32_t index, const char* curve) {
  const std::string msg = std::string(who) + ": point " + std::to_string(index) + " has a coordinate >= p or is not on the " +
                          curve;
  return set_err(c, KZG_ERR_ARG, msg.c_str());
}

inline int size_check(Ctx* c, size_t n, const char* who) {
  if (n > GM_MAX_POINTS) {
    const std::string msg = std::string(who) + ": more than 2^21 points";
    return set_err(c, KZG_ERR_ARG, msg.c_str());
  }
  return KZG_OK;
}

}  // namespace

}  // namespace kzg
