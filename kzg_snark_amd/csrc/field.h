// field.h -- prime-field arithmetic for the KZG engine, shared by gfx950 device
// code and the host side of the C-ABI library.
//
// Representation ("unsaturated limbs"): an element is N limbs of L bits held in
// 32-bit words, value = sum l[j] * 2^(L*j).  L = 29 (N = 9) for the ~255-bit
// fields, L = 30 (N = 13) for the 381-bit BLS12-381 base field.  The point of the
// slack bits is the multiplier: on gfx950 a 32x32+64 multiply-add
// (v_mad_u64_u32) issues at the same rate as an FP64 FMA (measured,
// tools/microbench/int_rates.hip) but has no carry-in, so with saturated
// 32-bit limbs every partial product needs extra carry instructions (hipcc's
// CIOS for 12 limbs: 288 mads + 295 64-bit adds + 620 moves).  With L-bit limbs
// a whole operand-scanning Montgomery product accumulates into 64-bit columns
// without ever overflowing, so each partial product is exactly one
// v_mad_u64_u32 and nothing else.
//
// Invariant of every value returned by this header ("weak-normal"): limbs
// l[0..N-2] < 2^L, top limb small and non-negative, value in [0, 2p).
// reduce() brings a value to the canonical range [0, p).
//
// Montgomery radix R = 2^(L*N); 4p < R for all four fields, so mul() maps
// weak-normal inputs to a weak-normal output:  (ab + mp)/R < 4p^2/R + p < 2p.
//
// Column bound: a 64-bit column absorbs FIT = 2^(64-2L) products of two L-bit limbs next to a carry (64 for L = 29,
// 16 for L = 30).  A Montgomery column adds up to 2N products, so N = 9, L = 29 never gets near it and N = 13, L = 30
// does: there the multiply-add chain of a column is CUT where it could carry out (plan_columns() below decides
// where, at compile time).  BLS12-381 Fp declares TOP_LIMB_BOUND = 2^26 and is planned by magnitudes -- half of a
// column's products are m_i * P[j] with the real, often small, limbs of p, and the top limb of an operand is far below
// 2^30 -- which needs 3 cuts per mul / sqr (columns 10, 11, 12) and 14 per mul2, where counting products needed 9
// and 24.  A cut costs two VALU instructions (a move and a multiply-add on the chain's high word) where shift, mask
// and 64-bit addition cost three: 21 VALU instructions fewer per mul / sqr, 44 per mul2, 9450 -> 9136 instructions
// in msm_accumulate_kernel<Bls12_381, 20> (tools/isa_histogram.py, profiles/r05_isa_histograms.txt); measured,
// 0.892 -> 0.849 G VALU wave-instructions per accumulate launch; +3.8 % commits/s on the box of the A/B
// (EXPERIMENTS.md E1, round 5).  The multiply-add's weight 2^(32-L) must stay out of the optimiser's sight: the
// multiply-add of a cut is one asm statement with the weight as an inline constant (Field::unpeel), where round 5
// defined the weight in an SGPR by an asm statement per cut: 9136 -> 9179 instructions with the exit probe of
// msm.hip, s_mov_b32 141 -> 86, VALU count unchanged; +2.9 % commits/s (profiles/r07_isa_histograms.txt,
// profiles/r07_cut_ab.txt, EXPERIMENTS.md E1, round 7).
//
// What the multipliers require of their operands is NOT "limbs < 2^L" but three things:
//  (1) per column, the product units stay within FIT = 2^(64-2L): a product of two limbs below 2^L is one unit, and
//      limbs below u*2^L and v*2^L make a product of u*v units.  mul<UNITS_AB> is told the units of one a*b product
//      and plans its columns with them.  Every function of this header but add_lazy / sub_lazy4
//      returns limbs below 2^L; the un-carried outputs of those two (below 2^32 = 8 * 2^29) are legal operands of
//      the plain mul<1> as long as (1) still holds without a cut, which ntt.hip relies on for L = 29, N = 9;
//  (2) the result range: (sum of the operand-value products + m*p)/R < 2p, i.e. the products sum below R*p;
//  (3) in a field that declares TOP_LIMB_BOUND (BLS12-381 Fp: 2^26, any normalised value up to 39p; (2) already caps
//      operands near 25p and ec.h passes nothing above 10p): top limb below the bound, the other limbs below
//      UNITS_AB * 2^L.  The columns of such a field are planned with these magnitudes, not with (1)'s count.
// The host-only audit build below (KZG_AUDIT) checks exactly these, per call.
#pragma once
#include <stdint.h>
#include "curve_constants.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KZG_HD __host__ __device__ __forceinline__
#else
#define KZG_HD inline __attribute__((always_inline))
#endif

// ---- audit build (host only) ----------------------------------------------------------------------
// How to use: compile a HOST translation unit with -DKZG_AUDIT, run any code of field.h / ec.h, then read
// kzg::audit::state(): `count` violated pre/postconditions, and the function, line and text of the first one.
// state().lift = true makes every multiplier return the representative in [p, 2p) (the top of its documented
// range), so the range tables of the callers are exercised at their stated bounds.  tests/shim/bounds_shim.cpp.
#if defined(KZG_AUDIT) && !defined(__HIP_DEVICE_COMPILE__)
#define KZG_AUDIT_ON 1
namespace kzg {
namespace audit {
struct State {
  unsigned long long count;
  const char* fn;
  const char* what;
  int line;
  bool lift;
};
inline State& state() {
  static State s = {0, "", "", 0, false};
  return s;
}
inline void fail(const char* fn, int line, const char* what) {
  State& s = state();
  if (s.count++ == 0) { s.fn = fn; s.line = line; s.what = what; }
}
// little multi-word integers for the range checks: 512 bits hold 13 limbs of 30 bits with 32-bit excess
struct Big {
  uint64_t w[8];
};
inline Big big_zero() { Big r; for (int i = 0; i < 8; ++i) r.w[i] = 0; return r; }
inline void big_add_shifted(Big& r, uint64_t v, int bit) {      // r += v * 2^bit
  const int k = bit >> 6, sh = bit & 63;
  unsigned __int128 c = (unsigned __int128)v << sh;
  for (int i = k; i < 8 && c; ++i) {
    c += r.w[i];
    r.w[i] = (uint64_t)c;
    c >>= 64;
  }
}
inline int big_cmp(const Big& a, const Big& b) {
  for (int i = 7; i >= 0; --i)
    if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
  return 0;
}
template <class F>
inline Big value(const uint32_t* l) {                            // sum l[j] 2^(L j), limbs taken as unsigned 32-bit
  Big r = big_zero();
  for (int j = 0; j < F::N; ++j) big_add_shifted(r, l[j], F::L * j);
  return r;
}
template <class F>
inline Big kp(uint32_t k) {                                      // k * p
  Big r = big_zero();
  for (int j = 0; j < F::N; ++j) big_add_shifted(r, (uint64_t)k * F::P[j], F::L * j);
  return r;
}
template <class F>
inline Big value_plus_kp(const uint32_t* l, uint32_t k) {        // value(l) + k * p
  Big r = value<F>(l);
  for (int j = 0; j < F::N; ++j) big_add_shifted(r, (uint64_t)k * F::P[j], F::L * j);
  return r;
}
template <class F>
inline bool below_kp(const uint32_t* l, uint32_t k) { return big_cmp(value<F>(l), kp<F>(k)) < 0; }
template <class F>
inline bool at_most_kp(const uint32_t* l, uint32_t k) { return big_cmp(value<F>(l), kp<F>(k)) <= 0; }
template <class F>
inline bool normalised(const uint32_t* l) {                      // lower limbs below 2^L
  for (int j = 0; j < F::N - 1; ++j)
    if (l[j] >> F::L) return false;
  return true;
}
}  // namespace audit
}  // namespace kzg
#define KZG_AUDIT_CHECK(cond, what) do { if (!(cond)) ::kzg::audit::fail(__func__, __LINE__, what); } while (0)
#else
#define KZG_AUDIT_CHECK(cond, what) ((void)0)
#endif

namespace kzg {

// c + a*b: one v_mad_u64_u32.  On the device every partial sum is also shown to an EMPTY asm statement as an input:
// LLVM's Reassociate pass only rewrites chains whose interior sums have a single use, so the column stays ONE
// multiply-add chain seeded with the carry instead of a chain from zero joined to the carry by a v_lshl_add_u64
// (one instruction per column).  Nothing is emitted for the statement and, unlike an asm DEFINITION, an asm use
// draws no hazard nops.
static KZG_HD uint64_t mad_wide(uint32_t a, uint32_t b, uint64_t c) {
  const uint64_t r = c + (uint64_t)a * b;
#ifdef KZG_AUDIT_ON
  if ((((unsigned __int128)a * b + c) >> 64) != 0) audit::fail(__func__, __LINE__, "column carries out of 64 bits");
#endif
#if defined(__HIP_DEVICE_COMPILE__) && !defined(KZG_NO_CHAIN_PIN)
  asm volatile("" ::"v"(r));
#endif
  return r;
}

// -DKZG_CUT_WEIGHT_CONST only (the other form of a cut's weight, Field::unpeel): the constant 1, which the device
// code must not see as a constant.  It exists in the DEVICE pass only, so the host side neither declares nor
// registers it: the library has no relocatable device code, every translation unit is a code object of its own with
// its own copy, initialised when the code object is loaded.  Not `static`: an internal variable is folded to its
// initialiser.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(KZG_NO_CHAIN_PIN) && defined(KZG_CUT_WEIGHT_CONST)
#define KZG_CUT_WEIGHT_WORD 1
__constant__ uint32_t cut_weight_unit = 1u;
#endif

template <class F>
struct Fe {
  uint32_t l[F::N];
};

// ---- column bound ------------------------------------------------------------------------------------
// A field may declare F::TOP_LIMB_BOUND: the top limb of every operand of its multipliers stays below it.
template <class F, class = void>
struct TopLimb {
  static constexpr bool declared = false;
  static constexpr uint32_t bound = 0;
};
template <class F>
struct TopLimb<F, decltype((void)F::TOP_LIMB_BOUND)> {
  static constexpr bool declared = true;
  static constexpr uint32_t bound = F::TOP_LIMB_BOUND;
  static_assert(bound >= 1 && bound <= (1u << F::L), "the top limb is a limb");
};

// Where the 64-bit multiply-add chains of a product-scanning Montgomery multiplier are cut.  Column k takes NG groups
// of products in turn -- the operand products of each of the NG - 1 terms, then m*p -- on top of the carry of column
// k - 1.  plan_columns() follows the worst case of every chain with 128-bit integers and cuts (greedily) right before
// the first group that could carry it out of 64 bits.  A cut sets the HIGH WORD of the chain aside: 2^32 is a multiple
// of 2^L, so the low L bits (all that m_k and the result limb read) are untouched, the chain goes on from its low
// word, and the word joins the outgoing carry as hi * 2^(32-L).  After a cut the walk goes on from 2^32 - 1, the
// largest low word any chain value can leave (the worst-case VALUE may well leave a small one), beside the largest
// high word: both are upper bounds, so every later decision, `fits` and the carry are.
//   magnitudes, for a field that declares TOP_LIMB_BOUND: operand limbs 0..N-2 <= UNITS * 2^L - 1 (see precondition
//     (1) in the header), top limb <= TOP_LIMB_BOUND - 1, m_i <= 2^L - 1 against the REAL limbs of p;
//   otherwise every limb of the operands and of p counts as 2^L - 1: the count rule -- FIT products and a carry fit.
template <int NCOL, int NG>
struct ColumnPlan {
  bool cut[NCOL][NG];        // cut[k][g]: set the high word aside before group g of column k
  int cuts;                  // how many
  bool fits;                 // no chain reaches 2^64
  uint64_t carry_max;        // the largest carry a column hands on
};

template <class F, int K, int UNITS, bool SQUARE>
constexpr ColumnPlan<2 * F::N - 1, K + 1> plan_columns() {
  typedef unsigned __int128 u128;
  constexpr int L = F::L, N = F::N;
  constexpr bool mag = TopLimb<F>::declared;
  const u128 LIMIT = (((u128)1) << 64) - 1;
  const u128 one = F::MASK;                                                   // a normalised limb
  const u128 low = (((u128)UNITS) << L) - 1;                                  // a lower operand limb of u <= UNITS units
  const u128 low2 = (((u128)UNITS) << (2 * L)) - (((u128)2) << L) + 1;        // (u 2^L - 1)(v 2^L - 1) with u v <= UNITS
  const u128 top = mag ? (u128)TopLimb<F>::bound - 1 : one;
  ColumnPlan<2 * N - 1, K + 1> plan = {};
  plan.fits = true;
  u128 carry = 0;
  for (int k = 0; k < 2 * N - 1; ++k) {
    const int lo = k < N ? 0 : k - N + 1, hi = k < N ? k : N - 1;
    u128 chain = carry, aside = 0;
    for (int g = 0; g <= K; ++g) {
      u128 group = 0;
      for (int i = lo; i <= hi; ++i) {
        const int j = k - i;
        if (g < K) {
          const bool ti = mag && i == N - 1, tj = mag && j == N - 1;
          const u128 ab = ti && tj ? top * top : ti || tj ? top * low : low2;
          group += !SQUARE ? ab : i < j ? 2 * ab : i == j ? ab : 0;          // sqr: off-diagonal once, doubled
        } else if (i < k || k >= N) {
          group += one * (mag ? (u128)F::P[j] : one);
        }
      }
      if (g == K && k < N) group += one * (mag ? (u128)F::P[0] : one);        // m_k p_0
      if (chain + group > LIMIT) {
        plan.cut[k][g] = true;
        ++plan.cuts;
        aside += chain >> 32;                        // the largest high word ...
        chain = 0xffffffffu;                         // ... and the largest LOW word: not the low word of the largest value
      }
      chain += group;
      if (chain > LIMIT) plan.fits = false;
    }
    carry = (chain >> L) + (aside << (32 - L));
    if (carry > LIMIT) plan.fits = false;
    else if ((uint64_t)carry > plan.carry_max) plan.carry_max = (uint64_t)carry;
  }
  return plan;
}
template <class F, int K, int UNITS, bool SQUARE>
struct Columns {
  static constexpr ColumnPlan<2 * F::N - 1, K + 1> plan = plan_columns<F, K, UNITS, SQUARE>();
  static_assert(plan.fits, "a column carries out of 64 bits even with its cuts");
  // no cut before the first group of a column: the carry and one term's products fit (mul, sqr, mul2 rely on it and
  // have no code for such a cut; dot<K> could take one but never needs it either)
  static constexpr bool first_group_fits() {
    for (int k = 0; k < 2 * F::N - 1; ++k)
      if (plan.cut[k][0]) return false;
    return true;
  }
  static_assert(first_group_fits(), "the carry and the first group of products do not fit one 64-bit chain");
};

template <class F>
struct Field {
  static constexpr int L = F::L;
  static constexpr int N = F::N;
  static constexpr int NW = F::NW;
  static constexpr uint32_t MASK = F::MASK;
  // products of two normalised limbs that fit one 64-bit column (with room for carries)
  static constexpr int CAP = (2 * L >= 64) ? 0 : (int)((1ull << (64 - 2 * L)) - 1);
  static_assert(CAP >= 15, "limb width too large for 64-bit columns");
  // Exact capacity of a product-scanning column: FIT = 2^(64-2L) products of two limbs <= 2^L - 1 plus the carry of
  // the previous column still fit 64 bits:  FIT (2^L - 1)^2 + 2^(64-L) = 2^64 - FIT 2^(L+1) + FIT + 2^(64-L) < 2^64
  // because FIT 2^(L+1) = 2^(65-L) > 2^(64-L) + FIT.  (L = 30: 16 products; L = 29: 64.)
  static constexpr int FIT = CAP + 1;
  using E = Fe<F>;

  // carry-normalise a window of 64-bit columns in place (value unchanged)
  template <int M>
  static KZG_HD void normalize_cols(uint64_t (&w)[M]) {
#pragma unroll
    for (int j = 0; j < M - 1; ++j) {
      const uint64_t c = w[j] >> L;
      w[j] &= (uint64_t)MASK;
      w[j + 1] += c;
    }
  }

  // A cut (ColumnPlan): the chain goes on from its low word, the high word waits for the outgoing carry, which it
  // joins by ONE multiply-add, hi * 2^(32-L) + carry.  A weight the optimiser can see is turned into
  // ((acc >> L) & ~(2^(32-L) - 1)) + carry -- a 64-bit shift, two ands and a 64-bit addition per cut, more than
  // the cut by shift and mask that this replaces -- so on the device the multiply-add is ONE asm statement with the
  // weight as an inline constant of the instruction (4 for L = 30): no s_mov_b32 per cut, nothing that stays live in
  // a register (the 168-VGPR reduce kernels have none to give).  -DKZG_CUT_WEIGHT_CONST builds the other form that
  // costs no register: no asm at all, the weight is cut_weight_unit << (32 - L) read from constant memory (above),
  // one s_load_dword and one s_lshl_b32 per KERNEL.  Both beat round 5's asm definition of the weight per cut; the
  // asm form measured +2.9 %, the constant-memory form +2.2 % (EXPERIMENTS.md E1, round 7).
  // The host (and KZG_NO_CHAIN_PIN) keeps the plain constant.
  static KZG_HD uint32_t peel(uint64_t& acc) {
    const uint32_t h = (uint32_t)(acc >> 32);
    acc = (uint32_t)acc;
    return h;
  }
  static KZG_HD uint64_t unpeel(uint32_t h, uint64_t carry) {
#if defined(KZG_CUT_WEIGHT_WORD)
    return mad_wide(h, cut_weight_unit << (32 - L), carry);
#elif defined(__HIP_DEVICE_COMPILE__) && !defined(KZG_NO_CHAIN_PIN)
    static_assert((1u << (32 - L)) <= 64, "the weight must be an inline constant of the instruction");
    uint64_t r, carry_out;
    asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(r), "=s"(carry_out) : "v"(h), "n"(1u << (32 - L)), "v"(carry));
    return r;
#else
    return mad_wide(h, 1u << (32 - L), carry);
#endif
  }

#ifdef KZG_AUDIT_ON
  // precondition (3) of the multipliers of a field that declares TOP_LIMB_BOUND
  static void audit_operand(const E& a, uint32_t units, const char* fn, int line) {
    if (!TopLimb<F>::declared) return;
    bool ok = a.l[N - 1] < TopLimb<F>::bound;
    for (int j = 0; j < N - 1; ++j) ok = ok && a.l[j] < ((uint64_t)units << L);
    if (!ok) audit::fail(fn, line, "operand limbs above the column bound (top limb < TOP_LIMB_BOUND, others < units * 2^L)");
  }
  // ... and of (1) as the plan takes it: limbs below u * 2^L and v * 2^L with u * v <= units
  static void audit_units(const E& a, const E& b, uint32_t units, const char* fn, int line) {
    if (!TopLimb<F>::declared) return;
    uint32_t ma = 0, mb = 0;
    for (int j = 0; j < N - 1; ++j) { ma = a.l[j] > ma ? a.l[j] : ma; mb = b.l[j] > mb ? b.l[j] : mb; }
    const uint64_t u = (ma >> L) + 1, v = (mb >> L) + 1;
    if (u <= units && v <= units && u * v > units) audit::fail(fn, line, "operand limbs above the column bound (u * v product units above UNITS_AB)");
  }
#define KZG_AUDIT_OPERAND(a, units) audit_operand(a, units, __func__, __LINE__)
#define KZG_AUDIT_UNITS(a, b, units) audit_units(a, b, units, __func__, __LINE__)
#else
#define KZG_AUDIT_OPERAND(a, units) ((void)0)
#define KZG_AUDIT_UNITS(a, b, units) ((void)0)
#endif

#ifdef KZG_AUDIT_ON
  // postcondition of every multiplier: weak-normal.  With audit::state().lift the representative in [p, 2p).
  static void audit_product(E& r, const char* fn, int line) {
    if (!audit::normalised<F>(r.l) || !audit::below_kp<F>(r.l, 2)) audit::fail(fn, line, "product not weak-normal (< 2p, limbs < 2^L)");
    if (audit::state().lift && audit::below_kp<F>(r.l, 1)) {
      uint32_t c = 0;
      for (int j = 0; j < N; ++j) {
        const uint32_t t = r.l[j] + F::P[j] + c;
        if (j < N - 1) { r.l[j] = t & MASK; c = t >> L; } else { r.l[j] = t; }
      }
    }
  }
  // true (unwrapped) value of a limb formed as a + (k - b) + c must fit an unsigned 32-bit word
  static bool audit_limb_ok(uint32_t a, uint32_t k, uint32_t b, uint32_t c) {
    const int64_t t = (int64_t)a + (int64_t)k - (int64_t)b + (int64_t)c;
    return t >= 0 && t < ((int64_t)1 << 32);
  }
#define KZG_AUDIT_PRODUCT(r) audit_product(r, __func__, __LINE__)
#else
#define KZG_AUDIT_PRODUCT(r) ((void)0)
#endif

  static KZG_HD E zero() {
    E r;
#pragma unroll
    for (int j = 0; j < N; ++j) r.l[j] = 0;
    return r;
  }
  // Montgomery form of 1
  static KZG_HD E one() {
    E r;
#pragma unroll
    for (int j = 0; j < N; ++j) r.l[j] = F::R1[j];
    return r;
  }
  // the plain integer 1 (mul(a, raw_one()) converts out of Montgomery form)
  static KZG_HD E raw_one() {
    E r = zero();
    r.l[0] = 1;
    return r;
  }
  static KZG_HD E r2() {
    E r;
#pragma unroll
    for (int j = 0; j < N; ++j) r.l[j] = F::R2[j];
    return r;
  }

  // canonical saturated little-endian words (NW x 32 bit) -> limbs.  The value
  // is taken as is (no reduction): callers pass values < p.
  static KZG_HD E from_words(const uint32_t* w) {
    E r;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int bit = j * L;
      const int k = bit >> 5, sh = bit & 31;
      uint64_t lo = (k < NW) ? w[k] : 0u;
      uint64_t hi = (k + 1 < NW) ? w[k + 1] : 0u;
      r.l[j] = (uint32_t)(((hi << 32) | lo) >> sh) & MASK;
    }
    return r;
  }
  // limbs -> canonical words.  Requires a canonical element (reduce() first).
  static KZG_HD void to_words(const E& a, uint32_t* w) {
    KZG_AUDIT_CHECK(audit::normalised<F>(a.l) && audit::below_kp<F>(a.l, 1), "input not canonical");
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      // word k covers bits [32k, 32k+32)
      const int j0 = (32 * k) / L;           // first limb touching the word
      const int off0 = 32 * k - j0 * L;      // bit offset inside limb j0
      uint64_t acc = (uint64_t)a.l[j0] >> off0;
      int have = L - off0;
      if (j0 + 1 < N) {
        acc |= (uint64_t)a.l[j0 + 1] << have;
        have += L;
      }
      if (have < 32 && j0 + 2 < N) acc |= (uint64_t)a.l[j0 + 2] << have;
      w[k] = (uint32_t)acc;
    }
  }

  // ---- multiplication: product scanning (column by column) --------------------------------------
  // Every simple integer instruction of gfx950 issues at the rate of v_mad_u64_u32 (measured,
  // tools/microbench/int_rates.hip), so what counts is the NUMBER of instructions.  Column k of the
  // Montgomery product collects  sum_(i+j=k) a_i b_j + sum_(i+j=k) m_i p_j  on top of the carry of
  // column k-1: the carry is the initial value of the column's multiply-add chain (no separate
  // 64-bit addition per column), the low half of the columns yields the quotient digits m_k, the
  // high half the result limbs.  (hipcc re-associates each column's sum so that the incoming carry is
  // added last -- one v_lshl_add_u64 per column remains; forcing a single chain with inline-asm
  // multiply-adds was worth another 0.4 % and was not kept)
  //
  // Column capacity: a chain that could carry out of 64 bits is cut where Columns<...>::plan says (plan_columns()
  // above): its high word is set aside and joins the outgoing carry, the low word stays in the chain.  `UNITS_AB` =
  // how many units one a*b product may take (operands with limbs up to 2^(L+1) from add_lazy count 2 or 4).
  template <int UNITS_AB = 1>
  static KZG_HD E mul(const E& a, const E& b) {
    using Col = Columns<F, 1, UNITS_AB, false>;
    KZG_AUDIT_OPERAND(a, UNITS_AB); KZG_AUDIT_OPERAND(b, UNITS_AB); KZG_AUDIT_UNITS(a, b, UNITS_AB);
    uint32_t m[N];
    E r;
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 2 * N - 1; ++k) {
      const int lo = k < N ? 0 : k - N + 1, hi = k < N ? k : N - 1;
      const bool cut = Col::plan.cut[k][1];              // before m*p (the carry and the a*b products always fit)
      uint32_t aside = 0;
#pragma unroll
      for (int i = lo; i <= hi; ++i) acc = mad_wide(a.l[i], b.l[k - i], acc);
      if (cut) aside = peel(acc);
#pragma unroll
      for (int i = lo; i <= hi; ++i)
        if (i < k || k >= N) acc = mad_wide(m[i], F::P[k - i], acc);
      if (k < N) {
        m[k] = ((uint32_t)acc * F::N0) & MASK;
        acc = mad_wide(m[k], F::P[0], acc);
      } else {
        r.l[k - N] = (uint32_t)acc & MASK;
      }
      acc >>= L;
      if (cut) acc = unpeel(aside, acc);
    }
    r.l[N - 1] = (uint32_t)acc;
    KZG_AUDIT_PRODUCT(r);
    return r;
  }
  // Montgomery square: off-diagonal products once, against the doubled operand.
  static KZG_HD E sqr(const E& a) {
    using Col = Columns<F, 1, 1, true>;
    KZG_AUDIT_OPERAND(a, 1);
    uint32_t m[N], a2[N];
#pragma unroll
    for (int j = 0; j < N; ++j) a2[j] = a.l[j] << 1;
    E r;
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 2 * N - 1; ++k) {
      const int lo = k < N ? 0 : k - N + 1, hi = k < N ? k : N - 1;
      const bool cut = Col::plan.cut[k][1];
      uint32_t aside = 0;
#pragma unroll
      for (int i = lo; i <= hi; ++i) {
        const int j = k - i;
        if (i < j) acc = mad_wide(a.l[i], a2[j], acc);
        else if (i == j) acc = mad_wide(a.l[i], a.l[i], acc);
      }
      if (cut) aside = peel(acc);
#pragma unroll
      for (int i = lo; i <= hi; ++i)
        if (i < k || k >= N) acc = mad_wide(m[i], F::P[k - i], acc);
      if (k < N) {
        m[k] = ((uint32_t)acc * F::N0) & MASK;
        acc = mad_wide(m[k], F::P[0], acc);
      } else {
        r.l[k - N] = (uint32_t)acc & MASK;
      }
      acc >>= L;
      if (cut) acc = unpeel(aside, acc);
    }
    r.l[N - 1] = (uint32_t)acc;
    KZG_AUDIT_PRODUCT(r);
    return r;
  }

  // a*b + c*d with ONE Montgomery reduction (weak-normal in and out: (4p^2+4p^2)/R + p < 2p
  // needs 8p < R, true for all four fields).
  static KZG_HD E mul2(const E& a, const E& b, const E& c, const E& d) {
    static_assert(F::BITS + 3 <= L * N, "mul2 needs 8p < R");
    using Col = Columns<F, 2, 1, false>;
    KZG_AUDIT_OPERAND(a, 1); KZG_AUDIT_OPERAND(b, 1); KZG_AUDIT_OPERAND(c, 1); KZG_AUDIT_OPERAND(d, 1);
    uint32_t m[N];
    E r;
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 2 * N - 1; ++k) {
      const int lo = k < N ? 0 : k - N + 1, hi = k < N ? k : N - 1;
      const bool cut1 = Col::plan.cut[k][1];             // between a*b and c*d
      const bool cut2 = Col::plan.cut[k][2];             // before m*p
      uint32_t aside1 = 0, aside2 = 0;
#pragma unroll
      for (int i = lo; i <= hi; ++i) acc = mad_wide(a.l[i], b.l[k - i], acc);
      if (cut1) aside1 = peel(acc);
#pragma unroll
      for (int i = lo; i <= hi; ++i) acc = mad_wide(c.l[i], d.l[k - i], acc);
      if (cut2) aside2 = peel(acc);
#pragma unroll
      for (int i = lo; i <= hi; ++i)
        if (i < k || k >= N) acc = mad_wide(m[i], F::P[k - i], acc);
      if (k < N) {
        m[k] = ((uint32_t)acc * F::N0) & MASK;
        acc = mad_wide(m[k], F::P[0], acc);
      } else {
        r.l[k - N] = (uint32_t)acc & MASK;
      }
      acc >>= L;
      if (cut1) acc = unpeel(aside1, acc);
      if (cut2) acc = unpeel(aside2, acc);
    }
    r.l[N - 1] = (uint32_t)acc;
    KZG_AUDIT_PRODUCT(r);
    return r;
  }

  // sum_{t<K} a[t]*b[t] with ONE Montgomery reduction: K*N^2 + N^2 + N multiply-adds instead of K*(2N^2 + N) --
  // the linear combinations of KZG.open (kzg.py:148-150) and of the prover's r(X).  Weak-normal (< 2p) in and out:
  // (K*4p^2 + m*p)/R < 2p needs 4K*p <= R (the static_assert rounds K up to a power of two, 16 at the most).  A column takes the a*b products of one term after the other and is cut
  // (the low word stays in the chain, the high word joins the outgoing carry) before a group that could carry it out.
  template <int K>
  static KZG_HD E dot(const E* a, const E* b) {
    static_assert(K >= 1 && K <= 16 && F::BITS + 2 + (K > 8 ? 4 : K > 4 ? 3 : K > 2 ? 2 : K > 1 ? 1 : 0) <= L * N, "dot needs 4K*p <= R");
    using Col = Columns<F, K, 1, false>;
#ifdef KZG_AUDIT_ON
    for (int t = 0; t < K; ++t) { KZG_AUDIT_OPERAND(a[t], 1); KZG_AUDIT_OPERAND(b[t], 1); }
#endif
    uint32_t m[N];
    E r;
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 2 * N - 1; ++k) {
      const int lo = k < N ? 0 : k - N + 1, hi = k < N ? k : N - 1;
      uint32_t aside[K + 1] = {};
#pragma unroll
      for (int t = 0; t < K; ++t) {
        if (Col::plan.cut[k][t]) aside[t] = peel(acc);
#pragma unroll
        for (int i = lo; i <= hi; ++i) acc = mad_wide(a[t].l[i], b[t].l[k - i], acc);
      }
      if (Col::plan.cut[k][K]) aside[K] = peel(acc);
#pragma unroll
      for (int i = lo; i <= hi; ++i)
        if (i < k || k >= N) acc = mad_wide(m[i], F::P[k - i], acc);
      if (k < N) {
        m[k] = ((uint32_t)acc * F::N0) & MASK;
        acc = mad_wide(m[k], F::P[0], acc);
      } else {
        r.l[k - N] = (uint32_t)acc & MASK;
      }
      acc >>= L;
#pragma unroll
      for (int t = 0; t <= K; ++t)
        if (Col::plan.cut[k][t]) acc = unpeel(aside[t], acc);
    }
    r.l[N - 1] = (uint32_t)acc;
    KZG_AUDIT_PRODUCT(r);
    return r;
  }

  // a + b, weak-normal in and out
  static KZG_HD E add(const E& a, const E& b) {
    E s, t;
    uint32_t cs = 0;
    int32_t ct = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const uint32_t x = a.l[j] + b.l[j];
      const uint32_t sj = x + cs;
      const int32_t tj = (int32_t)(x - F::P2[j]) + ct;
      if (j < N - 1) {
        cs = sj >> L;
        s.l[j] = sj & MASK;
        ct = tj >> L;
        t.l[j] = (uint32_t)tj & MASK;
      } else {
        s.l[j] = sj;
        t.l[j] = (uint32_t)tj;
      }
    }
    const bool neg = (int32_t)t.l[N - 1] < 0;
    E r;
#pragma unroll
    for (int j = 0; j < N; ++j) r.l[j] = neg ? s.l[j] : t.l[j];
    return r;
  }
  // a - b, weak-normal in and out
  static KZG_HD E sub(const E& a, const E& b) {
    E u, t;
    int32_t cu = 0, ct = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int32_t x = (int32_t)a.l[j] - (int32_t)b.l[j];
      const int32_t tj = x + ct;
      const int32_t uj = x + (int32_t)F::P2[j] + cu;
      if (j < N - 1) {
        ct = tj >> L;
        t.l[j] = (uint32_t)tj & MASK;
        cu = uj >> L;
        u.l[j] = (uint32_t)uj & MASK;
      } else {
        t.l[j] = (uint32_t)tj;
        u.l[j] = (uint32_t)uj;
      }
    }
    const bool neg = (int32_t)t.l[N - 1] < 0;
    E r;
#pragma unroll
    for (int j = 0; j < N; ++j) r.l[j] = neg ? u.l[j] : t.l[j];
    return r;
  }
  // ---- lazy forms (NTT butterflies): no value reduction, limbs may exceed 2^L --------------
  // a + b limb-wise.  Caller keeps limbs below 2^32.
  static KZG_HD E add_lazy(const E& a, const E& b) {
    E r;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      KZG_AUDIT_CHECK((uint64_t)a.l[j] + b.l[j] < (1ull << 32), "a limb wraps 32 bits");
      r.l[j] = a.l[j] + b.l[j];
    }
    return r;
  }
  // a - b + 4p limb-wise, for a normalised b < 2p (e.g. a mul() output): every limb of the
  // redistributed constant P4R dominates the matching limb of b, so no limb goes negative.
  // A normalised b between 2p and a + 4p is also taken (ntt.hip's first_step has one below 4p in pass 2): its lower
  // limbs are still dominated, and the top limb, formed modulo 2^32, is right as soon as the result is carried
  // (carry(), as put_out does) -- such a result must not go to a multiplier un-carried.
  static KZG_HD E sub_lazy4(const E& a, const E& b) {
    KZG_AUDIT_CHECK(audit::big_cmp(audit::value<F>(b.l), audit::value_plus_kp<F>(a.l, 4)) <= 0, "a - b + 4p is negative");
    E r;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      KZG_AUDIT_CHECK(j == N - 1 || F::P4R[j] >= b.l[j], "a limb of 4p does not dominate the subtrahend's");
      KZG_AUDIT_CHECK(j == N - 1 || (uint64_t)a.l[j] + (F::P4R[j] - b.l[j]) < (1ull << 32), "a limb wraps 32 bits");
      r.l[j] = a.l[j] + (F::P4R[j] - b.l[j]);
    }
    return r;
  }
  // carry propagation: limbs back below 2^L (the top limb absorbs the excess), value unchanged
  static KZG_HD E carry(const E& a) {
    E r;
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < N - 1; ++j) {
      KZG_AUDIT_CHECK((uint64_t)a.l[j] + c < (1ull << 32), "a limb wraps 32 bits");
      const uint32_t t = a.l[j] + c;
      r.l[j] = t & MASK;
      c = t >> L;
    }
    r.l[N - 1] = a.l[N - 1] + c;
    return r;
  }

  // ---- lazy forms with normalised limbs (the MSM inner loop) --------------------------------
  // mul / sqr / mul2 only need normalised limbs and a product of the operand VALUES below R*p
  // (R/p > 160 for the two base fields), not weak-normal operands.  So between multiplications
  // a difference is formed as a - b + K*p (K*p >= b, nothing else to decide) and carried, with
  // no conditional subtraction and no signed borrow chain: value in [0, a + K*p), limbs < 2^L.
  template <int K>
  static KZG_HD const uint32_t* pkr() {
    static_assert(K == 2 || K == 4 || K == 6 || K == 8, "no redistributed constant for this multiple of p");
    if constexpr (K == 2) return F::P2R;
    else if constexpr (K == 4) return F::P4R;
    else if constexpr (K == 6) return F::P6R;
    else return F::P8R;
  }
  // a - b + K*p for normalised a, b with b <= K*p.  Every lower limb of the redistributed K*p
  // dominates a normalised limb; the top limb may wrap below zero on the way and is put right by
  // the incoming carry (arithmetic mod 2^32, true value non-negative).
  template <int K>
  static KZG_HD E sub_carry(const E& a, const E& b) {
    const uint32_t* kp = pkr<K>();
    KZG_AUDIT_CHECK(audit::at_most_kp<F>(b.l, K), "subtrahend above K*p");
    KZG_AUDIT_CHECK(audit::normalised<F>(a.l) && audit::normalised<F>(b.l), "operand limbs not normalised");
    E r;
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < N - 1; ++j) {
      KZG_AUDIT_CHECK(audit_limb_ok(a.l[j], kp[j], b.l[j], c), "a limb of K*p does not dominate / wraps");
      const uint32_t t = a.l[j] + (kp[j] - b.l[j]) + c;
      r.l[j] = t & MASK;
      c = t >> L;
    }
    KZG_AUDIT_CHECK(audit_limb_ok(a.l[N - 1], kp[N - 1], b.l[N - 1], c), "top limb negative or above 2^32");
    r.l[N - 1] = a.l[N - 1] + (kp[N - 1] - b.l[N - 1]) + c;
    return r;
  }
  // (neg ? 2p - a : a) - b + K*p for normalised a < 2p and b <= K*p: the conditional negation of a is folded
  // into the carried difference (2 instructions per limb instead of a carried negation of its own).
  template <int K>
  static KZG_HD E sub_carry_cneg(const E& a, bool neg, const E& b) {
    const uint32_t* kp = pkr<K>();
    KZG_AUDIT_CHECK(audit::at_most_kp<F>(b.l, K), "subtrahend above K*p");
    KZG_AUDIT_CHECK(audit::normalised<F>(a.l) && audit::normalised<F>(b.l), "operand limbs not normalised");
    KZG_AUDIT_CHECK(audit::below_kp<F>(a.l, 2), "first operand not below 2p");
    E r;
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      KZG_AUDIT_CHECK(!neg || j == N - 1 || F::P2R[j] >= a.l[j], "a limb of 2p does not dominate the negated operand's");
      const uint32_t aj = neg ? F::P2R[j] - a.l[j] : a.l[j];
      KZG_AUDIT_CHECK(audit_limb_ok(neg ? F::P2R[j] : a.l[j], kp[j], (neg ? a.l[j] : 0u) + b.l[j], c),
                      j < N - 1 ? "a limb of K*p does not dominate / wraps" : "top limb negative or above 2^32");
      const uint32_t t = aj + (kp[j] - b.l[j]) + c;
      if (j < N - 1) { r.l[j] = t & MASK; c = t >> L; } else { r.l[j] = t; }
    }
    return r;
  }
  // a + b + b for normalised operands: value a + 2b, limbs normalised
  static KZG_HD E add_twice_carry(const E& a, const E& b) {
    E r;
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < N - 1; ++j) {
      KZG_AUDIT_CHECK((uint64_t)a.l[j] + 2 * (uint64_t)b.l[j] + c < (1ull << 32), "a limb wraps 32 bits");
      const uint32_t t = a.l[j] + 2 * b.l[j] + c;
      r.l[j] = t & MASK;
      c = t >> L;
    }
    KZG_AUDIT_CHECK((uint64_t)a.l[N - 1] + 2 * (uint64_t)b.l[N - 1] + c < (1ull << 32), "the top limb wraps 32 bits");
    r.l[N - 1] = a.l[N - 1] + 2 * b.l[N - 1] + c;
    return r;
  }

  static KZG_HD E dbl(const E& a) { return add(a, a); }
  static KZG_HD E neg(const E& a) { return sub(zero(), a); }

  // [0, 2p) -> [0, p)
  static KZG_HD E reduce(const E& a) {
    KZG_AUDIT_CHECK(audit::below_kp<F>(a.l, 2), "input not below 2p");
    E t;
    int32_t ct = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int32_t tj = (int32_t)a.l[j] - (int32_t)F::P[j] + ct;
      if (j < N - 1) {
        ct = tj >> L;
        t.l[j] = (uint32_t)tj & MASK;
      } else {
        t.l[j] = (uint32_t)tj;
      }
    }
    const bool neg = (int32_t)t.l[N - 1] < 0;
    E r;
#pragma unroll
    for (int j = 0; j < N; ++j) r.l[j] = neg ? a.l[j] : t.l[j];
    return r;
  }
  // [0, 2^(L*N)) with normalised limbs -> [0, p): the canonical value of a lazily accumulated sum
  // (NTT butterflies: up to 49p) without a multiplication.  Quotient estimate from the top limb:
  // q = floor(top * floor(2^52 / (ptop + 1)) / 2^52) with ptop = top limb of p never exceeds
  // floor(x / p) and falls short of it by at most 1 (the estimate loses < 2^-13 + rounding), so
  // x - q*p is in [0, 2p) and one conditional subtraction finishes.
  static KZG_HD E reduce_wide(const E& a) {
    constexpr uint64_t PTOP1 = (uint64_t)F::P[N - 1] + 1;
    constexpr uint64_t M = (1ull << 52) / PTOP1;
    static_assert(PTOP1 > (1ull << 20), "top limb of p too small for the 52-bit reciprocal");
    KZG_AUDIT_CHECK(audit::normalised<F>(a.l) && (a.l[N - 1] >> L) == 0, "limbs not normalised");
    const uint32_t q = (uint32_t)(((uint64_t)a.l[N - 1] * M) >> 52);
    E r;
    int64_t c = 0;
#pragma unroll
    for (int j = 0; j < N - 1; ++j) {
      const int64_t t = (int64_t)a.l[j] - (int64_t)((uint64_t)q * F::P[j]) + c;
      r.l[j] = (uint32_t)t & MASK;
      c = t >> L;
    }
    KZG_AUDIT_CHECK((int64_t)a.l[N - 1] - (int64_t)((uint64_t)q * F::P[N - 1]) + c >= 0, "quotient estimate above floor(x / p)");
    r.l[N - 1] = (uint32_t)((int64_t)a.l[N - 1] - (int64_t)((uint64_t)q * F::P[N - 1]) + c);
    KZG_AUDIT_CHECK(audit::below_kp<F>(r.l, 2), "quotient estimate leaves 2p or more");
    return reduce(r);
  }
  static KZG_HD bool is_zero(const E& a) {
    const E r = reduce(a);
    uint32_t acc = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) acc |= r.l[j];
    return acc == 0;
  }
  static KZG_HD bool eq(const E& a, const E& b) { return is_zero(sub(a, b)); }
  // zero test without the reduction: a weak-normal value is 0 mod p iff it is the integer 0 or
  // the integer p, and normalised limbs represent an integer uniquely
  static KZG_HD bool is_zero_weak(const E& a) {
    KZG_AUDIT_CHECK(audit::normalised<F>(a.l) && audit::below_kp<F>(a.l, 2), "input not weak-normal");
    uint32_t z = 0, q = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) { z |= a.l[j]; q |= a.l[j] ^ F::P[j]; }
    return z == 0 || q == 0;
  }
  // 2p - a for weak-normal a: normalised limbs, value in (0, 2p] (fine as a mul operand)
  static KZG_HD E neg_weak(const E& a) {
    E r;
    int32_t c = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int32_t t = (int32_t)F::P2[j] - (int32_t)a.l[j] + c;
      if (j < N - 1) { c = t >> L; r.l[j] = (uint32_t)t & MASK; } else { r.l[j] = (uint32_t)t; }
    }
    return r;
  }
  // flag ? p - a : a  for CANONICAL a (table coordinates): result weak-normal in [0, p]
  static KZG_HD E cneg_canonical(const E& a, bool flag) {
    KZG_AUDIT_CHECK(audit::normalised<F>(a.l) && audit::below_kp<F>(a.l, 1), "input not canonical");
    E r;
    int32_t c = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int32_t t = (int32_t)F::P[j] - (int32_t)a.l[j] + c;
      uint32_t v;
      if (j < N - 1) { c = t >> L; v = (uint32_t)t & MASK; } else { v = (uint32_t)t; }
      r.l[j] = flag ? v : a.l[j];
    }
    return r;
  }

  static KZG_HD E to_mont(const E& a) { return mul(a, r2()); }
  static KZG_HD E from_mont(const E& a) { return reduce(mul(a, raw_one())); }

  static KZG_HD E select(bool c, const E& a, const E& b) {
    E r;
#pragma unroll
    for (int j = 0; j < N; ++j) r.l[j] = c ? a.l[j] : b.l[j];
    return r;
  }

  // a^e for a Montgomery-form a; e given as `nw` saturated 32-bit words.
  // Not unrolled: used off the hot path (table construction, host finishing).
  static KZG_HD E pow_words(const E& a, const uint32_t* e, int nw) {
    E r = one();
    for (int k = nw - 1; k >= 0; --k) {
      for (int bit = 31; bit >= 0; --bit) {
        r = mul(r, r);
        if ((e[k] >> bit) & 1u) r = mul(r, a);
      }
    }
    return r;
  }
  // a^(p-2) (Montgomery form in and out); inv(0) = 0
  static KZG_HD E inv(const E& a) {
    uint32_t e[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) e[k] = F::PW[k];
    uint32_t borrow = 2;  // e = p - 2
    for (int k = 0; k < NW && borrow; ++k) {
      const uint32_t old = e[k];
      e[k] = old - borrow;
      borrow = old < borrow ? 1u : 0u;
    }
    return pow_words(a, e, NW);
  }
};

}  // namespace kzg
