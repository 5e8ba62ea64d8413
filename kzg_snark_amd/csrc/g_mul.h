// g_mul.h -- ONE scalar multiplication [k] P, for a point of G1's curve (Ec<C> / XYZZ<C>) and for a point of the twist
// (G2Bytes<C>::J), the arithmetic behind kzg_g1_mul_* / kzg_g2_mul_* (DESIGN.md 4.16).  Shared by the kernels of
// g_mul.hip and the host (tests/shim/g_mul_shim.cpp compiles this text with g++): nothing here is device-only.  At the
// end: how a call is cut into launches (GmPlan) and where a lane's table entries lie, for the same two readers.
//
// The scalar is eight 32-bit words and means the 256-bit integer AS GIVEN: it is not reduced modulo r, so a point
// outside the prime-order subgroup is multiplied by k itself ([r] Q != O there; cofactor clearing is a call of this).
//
// The ladder is verify_points.hip's: k + 0x88..8 read nibble by nibble is the signed radix-16 form of k (digit =
// nibble - 8 in [-8, 7], one more digit 0 / 1 from the carry out of the sum), so 64 windows of four doublings and at
// most one addition of +-|d| P from a table of 1P .. 8P.  The table lives wherever `Tab` puts it (store(e, point),
// load(e), e < GMUL_TABLE): a column of global memory per lane on the device, an array on the host.
//
// Exactness.  Every addition is the full one: an infinite operand, P + P (a doubling) and P + (-P) (infinity) are all
// finished.  They are all reachable: a point of small order q makes the table wrap (3P = O for q = 3, 8P = -5P for
// q = 13) and the accumulator meet +-its operand; on a point of the subgroup a scalar near a multiple of r does the
// same in the last window -- r = 1 (mod 16) on both curves, so k = 2r - 4 = -2 (mod 16) reaches window 0 with the
// accumulator at [2r - 2] P = [-2] P and adds digit -2: a doubling.  k = r + 1 ends with P + P likewise, k = r - d and
// 2r - d with O + [-d] P and [d] P + [-d] P's neighbours.  The table is built with the same addition (2P by the
// doubling, then +P each; for a point of order 3 that is 2P + P = O, then O + P).
//
// One loop holds the table's construction and the ladder, so a kernel holds one doubling and one addition: iteration
// `it` < GMUL_TABLE leaves (it + 1) P in the table, iteration GMUL_TABLE + j is window 63 - j.
#pragma once
#include "g2_bytes.h"

namespace kzg {

constexpr int GMUL_TABLE = 8;                            // multiples 1P .. 8P
constexpr int GMUL_WINDOWS = 64;                         // 4-bit windows of a 256-bit scalar

// e <- e + 0x88..8 (mod 2^256); returns the carry out, digit 64 of the signed form
static KZG_HD uint32_t gmul_recode(uint32_t* e) {
  uint32_t carry = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint64_t t = (uint64_t)e[k] + 0x88888888u + carry;
    e[k] = (uint32_t)t;
    carry = (uint32_t)(t >> 32);
  }
  return carry;
}
// the signed digit of window w of a recoded scalar.  Word w >> 3 is chosen by a chain of selects: no indexed register
// array (verify_points.hip's vpt_word)
static KZG_HD int gmul_digit(const uint32_t* e, int w) {
  uint32_t word = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) word = (w >> 3) == j ? e[j] : word;
  return (int)((word >> ((w & 7) * 4)) & 15u) - 8;
}

// [k] a on G1's curve (a: Montgomery form, on the curve or infinity), as an XYZZ point
template <class C, class Tab>
static KZG_HD XYZZ<C> g1_mul(const Affine<C>& a, const uint32_t* k, Tab& tab) {
  using G = Ec<C>;
  using Fd = Field<typename C::Fp>;
  uint32_t e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) e[j] = k[j];
  const uint32_t carry = gmul_recode(e);
  XYZZ<C> acc = G::from_affine(a);
#pragma unroll 1
  for (int it = 0; it < GMUL_TABLE + GMUL_WINDOWS; ++it) {
    const bool table = it < GMUL_TABLE;
    int ndbl = table ? (it == 1 ? 1 : 0) : 4, entry = table ? (it >= 2 ? 0 : -1) : -1;
    bool negate = false;
    if (!table) {
      if (it == GMUL_TABLE) acc = carry ? tab.load(0) : G::infinity();
      const int digit = gmul_digit(e, GMUL_WINDOWS - 1 - (it - GMUL_TABLE));
      negate = digit < 0;
      entry = (negate ? -digit : digit) - 1;             // -1: digit 0, nothing to add
    }
#pragma unroll 1
    for (int d = 0; d < ndbl; ++d) acc = G::dbl(acc);
    if (entry >= 0) {
      XYZZ<C> t = tab.load(entry);
      if (negate) t.y = Fd::neg(t.y);                    // -O = O: infinity is zz = 0, whatever y holds
      acc = G::add(acc, t);
    }
    if (table) tab.store(it, acc);
  }
  return acc;
}

// [k] (x, y) on the twist (Montgomery form, on the twist; inf: the point at infinity), Jacobian
template <class C, class Tab>
static KZG_HD Jac2<C> g2_mul(const Fp2<C>& x, const Fp2<C>& y, bool inf, const uint32_t* k, Tab& tab) {
  using G = G2Bytes<C>;
  using T = Tower<C>;
  using J = Jac2<C>;
  uint32_t e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) e[j] = k[j];
  const uint32_t carry = gmul_recode(e);
  J acc;
  acc.x = x; acc.y = y;
  acc.z = inf ? T::zero2() : T::one2();
#pragma unroll 1
  for (int it = 0; it < GMUL_TABLE + GMUL_WINDOWS; ++it) {
    const bool table = it < GMUL_TABLE;
    int ndbl = table ? (it == 1 ? 1 : 0) : 4, entry = table ? (it >= 2 ? 0 : -1) : -1;
    bool negate = false;
    if (!table) {
      if (it == GMUL_TABLE) {
        acc = tab.load(0);
        if (!carry) acc.z = T::zero2();
      }
      const int digit = gmul_digit(e, GMUL_WINDOWS - 1 - (it - GMUL_TABLE));
      negate = digit < 0;
      entry = (negate ? -digit : digit) - 1;
    }
    // G2Bytes::add leaves the sum of two equal finite points to its caller: the doubling loop runs once more for it
    bool pending = entry >= 0;
#pragma unroll 1
    for (;;) {
#pragma unroll 1
      for (int d = 0; d < ndbl; ++d) acc = G::dbl(acc);
      if (!pending) break;
      pending = false;
      J t = tab.load(entry);
      if (negate) t.y = T::neg2(t.y);
      ndbl = G::template add<false>(acc, t) ? 1 : 0;
    }
    if (table) tab.store(it, acc);
  }
  return acc;
}

// Jacobian -> canonical affine words x.c0 | x.c1 | y.c0 | y.c1 (zeros for infinity); returns the infinity flag.  One
// inversion in Fp.
template <class C>
static KZG_HD bool g2_to_words(const Jac2<C>& p, uint32_t* w) {
  using G = G2Bytes<C>;
  using T = Tower<C>;
  constexpr int NW = G::NW;
  if (G::is_inf(p)) {
#pragma unroll
    for (int j = 0; j < 4 * NW; ++j) w[j] = 0;
    return true;
  }
  // 1 / z = conj(z) / (z0^2 + z1^2), the power by g2_bytes.h's loop (one squaring and one product, not unrolled)
  const Fe<typename C::Fp> d = G::pow_fixed(G::Fd::add(G::Fd::sqr(p.z.c0), G::Fd::sqr(p.z.c1)), true);
  Fp2<C> zi = T::conj2(p.z);
  zi.c0 = G::Fd::mul(zi.c0, d);
  zi.c1 = G::Fd::mul(zi.c1, d);
  const Fp2<C> zi2 = T::sqr2(zi);
  G::to_words2(T::mul2(p.x, zi2), w);
  G::to_words2(T::mul2(p.y, T::mul2(zi2, zi)), w + 2 * NW);
  return false;
}

// the table of one multiplication in plain memory (the host)
template <class P>
struct GMulHostTab {
  P v[GMUL_TABLE];
  KZG_HD void store(int e, const P& p) { v[e] = p; }
  KZG_HD P load(int e) const { return v[e]; }
};

// k (8 canonical words) < the modulus of F
template <class F>
static KZG_HD bool gmul_scalar_below(const uint32_t* k) {
  return words_below_p<F>(k);
}

// ---- the launches of a call and a lane's column of the table (g_mul.hip; tests/test_g_mul_host.py through the shim) --
constexpr uint32_t GM_TB1 = 256;                          // lanes per workgroup, G1
constexpr uint32_t GM_TB2 = 64;                           // lanes per workgroup, G2: one wave
constexpr uint32_t GM_LAUNCH_LANES1 = 512 * GM_TB1;       // two workgroups per CU
constexpr uint32_t GM_LAUNCH_LANES2 = 256 * GM_TB2;       // one wave per CU
constexpr size_t GM_MAX_POINTS = (size_t)1 << 21;         // the power table's largest exponent

// the lanes of a call split evenly over the fewest launches of at most `cap` lanes (whole workgroups)
struct GmPlan {
  uint32_t blocks, launch_blocks;
  GmPlan(size_t n, uint32_t tb, uint32_t cap) {
    blocks = (uint32_t)((n + tb - 1) / tb);
    const uint32_t cap_blocks = cap / tb, launches = (blocks + cap_blocks - 1) / cap_blocks;
    launch_blocks = launches ? (blocks + launches - 1) / launches : 0;
  }
};

// the table of a launch of `slots` lanes: entry e is `pieces` vectors, piece q of entry e of lane `slot` at
// (e * pieces + q) * slots + slot -- a wave's lanes are adjacent.  The index is 32 bits wide: a table has fewer than
// 2^25 vectors.  gm_entry_index is piece 0 of an entry, gm_piece_index piece q from it.
static KZG_HD uint32_t gm_entry_index(int e, int pieces, uint32_t slots, uint32_t slot) {
  return (uint32_t)(e * pieces) * slots + slot;
}
static KZG_HD uint32_t gm_piece_index(uint32_t entry_idx, int q, uint32_t slots) { return entry_idx + (uint32_t)q * slots; }
// pieces of a table entry: an XYZZ point of G1's curve is 4 N limbs in pieces of 16 bytes, a Jacobian point of the twist
// 6 N limbs (N is odd) in pieces of 8 bytes
template <class C> constexpr int gm_g1_pieces() { return C::Fp::N; }
template <class C> constexpr int gm_g2_pieces() { return 3 * C::Fp::N; }
template <class C> constexpr size_t g1_column_bytes() { return (size_t)GMUL_TABLE * 4 * C::Fp::N * 4; }
template <class C> constexpr size_t g2_column_bytes() { return (size_t)GMUL_TABLE * 6 * C::Fp::N * 4; }

}  // namespace kzg
