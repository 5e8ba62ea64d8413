// g2_bytes.h -- compressed G2 points and membership in the prime-order subgroup of the twist, one point at a time: the
// square root in Fp2, the sign of y, the byte formats and the endomorphism-based subgroup tests.  The
// G2 half of g1_bytes.h, on Fp2<C> / Tower<C> of fp_tower.h and Field of field.h; shared by the kernels of g2_bytes.hip
// and the host (tests/shim/g2_bytes_shim.cpp compiles this text with g++): nothing here is device-only.
//
// Byte formats: big-endian x.c1 then x.c0 (x = x.c0 + x.c1 i), the flags of the G1 format in the top bits of byte 0.
//   BLS12-381  96 bytes, ZCash: bit 7 = compressed (must be 1), bit 6 = infinity, bit 5 = y is the larger root;
//              infinity = c0 and 95 zero bytes
//   BN254      64 bytes, gnark: top two bits 10 = finite with the smaller y, 11 = finite with the larger y,
//              01 = infinity (40 and 63 zero bytes), 00 = not a compressed point
// "larger" is lexicographic, c1 first: y.c1 > (p - 1) / 2, or y.c1 = 0 and y.c0 > (p - 1) / 2.
//
// Status of a point, first failure wins: 0 ok, 1 bad encoding (flags, a malformed infinity, x.c0 or x.c1 >= p),
// 2 x^3 + b' is not a square in Fp2 (for affine input: a coordinate >= p or a point off the twist), 3 on the twist but
// outside the subgroup of order r.  Status 3 exists on both curves: BN254's twist has a cofactor too.
//
// A blob reaches these functions as `raw`: its bytes read as SIZE / 4 little-endian 32-bit words in memory order, so
// canonical word k of x.c1 is the byte-swapped raw[NW - 1 - k] and of x.c0 the byte-swapped raw[2 NW - 1 - k].  An
// affine point is 4 NW canonical words x.c0 | x.c1 | y.c0 | y.c1, kzg_pairing_check's layout.
#pragma once
#include "fp_tower.h"
#include "g1_bytes.h"

namespace kzg {

constexpr int G2_OK = 0;
constexpr int G2_BAD_ENCODING = 1;
constexpr int G2_NOT_ON_CURVE = 2;
constexpr int G2_NOT_IN_SUBGROUP = 3;

// a point of the twist in Jacobian coordinates: (X / Z^2, Y / Z^3), Z = 0 for infinity
template <class C>
struct Jac2 {
  Fp2<C> x, y, z;
};

template <class F>
constexpr FpWords<F> inverse_exponent() {       // p - 2
  FpWords<F> r = {};
  uint32_t borrow = 2;
  for (int k = 0; k < F::NW; ++k) { r.w[k] = F::PW[k] - borrow; borrow = F::PW[k] < borrow ? 1u : 0u; }
  return r;
}

template <class C>
struct G2Bytes {
  using F = typename C::Fp;
  using Fd = Field<F>;
  using E = Fe<F>;
  using E2 = Fp2<C>;
  using T = Tower<C>;
  using J = Jac2<C>;
  using Root = FpRoot<F>;
  static constexpr int NW = F::NW;
  static constexpr int SIZE = 8 * NW;                    // bytes of a compressed point: 96 / 64
  static constexpr bool ZCASH = C::ID == 1;
  static constexpr int FLAG_BITS = ZCASH ? 3 : 2;
  static constexpr FpWords<F> INV_EXP = inverse_exponent<F>();

  // ---- the square root in Fp2 ------------------------------------------------------------------------------------
  // a^((p+1)/4) (inverse = false, FpRoot::pow_sqrt's power) or a^(p-2) (inverse = true; 0 for a = 0), the loop of
  // FpRoot::pow_sqrt with the exponent's words chosen from both constants (immediates, no table)
  static KZG_HD E pow_fixed(const E& a, bool inverse) {
    E r = Fd::one();
    bool started = false;
#pragma unroll 1
    for (int i = 32 * NW - 1; i >= 0; --i) {
      uint32_t w = 0;
#pragma unroll
      for (int j = 0; j < NW; ++j) w = (i >> 5) == j ? (inverse ? INV_EXP.w[j] : Root::EXP.w[j]) : w;
      const bool bit = (w >> (i & 31)) & 1u;
      if (started) r = Fd::sqr(r);
      if (bit) { r = started ? Fd::mul(r, a) : a; started = true; }
    }
    return r;
  }
  // The complex method, p = 3 (mod 4), i^2 = -1.  For a = a0 + a1 i with a1 != 0: a is a square iff its norm
  // n = a0^2 + a1^2 is a square of Fp; with s = sqrt(n), one of d = (a0 + s) / 2 and d' = (a0 - s) / 2 is a square
  // (d d' = -a1^2 / 4 is not one) and the root is x0 + x1 i with x0^2 = that one and x1 = a1 / (2 x0).  One power
  // serves both: t = d^((p+1)/4) squares to d (then x0 = t, x1 = a1 / (2t)) or to -d (then x1 = t and x0 = a1 / (2t),
  // since x0^2 - x1^2 = d' + d = a0).  a1 = 0: the root is sqrt(a0) when a0 is a residue and sqrt(-a0) i when not
  // (exactly one of a0, -a0 is a residue); a = 0 gives 0.  Three powers in Fp -- sqrt(n), t and the inversion --
  // against two powers in Fp2 for a^((p^2+7)/16)-style methods (the count is in DESIGN.md 4.14).
  // Montgomery form in, weak-normal out; false: a is not a square (root = 0).
  static KZG_HD bool sqrt2(const E2& a, E2& root) {
    E half;
#pragma unroll
    for (int j = 0; j < F::N; ++j) half.l[j] = C::HALF_MONT[j];
    const bool real = Fd::is_zero(a.c1);
    // the three powers in ONE loop, so the kernel holds one copy of the power: round 0: s = sqrt(n) (a1 = 0:
    // sqrt(a0)), round 1: t (a1 = 0: sqrt(-a0)), round 2: 1 / (2t)
    E in = Fd::select(real, a.c0, Fd::add(Fd::sqr(a.c0), Fd::sqr(a.c1)));
    E s = Fd::zero(), t = Fd::zero(), w = Fd::zero();
    bool first_sq = false, second_sq = false;
#pragma unroll 1
    for (int round = 0; round < 3; ++round) {
      const E out = pow_fixed(in, round == 2);
      if (round == 2) { w = Fd::mul(a.c1, out); break; }
      const bool sq = Fd::eq(Fd::sqr(out), in);
      if (round == 0) {
        s = out; first_sq = sq;
        in = Fd::select(real, Fd::neg(a.c0), Fd::mul(Fd::add(a.c0, s), half));
      } else {
        t = out; second_sq = sq;
        in = Fd::dbl(t);
      }
    }
    root = T::zero2();
    if (real) {
      if (first_sq) root.c0 = s; else root.c1 = t;
      return true;
    }
    if (!first_sq) return false;
    root.c0 = Fd::select(second_sq, t, w);
    root.c1 = Fd::select(second_sq, w, t);
    return true;
  }

  // canonical words of y: is y the larger of y, -y?
  static KZG_HD bool larger_y(const uint32_t* y0, const uint32_t* y1) {
    uint32_t any1 = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) any1 |= y1[k];
    return any1 ? Root::words_above_half(y1) : Root::words_above_half(y0);
  }

  // ---- the group law on the twist, Jacobian, exact for every input ----------------------------------------------------
  static KZG_HD bool is_inf(const J& p) { return T::is_zero2(p.z); }
  // 2P (a = 0; dbl-2009-l).  Z = 0 stays 0, and Y = 0 gives Z3 = 0: the double of a point of order 2 is infinity.
  static KZG_HD J dbl(const J& p) {
    const E2 A = T::sqr2(p.x), B = T::sqr2(p.y), Cc = T::sqr2(B);
    E2 D = T::sub2(T::sub2(T::sqr2(T::add2(p.x, B)), A), Cc);
    D = T::dbl2(D);
    const E2 Ee = T::add2(T::dbl2(A), A);
    J r;
    r.x = T::sub2(T::sqr2(Ee), T::dbl2(D));
    r.y = T::sub2(T::mul2(Ee, T::sub2(D, r.x)), T::dbl2(T::dbl2(T::dbl2(Cc))));
    r.z = T::dbl2(T::mul2(p.y, p.z));
    return r;
  }
  // p <- p + q (add-2007-bl without its doublings; MIXED: q.z is taken for 1 and never read, madd-2007-bl).  Returns
  // true, and leaves p as it was, when p and q are the same finite point: the caller doubles p instead.  Every other
  // case is finished here: an infinite operand, and q = -p.
  template <bool MIXED>
  static KZG_HD bool add(J& p, const J& q) {
    if (!MIXED && is_inf(q)) return false;
    if (is_inf(p)) {
      p.x = q.x; p.y = q.y;
      if (MIXED) p.z = T::one2(); else p.z = q.z;
      return false;
    }
    const E2 z1z1 = T::sqr2(p.z);
    E2 u1 = p.x, s1 = p.y;
    if (!MIXED) {
      const E2 z2z2 = T::sqr2(q.z);
      u1 = T::mul2(p.x, z2z2);
      s1 = T::mul2(T::mul2(p.y, q.z), z2z2);
    }
    const E2 h = T::sub2(T::mul2(q.x, z1z1), u1);
    const E2 rr = T::sub2(T::mul2(T::mul2(q.y, p.z), z1z1), s1);
    if (T::is_zero2(h)) {
      if (T::is_zero2(rr)) return true;
      p.z = T::zero2();
      return false;
    }
    const E2 hh = T::sqr2(h), hhh = T::mul2(h, hh), v = T::mul2(u1, hh);
    p.z = T::mul2(MIXED ? p.z : T::mul2(p.z, q.z), h);
    p.x = T::sub2(T::sub2(T::sqr2(rr), hhh), T::dbl2(v));
    p.y = T::sub2(T::mul2(rr, T::sub2(v, p.x)), T::mul2(s1, hhh));
    return false;
  }
  // psi = twist o Frobenius o untwist, an endomorphism of E'(Fp2) that acts on G2 as multiplication by p (mod r):
  // (x, y) -> (conj(x) PSI_X, conj(y) PSI_Y); in Jacobian coordinates Z goes to conj(Z)
  static KZG_HD J psi(const J& p) {
    J r;
    r.x = T::mul2(T::conj2(p.x), T::const2(C::PSI_X));
    r.y = T::mul2(T::conj2(p.y), T::const2(C::PSI_Y));
    r.z = T::conj2(p.z);
    return r;
  }

  // Is the finite point (x, y) ON THE TWIST (Montgomery form) in the subgroup of order r?  Both tests are exact:
  //   BLS12-381: psi(Q) = [u] Q (Scott, "A note on group membership tests for G1, G2 and GT on BLS pairing-friendly
  //     curves", 2021).  u < 0: the test is psi(Q) + [|u|] Q = O.
  //   BN254: [u + 1] Q + psi([u] Q) + psi^2([u] Q) = psi^3([2u] Q) (El Housni, Guillevic, Piellard, "Co-factor
  //     clearing and subgroup membership testing on pairing-friendly curves", 2022), as
  //     [u] Q + Q + psi(A) + psi^2(A) - psi^3(A) - psi^3(A) = O with A = [u] Q.
  // ONE loop runs both: the BODY steps of the double-and-add of |u| from the bit below its top bit (63 steps on
  // BLS12-381, 62 on BN254), then the additions of the closing sum, so the kernel holds one doubling and one addition.  An addition that meets its own operand (a point
  // of small order can) asks for a doubling, which the loop's doubling does.
  static constexpr int top_bit(uint64_t v) { int t = 63; while (!((v >> t) & 1ull)) --t; return t; }
  static constexpr int BODY = top_bit(C::U_ABS);
  static constexpr int TAIL = ZCASH ? 1 : 5;
  // src.get(x, y): the affine point in Montgomery form.  It is fetched again at every addition (six on BLS12-381)
  // instead of being kept: a kernel lane holds the accumulator and one operand, and reads Q from memory.
  template <class Src>
  static KZG_HD bool in_subgroup(const Src& src) {
    J acc, opnd;
    src.get(acc.x, acc.y);
    acc.z = T::one2();
    opnd = acc;
    bool redo = false;
#pragma unroll 1
    for (int step = 0; step < BODY + TAIL;) {
      const bool body = step < BODY;
      if (body || redo) acc = dbl(acc);
      if (redo) { redo = false; ++step; continue; }
      const int k = step - BODY;
      const bool adds = body ? ((C::U_ABS >> (body ? BODY - 1 - step : 0)) & 1ull) != 0 : true;
      if (adds) {
        // the operand.  Body: Q.  Closing step k: BLS12-381: psi(Q).  BN254: Q, psi(A), psi^2(A), -psi^3(A),
        // -psi^3(A) with A = [u] Q, the accumulator after the body (opnd holds A, then its images).
        if (ZCASH) {
          src.get(opnd.x, opnd.y);
          if (!body) opnd = psi(opnd);
        } else {
          if (k == 0) opnd = acc;
          if (k >= 1 && k <= 3) { opnd = psi(opnd); if (k == 3) opnd.y = T::neg2(opnd.y); }
        }
        if (ZCASH) {
          redo = add<true>(acc, opnd);
        } else {
          J q = opnd;
          if (k <= 0) { src.get(q.x, q.y); q.z = T::one2(); }
          redo = add<false>(acc, q);
        }
        if (redo) continue;
      }
      ++step;
    }
    return is_inf(acc);
  }
  // the point kept by value (the host, and tests)
  struct Held {
    E2 x, y;
    KZG_HD void get(E2& ox, E2& oy) const { ox = x; oy = y; }
  };
  // the point as canonical words in memory, converted at every fetch
  struct InWords {
    const uint32_t* w;
    KZG_HD void get(E2& ox, E2& oy) const {
      ox.c0 = Fd::to_mont(Fd::from_words(w)); ox.c1 = Fd::to_mont(Fd::from_words(w + NW));
      oy.c0 = Fd::to_mont(Fd::from_words(w + 2 * NW)); oy.c1 = Fd::to_mont(Fd::from_words(w + 3 * NW));
    }
  };

  // ---- bytes ----------------------------------------------------------------------------------------------------------
  static KZG_HD void to_words2(const E2& a, uint32_t* w) {
    Fd::to_words(Fd::from_mont(a.c0), w);
    Fd::to_words(Fd::from_mont(a.c1), w + NW);
  }

  // blob -> canonical affine words (x.c0 | x.c1 | y.c0 | y.c1, zeros for infinity or a failed point) and the flag
  static KZG_HD int decode(const uint32_t* raw, bool check_subgroup, uint32_t* out, bool& inf) {
    uint32_t w0[NW], w1[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) { w1[k] = bswap32(raw[NW - 1 - k]); w0[k] = bswap32(raw[2 * NW - 1 - k]); }
#pragma unroll
    for (int k = 0; k < 4 * NW; ++k) out[k] = 0;
    inf = false;
    const uint32_t flags = w1[NW - 1] >> (32 - FLAG_BITS);
    w1[NW - 1] &= 0xffffffffu >> FLAG_BITS;
    uint32_t any = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) any |= w0[k] | w1[k];
    bool larger;
    if constexpr (ZCASH) {
      if (!(flags & 4u)) return G2_BAD_ENCODING;
      if (flags & 2u) {
        if (flags != 6u || any) return G2_BAD_ENCODING;
        inf = true;
        return G2_OK;
      }
      larger = flags & 1u;
    } else {
      if (flags == 0u) return G2_BAD_ENCODING;
      if (flags == 1u) {
        if (any) return G2_BAD_ENCODING;
        inf = true;
        return G2_OK;
      }
      larger = flags == 3u;
    }
    if (!words_below_p<F>(w0) || !words_below_p<F>(w1)) return G2_BAD_ENCODING;
    E2 x, y;
    x.c0 = Fd::to_mont(Fd::from_words(w0));
    x.c1 = Fd::to_mont(Fd::from_words(w1));
    if (!sqrt2(T::add2(T::mul2(T::sqr2(x), x), T::const2(C::TWIST_B)), y)) return G2_NOT_ON_CURVE;
    uint32_t yw[2 * NW];
    to_words2(y, yw);
    if (larger_y(yw, yw + NW) != larger) {
      y = T::neg2(y);
      to_words2(y, yw);
    }
    if (check_subgroup && !in_subgroup(Held{x, y})) return G2_NOT_IN_SUBGROUP;
#pragma unroll
    for (int k = 0; k < NW; ++k) { out[k] = w0[k]; out[NW + k] = w1[k]; out[2 * NW + k] = yw[k]; out[3 * NW + k] = yw[NW + k]; }
    return G2_OK;
  }

  // canonical affine words of a point of the twist (or infinity) -> blob.  Only x and the sign of y enter.
  static KZG_HD void encode(const uint32_t* w, bool inf, uint32_t* raw) {
    const bool larger = !inf && larger_y(w + 2 * NW, w + 3 * NW);
    const uint32_t flags = ZCASH ? (inf ? 6u : larger ? 5u : 4u) : (inf ? 1u : larger ? 3u : 2u);
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      uint32_t v1 = inf ? 0u : w[NW + k];
      if (k == NW - 1) v1 |= flags << (32 - FLAG_BITS);
      raw[NW - 1 - k] = bswap32(v1);
      raw[2 * NW - 1 - k] = bswap32(inf ? 0u : w[k]);
    }
  }

  // status of an affine point: 0, 2 (a coordinate >= p or off the twist: fp_tower.h's import_g2) or 3.  w stays
  // readable throughout: the subgroup test fetches the point from it
  static KZG_HD int check_affine(const uint32_t* w, bool inf) {
    if (inf) return G2_OK;
    {
      E2 x, y;
      if (!T::import_g2(w, x, y)) return G2_NOT_ON_CURVE;
    }
    return in_subgroup(InWords{w}) ? G2_OK : G2_NOT_IN_SUBGROUP;
  }
};

}  // namespace kzg
