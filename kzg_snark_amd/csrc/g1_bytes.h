// g1_bytes.h -- compressed G1 points and membership in the prime-order subgroup, one point at a time: the square
// root in Fp, the sign of y, the byte formats and the subgroup test.  Shared by the kernels of
// g1_bytes.hip and the host (tests/shim/g1_bytes_shim.cpp compiles this text with g++), like field.h and ec.h.
//
// Byte formats: big-endian x, flags in the top bits of byte 0.
//   BLS12-381  48 bytes, ZCash: bit 7 = compressed (must be 1), bit 6 = infinity, bit 5 = y is the larger root;
//              infinity = bit 6 set, bit 5 clear, every other bit zero
//   BN254      32 bytes, gnark: top two bits 10 = finite with the smaller y, 11 = finite with the larger y,
//              01 = infinity (the other 254 bits zero), 00 = not a compressed point
// "larger": canonical y > (p - 1) / 2.  y = 0 cannot occur: neither curve has a point of order 2 (h r is odd).
//
// Status of a point, first failure wins: 0 ok, 1 bad encoding (flags, a malformed infinity, x >= p), 2 x^3 + b is
// not a square (no such point; for affine input: a coordinate >= p or a point off the curve), 3 on the curve but
// outside the subgroup.
//
// A blob reaches these functions as `raw`: its bytes read as SIZE / 4 little-endian 32-bit words in memory order
// (what a vector load leaves in registers), so canonical word k of x is the byte-swapped raw[NW - 1 - k].
#pragma once
#include "ec.h"
#include "g1_words.h"

namespace kzg {

constexpr int G1_OK = 0;
constexpr int G1_BAD_ENCODING = 1;
constexpr int G1_NOT_ON_CURVE = 2;
constexpr int G1_NOT_IN_SUBGROUP = 3;

static KZG_HD uint32_t bswap32(uint32_t v) {
  return (v >> 24) | ((v >> 8) & 0x0000ff00u) | ((v << 8) & 0x00ff0000u) | (v << 24);
}

// compile-time words of (p + 1) / 4 and (p - 1) / 2
template <class F>
struct FpWords {
  uint32_t w[F::NW];
};
template <class F>
constexpr FpWords<F> sqrt_exponent() {          // (p + 1) / 4, p = 3 (mod 4)
  FpWords<F> t = {};
  uint64_t c = 1;
  for (int k = 0; k < F::NW; ++k) { c += F::PW[k]; t.w[k] = (uint32_t)c; c >>= 32; }
  FpWords<F> r = {};
  for (int k = 0; k < F::NW; ++k) r.w[k] = (t.w[k] >> 2) | (k + 1 < F::NW ? t.w[k + 1] << 30 : (uint32_t)c << 30);
  return r;
}
template <class F>
constexpr FpWords<F> half_modulus() {           // (p - 1) / 2 = p >> 1, p odd
  FpWords<F> r = {};
  for (int k = 0; k < F::NW; ++k) r.w[k] = (F::PW[k] >> 1) | (k + 1 < F::NW ? F::PW[k + 1] << 31 : 0u);
  return r;
}

template <class F>
struct FpRoot {
  using Fd = Field<F>;
  using E = Fe<F>;
  static_assert((F::PW[0] & 3u) == 3u, "the square root by one power needs p = 3 (mod 4)");
  static constexpr FpWords<F> EXP = sqrt_exponent<F>();
  static constexpr FpWords<F> HALF = half_modulus<F>();

  // word k of the exponent for a k only known at run time, as a chain of selects over compile-time constants: the
  // words stay immediates of the instruction stream (the same for every lane), no table in memory, no indexed array
  static KZG_HD uint32_t exp_word(int k) {
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < F::NW; ++j) w = k == j ? EXP.w[j] : w;
    return w;
  }

  // a^((p+1)/4) by square-and-multiply from the top bit, ONE loop body (a square, and a product under a branch every
  // lane takes alike): BITS - 2 squarings and about half as many products.  A fixed 4-bit window would halve the
  // products but keeps 15 powers of a alive -- 195 registers for BLS12-381 next to the multiplier's own -- so it is
  // not taken.  Montgomery form in, weak-normal Montgomery form out.
  static KZG_HD E pow_sqrt(const E& a) {
    E r = Fd::one();
    bool started = false;
#pragma unroll 1
    for (int i = 32 * F::NW - 1; i >= 0; --i) {
      const bool bit = (exp_word(i >> 5) >> (i & 31)) & 1u;
      if (started) r = Fd::sqr(r);
      if (bit) { r = started ? Fd::mul(r, a) : a; started = true; }
    }
    return r;
  }
  // root = a candidate square root of a; true iff a is a square (the candidate squared is compared with a: the
  // residue test).  a = 0 gives root 0, true.
  static KZG_HD bool sqrt(const E& a, E& root) {
    root = pow_sqrt(a);
    return Fd::eq(Fd::sqr(root), a);
  }
  // canonical words > (p - 1) / 2, from the top word down
  static KZG_HD bool words_above_half(const uint32_t* w) {
    bool lt = false, gt = false;
#pragma unroll
    for (int k = F::NW - 1; k >= 0; --k) {
      const uint32_t h = HALF.w[k];
      if (!lt && !gt) { lt = w[k] < h; gt = w[k] > h; }
    }
    return gt;
  }
};

// a square root of a in Fp (Montgomery form in, weak-normal out); false: a is not a square
template <class F>
static KZG_HD bool fp_sqrt(const Fe<F>& a, Fe<F>& root) { return FpRoot<F>::sqrt(a, root); }

template <class C>
struct G1Bytes {
  using F = typename C::Fp;
  using Fd = Field<F>;
  using E = Fe<F>;
  using Root = FpRoot<F>;
  static constexpr int NW = F::NW;
  static constexpr int SIZE = 4 * NW;                    // bytes of a compressed point: 48 / 32
  static constexpr bool ZCASH = C::ID == 1;              // BLS12-381; otherwise gnark's two-flag format (BN254)
  static constexpr int FLAG_BITS = ZCASH ? 3 : 2;
  static_assert(F::BITS + FLAG_BITS <= 32 * NW, "the flags share the top byte with x");

  static KZG_HD E curve_b() {
    E b;
#pragma unroll
    for (int j = 0; j < F::N; ++j) b.l[j] = C::B_MONT[j];
    return b;
  }

  // [|u|] pt by double-and-add from the top bit of the 64-bit curve parameter: 63 doublings, 5 additions (u has six
  // set bits).  One loop body; ec.h's dbl / add are exact for every input, infinity included.
  static KZG_HD XYZZ<C> mul_u(const XYZZ<C>& pt) {
    XYZZ<C> acc = pt;
#pragma unroll 1
    for (int b = 62; b >= 0; --b) {
      acc = Ec<C>::dbl(acc);
      if ((C::U_ABS >> b) & 1ull) acc = Ec<C>::add(acc, pt);
    }
    return acc;
  }

  // Is the finite point (x, y) ON THE CURVE (Montgomery form) in the subgroup of prime order r?
  //   BLS12-381: r = u^4 - u^2 + 1 and the endomorphism phi(x, y) = (beta x, y) acts on G1 as -u^2, so a point of G1
  //     satisfies phi(P) = -[u^2] P; conversely a point of E(Fp) that satisfies it lies in G1 (Scott, "A note on group
  //     membership tests for G1, G2 and GT on BLS pairing-friendly curves", 2021): the test is exact.  [u^2] P is
  //     [u]([u] P), at most 126 doublings and 10 additions against 255 and ~128 for [r] P; the comparison is
  //     projective (beta x ZZ = X, y ZZZ = -Y), no inversion.  A finite P with [u^2] P = O is outside G1: rejected.
  //   BN254: the cofactor is 1, every point of the curve is in the subgroup: nothing to compute.
  static KZG_HD bool in_subgroup(const E& x, const E& y) {
    if constexpr (ZCASH) {
      XYZZ<C> q;
      q.x = x; q.y = y; q.zz = Fd::one(); q.zzz = Fd::one();
#pragma unroll 1
      for (int rep = 0; rep < 2; ++rep) q = mul_u(q);
      if (Ec<C>::is_inf(q)) return false;
      E beta;
#pragma unroll
      for (int j = 0; j < F::N; ++j) beta.l[j] = C::BETA_MONT[j];
      const bool x_ok = Fd::eq(Fd::mul(Fd::mul(beta, x), q.zz), q.x);
      const bool y_ok = Fd::is_zero(Fd::add(Fd::mul(y, q.zzz), q.y));
      return x_ok && y_ok;
    } else {
      (void)x; (void)y;
      return true;
    }
  }

  // blob -> canonical affine words (wx | wy, zeros for infinity or a failed point) and the infinity flag
  static KZG_HD int decode(const uint32_t* raw, bool check_subgroup, uint32_t* wx, uint32_t* wy, bool& inf) {
    uint32_t w[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) { w[k] = bswap32(raw[NW - 1 - k]); wx[k] = 0; wy[k] = 0; }
    inf = false;
    const uint32_t flags = w[NW - 1] >> (32 - FLAG_BITS);
    w[NW - 1] &= 0xffffffffu >> FLAG_BITS;
    uint32_t any = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) any |= w[k];
    bool larger;
    if constexpr (ZCASH) {
      if (!(flags & 4u)) return G1_BAD_ENCODING;
      if (flags & 2u) {
        if (flags != 6u || any) return G1_BAD_ENCODING;
        inf = true;
        return G1_OK;
      }
      larger = flags & 1u;
    } else {
      if (flags == 0u) return G1_BAD_ENCODING;
      if (flags == 1u) {
        if (any) return G1_BAD_ENCODING;
        inf = true;
        return G1_OK;
      }
      larger = flags == 3u;
    }
    if (!words_below_p<F>(w)) return G1_BAD_ENCODING;
    const E x = Fd::to_mont(Fd::from_words(w));
    E y;
    if (!fp_sqrt<F>(Fd::add(Fd::mul(Fd::sqr(x), x), curve_b()), y)) return G1_NOT_ON_CURVE;
    uint32_t yw[NW];
    Fd::to_words(Fd::from_mont(y), yw);
    if (Root::words_above_half(yw) != larger) {
      y = Fd::neg(y);
      Fd::to_words(Fd::from_mont(y), yw);
    }
    if (check_subgroup && !in_subgroup(x, y)) return G1_NOT_IN_SUBGROUP;
#pragma unroll
    for (int k = 0; k < NW; ++k) { wx[k] = w[k]; wy[k] = yw[k]; }
    return G1_OK;
  }

  // canonical affine words of a point of the curve (or infinity) -> blob.  Only x and the sign of y enter.
  static KZG_HD void encode(const uint32_t* wx, const uint32_t* wy, bool inf, uint32_t* raw) {
    uint32_t w[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) w[k] = inf ? 0u : wx[k];
    const bool larger = !inf && Root::words_above_half(wy);
    const uint32_t flags = ZCASH ? (inf ? 6u : larger ? 5u : 4u) : (inf ? 1u : larger ? 3u : 2u);
    w[NW - 1] |= flags << (32 - FLAG_BITS);
#pragma unroll
    for (int k = 0; k < NW; ++k) raw[NW - 1 - k] = bswap32(w[k]);
  }

  // status of an affine point: 0, 2 (a coordinate >= p or off the curve: g1_words.h's import_affine) or 3
  static KZG_HD int check_affine(const uint32_t* wx, const uint32_t* wy, bool inf) {
    if (inf) return G1_OK;
    E x, y;
    if (!import_affine<C>(wx, wy, x, y)) return G1_NOT_ON_CURVE;
    return in_subgroup(x, y) ? G1_OK : G1_NOT_IN_SUBGROUP;
  }
};

}  // namespace kzg
