// sha256.h -- the SHA-256 compression function (FIPS 180-4) and the reduction of a digest into a scalar field, one
// text for the kernels of blob.hip and for the host (tests/shim/blob_shim.cpp compiles it with g++), like g1_bytes.h
// (DESIGN.md 4.11).
//
// sha256_compress is 64 rounds written out: the eight working variables rotate by NAME from round to round and the
// message schedule is a rolling window of 16 words, every index a literal.  Nothing is indexed at run time, so state,
// window and temporaries live in registers (an array indexed by a loop counter would go to scratch).
#pragma once
#include <stdint.h>
#include "field.h"

namespace kzg {

#if defined(__has_builtin)
#if __has_builtin(__builtin_rotateright32)
#define KZG_SHA_ROTR(x, n) __builtin_rotateright32((x), (n))
#endif
#endif
#ifndef KZG_SHA_ROTR
#define KZG_SHA_ROTR(x, n) (((x) >> (n)) | ((x) << (32 - (n))))      // a compiler without the builtin: the rotate idiom
#endif

// the four bytes of a 32-bit load in the other order: a big-endian word from little-endian memory and back
static KZG_HD uint32_t sha_bswap32(uint32_t v) { return __builtin_bswap32(v); }

struct Sha256 {
  // the first 32 bits of the fractional parts of the cube roots of the first 64 primes
  static constexpr uint32_t K[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
      0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
      0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
      0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
      0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
      0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
      0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
      0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
  // the first 32 bits of the fractional parts of the square roots of the first 8 primes
  static constexpr uint32_t H0[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                                     0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
};

static KZG_HD void sha256_init(uint32_t state[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) state[k] = Sha256::H0[k];
}

// round I (a literal) on the working variables named a .. h; for I >= 16 the window word I mod 16 is first replaced by
// W[I] = s1(W[I-2]) + W[I-7] + s0(W[I-15]) + W[I-16]
#define KZG_SHA_ROUND(a, b, c, d, e, f, g, h, I)                                                                    \
  do {                                                                                                              \
    if ((I) >= 16) {                                                                                                \
      const uint32_t w2 = m[((I) + 14) & 15], w15 = m[((I) + 1) & 15];                                              \
      m[(I) & 15] += (KZG_SHA_ROTR(w2, 17) ^ KZG_SHA_ROTR(w2, 19) ^ (w2 >> 10)) + m[((I) + 9) & 15] +               \
                     (KZG_SHA_ROTR(w15, 7) ^ KZG_SHA_ROTR(w15, 18) ^ (w15 >> 3));                                   \
    }                                                                                                               \
    const uint32_t t1 = (h) + (KZG_SHA_ROTR(e, 6) ^ KZG_SHA_ROTR(e, 11) ^ KZG_SHA_ROTR(e, 25)) +                    \
                        ((g) ^ ((e) & ((f) ^ (g)))) + Sha256::K[I] + m[(I) & 15];                                   \
    const uint32_t t2 = (KZG_SHA_ROTR(a, 2) ^ KZG_SHA_ROTR(a, 13) ^ KZG_SHA_ROTR(a, 22)) +                          \
                        (((a) & (b)) | ((c) & ((a) | (b))));                                                        \
    (d) += t1;                                                                                                      \
    (h) = t1 + t2;                                                                                                  \
  } while (0)
// rounds I .. I + 7: after eight rounds the names are back where they started
#define KZG_SHA_ROUNDS8(I)                       \
  KZG_SHA_ROUND(a, b, c, d, e, f, g, h, (I) + 0); \
  KZG_SHA_ROUND(h, a, b, c, d, e, f, g, (I) + 1); \
  KZG_SHA_ROUND(g, h, a, b, c, d, e, f, (I) + 2); \
  KZG_SHA_ROUND(f, g, h, a, b, c, d, e, (I) + 3); \
  KZG_SHA_ROUND(e, f, g, h, a, b, c, d, (I) + 4); \
  KZG_SHA_ROUND(d, e, f, g, h, a, b, c, (I) + 5); \
  KZG_SHA_ROUND(c, d, e, f, g, h, a, b, (I) + 6); \
  KZG_SHA_ROUND(b, c, d, e, f, g, h, a, (I) + 7)

// state <- the compression of one 64-byte block; w: its sixteen words as BIG-endian numbers (FIPS 180-4 6.2.2)
static KZG_HD void sha256_compress(uint32_t state[8], const uint32_t w[16]) {
  uint32_t m[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) m[k] = w[k];
  uint32_t a = state[0], b = state[1], c = state[2], d = state[3], e = state[4], f = state[5], g = state[6],
           h = state[7];
  KZG_SHA_ROUNDS8(0);
  KZG_SHA_ROUNDS8(8);
  KZG_SHA_ROUNDS8(16);
  KZG_SHA_ROUNDS8(24);
  KZG_SHA_ROUNDS8(32);
  KZG_SHA_ROUNDS8(40);
  KZG_SHA_ROUNDS8(48);
  KZG_SHA_ROUNDS8(56);
  state[0] += a; state[1] += b; state[2] += c; state[3] += d;
  state[4] += e; state[5] += f; state[6] += g; state[7] += h;
}

#undef KZG_SHA_ROUNDS8
#undef KZG_SHA_ROUND

// floor(2^256 / r) for the modulus of F (r is odd: it does not divide 2^256): how many times r can be taken from a
// 256-bit number.  2 on BLS12-381 (r ~ 2^254.86), 5 on BN254 (r ~ 2^253.6).
template <class F>
constexpr int digest_trips() {
  static_assert(F::NW == 8, "scalar fields of 8 words");
  uint32_t acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  int trips = 0;
  while (true) {
    uint64_t c = 0;
    for (int k = 0; k < 8; ++k) { c += (uint64_t)acc[k] + F::PW[k]; acc[k] = (uint32_t)c; c >>= 32; }
    acc[8] += (uint32_t)c;
    if (acc[8]) return trips;                     // (trips + 1) r >= 2^256
    ++trips;
  }
}
static_assert(digest_trips<BlsFr>() == 2 && digest_trips<BnFr>() == 5, "floor(2^256 / r)");

// the digest read as ONE 256-bit big-endian integer (digest[0] its top word), reduced mod r: out = four canonical
// little-endian 64-bit limbs.  digest_trips conditional subtractions, a fixed count per field: a 256-bit number is
// below (trips + 1) r.
template <class F>
static KZG_HD void fr_from_digest(const uint32_t digest[8], uint64_t out[4]) {
  uint32_t v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = digest[7 - k];
#pragma unroll
  for (int trip = 0; trip < digest_trips<F>(); ++trip) {
    uint32_t t[8];
    uint32_t borrow = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint64_t d = (uint64_t)v[k] - F::PW[k] - borrow;
      t[k] = (uint32_t)d;
      borrow = (uint32_t)(d >> 63);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = borrow ? v[k] : t[k];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) out[j] = (uint64_t)v[2 * j] | ((uint64_t)v[2 * j + 1] << 32);
}

}  // namespace kzg
