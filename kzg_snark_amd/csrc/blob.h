// blob.h -- an EIP-4844 blob as bytes, one blob (or one element) at a time: the canonicity check of a 32-byte
// big-endian field element, its inverse (limbs back to bytes) and the Fiat-Shamir challenge of a blob
// and its commitment.  Shared by the kernels of blob.hip and the host (tests/shim/blob_shim.cpp and
// cells_shim.cpp compile this text with g++), like g1_bytes.h.
//
// The challenge of blob j is the SHA-256 digest, reduced mod r, of
//     "FSBLOBVERIFY_V1_" | n as 16 bytes big-endian | blob (n * 32 bytes) | commitment (G bytes)
// (compute_challenge of EIP-4844's polynomial-commitments specification; n = 4096, G = 48 there).  G is the size of a
// compressed G1 point as g1_bytes.h fixes it: 48 on BLS12-381 (ZCash's format), 32 on BN254 (gnark's).  BN254 has no
// standard for this hash: it is the same construction over its own r and its own point bytes.
//
// Block layout (64-byte blocks, n a power of two >= 2): the 32-byte header makes block 0 = header | element 0; block k,
// 0 < k < n/2, = elements 2k - 1 and 2k; what is left -- element n - 1, the commitment, the FIPS 180-4 padding (0x80,
// zeros, the bit length as 8 bytes big-endian) -- fills the tail blocks, whose number and content follow from the
// lengths alone: on BLS12-381 element | 32 commitment bytes, then 16 commitment bytes | padding; on BN254
// element | commitment, then a block of padding alone.  n/2 + 2 blocks in all on both: 2,050 at n = 4096.
//
// Memory reaches these functions as `raw` words: bytes read as little-endian 32-bit words in memory order (what a
// vector load leaves in registers), as in g1_bytes.h.
#pragma once
#include "sha256.h"
#include "g1_words.h"

// Between the loads of the next block and the rounds of this one: the instruction scheduler, left alone, sinks the
// loads to the end of the rounds (fewer live registers) and the wave then waits for its gather with nothing to do.
#if defined(__HIP_DEVICE_COMPILE__)
#define KZG_BLOB_LOADS_FIRST() __builtin_amdgcn_sched_barrier(0)
#else
#define KZG_BLOB_LOADS_FIRST() ((void)0)
#endif

namespace kzg {

// "FSBLOBVERIFY_V1_" as four big-endian words
constexpr uint32_t BLOB_DOMAIN[4] = {0x4653424cu, 0x4f425645u, 0x52494659u, 0x5f56315fu};

// One element: raw[8] (32 big-endian bytes as loaded) -> w[8] canonical little-endian words.  true iff the number is
// below r; otherwise w is all zeros.
template <class F>
static KZG_HD bool blob_element(const uint32_t raw[8], uint32_t w[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = sha_bswap32(raw[7 - k]);
  const bool ok = words_below_p<F>(w);
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = ok ? w[k] : 0u;
  return ok;
}

// The inverse: w[8] canonical little-endian words -> raw[8], the 32 big-endian bytes as they are stored.  true iff the
// number is below r; otherwise raw is all zeros.
template <class F>
static KZG_HD bool blob_output_element(const uint32_t w[8], uint32_t raw[8]) {
  const bool ok = words_below_p<F>(w);
#pragma unroll
  for (int k = 0; k < 8; ++k) raw[k] = ok ? sha_bswap32(w[7 - k]) : 0u;
  return ok;
}

// The challenge of one blob of n = 2^log_n elements, log_n >= 1.  load(q, out[4]) delivers the raw words of 16-byte
// piece q of the blob, q < 2n; comm: the G / 4 raw words of the commitment.  z: four canonical 64-bit limbs.
// The pieces of block t + 1 are asked for BEFORE block t is compressed: on the device one lane walks one blob, the
// lanes of a wave are a whole blob apart and every load is a long-latency gather that the 64 rounds then cover.
template <class F, int G, class Load>
static KZG_HD void blob_challenge(uint32_t log_n, const Load& load, const uint32_t* comm, uint64_t z[4]) {
  static_assert(G % 4 == 0 && G > 0, "the commitment is a whole number of words");
  constexpr int TAIL_WORDS = 8 + G / 4;                               // element n - 1 and the commitment
  constexpr int TAIL_BLOCKS = (4 * TAIL_WORDS + 1 + 8 + 63) / 64;     // ... a byte 0x80 and the length, in whole blocks
  const uint32_t n = 1u << log_n;                                     // log_n <= 24: piece indices fit 32 bits
  const uint64_t bits = (32 + 32 * (uint64_t)n + G) * 8;
  uint32_t state[8], cur[16], nxt[16];
  sha256_init(state);
#pragma unroll
  for (int k = 0; k < 4; ++k) cur[k] = BLOB_DOMAIN[k];
  cur[4] = 0; cur[5] = 0; cur[6] = 0; cur[7] = n;                     // n as 16 bytes big-endian
  load(0u, nxt);
  load(1u, nxt + 4);
#pragma unroll
  for (int k = 0; k < 8; ++k) cur[8 + k] = sha_bswap32(nxt[k]);
  // blocks 0 .. n/2 - 2, each compressed under the loads of the next one
#pragma unroll 1
  for (uint32_t k = 1; k < n / 2; ++k) {
#pragma unroll
    for (int q = 0; q < 4; ++q) load(4 * k - 2 + q, nxt + 4 * q);
    KZG_BLOB_LOADS_FIRST();
    sha256_compress(state, cur);
#pragma unroll
    for (int i = 0; i < 16; ++i) cur[i] = sha_bswap32(nxt[i]);
  }
  // block n/2 - 1 under the loads of element n - 1, then the tail
  uint32_t tail[16 * TAIL_BLOCKS];
  load(2 * n - 2, nxt);
  load(2 * n - 1, nxt + 4);
  KZG_BLOB_LOADS_FIRST();
  sha256_compress(state, cur);
#pragma unroll
  for (int i = 0; i < 8; ++i) tail[i] = sha_bswap32(nxt[i]);
#pragma unroll
  for (int i = 0; i < G / 4; ++i) tail[8 + i] = sha_bswap32(comm[i]);
  tail[TAIL_WORDS] = 0x80000000u;
#pragma unroll
  for (int i = TAIL_WORDS + 1; i < 16 * TAIL_BLOCKS - 2; ++i) tail[i] = 0u;
  tail[16 * TAIL_BLOCKS - 2] = (uint32_t)(bits >> 32);
  tail[16 * TAIL_BLOCKS - 1] = (uint32_t)bits;
#pragma unroll
  for (int t = 0; t < TAIL_BLOCKS; ++t) sha256_compress(state, tail + 16 * t);
  fr_from_digest<F>(state, z);
}

}  // namespace kzg
