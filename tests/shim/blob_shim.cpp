// Host-only test shim: kzg_snark_amd/csrc/sha256.h and blob.h (the text the gfx950 kernels of blob.hip compile) behind a
// tiny C interface, so tests/test_blob_host.py can check the compression function, the reduction of a digest, the
// canonicity check of an element and the challenge of a blob against hashlib and Python integers without a GPU.  Built
// plain, with -DKZG_AUDIT, and with -DBLOB_SHIM_MAIN as a program of its own for the sanitizers.  Test infrastructure
// only.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../kzg_snark_amd/csrc/blob.h"
using namespace kzg;

// state <- H0
extern "C" void bs_sha256_init(uint32_t* state) { sha256_init(state); }
// state <- the compression of one 64-byte block given as bytes
extern "C" void bs_sha256_block(uint32_t* state, const uint8_t* block) {
  uint32_t raw[16], w[16];
  memcpy(raw, block, 64);
  for (int k = 0; k < 16; ++k) w[k] = sha_bswap32(raw[k]);
  sha256_compress(state, w);
}
// the 32 bytes of a digest (big-endian) -> four canonical limbs of the number mod r
extern "C" int bs_fr_from_digest(int curve, const uint8_t* digest, uint64_t* out) {
  uint32_t raw[8], d[8];
  memcpy(raw, digest, 32);
  for (int k = 0; k < 8; ++k) d[k] = sha_bswap32(raw[k]);
  if (curve == 0) { fr_from_digest<BnFr>(d, out); return 0; }
  if (curve == 1) { fr_from_digest<BlsFr>(d, out); return 0; }
  return -1;
}
extern "C" int bs_digest_trips(int curve) {
  return curve == 0 ? digest_trips<BnFr>() : curve == 1 ? digest_trips<BlsFr>() : -1;
}
// one element of 32 big-endian bytes -> four canonical limbs (zeros when >= r); 1 iff canonical
extern "C" int bs_element(int curve, const uint8_t* bytes, uint64_t* out) {
  uint32_t raw[8], w[8];
  memcpy(raw, bytes, 32);
  bool ok;
  if (curve == 0) ok = blob_element<BnFr>(raw, w);
  else if (curve == 1) ok = blob_element<BlsFr>(raw, w);
  else return -1;
  for (int j = 0; j < 4; ++j) out[j] = (uint64_t)w[2 * j] | ((uint64_t)w[2 * j + 1] << 32);
  return ok ? 1 : 0;
}

// the 16-byte pieces of a blob in host memory; counts the pieces asked for and remembers the highest
struct HostPieces {
  const uint8_t* base;
  uint64_t* asked;
  uint32_t* highest;
  void operator()(uint32_t q, uint32_t* out) const {
    memcpy(out, base + (size_t)q * 16, 16);
    ++*asked;
    if (q > *highest) *highest = q;
  }
};
extern "C" int bs_commitment_size(int curve) { return curve == 0 ? 32 : curve == 1 ? 48 : -1; }
// the challenge of one blob of 2^log_n elements and its commitment; *pieces: how many 16-byte pieces were read
extern "C" int bs_challenge(int curve, uint32_t log_n, const uint8_t* blob, const uint8_t* commitment, uint64_t* z,
                            uint64_t* pieces) {
  uint32_t comm[12], highest = 0;
  uint64_t asked = 0;
  const HostPieces load{blob, &asked, &highest};
  if (curve == 0) {
    memcpy(comm, commitment, 32);
    blob_challenge<BnFr, 32>(log_n, load, comm, z);
  } else if (curve == 1) {
    memcpy(comm, commitment, 48);
    blob_challenge<BlsFr, 48>(log_n, load, comm, z);
  } else {
    return -1;
  }
  if (pieces) *pieces = asked;
  return highest == (2u << log_n) - 1 ? 0 : -2;          // the last piece read is the blob's last, none beyond
}

#ifdef KZG_AUDIT_ON
extern "C" unsigned long long bs_audit_count() { return audit::state().count; }
#endif

#ifdef BLOB_SHIM_MAIN
// The drivers above on inputs made here, every buffer allocated at its exact size so that a read or write beyond it
// is a sanitizer report: SHA-256 of "abc" and of the empty message; the digest reduction at 0, r - 1, r, 2^256 - 1;
// the element check at r - 1 and r; challenges of blobs of 2 .. 64 elements (every piece read exactly once).
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { ++fails; printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

static void be_bytes(const uint32_t* pw, int add, uint8_t* out) {      // the 8 words of r, plus a small int, big-endian
  uint32_t w[8];
  int64_t c = add;
  for (int k = 0; k < 8; ++k) { c += pw[k]; w[k] = (uint32_t)c; c >>= 32; }
  for (int k = 0; k < 8; ++k)
    for (int q = 0; q < 4; ++q) out[4 * (7 - k) + q] = (uint8_t)(w[k] >> (24 - 8 * q));
}

template <class F>
static void self_test(int curve) {
  uint8_t* d = (uint8_t*)malloc(32);
  uint64_t* out = (uint64_t*)malloc(32);
  memset(d, 0, 32);
  EXPECT(bs_fr_from_digest(curve, d, out) == 0 && !(out[0] | out[1] | out[2] | out[3]));
  be_bytes(F::PW, 0, d);                                  // r -> 0
  bs_fr_from_digest(curve, d, out);
  EXPECT(!(out[0] | out[1] | out[2] | out[3]));
  EXPECT(bs_element(curve, d, out) == 0 && !(out[0] | out[1] | out[2] | out[3]));
  be_bytes(F::PW, -1, d);                                 // r - 1 stays
  bs_fr_from_digest(curve, d, out);
  EXPECT(out[0] == (((uint64_t)F::PW[1] << 32) | (F::PW[0] - 1)) && out[3] == (((uint64_t)F::PW[7] << 32) | F::PW[6]));
  EXPECT(bs_element(curve, d, out) == 1 && out[0] == (((uint64_t)F::PW[1] << 32) | (F::PW[0] - 1)));
  be_bytes(F::PW, 1, d);                                  // r + 1 -> 1
  bs_fr_from_digest(curve, d, out);
  EXPECT(out[0] == 1 && !(out[1] | out[2] | out[3]));
  memset(d, 0xff, 32);                                    // 2^256 - 1: every trip of the loop; below r afterwards
  bs_fr_from_digest(curve, d, out);
  EXPECT((out[3] >> 32) <= F::PW[7]);
  EXPECT(bs_element(curve, d, out) == 0 && !(out[0] | out[1] | out[2] | out[3]));
  const int G = bs_commitment_size(curve);
  uint8_t* comm = (uint8_t*)malloc(G);
  for (int k = 0; k < G; ++k) comm[k] = (uint8_t)(0xa5 ^ k);
  uint64_t prev[4] = {0, 0, 0, 0};
  for (uint32_t log_n = 1; log_n <= 6; ++log_n) {
    const size_t size = (size_t)32 << log_n;
    uint8_t* blob = (uint8_t*)malloc(size);
    for (size_t k = 0; k < size; ++k) blob[k] = (uint8_t)(k * 131 + log_n);
    uint64_t pieces = 0, z2[4];
    EXPECT(bs_challenge(curve, log_n, blob, comm, out, &pieces) == 0);
    EXPECT(pieces == ((uint64_t)2 << log_n));             // every piece once
    EXPECT(memcmp(out, prev, 32) != 0);
    blob[size - 1] ^= 1;                                  // the last byte enters the hash
    EXPECT(bs_challenge(curve, log_n, blob, comm, z2, &pieces) == 0 && memcmp(out, z2, 32) != 0);
    memcpy(prev, out, 32);
    free(blob);
  }
  free(comm);
  free(out);
  free(d);
}

int main() {
  // FIPS 180-4 / NIST's example: SHA-256("abc")
  uint8_t* block = (uint8_t*)calloc(64, 1);
  uint32_t* state = (uint32_t*)malloc(32);
  memcpy(block, "abc", 3);
  block[3] = 0x80;
  block[63] = 24;
  bs_sha256_init(state);
  bs_sha256_block(state, block);
  EXPECT(state[0] == 0xba7816bfu && state[1] == 0x8f01cfeau && state[6] == 0xb410ff61u && state[7] == 0xf20015adu);
  memset(block, 0, 64);                                   // the empty message
  block[0] = 0x80;
  bs_sha256_init(state);
  bs_sha256_block(state, block);
  EXPECT(state[0] == 0xe3b0c442u && state[7] == 0x7852b855u);
  free(state);
  free(block);
  EXPECT(bs_digest_trips(0) == 5 && bs_digest_trips(1) == 2);
  self_test<BnFr>(0);
  self_test<BlsFr>(1);
#ifdef KZG_AUDIT_ON
  const audit::State& s = audit::state();
  if (s.count) { printf("%llu audit violations, first in %s (line %d): %s\n", s.count, s.fn, s.line, s.what); return 2; }
#endif
  if (fails) { printf("%d checks failed\n", fails); return 1; }
  printf("no violations\n");
  return 0;
}
#endif
