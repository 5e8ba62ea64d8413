// Host-only test shim: the output element of kzg_snark_amd/csrc/blob.h (the text blob_output_kernel compiles) behind a
// tiny C interface, so tests/test_cells_host.py can check it against int.to_bytes without a GPU, and that it undoes
// blob_element.  Built plain, with -DKZG_AUDIT, and with -DCELLS_SHIM_MAIN as a program of its own for the sanitizers.
// Test infrastructure only.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../kzg_snark_amd/csrc/blob.h"
using namespace kzg;

// four little-endian limbs -> 32 big-endian bytes (zeros when >= r); 1 iff below r
extern "C" int cs_output_element(int curve, const uint64_t* limbs, uint8_t* bytes) {
  uint32_t w[8], raw[8];
  for (int j = 0; j < 4; ++j) { w[2 * j] = (uint32_t)limbs[j]; w[2 * j + 1] = (uint32_t)(limbs[j] >> 32); }
  bool ok;
  if (curve == 0) ok = blob_output_element<BnFr>(w, raw);
  else if (curve == 1) ok = blob_output_element<BlsFr>(w, raw);
  else return -1;
  memcpy(bytes, raw, 32);
  return ok ? 1 : 0;
}
// bytes -> limbs -> bytes through blob_element and blob_output_element; 1 iff both call the element canonical
extern "C" int cs_round_trip(int curve, const uint8_t* in, uint8_t* out) {
  uint32_t raw[8], w[8], back[8];
  memcpy(raw, in, 32);
  bool a, b;
  if (curve == 0) { a = blob_element<BnFr>(raw, w); b = blob_output_element<BnFr>(w, back); }
  else if (curve == 1) { a = blob_element<BlsFr>(raw, w); b = blob_output_element<BlsFr>(w, back); }
  else return -1;
  memcpy(out, back, 32);
  return a && b ? 1 : 0;
}

#ifdef KZG_AUDIT_ON
extern "C" unsigned long long cs_audit_count() { return audit::state().count; }
#endif

#ifdef CELLS_SHIM_MAIN
// The drivers above on buffers of their exact size: 0, 1, r - 1, r, 2^256 - 1 and a value of 32 distinct bytes.
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { ++fails; printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

template <class F>
static void self_test(int curve) {
  uint64_t* limbs = (uint64_t*)malloc(32);
  uint8_t* bytes = (uint8_t*)malloc(32);
  uint8_t* back = (uint8_t*)malloc(32);
  uint8_t* zero = (uint8_t*)calloc(32, 1);
  memset(limbs, 0, 32);
  EXPECT(cs_output_element(curve, limbs, bytes) == 1 && memcmp(bytes, zero, 32) == 0);
  limbs[0] = 1;
  EXPECT(cs_output_element(curve, limbs, bytes) == 1 && bytes[31] == 1 && bytes[0] == 0 && bytes[30] == 0);
  for (int j = 0; j < 4; ++j) limbs[j] = (uint64_t)F::PW[2 * j] | ((uint64_t)F::PW[2 * j + 1] << 32);
  EXPECT(cs_output_element(curve, limbs, bytes) == 0 && memcmp(bytes, zero, 32) == 0);              // r
  limbs[0] -= 1;                                                                                   // r - 1 (r is odd)
  EXPECT(cs_output_element(curve, limbs, bytes) == 1 && bytes[0] == (uint8_t)(F::PW[7] >> 24));
  EXPECT(bytes[31] == (uint8_t)(F::PW[0] - 1));
  EXPECT(cs_round_trip(curve, bytes, back) == 1 && memcmp(bytes, back, 32) == 0);
  memset(limbs, 0xff, 32);
  EXPECT(cs_output_element(curve, limbs, bytes) == 0 && memcmp(bytes, zero, 32) == 0);              // 2^256 - 1
  for (int k = 0; k < 32; ++k) bytes[k] = (uint8_t)(k + 1);                                         // 0x0102...20 < r
  EXPECT(cs_round_trip(curve, bytes, back) == 1 && memcmp(bytes, back, 32) == 0);
  free(zero);
  free(back);
  free(bytes);
  free(limbs);
}

int main() {
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
