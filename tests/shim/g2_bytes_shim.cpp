// Host-only test shim: kzg_snark_amd/csrc/g2_bytes.h (the text the gfx950 kernels of g2_bytes.hip compile) behind a tiny
// C interface, so tests/test_g2_bytes_host.py can check the square root in Fp2, the two subgroup tests and the byte
// formats against Python integers without a GPU.  Built plain and with -DKZG_AUDIT (field.h's pre/postcondition
// hooks).  Test infrastructure only.
#include <stdio.h>
#include <string.h>
#include "../../kzg_snark_amd/csrc/g2_bytes.h"
using namespace kzg;

// a: canonical words c0 | c1 of an element of Fp2; out: the root (zeros when there is none); 1 iff a is a square
template <class C>
static int do_sqrt(const uint32_t* a, uint32_t* out) {
  using G = G2Bytes<C>;
  using Fd = typename G::Fd;
  Fp2<C> v, root;
  v.c0 = Fd::to_mont(Fd::from_words(a));
  v.c1 = Fd::to_mont(Fd::from_words(a + G::NW));
  const bool ok = G::sqrt2(v, root);
  G::to_words2(root, out);
  return ok ? 1 : 0;
}
extern "C" int g2b_sqrt(int curve, const uint32_t* a, uint32_t* out) {
  if (curve == 0) return do_sqrt<Bn254>(a, out);
  if (curve == 1) return do_sqrt<Bls12_381>(a, out);
  return -1;
}
extern "C" int g2b_size(int curve) { return curve == 0 ? G2Bytes<Bn254>::SIZE : curve == 1 ? G2Bytes<Bls12_381>::SIZE : -1; }

template <class C>
static int do_decode(const uint8_t* bytes, int check, uint32_t* xy, int* inf) {
  using G = G2Bytes<C>;
  uint32_t raw[2 * G::NW];
  memcpy(raw, bytes, G::SIZE);
  bool is_inf = false;
  const int st = G::decode(raw, check != 0, xy, is_inf);
  *inf = is_inf ? 1 : 0;
  return st;
}
extern "C" int g2b_decode(int curve, const uint8_t* bytes, int check, uint32_t* xy, int* inf) {
  if (curve == 0) return do_decode<Bn254>(bytes, check, xy, inf);
  if (curve == 1) return do_decode<Bls12_381>(bytes, check, xy, inf);
  return -1;
}
template <class C>
static int do_encode(const uint32_t* xy, int inf, uint8_t* bytes) {
  using G = G2Bytes<C>;
  uint32_t raw[2 * G::NW];
  G::encode(xy, inf != 0, raw);
  memcpy(bytes, raw, G::SIZE);
  return 0;
}
extern "C" int g2b_encode(int curve, const uint32_t* xy, int inf, uint8_t* bytes) {
  if (curve == 0) return do_encode<Bn254>(xy, inf, bytes);
  if (curve == 1) return do_encode<Bls12_381>(xy, inf, bytes);
  return -1;
}
// status of an affine point (canonical words x.c0 | x.c1 | y.c0 | y.c1): 0, 2 or 3
extern "C" int g2b_check(int curve, const uint32_t* xy, int inf) {
  if (curve == 0) return G2Bytes<Bn254>::check_affine(xy, inf != 0);
  if (curve == 1) return G2Bytes<Bls12_381>::check_affine(xy, inf != 0);
  return -1;
}

#ifdef KZG_AUDIT_ON
extern "C" void g2b_audit_reset() { audit::state() = audit::State{0, "", "", 0, false}; }
extern "C" unsigned long long g2b_audit_read(char* fn, char* what, int cap, int* line) {
  const audit::State& s = audit::state();
  snprintf(fn, cap, "%s", s.fn);
  snprintf(what, cap, "%s", s.what);
  *line = s.line;
  return s.count;
}
#endif
