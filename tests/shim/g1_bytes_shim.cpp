// Host-only test shim: kzg_snark_amd/csrc/g1_bytes.h and, through it, g1_words.h (the text the gfx950 kernels compile)
// behind a tiny C interface, so tests/test_g1_bytes_host.py can check the square root, the subgroup test, the byte
// formats and the point <-> canonical-words codec against Python integers without a GPU.  Built plain, with -DKZG_AUDIT (field.h's pre/postcondition hooks), and with
// -DG1_BYTES_SHIM_MAIN as a program of its own for the sanitizers.  Test infrastructure only.
#include <stdio.h>
#include <string.h>
#include "../../kzg_snark_amd/csrc/g1_bytes.h"
using namespace kzg;

template <class F>
static int do_sqrt(const uint32_t* a, uint32_t* out) {
  using Fd = Field<F>;
  Fe<F> root;
  const bool ok = fp_sqrt<F>(Fd::to_mont(Fd::from_words(a)), root);
  Fd::to_words(Fd::from_mont(root), out);
  return ok ? 1 : 0;
}
// a: canonical words of an element of the base field of `curve`; out: the candidate root; 1 iff a is a square
extern "C" int gb_sqrt(int curve, const uint32_t* a, uint32_t* out) {
  if (curve == 0) return do_sqrt<BnFp>(a, out);
  if (curve == 1) return do_sqrt<BlsFp>(a, out);
  return -1;
}
extern "C" int gb_size(int curve) { return curve == 0 ? G1Bytes<Bn254>::SIZE : curve == 1 ? G1Bytes<Bls12_381>::SIZE : -1; }

template <class C>
static int do_decode(const uint8_t* bytes, int check, uint32_t* xy, int* inf) {
  using G = G1Bytes<C>;
  uint32_t raw[G::NW];
  memcpy(raw, bytes, G::SIZE);
  bool is_inf = false;
  const int st = G::decode(raw, check != 0, xy, xy + G::NW, is_inf);
  *inf = is_inf ? 1 : 0;
  return st;
}
extern "C" int gb_decode(int curve, const uint8_t* bytes, int check, uint32_t* xy, int* inf) {
  if (curve == 0) return do_decode<Bn254>(bytes, check, xy, inf);
  if (curve == 1) return do_decode<Bls12_381>(bytes, check, xy, inf);
  return -1;
}
template <class C>
static int do_encode(const uint32_t* xy, int inf, uint8_t* bytes) {
  using G = G1Bytes<C>;
  uint32_t raw[G::NW];
  G::encode(xy, xy + G::NW, inf != 0, raw);
  memcpy(bytes, raw, G::SIZE);
  return 0;
}
extern "C" int gb_encode(int curve, const uint32_t* xy, int inf, uint8_t* bytes) {
  if (curve == 0) return do_encode<Bn254>(xy, inf, bytes);
  if (curve == 1) return do_encode<Bls12_381>(xy, inf, bytes);
  return -1;
}
// status of an affine point (canonical words x | y): 0, 2 or 3
extern "C" int gb_check(int curve, const uint32_t* xy, int inf) {
  if (curve == 0) return G1Bytes<Bn254>::check_affine(xy, xy + BnFp::NW, inf != 0);
  if (curve == 1) return G1Bytes<Bls12_381>::check_affine(xy, xy + BlsFp::NW, inf != 0);
  return -1;
}

// g1_words.h's rule on canonical words x | y: 1 iff both coordinates are below p and the point is on the curve
extern "C" int gb_import(int curve, const uint32_t* xy) {
  if (curve == 0) { Fe<BnFp> x, y; return import_affine<Bn254>(xy, xy + BnFp::NW, x, y) ? 1 : 0; }
  if (curve == 1) { Fe<BlsFp> x, y; return import_affine<Bls12_381>(xy, xy + BlsFp::NW, x, y) ? 1 : 0; }
  return -1;
}
// affine_to_words of affine_from_words: out = the words of (xy, inf) taken modulo p; returns the infinity flag
extern "C" int gb_words_round_trip(int curve, const uint32_t* xy, int inf, uint32_t* out) {
  if (curve == 0) return affine_to_words<Bn254>(affine_from_words<Bn254>(xy, inf != 0), out) ? 1 : 0;
  if (curve == 1) return affine_to_words<Bls12_381>(affine_from_words<Bls12_381>(xy, inf != 0), out) ? 1 : 0;
  return -1;
}
// What kzg_srs_load_g1 asks of a finite key point, written out on its own (not through g1_words.h): the curve
// equation on the coordinates taken modulo p, no range check.  1 = the key is accepted.
template <class C>
static int do_key_rule(const uint32_t* xy) {
  using Fd = Field<typename C::Fp>;
  return Ec<C>::on_curve(Fd::reduce(Fd::to_mont(Fd::from_words(xy))),
                         Fd::reduce(Fd::to_mont(Fd::from_words(xy + C::Fp::NW)))) ? 1 : 0;
}
extern "C" int gb_key_rule(int curve, const uint32_t* xy) {
  if (curve == 0) return do_key_rule<Bn254>(xy);
  if (curve == 1) return do_key_rule<Bls12_381>(xy);
  return -1;
}

#ifdef KZG_AUDIT_ON
extern "C" void gb_audit_reset() { audit::state() = audit::State{0, "", "", 0, false}; }
extern "C" unsigned long long gb_audit_read(char* fn, char* what, int cap, int* line) {
  const audit::State& s = audit::state();
  snprintf(fn, cap, "%s", s.fn);
  snprintf(what, cap, "%s", s.what);
  *line = s.line;
  return s.count;
}
#endif

#ifdef G1_BYTES_SHIM_MAIN
// The drivers above on inputs made here: k G (k = 1..6, both signs of y by negation) encoded, decoded with the
// subgroup test and compared; infinity; malformed blobs; square roots of 0, 1, squares and their negatives (p = 3
// mod 4: exactly one of a, -a is a square) with all-ones limbs; on BLS12-381 the order-3 point (0, 2); the
// canonical-words codec of g1_words.h at its edges (x = p, y = p, x = p - 1, all-ones words, a flagged infinity with
// stray words) and the key-loading rule on x + p.
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { ++fails; printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

template <class C>
static void self_test(int curve, const uint32_t* gen_xy) {
  using F = typename C::Fp;
  using Fd = Field<F>;
  using G = G1Bytes<C>;
  constexpr int NW = F::NW;
  Affine<C> g;
  g.x = Fd::to_mont(Fd::from_words(gen_xy)); g.y = Fd::to_mont(Fd::from_words(gen_xy + NW)); g.inf = false;
  XYZZ<C> acc = Ec<C>::infinity();
  uint8_t blob[G::SIZE], blob2[G::SIZE];
  for (int k = 1; k <= 6; ++k) {
    acc = Ec<C>::madd(acc, g.x, g.y);
    Affine<C> a = Ec<C>::to_affine(acc);
    for (int sign = 0; sign < 2; ++sign) {
      uint32_t xy[2 * NW], back[2 * NW];
      int inf = 0;
      Fd::to_words(Fd::from_mont(a.x), xy);
      Fd::to_words(Fd::from_mont(sign ? Fd::neg(a.y) : a.y), xy + NW);
      EXPECT(gb_check(curve, xy, 0) == 0);
      gb_encode(curve, xy, 0, blob);
      EXPECT(gb_decode(curve, blob, 1, back, &inf) == 0 && inf == 0 && memcmp(xy, back, sizeof(xy)) == 0);
      gb_encode(curve, back, 0, blob2);
      EXPECT(memcmp(blob, blob2, G::SIZE) == 0);
      xy[NW] ^= 1u;                                       // off the curve
      EXPECT(gb_check(curve, xy, 0) == 2);
    }
  }
  uint32_t zero[2 * NW] = {0}, out[2 * NW];
  int inf = 0;
  gb_encode(curve, zero, 1, blob);
  EXPECT(gb_decode(curve, blob, 1, out, &inf) == 0 && inf == 1);
  blob[G::SIZE - 1] = 1;                                  // infinity with a stray bit
  EXPECT(gb_decode(curve, blob, 1, out, &inf) == 1);
  memset(blob, 0, G::SIZE);                               // no flag at all
  EXPECT(gb_decode(curve, blob, 1, out, &inf) == 1);
  memset(blob, 0xff, G::SIZE);                            // x >= p (finite, larger y)
  if (curve == 1) blob[0] = 0xbf;
  EXPECT(gb_decode(curve, blob, 1, out, &inf) == 1);
  // square roots: a = s^2 for s with all-ones lower limbs, and -a
  for (int top = 0; top < 3; ++top) {
    Fe<F> s;
    for (int j = 0; j < F::N - 1; ++j) s.l[j] = F::MASK;
    s.l[F::N - 1] = top == 0 ? 0 : F::P[F::N - 1] - top;
    const Fe<F> a = Fd::sqr(s);
    uint32_t aw[NW], rw[NW], nw[NW];
    Fd::to_words(Fd::from_mont(a), aw);
    Fd::to_words(Fd::from_mont(Fd::neg(a)), nw);
    EXPECT(gb_sqrt(curve, aw, rw) == 1);
    const Fe<F> r = Fd::to_mont(Fd::from_words(rw));
    EXPECT(Fd::eq(Fd::sqr(r), a));
    EXPECT(gb_sqrt(curve, nw, rw) == 0);
  }
  uint32_t one[NW] = {1}, zw[NW] = {0}, rw[NW];
  EXPECT(gb_sqrt(curve, zw, rw) == 1 && rw[0] == 0);
  EXPECT(gb_sqrt(curve, one, rw) == 1);
  // g1_words.h: the rule, the round trip and the key-loading rule on the generator and around p
  {
    uint32_t pw[NW], q[2 * NW], back[2 * NW];
    for (int k = 0; k < NW; ++k) pw[k] = F::PW[k];
    EXPECT(gb_import(curve, gen_xy) == 1 && gb_key_rule(curve, gen_xy) == 1);
    EXPECT(gb_words_round_trip(curve, gen_xy, 0, back) == 0 && memcmp(back, gen_xy, sizeof(back)) == 0);
    memcpy(q, gen_xy, sizeof(q)); memcpy(q, pw, sizeof(pw));                       // x = p
    EXPECT(gb_import(curve, q) == 0);
    memcpy(q, gen_xy, sizeof(q)); memcpy(q + NW, pw, sizeof(pw));                  // y = p
    EXPECT(gb_import(curve, q) == 0);
    memcpy(q, gen_xy, sizeof(q)); memcpy(q, pw, sizeof(pw)); q[0] -= 1;            // (p - 1, y): in range, off the curve
    EXPECT(words_below_p<F>(q) && words_below_p<F>(q + NW) && gb_import(curve, q) == 0 && gb_key_rule(curve, q) == 0);
    memset(q, 0xff, sizeof(q));                                                    // all-ones words
    EXPECT(gb_import(curve, q) == 0);
    EXPECT(gb_words_round_trip(curve, q, 1, back) == 1);                           // the flag wins over stray words
    for (int k = 0; k < 2 * NW; ++k) EXPECT(back[k] == 0);
    // x + p (there is room: p < 2^255, p < 2^382): the rule refuses it, the round trip and key loading take it as x
    memcpy(q, gen_xy, sizeof(q));
    uint64_t carry = 0;
    for (int k = 0; k < NW; ++k) { carry += (uint64_t)q[k] + pw[k]; q[k] = (uint32_t)carry; carry >>= 32; }
    EXPECT(carry == 0 && !words_below_p<F>(q));
    EXPECT(gb_import(curve, q) == 0);
    EXPECT(gb_key_rule(curve, q) == 1);
    EXPECT(gb_words_round_trip(curve, q, 0, back) == 0 && memcmp(back, gen_xy, sizeof(back)) == 0);
  }
  if (curve == 1) {                                       // (0, 2): order 3, on the curve y^2 = x^3 + 4
    uint32_t xy[2 * NW] = {0};
    xy[NW] = 2;
    EXPECT(gb_check(curve, xy, 0) == 3);
    gb_encode(curve, xy, 0, blob);
    EXPECT(gb_decode(curve, blob, 1, out, &inf) == 3);
    EXPECT(gb_decode(curve, blob, 0, out, &inf) == 0 && out[NW] == 2);
  }
}

int main() {
  static const uint32_t GEN_BN[16] = {1, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0};
  static const uint32_t GEN_BLS[24] = {
      0xdb22c6bbu, 0xfb3af00au, 0xf97a1aefu, 0x6c55e83fu, 0x171bac58u, 0xa14e3a3fu, 0x9774b905u, 0xc3688c4fu,
      0x4fa9ac0fu, 0x2695638cu, 0x3197d794u, 0x17f1d3a7u,
      0x46c5e7e1u, 0x0caa2329u, 0xa2888ae4u, 0xd03cc744u, 0x2c04b3edu, 0x00db18cbu, 0xd5d00af6u, 0xfcf5e095u,
      0x741d8ae4u, 0xa09e30edu, 0xe3aaa0f1u, 0x08b3f481u};
  self_test<Bn254>(0, GEN_BN);
  self_test<Bls12_381>(1, GEN_BLS);
#ifdef KZG_AUDIT_ON
  const audit::State& s = audit::state();
  if (s.count) { printf("%llu audit violations, first in %s (line %d): %s\n", s.count, s.fn, s.line, s.what); return 2; }
#endif
  if (fails) { printf("%d checks failed\n", fails); return 1; }
  printf("no violations\n");
  return 0;
}
#endif
