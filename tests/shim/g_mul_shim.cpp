// Host-only test shim: kzg_snark_amd/csrc/g_mul.h (the text the gfx950 kernels of g_mul.hip compile) behind a tiny C
// interface, so tests/test_g_mul_host.py can check [k] P in both groups of both curves against curve.py's group law
// without a GPU.  With -DG_MUL_SHIM_MAIN it is a program of its own that replays a file of cases (the sanitizer run).
// Test infrastructure only.
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../kzg_snark_amd/csrc/g_mul.h"
using namespace kzg;

// xy: canonical words x | y; k: 8 words; out: canonical words (zeros for infinity).  0 ok, 1 not a point of the curve
template <class C>
static int do_g1(const uint32_t* xy, int inf, const uint32_t* k, uint32_t* out, int* out_inf) {
  constexpr int NW = C::Fp::NW;
  Affine<C> a = affine_from_words<C>(xy, true);
  if (!inf) {
    a.inf = false;
    if (!import_affine<C>(xy, xy + NW, a.x, a.y)) return 1;
  }
  GMulHostTab<XYZZ<C>> tab;
  *out_inf = affine_to_words<C>(Ec<C>::to_affine(g1_mul<C>(a, k, tab)), out) ? 1 : 0;
  return 0;
}
// xy: canonical words x.c0 | x.c1 | y.c0 | y.c1
template <class C>
static int do_g2(const uint32_t* xy, int inf, const uint32_t* k, uint32_t* out, int* out_inf) {
  Fp2<C> x = Tower<C>::zero2(), y = Tower<C>::zero2();
  if (!inf && !Tower<C>::import_g2(xy, x, y)) return 1;
  GMulHostTab<Jac2<C>> tab;
  *out_inf = g2_to_words<C>(g2_mul<C>(x, y, inf != 0, k, tab), out) ? 1 : 0;
  return 0;
}
extern "C" int gm_mul(int curve, int group, const uint32_t* xy, int inf, const uint32_t* k, uint32_t* out, int* out_inf) {
  if (curve == 0) return group == 1 ? do_g1<Bn254>(xy, inf, k, out, out_inf) : do_g2<Bn254>(xy, inf, k, out, out_inf);
  if (curve == 1) return group == 1 ? do_g1<Bls12_381>(xy, inf, k, out, out_inf) : do_g2<Bls12_381>(xy, inf, k, out, out_inf);
  return -1;
}
// one case of a replay file, 32-bit words: curve, group (1 | 2), inf, the point (48 words, the unused tail zero), the
// scalar (8), the expected flag, the expected point (48)
constexpr int GM_POINT_WORDS = 48;
constexpr int GM_CASE_WORDS = 3 + GM_POINT_WORDS + 8 + 1 + GM_POINT_WORDS;
extern "C" int gm_case_words() { return GM_CASE_WORDS; }

#ifdef G_MUL_SHIM_MAIN
int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s <cases>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<uint32_t> rec(GM_CASE_WORDS);
  size_t cases = 0, bad = 0;
  while (fread(rec.data(), 4, GM_CASE_WORDS, f) == (size_t)GM_CASE_WORDS) {
    const uint32_t* r = rec.data();
    const int curve = (int)r[0], group = (int)r[1], inf = (int)r[2];
    const int words = (group == 1 ? 2 : 4) * (curve == 0 ? 8 : 12);
    std::vector<uint32_t> xy(r + 3, r + 3 + words), k(r + 3 + GM_POINT_WORDS, r + 3 + GM_POINT_WORDS + 8), out(words);
    int out_inf = -1;
    const int rc = gm_mul(curve, group, xy.data(), inf, k.data(), out.data(), &out_inf);
    const uint32_t* want = r + 3 + GM_POINT_WORDS + 8;
    if (rc != 0 || out_inf != (int)want[0] || memcmp(out.data(), want + 1, words * 4) != 0) {
      if (!bad) fprintf(stderr, "case %zu (curve %d, group %d): rc %d, flag %d, expected %u\n", cases, curve, group, rc, out_inf, want[0]);
      ++bad;
    }
    ++cases;
  }
  fclose(f);
  printf("%zu cases, %zu mismatches\n", cases, bad);
  return bad || !cases ? 1 : 0;
}
#endif
