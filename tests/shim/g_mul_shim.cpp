// Host-only test shim: kzg_snark_amd/csrc/g_mul.h (the text the gfx950 kernels of g_mul.hip compile) behind a tiny C
// interface, so tests/test_g_mul_host.py can check [k] P in both groups of both curves against curve.py's group law
// without a GPU, and the launch plan and table indices of g_mul.hip's drivers.  With -DG_MUL_SHIM_MAIN it is a program of its own that replays a file of cases (the sanitizer run).
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
// ---- the launches of a call (GmPlan) and the table's index arithmetic, as g_mul.hip uses them ----------------------
// 0 / 1: lanes per workgroup of G1 / G2, 2 / 3: lanes per launch, 4: the largest n
extern "C" uint64_t gm_const(int which) {
  const uint64_t v[] = {GM_TB1, GM_TB2, GM_LAUNCH_LANES1, GM_LAUNCH_LANES2, GM_MAX_POINTS};
  return which >= 0 && which < 5 ? v[which] : 0;
}
extern "C" void gm_plan(uint64_t n, int group, uint32_t* blocks, uint32_t* launch_blocks) {
  const GmPlan plan((size_t)n, group == 1 ? GM_TB1 : GM_TB2, group == 1 ? GM_LAUNCH_LANES1 : GM_LAUNCH_LANES2);
  *blocks = plan.blocks;
  *launch_blocks = plan.launch_blocks;
}
template <class C>
static void table_of(int group, uint32_t g, uint32_t launch_blocks, uint32_t* pieces, uint32_t* top, uint64_t* vectors) {
  const uint32_t tb = group == 1 ? GM_TB1 : GM_TB2, slots = g * tb;
  const int p = group == 1 ? gm_g1_pieces<C>() : gm_g2_pieces<C>();
  *pieces = (uint32_t)p;
  // the last piece of the last entry of the last lane, by the kernels' own 32-bit arithmetic
  *top = gm_piece_index(gm_entry_index(GMUL_TABLE - 1, p, slots, slots - 1), p - 1, slots);
  // what the host drivers allocate for launches of at most launch_blocks workgroups, in vectors (G1: 16 bytes, G2: 8)
  *vectors = (group == 1 ? g1_column_bytes<C>() / 16 : g2_column_bytes<C>() / 8) * tb * launch_blocks;
}
// a launch of g >= 1 workgroups over a table allocated for launch_blocks: pieces per entry, the largest index it touches,
// the vectors allocated.  0 ok, -1 no such curve
extern "C" int gm_table(int curve, int group, uint32_t g, uint32_t launch_blocks, uint32_t* pieces, uint32_t* top,
                        uint64_t* vectors) {
  if (curve == 0) return table_of<Bn254>(group, g, launch_blocks, pieces, top, vectors), 0;
  if (curve == 1) return table_of<Bls12_381>(group, g, launch_blocks, pieces, top, vectors), 0;
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
