// Host-only test shim: kzg_snark_amd/csrc/fp_tower.h (the text csrc/pairing.hip compiles for gfx950) behind a tiny C
// interface, with the lanes of a wave replaced by HostLanes' loop around the same interpreter and program, so tests/test_pairing_host.py can compare the tower
// arithmetic and whole pairings with kzg_snark_amd/pairing.py's integers without a GPU.  Field elements cross the
// interface as raw limbs in Montgomery form (N words each), so a test chooses the limb image of an operand; points
// and pairing values cross as canonical 32-bit words, the C ABI's format.  LockstepLanes is a second exchange that
// holds a phase to fp_tower.h's contract (no lane reads or writes what another lane of the phase writes).  Built plain, with -DKZG_AUDIT (field.h's
// pre/postcondition hooks), and with -DPAIRING_SHIM_MAIN as a program of its own for the sanitizers.  Test
// infrastructure only.
#include <stdio.h>
#include <string.h>
#include "../../kzg_snark_amd/csrc/fp_tower.h"
using namespace kzg;

enum { OP_MUL = 0, OP_SQR = 1, OP_INV = 2, OP_MUL_XI = 3, OP_SPARSE = 4, OP_CONJ_W = 5, OP_FROB1 = 6, OP_FROB2 = 7,
       OP_FROB3 = 8, OP_CYC_SQR = 9 };

template <class C>
static void get2(const uint32_t* w, Fp2<C>& a) {
  constexpr int N = C::Fp::N;
  memcpy(a.c0.l, w, 4 * N);
  memcpy(a.c1.l, w + N, 4 * N);
}
template <class C>
static void put2(const Fp2<C>& a, uint32_t* w) {
  constexpr int N = C::Fp::N;
  memcpy(w, a.c0.l, 4 * N);
  memcpy(w + N, a.c1.l, 4 * N);
}

template <class C>
static int do_fp2(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  using T = Tower<C>;
  Fp2<C> x, y, r;
  get2<C>(a, x);
  get2<C>(b, y);
  if (op == OP_MUL) r = T::mul2(x, y);
  else if (op == OP_SQR) r = T::sqr2(x);
  else if (op == OP_INV) r = T::inv2(x);
  else if (op == OP_MUL_XI) r = T::mul_xi(x);
  else return -1;
  put2<C>(r, out);
  return 0;
}
// a, b, out: 2 N raw Montgomery limbs (c0 | c1)
extern "C" int ps_fp2(int curve, int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  if (curve == 0) return do_fp2<Bn254>(op, a, b, out);
  if (curve == 1) return do_fp2<Bls12_381>(op, a, b, out);
  return -1;
}

template <class C>
static int do_fp12(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  using T = Tower<C>;
  constexpr int N = C::Fp::N;
  PairingShared<C>* sh = new PairingShared<C>();
  HostLanes x;
  T::load_constants(x, sh);
  PairingProgram* p = new PairingProgram();
  p->n = 0;
  int result = R_T2, rc = 0;
  for (int k = 0; k < 6; ++k) { get2<C>(a + 2 * N * k, sh->v[6 * R_T0 + k]); get2<C>(b + 2 * N * k, sh->v[6 * R_T1 + k]); }
  if (op == OP_MUL) p->mul(R_T2, R_T0, R_T1);
  else if (op == OP_SQR) p->mul(R_T2, R_T0, R_T0);
  else if (op == OP_INV) p->inv(R_T2, R_T0);
  else if (op == OP_CONJ_W) p->conj(R_T2, R_T0);
  else if (op >= OP_FROB1 && op <= OP_FROB3) p->frob(R_T2, R_T0, op - OP_FROB1 + 1);
  else if (op == OP_CYC_SQR) p->cyc_sqr(R_T2, R_T0);
  else if (op == OP_SPARSE) {                    // f = a, the line of pair 0 = the coefficients of b that a line has
    p->emit(OP_COPY, R_F, R_T0);
    p->lines();
    int slot = 0;
    for (int k = 0; k < 6; ++k)
      if ((T::LINE_MASK >> k) & 1u) sh->v[S_PAIR + PS_LN + slot++] = sh->v[6 * R_T1 + k];
    sh->skip[0] = 0;
    result = R_F;
  } else rc = -1;
  T::run(x, sh, p->ins, p->n, 1);
  for (int k = 0; k < 6; ++k) put2<C>(sh->v[6 * result + k], out + 2 * N * k);
  delete p;
  delete sh;
  return rc;
}
// a, b, out: 12 N raw Montgomery limbs, coefficient k at 2 N k.  OP_SPARSE reads the coefficients of b that a line has.
extern "C" int ps_fp12(int curve, int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  if (curve == 0) return do_fp12<Bn254>(op, a, b, out);
  if (curve == 1) return do_fp12<Bls12_381>(op, a, b, out);
  return -1;
}
extern "C" unsigned ps_line_mask(int curve) { return curve == 0 ? Tower<Bn254>::LINE_MASK : Tower<Bls12_381>::LINE_MASK; }
extern "C" int ps_gt_multiple(int curve) { return curve == 0 ? Bn254::GT_MULTIPLE : Bls12_381::GT_MULTIPLE; }

template <class C>
static int do_equation(const uint32_t* g1, const uint8_t* g1_inf, const uint32_t* g2, const uint8_t* g2_inf, int k,
                       uint32_t* out_gt) {
  PairingShared<C>* sh = new PairingShared<C>();
  HostLanes x;
  const int st = Tower<C>::equation(x, sh, g1, g1_inf, g2, g2_inf, k, out_gt);
  delete sh;
  return st;
}
// one equation of k pairs in the C ABI's layout; out_gt: 12 NW canonical words
extern "C" int ps_equation(int curve, const uint32_t* g1, const uint8_t* g1_inf, const uint32_t* g2, const uint8_t* g2_inf,
                           int k, uint32_t* out_gt) {
  if (k < 1 || k > PAIRING_MAX_PAIRS) return -1;
  if (curve == 0) return do_equation<Bn254>(g1, g1_inf, g2, g2_inf, k, out_gt);
  if (curve == 1) return do_equation<Bls12_381>(g1, g1_inf, g2, g2_inf, k, out_gt);
  return -1;
}

// The lockstep exchange: a phase with the semantics fp_tower.h's contract assumes -- every lane of a phase starts from
// the state the phase began with, so a body that reads a slot another lane of the same phase writes sees the OLD value
// (HostLanes shows it the new one to every later lane, the wave shows it either).  each() snapshots the shared state,
// and per lane restores the snapshot, runs body(t), and moves the words body(t) changed into the post-state, which it
// installs after the last lane.  A word changed by two different lanes of one phase is a conflict.  `reverse` runs
// body(n - 1), ..., body(0): nothing changes under the contract.  Only PairingShared is exchanged: what a body writes
// elsewhere (out_gt) is written by one lane per word.
template <class C>
struct LockstepLanes {
  using Sh = PairingShared<C>;
  static constexpr size_t WORDS = sizeof(Sh) / sizeof(uint32_t);
  static_assert(sizeof(Sh) % sizeof(uint32_t) == 0 && alignof(Sh) == alignof(uint32_t), "PairingShared is 32-bit words");
  Sh* sh;
  bool reverse;
  uint32_t* snap;
  uint32_t* post;
  int* owner;
  unsigned long long conflicts = 0, phases = 0, widest = 0;

  LockstepLanes(Sh* s, bool rev) : sh(s), reverse(rev), snap(new uint32_t[WORDS]), post(new uint32_t[WORDS]),
                                   owner(new int[WORDS]) {}
  ~LockstepLanes() { delete[] snap; delete[] post; delete[] owner; }
  LockstepLanes(const LockstepLanes&) = delete;
  LockstepLanes& operator=(const LockstepLanes&) = delete;

  template <class Fn>
  void each(int n, Fn fn) {
    ++phases;
    if ((unsigned long long)n > widest) widest = (unsigned long long)n;
    memcpy(snap, sh, sizeof(Sh));
    memcpy(post, sh, sizeof(Sh));
    for (size_t w = 0; w < WORDS; ++w) owner[w] = -1;
    uint32_t* live = reinterpret_cast<uint32_t*>(sh);     // every member of PairingShared is an array of uint32_t
    for (int i = 0; i < n; ++i) {
      const int t = reverse ? n - 1 - i : i;
      fn(t);                                              // on the snapshot: the words lane t changed are put back below
      for (size_t w = 0; w < WORDS; ++w) {
        if (live[w] == snap[w]) continue;
        if (owner[w] >= 0 && owner[w] != t) ++conflicts;
        owner[w] = t;
        post[w] = live[w];
        live[w] = snap[w];
      }
    }
    memcpy(sh, post, sizeof(Sh));
  }
  static uint32_t uniform(uint32_t v) { return v; }
};

template <class C>
static int do_equation_lockstep(bool reverse, const uint32_t* g1, const uint8_t* g1_inf, const uint32_t* g2,
                                const uint8_t* g2_inf, int k, uint32_t* out_gt, unsigned long long* info) {
  PairingShared<C>* sh = new PairingShared<C>();
  int st;
  {
    LockstepLanes<C> x(sh, reverse);
    st = Tower<C>::equation(x, sh, g1, g1_inf, g2, g2_inf, k, out_gt);
    if (info) { info[0] = x.conflicts; info[1] = x.phases; info[2] = x.widest; }
  }
  delete sh;
  return st;
}
static int equation_lockstep(bool reverse, int curve, const uint32_t* g1, const uint8_t* g1_inf, const uint32_t* g2,
                             const uint8_t* g2_inf, int k, uint32_t* out_gt, unsigned long long* info) {
  if (k < 1 || k > PAIRING_MAX_PAIRS) return -1;
  if (curve == 0) return do_equation_lockstep<Bn254>(reverse, g1, g1_inf, g2, g2_inf, k, out_gt, info);
  if (curve == 1) return do_equation_lockstep<Bls12_381>(reverse, g1, g1_inf, g2, g2_inf, k, out_gt, info);
  return -1;
}
// ps_equation through the lockstep exchange; info (may be null): conflicts, phases, the lanes of the widest phase
extern "C" int ps_equation_lockstep(int curve, const uint32_t* g1, const uint8_t* g1_inf, const uint32_t* g2,
                                    const uint8_t* g2_inf, int k, uint32_t* out_gt, unsigned long long* info) {
  return equation_lockstep(false, curve, g1, g1_inf, g2, g2_inf, k, out_gt, info);
}
// the same with the lanes of every phase in reverse order
extern "C" int ps_equation_lockstep_reverse(int curve, const uint32_t* g1, const uint8_t* g1_inf, const uint32_t* g2,
                                            const uint8_t* g2_inf, int k, uint32_t* out_gt, unsigned long long* info) {
  return equation_lockstep(true, curve, g1, g1_inf, g2, g2_inf, k, out_gt, info);
}

#ifdef KZG_AUDIT_ON
extern "C" void ps_audit_reset(int lift) { audit::state() = audit::State{0, "", "", 0, lift != 0}; }
extern "C" unsigned long long ps_audit_read(char* fn, char* what, int cap, int* line) {
  const audit::State& s = audit::state();
  snprintf(fn, cap, "%s", s.fn);
  snprintf(what, cap, "%s", s.what);
  *line = s.line;
  return s.count;
}
#endif

#ifdef PAIRING_SHIM_MAIN
// The drivers above on inputs made here: e(G1, G2) is not one; e(G1, G2) e(-G1, G2) is, through the lockstep exchange
// as well (its snapshots and merges run under the sanitizers here); an infinity flag skips a pair;
// a G2 point off the twist and a coordinate equal to p give status 2 and a zeroed value; a a^-1 = 1, (a^p)^p = a^(p^2),
// a sparse product equals the full one, on tower values made from the limbs of p.
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { ++fails; printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

template <class C>
static void self_test(int curve, const uint32_t* g1, const uint32_t* neg_y, const uint32_t* g2) {
  using F = typename C::Fp;
  using Fd = Field<F>;
  constexpr int NW = F::NW, N = F::N;
  uint32_t p1[4 * NW], q[8 * NW], gt[12 * NW], gt2[12 * NW];
  uint8_t inf[2] = {0, 0};
  memcpy(p1, g1, 8 * NW); memcpy(p1 + 2 * NW, g1, 4 * NW); memcpy(p1 + 3 * NW, neg_y, 4 * NW);
  memcpy(q, g2, 16 * NW); memcpy(q + 4 * NW, g2, 16 * NW);
  EXPECT(ps_equation(curve, p1, nullptr, q, nullptr, 1, gt) == 1);
  EXPECT(ps_equation(curve, p1, nullptr, q, nullptr, 2, gt2) == 0 && gt2[0] == 1 && gt2[1] == 0 && gt2[2 * NW] == 0);
  // the same equation through the lockstep exchange: no word written twice in a phase, the widest phase is an Fp12
  // product's 36 lanes, and the value is the sequential one
  unsigned long long info[3] = {9, 0, 0};
  memset(gt2, 0xff, sizeof(gt2));
  EXPECT(ps_equation_lockstep(curve, p1, nullptr, q, nullptr, 2, gt2, info) == 0 && gt2[0] == 1 && gt2[1] == 0 &&
         gt2[2 * NW] == 0 && info[0] == 0 && info[1] > 1000 && info[2] == 36);
  inf[1] = 1;
  EXPECT(ps_equation(curve, p1, inf, q, nullptr, 2, gt2) == 1 && memcmp(gt, gt2, sizeof(gt)) == 0);
  inf[0] = 1;
  EXPECT(ps_equation(curve, p1, nullptr, q, inf, 2, gt2) == 0);
  q[4 * NW] ^= 1u;                                                   // off the twist
  EXPECT(ps_equation(curve, p1, nullptr, q, nullptr, 2, gt2) == 2 && gt2[0] == 0);
  memcpy(q + 4 * NW, g2, 16 * NW);
  for (int k = 0; k < NW; ++k) q[5 * NW + k] = F::PW[k];            // x.c1 = p
  EXPECT(ps_equation(curve, p1, nullptr, q, nullptr, 2, gt2) == 2);
  // tower values from the limbs at hand
  uint32_t a[12 * N], b[12 * N], r[12 * N], s[12 * N], one[12 * N];
  for (int k = 0; k < 12; ++k) {
    Fe<F> v = Fd::zero(), w = Fd::zero();
    for (int j = 0; j < N; ++j) { v.l[j] = (F::P[j] ^ (0x1234567u * (k + 1))) & F::MASK; w.l[j] = (F::R2[j] + k) & F::MASK; }
    v.l[N - 1] = F::P[N - 1] >> 1; w.l[N - 1] = F::P[N - 1] >> 2;
    memcpy(a + k * N, v.l, 4 * N);
    memcpy(b + k * N, w.l, 4 * N);
  }
  memset(one, 0, sizeof(one));
  memcpy(one, F::R1, 4 * N);
  auto same = [&](const uint32_t* u, const uint32_t* v) {
    for (int k = 0; k < 12; ++k) {
      Fe<F> x, y;
      memcpy(x.l, u + k * N, 4 * N); memcpy(y.l, v + k * N, 4 * N);
      if (!Fd::eq(x, y)) return false;
    }
    return true;
  };
  EXPECT(ps_fp12(curve, OP_INV, a, a, r) == 0 && ps_fp12(curve, OP_MUL, a, r, s) == 0 && same(s, one));
  EXPECT(ps_fp12(curve, OP_FROB1, a, a, r) == 0 && ps_fp12(curve, OP_FROB1, r, r, s) == 0 &&
         ps_fp12(curve, OP_FROB2, a, a, r) == 0 && same(r, s));
  const unsigned mask = ps_line_mask(curve);
  for (int k = 0; k < 6; ++k)
    if (!((mask >> k) & 1u)) memset(b + 2 * N * k, 0, 8 * N);
  EXPECT(ps_fp12(curve, OP_SPARSE, a, b, r) == 0 && ps_fp12(curve, OP_MUL, a, b, s) == 0 && same(r, s));
  EXPECT(ps_fp12(curve, OP_SQR, a, a, r) == 0 && ps_fp12(curve, OP_MUL, a, a, s) == 0 && same(r, s));
  memset(a, 0, sizeof(a));
  EXPECT(ps_fp12(curve, OP_INV, a, a, r) == 0 && same(r, a));       // inv(0) = 0
}

int main() {
  static const uint32_t G1_BN[16] = {1, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0};
  static const uint32_t NEGY_BN[8] = {0xd87cfd45u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u, 0x8181585du, 0xb85045b6u,
                                      0xe131a029u, 0x30644e72u};
  static const uint32_t G2_BN[32] = {
      0xd992f6edu, 0x46debd5cu, 0xf75edaddu, 0x674322d4u, 0x5e5c4479u, 0x426a0066u, 0x121f1e76u, 0x1800deefu,
      0xaef312c2u, 0x97e485b7u, 0x35a9e712u, 0xf1aa4933u, 0x31fb5d25u, 0x7260bfb7u, 0x920d483au, 0x198e9393u,
      0x66fa7daau, 0x4ce6cc01u, 0x0c43d37bu, 0xe3d1e769u, 0x8dcb408fu, 0x4aab7180u, 0xdb8c6debu, 0x12c85ea5u,
      0xd122975bu, 0x55acdadcu, 0x70b38ef3u, 0xbc4b3133u, 0x690c3395u, 0xec9e99adu, 0x585ff075u, 0x090689d0u};
  static const uint32_t G1_BLS[24] = {
      0xdb22c6bbu, 0xfb3af00au, 0xf97a1aefu, 0x6c55e83fu, 0x171bac58u, 0xa14e3a3fu, 0x9774b905u, 0xc3688c4fu,
      0x4fa9ac0fu, 0x2695638cu, 0x3197d794u, 0x17f1d3a7u,
      0x46c5e7e1u, 0x0caa2329u, 0xa2888ae4u, 0xd03cc744u, 0x2c04b3edu, 0x00db18cbu, 0xd5d00af6u, 0xfcf5e095u,
      0x741d8ae4u, 0xa09e30edu, 0xe3aaa0f1u, 0x08b3f481u};
  static const uint32_t NEGY_BLS[12] = {0xb939c2cau, 0xad54dcd6u, 0x0ecb751bu, 0x4e6f38bau, 0xcaac4236u, 0x6655b9d5u,
                                        0x1db507c9u, 0x67816aefu, 0xcf2e21f2u, 0xaa7d76c8u, 0x55d545a8u, 0x114d1d68u};
  static const uint32_t G2_BLS[48] = {
      0xc121bdb8u, 0xd48056c8u, 0xa805bbefu, 0x0bac0326u, 0x7ae3d177u, 0xb4510b64u, 0xfa403b02u, 0xc6e47ad4u,
      0x2dc51051u, 0x26080527u, 0xf08f0a91u, 0x024aa2b2u,
      0x5d042b7eu, 0xe5ac7d05u, 0x13945d57u, 0x334cf112u, 0xdc7f5049u, 0xb5da61bbu, 0x9920b61au, 0x596bd0d0u,
      0x88274f65u, 0x7dacd3a0u, 0x52719f60u, 0x13e02b60u,
      0x08b82801u, 0xe1935486u, 0x3baca289u, 0x923ac9ccu, 0x5160d12cu, 0x6d429a69u, 0x8cbdd3a7u, 0xadfd9baau,
      0xda2e351au, 0x8cc9cdc6u, 0x727d6e11u, 0x0ce5d527u,
      0xf05f79beu, 0xaaa9075fu, 0x5cec1da1u, 0x3f370d27u, 0x572e99abu, 0x267492abu, 0x85a763afu, 0xcb3e287eu,
      0x2bc28b99u, 0x32acd2b0u, 0x2ea734ccu, 0x0606c4a0u};
  self_test<Bn254>(0, G1_BN, NEGY_BN, G2_BN);
  self_test<Bls12_381>(1, G1_BLS, NEGY_BLS, G2_BLS);
#ifdef KZG_AUDIT_ON
  const audit::State& s = audit::state();
  if (s.count) { printf("%llu audit violations, first in %s (line %d): %s\n", s.count, s.fn, s.line, s.what); return 2; }
#endif
  if (fails) { printf("%d checks failed\n", fails); return 1; }
  printf("no violations\n");
  return 0;
}
#endif
