// Host-only test shim, second of two: drives kzg_snark_amd/csrc/field.h and ec.h (the headers the gfx950 kernels
// compile) with RAW LIMBS -- nothing enters through to_mont(from_words(canonical)) -- so that the tops of the lazy
// ranges (2p-1, 8p-1, 10p-1, 64p-1) and all-ones limb patterns can be reached on purpose.  Built with -DKZG_AUDIT:
// every call also runs the pre/postcondition hooks of field.h, read back through bs_audit_read().
// The same file builds as a standalone program (-DBOUNDS_SHIM_MAIN) that runs the drivers on patterns of its own;
// tests/test_field_bounds_host.py builds that with the address and undefined-behaviour sanitizers.
// Test infrastructure only.
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../kzg_snark_amd/csrc/field.h"
#include "../../kzg_snark_amd/csrc/ec.h"
using namespace kzg;

#ifndef KZG_AUDIT_ON
#error "bounds_shim.cpp is meant to be built with -DKZG_AUDIT"
#endif

// ---- layout and constants, from the header (Python keeps no copy) ---------------------------------
template <class F>
static int info(int* geo, uint32_t* p, uint32_t* r1) {
  geo[0] = F::L; geo[1] = F::N; geo[2] = F::NW; geo[3] = F::BITS; geo[4] = Field<F>::FIT; geo[5] = Field<F>::CAP;
  for (int j = 0; j < F::N; ++j) { p[j] = F::P[j]; r1[j] = F::R1[j]; }
  return 0;
}
#define BS_FIELDS(CALL)                 \
  switch (field) {                      \
    case 0: return CALL(BnFr);          \
    case 1: return CALL(BnFp);          \
    case 2: return CALL(BlsFr);         \
    case 3: return CALL(BlsFp);         \
  }                                     \
  return -1;

extern "C" int bs_info(int field, int* geo, uint32_t* p, uint32_t* r1) {
#define C_(F) info<F>(geo, p, r1)
  BS_FIELDS(C_)
#undef C_
}
// the redistributed multiples of p (K = 2, 4, 6, 8), for the dominance test
template <class F>
static int pkr_of(int K, uint32_t* out) {
  const uint32_t* t = K == 2 ? F::P2R : K == 4 ? F::P4R : K == 6 ? F::P6R : K == 8 ? F::P8R : nullptr;
  if (!t) return -1;
  for (int j = 0; j < F::N; ++j) out[j] = t[j];
  return 0;
}
extern "C" int bs_pkr(int field, int K, uint32_t* out) {
#define C_(F) pkr_of<F>(K, out)
  BS_FIELDS(C_)
#undef C_
}

extern "C" void bs_audit_reset(int lift) {
  audit::State& s = audit::state();
  s.count = 0; s.fn = ""; s.what = ""; s.line = 0; s.lift = lift != 0;
}
extern "C" unsigned long long bs_audit_read(char* fn, char* what, int cap, int* line) {
  const audit::State& s = audit::state();
  snprintf(fn, cap, "%s", s.fn);
  snprintf(what, cap, "%s", s.what);
  *line = s.line;
  return s.count;
}

// ---- one column at capacity: FIT products of two all-ones limbs on top of the largest carry ---------
// (the claim in the comment above Field::FIT).  nprod products go through mad_wide, whose audit hook records a
// carry out of 64 bits.
template <class F>
static int column(int nprod) {
  uint64_t acc = (1ull << (64 - F::L)) - 1;          // the largest carry: a full column shifted down by L
  for (int i = 0; i < nprod; ++i) acc = mad_wide(F::MASK, F::MASK, acc);
  return (int)(acc & 1);
}
extern "C" int bs_column(int field, int nprod) {
#define C_(F) column<F>(nprod)
  BS_FIELDS(C_)
#undef C_
}

// ---- every public function of Field<F>, raw limbs in and out -----------------------------------------
template <class F>
static int field_op(int op, const uint32_t* in, uint32_t* out) {
  using Fd = Field<F>;
  using E = Fe<F>;
  constexpr int N = F::N;
  auto get = [&](int i) { E e; for (int j = 0; j < N; ++j) e.l[j] = in[i * N + j]; return e; };
  auto put = [&](const E& e) { for (int j = 0; j < N; ++j) out[j] = e.l[j]; return 0; };
  auto dotk = [&](auto kc) {
    constexpr int K = decltype(kc)::value;
    E a[K], b[K];
    for (int t = 0; t < K; ++t) { a[t] = get(t); b[t] = get(K + t); }
    return put(Fd::template dot<K>(a, b));
  };
  switch (op) {
    case 0: return put(Fd::mul(get(0), get(1)));
    case 1: return put(Fd::sqr(get(0)));
    case 2: return put(Fd::mul2(get(0), get(1), get(2), get(3)));
    case 3: return dotk(std::integral_constant<int, 1>());
    case 4: return dotk(std::integral_constant<int, 2>());
    case 5: return dotk(std::integral_constant<int, 3>());
    case 6: return dotk(std::integral_constant<int, 6>());
    case 7: return dotk(std::integral_constant<int, 16>());    // the largest K the static_assert admits
    case 8: return put(Fd::add(get(0), get(1)));
    case 9: return put(Fd::sub(get(0), get(1)));
    case 10: return put(Fd::dbl(get(0)));
    case 11: return put(Fd::neg(get(0)));
    case 12: return put(Fd::neg_weak(get(0)));
    case 13: return put(Fd::reduce(get(0)));
    case 14: return put(Fd::reduce_wide(get(0)));
    case 15: return put(Fd::carry(get(0)));
    case 16: return put(Fd::add_lazy(get(0), get(1)));
    case 17: return put(Fd::sub_lazy4(get(0), get(1)));
    case 18: return put(Fd::template sub_carry<2>(get(0), get(1)));
    case 19: return put(Fd::template sub_carry<4>(get(0), get(1)));
    case 20: return put(Fd::template sub_carry<6>(get(0), get(1)));
    case 21: return put(Fd::template sub_carry<8>(get(0), get(1)));
    case 22: return put(Fd::template sub_carry_cneg<2>(get(0), false, get(1)));
    case 23: return put(Fd::template sub_carry_cneg<2>(get(0), true, get(1)));
    case 24: return put(Fd::add_twice_carry(get(0), get(1)));
    case 25: return put(Fd::cneg_canonical(get(0), false));
    case 26: return put(Fd::cneg_canonical(get(0), true));
    case 27: return Fd::is_zero(get(0)) ? 1 : 0;
    case 28: return Fd::is_zero_weak(get(0)) ? 1 : 0;
    case 29: return put(Fd::from_words(in));                    // in: NW saturated words
    case 30: Fd::to_words(get(0), out); return 0;               // out: NW saturated words
    case 31: return put(Fd::to_mont(get(0)));
    case 32: return put(Fd::from_mont(get(0)));
    case 33: return put(Fd::inv(get(0)));
    case 34: return dotk(std::integral_constant<int, 4>());
    case 35: return dotk(std::integral_constant<int, 5>());
    case 36: return Fd::eq(get(0), get(1)) ? 1 : 0;
  }
  return -1;
}
extern "C" int bs_field_op(int field, int op, const uint32_t* in, uint32_t* out) {
#define C_(F) field_op<F>(op, in, out)
  BS_FIELDS(C_)
#undef C_
}

// ---- ec.h, raw Montgomery-form limbs ------------------------------------------------------------
// in: acc (X, Y, ZZ, ZZZ), affine (x2, y2), second acc (X, Y, ZZ, ZZZ): 10 elements.  out: 4 elements.
template <class C>
static int ec_op(int op, const uint32_t* in, uint32_t* out) {
  using F = typename C::Fp;
  using E = Fe<F>;
  using G = Ec<C>;
  constexpr int N = F::N;
  auto get = [&](int i) { E e; for (int j = 0; j < N; ++j) e.l[j] = in[i * N + j]; return e; };
  auto putp = [&](const XYZZ<C>& p) {
    for (int j = 0; j < N; ++j) { out[j] = p.x.l[j]; out[N + j] = p.y.l[j]; out[2 * N + j] = p.zz.l[j]; out[3 * N + j] = p.zzz.l[j]; }
  };
  XYZZ<C> a, b;
  a.x = get(0); a.y = get(1); a.zz = get(2); a.zzz = get(3);
  const E x2 = get(4), y2 = get(5);
  b.x = get(6); b.y = get(7); b.zz = get(8); b.zzz = get(9);
  switch (op) {
    case 0: putp(G::madd(a, x2, y2)); return 0;
    case 1:
    case 2: {
      bool fin = true;
      putp(G::madd_finite(a, x2, y2, op == 2, fin));
      return fin ? 1 : 0;
    }
    case 3: putp(G::add(a, b)); return 0;
    case 4: putp(G::dbl(a)); return 0;
    case 5: putp(G::dbl_affine(x2, y2)); return 0;
    case 6: {
      const Affine<C> r = G::to_affine(a);
      for (int j = 0; j < N; ++j) { out[j] = r.x.l[j]; out[N + j] = r.y.l[j]; }
      return r.inf ? 1 : 0;
    }
    case 7: return G::on_curve(x2, y2) ? 1 : 0;
  }
  return -1;
}
extern "C" int bs_ec_op(int curve, int op, const uint32_t* in, uint32_t* out) {
  if (curve == 0) return ec_op<Bn254>(op, in, out);
  if (curve == 1) return ec_op<Bls12_381>(op, in, out);
  return -1;
}

// A long flag-tracked accumulation, the loop body of msm_accumulate_kernel (msm.hip; restated in field_shim.cpp
// cases 4 and 5): pool of npool canonical Montgomery-form affine points (x, y: 2 elements each), step s adds
// (neg[s] ? - : +) pool[idx[s]].  Ends as the MSM's consumers do: add(acc, from_affine(pool[0])), dbl, to_affine.
// out: canonical plain x, y (N limbs each).  Returns 1 if the result is infinity, 0 if finite, -2 if the X of the
// accumulator reached 8p at some step.
template <class C>
static int ec_chain(const uint32_t* pool, int npool, const uint8_t* idx, const uint8_t* negs, int steps, uint32_t* out) {
  using F = typename C::Fp;
  using Fd = Field<F>;
  using E = Fe<F>;
  using G = Ec<C>;
  constexpr int N = F::N;
  auto get = [&](int i) { E e; for (int j = 0; j < N; ++j) e.l[j] = pool[i * N + j]; return e; };
  bool fin = false;
  XYZZ<C> t = G::infinity();
  t.zz = Fd::one(); t.zzz = Fd::one();
  for (int s = 0; s < steps; ++s) {
    if (idx[s] >= npool) return -1;
    const E x = get(2 * idx[s]), y = get(2 * idx[s] + 1);
    const bool negate = negs[s] != 0;
    if (!fin) { t.x = x; t.y = Fd::cneg_canonical(y, negate); t.zz = Fd::one(); t.zzz = Fd::one(); fin = true; }
    else {
      t = G::madd_finite(t, x, y, negate, fin);
      if (!fin) { t.zz = Fd::one(); t.zzz = Fd::one(); }
    }
    if (fin && !audit::below_kp<F>(t.x.l, 8)) return -2;
  }
  Affine<C> first;
  first.x = get(0); first.y = get(1); first.inf = false;
  const XYZZ<C> acc = fin ? t : G::infinity();
  const Affine<C> r = G::to_affine(G::dbl(G::add(acc, G::from_affine(first))));
  if (r.inf) return 1;
  const E rx = Fd::from_mont(r.x), ry = Fd::from_mont(r.y);
  for (int j = 0; j < N; ++j) { out[j] = rx.l[j]; out[N + j] = ry.l[j]; }
  return 0;
}
extern "C" int bs_ec_chain(int curve, const uint32_t* pool, int npool, const uint8_t* idx, const uint8_t* negs, int steps,
                           uint32_t* out) {
  if (curve == 0) return ec_chain<Bn254>(pool, npool, idx, negs, steps, out);
  if (curve == 1) return ec_chain<Bls12_381>(pool, npool, idx, negs, steps, out);
  return -1;
}

// ---- the NTT's lazy arithmetic, restated ------------------------------------------------------------
// The op sequences of csrc/ntt.hip, on four elements x[0..3] in place (limbs as they lie in LDS):
//   kind 0: first_step (ntt.hip, `first_step`: levels 1 and 2; tw[0] = w^(n/4))
//   kind 1: radix4_step (ntt.hip, `radix4_step`: levels s, s+1; tw[0..2] = Tw3 a, b, c)
//   kind 2: the odd-k radix-2 level ("odd k: one radix-2 level first" in ntt_pass_kernel) on (x[0], x[1]) and (x[2], x[3])
// `shift` > 0 is the misuse the audit must notice: the operands of the un-carried products scaled to limbs of 2^(L+shift).
template <class F>
static void ntt_step(int kind, Fe<F>* x, const Fe<F>* tw, int shift) {
  using Fd = Field<F>;
  using E = Fe<F>;
  auto widen = [&](E v) {
    if (shift) for (int j = 0; j < F::N; ++j) v.l[j] = (uint32_t)((1ull << (F::L + shift)) - 1);
    return v;
  };
  auto out = [](const E& v) { return Fd::carry(v); };       // put_out
  if (kind == 0) {
    const E x0 = x[0], x2 = x[2], t1 = x[1], t3 = x[3];
    const E b0 = Fd::add_lazy(x0, t1), b1 = Fd::sub_lazy4(x0, t1);
    const E u2 = Fd::carry(Fd::add_lazy(x2, t3));
    const E u3 = Fd::mul(widen(Fd::sub_lazy4(x2, t3)), tw[0]);
    x[0] = out(Fd::add_lazy(b0, u2));
    x[2] = out(Fd::sub_lazy4(b0, u2));
    x[1] = out(Fd::add_lazy(b1, u3));
    x[3] = out(Fd::sub_lazy4(b1, u3));
  } else if (kind == 1) {
    const E x0 = x[0], x2 = x[2];
    const E t1 = Fd::mul(x[1], tw[0]), t3 = Fd::mul(x[3], tw[0]);
    const E b0 = Fd::add_lazy(x0, t1), b1 = Fd::sub_lazy4(x0, t1);
    const E u2 = Fd::mul(widen(Fd::add_lazy(x2, t3)), tw[1]), u3 = Fd::mul(widen(Fd::sub_lazy4(x2, t3)), tw[2]);
    x[0] = out(Fd::add_lazy(b0, u2));
    x[2] = out(Fd::sub_lazy4(b0, u2));
    x[1] = out(Fd::add_lazy(b1, u3));
    x[3] = out(Fd::sub_lazy4(b1, u3));
  } else {
    for (int h = 0; h < 4; h += 2) {
      const E a = x[h], b = x[h + 1];
      x[h] = Fd::carry(Fd::add_lazy(a, b));
      x[h + 1] = Fd::carry(Fd::sub_lazy4(a, b));
    }
  }
}
// The pass epilogue (the store loop of ntt_pass_kernel): 0 = EPI_REDUCE (reduce_wide), 1 = EPI_FACTOR (two products,
// left weak-normal), 2 = EPI_TABLE (one product, weak-normal), 3 = EPI_SCALE (reduce(mul)).
template <class F>
static Fe<F> ntt_epilogue(int epi, const Fe<F>& x, const Fe<F>* f) {
  using Fd = Field<F>;
  if (epi == 0) return Fd::reduce_wide(x);
  if (epi == 1) return Fd::mul(Fd::mul(x, f[0]), f[1]);
  if (epi == 2) return Fd::mul(x, f[0]);
  return Fd::reduce(Fd::mul(x, f[0]));
}
// nsteps fused steps on x[4] (raw limbs), outputs fed back; step i takes kinds[i] and the three twiddles tw[3i..3i+2].
// after[i*4 .. i*4+3]: the four elements after step i (so Python can follow the growth).  Then the epilogue on each
// element with factors f[0..1] -> fin[4].
template <class F>
static int ntt_run(const uint32_t* x_in, const int* kinds, const uint32_t* tw_in, int nsteps, int shift, int epi,
                   const uint32_t* f_in, uint32_t* after, uint32_t* fin) {
  using E = Fe<F>;
  constexpr int N = F::N;
  auto load = [&](const uint32_t* p) { E e; for (int j = 0; j < N; ++j) e.l[j] = p[j]; return e; };
  E x[4];
  for (int i = 0; i < 4; ++i) x[i] = load(x_in + i * N);
  for (int s = 0; s < nsteps; ++s) {
    const E tw[3] = {load(tw_in + (3 * s) * N), load(tw_in + (3 * s + 1) * N), load(tw_in + (3 * s + 2) * N)};
    ntt_step<F>(kinds[s], x, tw, shift);
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < N; ++j) after[(s * 4 + i) * N + j] = x[i].l[j];
  }
  const E f[2] = {load(f_in), load(f_in + N)};
  for (int i = 0; i < 4; ++i) {
    const E r = ntt_epilogue<F>(epi, x[i], f);
    for (int j = 0; j < N; ++j) fin[i * N + j] = r.l[j];
  }
  return 0;
}
extern "C" int bs_ntt_run(int field, const uint32_t* x, const int* kinds, const uint32_t* tw, int nsteps, int shift, int epi,
                          const uint32_t* f, uint32_t* after, uint32_t* fin) {
  if (field == 0) return ntt_run<BnFr>(x, kinds, tw, nsteps, shift, epi, f, after, fin);
  if (field == 2) return ntt_run<BlsFr>(x, kinds, tw, nsteps, shift, epi, f, after, fin);
  return -1;
}

// ---- the lazy sites of poly.hip, restated -------------------------------------------------------------
// site 0: `lane8_sum_reduced` / the chunk sums of tile_combine_kernel: eight weak-normal values added limb by limb
//         (lane8_sum: plain 32-bit additions), then reduce_wide(carry(sum)).  in: 8 elements.
// site 1: `dot_upto` as lincomb_kernel and tile_combine_kernel call it: cnt <= 6 canonical coefficients (load_words)
//         against Montgomery-form powers (weak-normal), the groups joined by Field::add.  in: 2*cnt elements (c, then x).
template <class F>
static int poly_site(int site, int cnt, const uint32_t* in, uint32_t* out) {
  using Fd = Field<F>;
  using E = Fe<F>;
  constexpr int N = F::N;
  auto get = [&](int i) { E e; for (int j = 0; j < N; ++j) e.l[j] = in[i * N + j]; return e; };
  E r;
  if (site == 0) {
    E s = Fd::zero();
    for (int i = 0; i < 8; ++i) s = Fd::add_lazy(s, get(i));       // one 32-bit addition per limb, as the DPP sum
    r = Fd::reduce_wide(Fd::carry(s));
  } else {
    E c[6], x[6];
    for (int g = 0; g < 6; ++g) { c[g] = g < cnt ? get(g) : Fd::zero(); x[g] = get(cnt + (g < cnt ? g : 0)); }
    switch (cnt) {
      case 1: r = Fd::template dot<1>(c, x); break;
      case 2: r = Fd::template dot<2>(c, x); break;
      case 3: r = Fd::template dot<3>(c, x); break;
      case 4: r = Fd::template dot<4>(c, x); break;
      case 5: r = Fd::template dot<5>(c, x); break;
      default: r = Fd::template dot<6>(c, x);
    }
  }
  for (int j = 0; j < N; ++j) out[j] = r.l[j];
  return 0;
}
extern "C" int bs_poly_site(int field, int site, int cnt, const uint32_t* in, uint32_t* out) {
  if (field == 0) return poly_site<BnFr>(site, cnt, in, out);
  if (field == 2) return poly_site<BlsFr>(site, cnt, in, out);
  return -1;
}

// ---- standalone program: the same drivers over patterns of its own (for the sanitizers) ---------------------
#ifdef BOUNDS_SHIM_MAIN
// value K*p - 1 - d as raw limbs, with the lower limbs taken from `pat` where that keeps the value below K*p:
// all lower limbs all-ones, top limb one under the top limb of K*p - 1 (or equal to it, with the limbs of K*p - 1)
template <class F>
static Fe<F> top_of(uint32_t K, int variant) {
  Fe<F> e;
  uint64_t c = 0;
  for (int j = 0; j < F::N; ++j) {                    // K*p, carried
    c += (uint64_t)K * F::P[j];
    e.l[j] = j < F::N - 1 ? (uint32_t)(c & F::MASK) : (uint32_t)c;
    if (j < F::N - 1) c >>= F::L;
  }
  int j = 0;                                          // minus 1
  while (e.l[j] == 0) e.l[j++] = F::MASK;
  e.l[j] -= 1;
  if (variant == 1 && e.l[F::N - 1] > 0) {            // all-ones lower limbs under the top limb
    e.l[F::N - 1] -= 1;
    for (int i = 0; i < F::N - 1; ++i) e.l[i] = F::MASK;
  }
  return e;
}
template <class F>
static void self_field() {
  using Fd = Field<F>;
  using E = Fe<F>;
  uint32_t in[32 * F::N], out[4 * F::N];
  for (int variant = 0; variant < 2; ++variant) {
    const E w = top_of<F>(2, variant), c = top_of<F>(1, variant);
    for (int i = 0; i < 32; ++i) memcpy(in + i * F::N, (i & 1 ? w : top_of<F>(2, 1 - variant)).l, sizeof(w.l));
    for (int op = 0; op <= 13; ++op) field_op<F>(op, in, out);
    for (int op = 15; op <= 19; ++op) field_op<F>(op, in, out);
    field_op<F>(22, in, out); field_op<F>(23, in, out); field_op<F>(24, in, out);
    field_op<F>(34, in, out); field_op<F>(35, in, out);
    memcpy(in, top_of<F>(64, variant).l, sizeof(w.l));
    field_op<F>(14, in, out);
    memcpy(in, top_of<F>(8, variant).l, sizeof(w.l));
    memcpy(in + F::N, top_of<F>(6, variant).l, sizeof(w.l));
    field_op<F>(20, in, out);
    memcpy(in + F::N, top_of<F>(8, variant).l, sizeof(w.l));
    field_op<F>(21, in, out);
    memcpy(in, c.l, sizeof(c.l));
    for (int op = 25; op <= 28; ++op) field_op<F>(op, in, out);
    for (int op = 30; op <= 33; ++op) field_op<F>(op, in, out);
    uint32_t words[F::NW];
    Fd::to_words(c, words);
    field_op<F>(29, words, out);
  }
  for (int n = 1; n <= Fd::FIT; ++n) column<F>(n);
}
template <class F>
static void self_ntt() {
  using E = Fe<F>;
  uint32_t x[4 * F::N], tw[18 * F::N], f[2 * F::N], after[6 * 4 * F::N], fin[4 * F::N];
  const E c = top_of<F>(1, 1), c0 = top_of<F>(1, 0);
  for (int i = 0; i < 4; ++i) memcpy(x + i * F::N, (i & 1 ? c : c0).l, sizeof(c.l));
  for (int i = 0; i < 18; ++i) memcpy(tw + i * F::N, (i % 3 ? c : c0).l, sizeof(c.l));
  memcpy(f, c.l, sizeof(c.l)); memcpy(f + F::N, c0.l, sizeof(c.l));
  const int even[6] = {0, 1, 1, 1, 1, 1}, odd[6] = {2, 1, 1, 1, 1, 1};
  for (int epi = 0; epi < 4; ++epi) {
    ntt_run<F>(x, even, tw, 6, 0, epi, f, after, fin);
    ntt_run<F>(x, odd, tw, 6, 0, epi, f, after, fin);
  }
  uint32_t in[12 * F::N], out[F::N];
  for (int i = 0; i < 12; ++i) memcpy(in + i * F::N, (i < 6 ? c : top_of<F>(2, i & 1)).l, sizeof(c.l));
  for (int cnt = 1; cnt <= 6; ++cnt) {
    for (int i = 0; i < cnt; ++i) memcpy(in + (cnt + i) * F::N, top_of<F>(2, i & 1).l, sizeof(c.l));
    poly_site<F>(1, cnt, in, out);
  }
  for (int i = 0; i < 8; ++i) memcpy(in + i * F::N, top_of<F>(2, i & 1).l, sizeof(c.l));
  poly_site<F>(0, 0, in, out);
}
// generator-based chain: the Montgomery form of the generator (1, 2) / the BLS12-381 generator is not known here without
// a conversion, so the chain starts from to_mont(from_words(...)) of the affine generator given by the caller
template <class C>
static int self_ec(const uint32_t* gx_words, const uint32_t* gy_words) {
  using F = typename C::Fp;
  using Fd = Field<F>;
  using E = Fe<F>;
  using G = Ec<C>;
  const E gx = Fd::reduce(Fd::to_mont(Fd::from_words(gx_words))), gy = Fd::reduce(Fd::to_mont(Fd::from_words(gy_words)));
  if (!G::on_curve(gx, gy)) return 1;
  // pool: G, 2G, 3G, 5G as canonical Montgomery affine points
  std::vector<uint32_t> pool;
  XYZZ<C> t = G::from_affine(Affine<C>{gx, gy, false});
  XYZZ<C> mult[4];
  mult[0] = t;
  mult[1] = G::dbl(t);
  mult[2] = G::madd(mult[1], gx, gy);
  mult[3] = G::add(mult[2], mult[1]);
  for (int i = 0; i < 4; ++i) {
    const Affine<C> a = G::to_affine(mult[i]);
    const E x = Fd::reduce(a.x), y = Fd::reduce(a.y);
    if (!G::on_curve(x, y)) return 2;
    pool.insert(pool.end(), x.l, x.l + F::N);
    pool.insert(pool.end(), y.l, y.l + F::N);
  }
  std::vector<uint8_t> idx(600), negs(600);
  uint32_t s = 12345;
  for (int i = 0; i < 600; ++i) {
    s = s * 1664525u + 1013904223u;
    idx[i] = (s >> 24) & 3;
    negs[i] = (s >> 20) & 1;
    if (i % 50 == 10) { idx[i] = idx[i - 1]; negs[i] = negs[i - 1]; }        // P + P
    if (i % 50 == 30) { idx[i] = idx[i - 1]; negs[i] = !negs[i - 1]; }       // back where it was
  }
  uint32_t out[2 * F::N];
  const int rc = ec_chain<C>(pool.data(), 4, idx.data(), negs.data(), 600, out);
  return rc < 0 ? 3 : 0;
}
int main() {
  bs_audit_reset(0);
  for (int lift = 0; lift < 2; ++lift) {
    audit::state().lift = lift != 0;
    self_field<BnFr>(); self_field<BnFp>(); self_field<BlsFr>(); self_field<BlsFp>();
    self_ntt<BnFr>(); self_ntt<BlsFr>();
    const uint32_t bn_gx[8] = {1, 0, 0, 0, 0, 0, 0, 0}, bn_gy[8] = {2, 0, 0, 0, 0, 0, 0, 0};
    // the BLS12-381 G1 generator (public constant), little-endian 32-bit words
    const uint32_t bls_gx[12] = {0xdb22c6bbu, 0xfb3af00au, 0xf97a1aefu, 0x6c55e83fu, 0x171bac58u, 0xa14e3a3fu,
                                 0x9774b905u, 0xc3688c4fu, 0x4fa9ac0fu, 0x2695638cu, 0x3197d794u, 0x17f1d3a7u};
    const uint32_t bls_gy[12] = {0x46c5e7e1u, 0x0caa2329u, 0xa2888ae4u, 0xd03cc744u, 0x2c04b3edu, 0x00db18cbu,
                                 0xd5d00af6u, 0xfcf5e095u, 0x741d8ae4u, 0xa09e30edu, 0xe3aaa0f1u, 0x08b3f481u};
    const int e0 = self_ec<Bn254>(bn_gx, bn_gy), e1 = self_ec<Bls12_381>(bls_gx, bls_gy);
    if (e0 || e1) { fprintf(stderr, "ec self-test failed: %d %d\n", e0, e1); return 3; }
  }
  const audit::State& s = audit::state();
  if (s.count) {
    fprintf(stderr, "audit: %llu violations, first in %s (field.h:%d): %s\n", s.count, s.fn, s.line, s.what);
    return 2;
  }
  printf("bounds shim self-test: no violations\n");
  return 0;
}
#endif
