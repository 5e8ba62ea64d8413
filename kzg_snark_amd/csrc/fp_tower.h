// fp_tower.h -- Fp2 / Fp12 arithmetic, the twist and the optimal-ate pairing for BN254 and BLS12-381,
// on Field<BnFp> / Field<BlsFp> of field.h.  The ONE statement of the pairing: csrc/pairing.hip compiles this text for
// gfx950 and tests/shim/pairing_shim.cpp compiles it with g++; like g1_bytes.h, nothing here is device-only.
//
// Fields.  Fp2 = Fp[i]/(i^2 + 1); Fp12 = Fp2[w]/(w^6 - xi), xi = XI_RE + i (9 + i on BN254, 1 + i on BLS12-381): a
// tower value is its six Fp2 coefficients c[0..5] of 1, w, ..., w^5.  This is the field of kzg_snark_amd/pairing.py:
// sum (a_k + b_k i) w^k is its coefficient list with entry k = a_k - XI_RE b_k and entry k + 6 = b_k (embed_fp2).
// The twist is E': y^2 = x^3 + b', b' = b / xi (BN254, "D") or b xi (BLS12-381, "M"); E'(Fp2) -> E(Fp12) is
// (x, y) -> (x w^2, y w^3) on D and (x / w^2, y / w^3) on M, as pairing.py's untwist.
//
// Lanes.  A pairing equation is worked on by the lanes of one wave.  Everything that crosses lanes is an Fp2 SLOT of a
// PairingShared<C> (LDS on the device, plain memory on the host).  The computation is a PROGRAM of phases (Ins below),
// built at compile time from the loop parameter and the exponents, and Tower::run() is its interpreter: one phase is
// `x.each(n, body)` -- lane t < n runs body(t) on slots it reads and leaves its results in slots -- and what each()
// returns after is visible to every lane.  x is the exchange: WaveLanes of pairing.hip (lane t of the wave runs body(t),
// body(t + 64), ..., then the wave meets), or HostLanes below, which runs body(0), ..., body(n - 1) in turn.  A body
// never reads a slot that another lane writes in the same phase.  Two kinds of phases:
//   product phases: lane t forms ONE Fp2 product dst = a * b of two slots -- the 36 products of an Fp12
//     multiplication, the 18 of a multiplication by a line, the 9 of a cyclotomic squaring, the 6 of a Frobenius map,
//     and the 1..6 products per pair of a point step, for all k pairs at once (k * 6 lanes at the most).  Every product
//     of the pairing goes through the one call of mul2() in run(), so the kernel holds one copy of the multiplier;
//   linear phases: sums, differences and small multiples of slots (the six coefficients of a product, the end of a
//     point step), and one phase with the single Fp inversion.
// The interpreter exists because a gfx950 kernel that calls functions keeps callee-saved registers in scratch memory,
// and one that inlines a multiplier per call site is hundreds of thousands of instructions long.
//
// Limb bounds.  Every value held in a slot is weak-normal (limbs below 2^L, value below 2p): sums and differences go
// through Field::add / sub / dbl / neg, which reduce.  The lazy sequences: the carried sums lz_add() that end in one
// reduce_wide -- up to six products in reduce12(), 9a +- b in mul_xi(), 3T +- 2c in cyc_finish(), bounds stated at each
// -- and the Fp2 product
//     re = mul2(a0, b0, neg_weak(a1), b1),   im = mul2(a0, b1, a1, b0):
// neg_weak(a1) = 2p - a1 has normalised limbs, its top limb is at most 2p's (far below TOP_LIMB_BOUND) and its value is
// in (0, 2p], so the two products of a mul2 sum to at most 8p^2 and (8p^2 + m p) / R < 2p because 8p < R / 16 in both
// base fields (R / p >= 128): mul2's precondition (2) with room, (1) and (3) as for any normalised operand.
//
// The final exponentiation raises to GT_MULTIPLE (p^12 - 1) / r: the easy part (p^6 - 1)(p^2 + 1), then the hard part
// by exponentiations by u with cyclotomic squarings -- BN254: (p^4 - p^2 + 1) / r = p^3 + l2 p^2 + l1 p + l0 with
// l2 = 6u^2 + 1, l1 = -36u^3 - 18u^2 - 12u + 1, l0 = -36u^3 - 30u^2 - 18u - 2 (GT_MULTIPLE = 1); BLS12-381:
// 3 (p^4 - p^2 + 1) / r = (u - 1)^2 (u + p)(u^2 + p^2 - 1) + 3 (GT_MULTIPLE = 3).  gen_constants.py asserts both.
#pragma once
#include "g1_words.h"

namespace kzg {

template <class C>
struct Fp2 {
  Fe<typename C::Fp> c0, c1;     // c0 + c1 i, Montgomery form
};

constexpr int PAIRING_MAX_PAIRS = 16;

// ---- slots -------------------------------------------------------------------------------------------------------
// Tower registers: register g is the six slots 6g .. 6g + 5.  R_F is the Miller accumulator and the result.
enum : int { R_F = 0, R_T0, R_T1, R_T2, R_T3, R_T4, R_T5, R_COUNT };
enum : int {
  S_PROD = 6 * R_COUNT,            // 36: the products of the phase before a linear phase
  S_FROB = S_PROD + 36,            // 18: xi^(k (p^j - 1) / 6) at 6 (j - 1) + k
  S_B3 = S_FROB + 18,              // 3 b'
  S_PAIR = S_B3 + 1,               // the pairs: PS_COUNT slots each
};
// the slots of one pair: R = (X : Y : Z) on the twist, Q affine on the twist, Q' = the point an addition step adds,
// P (its coordinates as Fp2 values with c1 = 0), the three coefficients of the pair's line, temporaries
enum : int { PS_X = 0, PS_Y, PS_Z, PS_QX, PS_QY, PS_QA, PS_QB, PS_PX, PS_PY, PS_LN, PS_T0 = PS_LN + 3, PS_COUNT = PS_T0 + 9 };
constexpr int S_COUNT = S_PAIR + PAIRING_MAX_PAIRS * PS_COUNT;

template <class C>
struct PairingShared {
  Fp2<C> v[S_COUNT];
  uint32_t skip[PAIRING_MAX_PAIRS];           // a point of the pair is infinity
  uint32_t flag[PAIRING_MAX_PAIRS];           // per-lane verdicts on their way to every lane
};

// ---- the program -------------------------------------------------------------------------------------------------
struct Ins {
  uint8_t op, r, a, b;
};
enum : int {
  // product phases (dst = a * b per lane)
  OP_PROD12 = 0,      // prod[6i + j] = reg a [i] * reg b [j], 36 lanes
  OP_PRODLINE,        // prod[6i + j] = reg a [i] * (coefficient j of the current pair's line), 18 lanes
  OP_PRODCYC,         // the nine products of a cyclotomic squaring of reg a
  OP_PRODFROB,        // reg r [t] = reg a [t] * FROB[b - 1][t], 6 lanes
  OP_PRODTAB,         // the products of job table a (reg b for its BASE_REG operands), per pair or once
  OP_PROD_LAST = OP_PRODTAB,
  // linear phases
  OP_RED12,           // reg r = the six coefficients of the product in prod; b = 1: of a product by a line
  OP_CYCFIN,          // reg r = (reg a)^2 from the nine products (cyclotomic subgroup)
  OP_CONJ,            // reg r = conj(reg a): w -> -w, the p^6-power Frobenius
  OP_CONJ2,           // reg r [t] = complex conjugate of reg a [t]
  OP_COPY,            // reg r = reg a
  OP_ONE,             // reg r = 1
  OP_DBL_C1, OP_DBL_C2, OP_ADD_C1, OP_ADD_C2, OP_ADD_C3,      // the linear parts of the point steps, k lanes
  OP_QPREP,           // Q' of every pair: a = 0: Q; 1: conj(Q) (then table QP1: pi(Q)); 2: Q (then QP2: -pi^2(Q))
  OP_INV_C1, OP_INV_C2,                                        // the linear parts of the inversion
  // control, no phase: the instructions a .. between BEGIN and END run once per pair that is not skipped
  OP_PAIRS_BEGIN, OP_PAIRS_END,
};
enum : int { TAB_DBL1 = 0, TAB_DBL1B, TAB_DBL2, TAB_ADD1, TAB_ADD2, TAB_ADD3, TAB_ADD4, TAB_QP1, TAB_QP2, TAB_INV1,
             TAB_INV2, TAB_INV3, TAB_COUNT };
// an operand of a job: a slot of the lane's pair, an absolute slot, or coefficient idx of the instruction's register
enum : int { BASE_PAIR = 0, BASE_ABS = 1, BASE_REG = 2 };
struct Job {
  uint16_t dst, a, b;                         // base << 12 | index
};
constexpr uint16_t jp(int idx) { return (uint16_t)(BASE_PAIR << 12 | idx); }
constexpr uint16_t ja(int idx) { return (uint16_t)(BASE_ABS << 12 | idx); }
constexpr uint16_t jr(int idx) { return (uint16_t)(BASE_REG << 12 | idx); }
constexpr int TAB_MAX_JOBS = 6;
struct JobTable {
  int jobs;
  bool per_pair;
  Job job[TAB_MAX_JOBS];
};

// The point steps, homogeneous projective on the twist, no inversion (Costello, Lange, Naehrig, "Faster pairing
// computations on curves with high-degree twists", a = 0), cut into product phases and linear phases.  A line is left
// as a tower value scaled by a factor of a proper subfield, which the final exponentiation removes:
//   D twist: l = ly + lx w + lf w^3;  M twist: l = lf + lx w^2 + ly w^3   (ly carries yP, lx carries xP, lf is free)
// and kept as the three coefficients that are not zero, in the order of their powers of w.
// Doubling, R <- 2R.  With A = XY, B = Y^2, E = 3b' Z^2, F = 3E, H = 2YZ, J = X^2:
//   4 (X3, Y3, Z3) = (2A(B - F), (B + F)^2 - 12 E^2, 4BH),  ly = -H yP, lx = 3J xP, lf = E - B.
//   DBL1: T0 = XY, T1 = Y^2, T2 = Z^2, T3 = YZ, T4 = X^2;  DBL1B: T2 = 3b' T2 (E);
//   DBL_C1: T5 = 3E, T3 = 2 T3 (H), T6 = B - F, T7 = B + F, lf = E - B;
//   DBL2: X = T0 T6, T7 = T7^2, T2 = E^2, Z = T1 T3, T5 = H yP, T4 = J xP;
//   DBL_C2: X = 2X, Y = T7 - 12 T2, Z = 4Z, ly = -T5, lx = 3 T4.
// Addition, R <- R + Q' (Q' = (x2, y2) affine).  With th = Y - y2 Z, la = X - x2 Z, c = th^2, d = la^2, e = la d,
// f = Z c, g = X d, h = e + f - 2g:  (X3, Y3, Z3) = (la h, th (g - h) - e Y, Z e),  ly = la yP, lx = -th xP,
// lf = th x2 - la y2.
//   ADD1: T0 = y2 Z, T1 = x2 Z;  ADD_C1: T0 = Y - T0 (th), T1 = X - T1 (la);
//   ADD2: T2 = th^2, T3 = la^2, T4 = th x2, T5 = la y2;  ADD3: T6 = la T3 (e), T7 = Z T2 (f), T8 = X T3 (g);
//   ADD_C2: T2 = e + f - 2g (h), T3 = g - h, lf = T4 - T5;
//   ADD4: X = la h, T4 = th T3, T5 = e Y, Z = Z e, ly = la yP, T7 = th xP;  ADD_C3: Y = T4 - T5, lx = -T7.
// The inversion of N = n0 + n1 v + n2 v^2 in Fp6 = Fp2[v]/(v^3 - xi) (the coefficients 0, 2, 4 of a register):
//   INV1: n0^2, n1 n2, n2^2, n0 n1, n1^2, n0 n2;  INV_C1: A = n0^2 - xi n1 n2, B = xi n2^2 - n0 n1, C = n1^2 - n0 n2;
//   INV2: n0 A, n2 B, n1 C;  INV_C2: Fi = 1 / (n0 A + xi (n2 B + n1 C)), one inversion in Fp;
//   INV3: (n0, n1, n2) <- (A Fi, B Fi, C Fi).
template <class C>
struct PairingTables {
  static constexpr int LN_Y = C::TWIST_D ? PS_LN : PS_LN + 2, LN_X = PS_LN + 1, LN_F = C::TWIST_D ? PS_LN + 2 : PS_LN;
  static constexpr int T0 = PS_T0, T1 = PS_T0 + 1, T2 = PS_T0 + 2, T3 = PS_T0 + 3, T4 = PS_T0 + 4, T5 = PS_T0 + 5,
                       T6 = PS_T0 + 6, T7 = PS_T0 + 7, T8 = PS_T0 + 8;
  static constexpr int P = S_PROD;
  static constexpr JobTable TAB[TAB_COUNT] = {
      /* DBL1  */ {5, true, {{jp(T0), jp(PS_X), jp(PS_Y)}, {jp(T1), jp(PS_Y), jp(PS_Y)}, {jp(T2), jp(PS_Z), jp(PS_Z)},
                             {jp(T3), jp(PS_Y), jp(PS_Z)}, {jp(T4), jp(PS_X), jp(PS_X)}}},
      /* DBL1B */ {1, true, {{jp(T2), ja(S_B3), jp(T2)}}},
      /* DBL2  */ {6, true, {{jp(PS_X), jp(T0), jp(T6)}, {jp(T7), jp(T7), jp(T7)}, {jp(T2), jp(T2), jp(T2)},
                             {jp(PS_Z), jp(T1), jp(T3)}, {jp(T5), jp(T3), jp(PS_PY)}, {jp(T4), jp(T4), jp(PS_PX)}}},
      /* ADD1  */ {2, true, {{jp(T0), jp(PS_QB), jp(PS_Z)}, {jp(T1), jp(PS_QA), jp(PS_Z)}}},
      /* ADD2  */ {4, true, {{jp(T2), jp(T0), jp(T0)}, {jp(T3), jp(T1), jp(T1)}, {jp(T4), jp(T0), jp(PS_QA)},
                             {jp(T5), jp(T1), jp(PS_QB)}}},
      /* ADD3  */ {3, true, {{jp(T6), jp(T1), jp(T3)}, {jp(T7), jp(PS_Z), jp(T2)}, {jp(T8), jp(PS_X), jp(T3)}}},
      /* ADD4  */ {6, true, {{jp(PS_X), jp(T1), jp(T2)}, {jp(T4), jp(T0), jp(T3)}, {jp(T5), jp(T6), jp(PS_Y)},
                             {jp(PS_Z), jp(PS_Z), jp(T6)}, {jp(LN_Y), jp(T1), jp(PS_PY)}, {jp(T7), jp(T0), jp(PS_PX)}}},
      /* QP1   */ {2, true, {{jp(PS_QA), jp(PS_QA), ja(S_FROB + 2)}, {jp(PS_QB), jp(PS_QB), ja(S_FROB + 3)}}},
      /* QP2   */ {1, true, {{jp(PS_QA), jp(PS_QA), ja(S_FROB + 6 + 2)}}},
      /* INV1  */ {6, false, {{ja(P + 0), jr(0), jr(0)}, {ja(P + 1), jr(2), jr(4)}, {ja(P + 2), jr(4), jr(4)},
                              {ja(P + 3), jr(0), jr(2)}, {ja(P + 4), jr(2), jr(2)}, {ja(P + 5), jr(0), jr(4)}}},
      /* INV2  */ {3, false, {{ja(P + 9), jr(0), ja(P + 6)}, {ja(P + 10), jr(4), ja(P + 7)}, {ja(P + 11), jr(2), ja(P + 8)}}},
      /* INV3  */ {3, false, {{jr(0), ja(P + 6), ja(P + 12)}, {jr(2), ja(P + 7), ja(P + 12)}, {jr(4), ja(P + 8), ja(P + 12)}}},
  };
};

// The program of one equation after its points are in their slots: the Miller loop of all pairs into R_F (one squaring
// of the accumulator per loop bit however many pairs there are), then the final exponentiation of R_F in place.
struct PairingProgram {
  static constexpr int CAP = 4096;
  Ins ins[CAP];
  int n;

  constexpr void emit(int op, int r = 0, int a = 0, int b = 0) {
    ins[n].op = (uint8_t)op; ins[n].r = (uint8_t)r; ins[n].a = (uint8_t)a; ins[n].b = (uint8_t)b;
    ++n;
  }
  constexpr void mul(int r, int a, int b) { emit(OP_PROD12, 0, a, b); emit(OP_RED12, r); }
  constexpr void cyc_sqr(int r, int a) { emit(OP_PRODCYC, 0, a); emit(OP_CYCFIN, r, a); }
  constexpr void conj(int r, int a) { emit(OP_CONJ, r, a); }
  constexpr void frob(int r, int a, int j) {
    if (j & 1) { emit(OP_CONJ2, r, a); emit(OP_PRODFROB, r, r, j); }
    else emit(OP_PRODFROB, r, a, j);
  }
  // reg r = 1 / reg a with one inversion in Fp: N = a conj(a) lies in Fp6 (coefficients 0, 2, 4), is inverted there,
  // and r = conj(a) N^-1.  inv(0) = 0.  Uses R_T4, R_T5.
  constexpr void inv(int r, int a) {
    conj(R_T4, a);
    mul(R_T5, a, R_T4);
    emit(OP_PRODTAB, 0, TAB_INV1, R_T5); emit(OP_INV_C1);
    emit(OP_PRODTAB, 0, TAB_INV2, R_T5); emit(OP_INV_C2);
    emit(OP_PRODTAB, 0, TAB_INV3, R_T5);
    mul(r, R_T4, R_T5);
  }
  // reg r = (reg a)^e for a in the cyclotomic subgroup, e >= 1; r is not a
  constexpr void cyc_pow(int r, int a, uint64_t e) {
    int top = 63;
    while (top > 0 && !((e >> top) & 1u)) --top;
    emit(OP_COPY, r, a);
    for (int bit = top - 1; bit >= 0; --bit) {
      cyc_sqr(r, r);
      if ((e >> bit) & 1u) mul(r, r, a);
    }
  }
  // f <- f * (the line of every pair that is not skipped)
  constexpr void lines() {
    emit(OP_PAIRS_BEGIN, 0, 2);
    emit(OP_PRODLINE, 0, R_F);
    emit(OP_RED12, R_F, 0, 1);
    emit(OP_PAIRS_END, 0, 2);
  }
  constexpr void double_step() {
    emit(OP_PRODTAB, 0, TAB_DBL1); emit(OP_PRODTAB, 0, TAB_DBL1B); emit(OP_DBL_C1);
    emit(OP_PRODTAB, 0, TAB_DBL2); emit(OP_DBL_C2);
    lines();
  }
  // which = 0: Q' = Q; 1: Q' = pi(Q); 2: Q' = -pi^2(Q), the two extra additions of a BN curve, in twist coordinates
  // (conj(x) g12, conj(y) g13) and (x g22, y) with gjk = xi^(k (p^j - 1) / 6)
  constexpr void add_step(int which) {
    emit(OP_QPREP, 0, which);
    if (which == 1) emit(OP_PRODTAB, 0, TAB_QP1);
    if (which == 2) emit(OP_PRODTAB, 0, TAB_QP2);
    emit(OP_PRODTAB, 0, TAB_ADD1); emit(OP_ADD_C1);
    emit(OP_PRODTAB, 0, TAB_ADD2); emit(OP_PRODTAB, 0, TAB_ADD3); emit(OP_ADD_C2);
    emit(OP_PRODTAB, 0, TAB_ADD4); emit(OP_ADD_C3);
    lines();
  }
};

template <class C>
constexpr PairingProgram make_pairing_program() {
  PairingProgram p = {};
  constexpr int f = R_F, t0 = R_T0, t1 = R_T1, t2 = R_T2, t3 = R_T3, t4 = R_T4, t5 = R_T5;
  auto pow_u = [&](int r, int a) {              // reg r = (reg a)^u, u the curve's parameter (negative on BLS12-381)
    p.cyc_pow(r, a, C::U_ABS);
    if (C::U_NEG) p.conj(r, r);
  };
  // ---- Miller loop over |u| (BLS12-381) or 6u + 2 (BN254, with two more additions).  For u < 0 the textbook pairing
  // conjugates the result of the loop over |u|; kzg_snark_amd/pairing.py, the host statement every verdict of this
  // library has come from, does not, and the device computes ITS value: f_{|u|,Q}(P), the inverse of the textbook
  // value after the final exponentiation and a bilinear, non-degenerate pairing all the same.
  p.emit(OP_ONE, f);
  for (int bit = C::ATE_LOOP_BITS - 2; bit >= 0; --bit) {
    p.mul(f, f, f);
    p.double_step();
    if ((C::ATE_LOOP[bit >> 5] >> (bit & 31)) & 1u) p.add_step(0);
  }
  if (C::TWIST_D) { p.add_step(1); p.add_step(2); }
  // ---- final exponentiation, easy part: f^((p^6 - 1)(p^2 + 1))
  p.conj(t0, f);
  p.inv(t1, f);
  p.mul(f, t0, t1);
  p.frob(t0, f, 2);
  p.mul(f, t0, f);
  if (C::TWIST_D) {
    // BN254: f^(p^3) (f^(6u^2 + 1))^(p^2) (f^l1)^p f^l0
    pow_u(t0, f);                              // f^u
    pow_u(t1, t0);                             // f^(u^2)
    pow_u(t2, t1);                             // f^(u^3)
    p.cyc_pow(t3, t2, 36);                     // f^(36 u^3)
    p.cyc_pow(t2, t1, 6);                      // f^(6 u^2)
    p.cyc_sqr(t4, t2);                         // f^(12 u^2)
    p.mul(t5, t4, t2);                         // f^(18 u^2)
    p.mul(t4, t5, t4);                         // f^(30 u^2)
    p.mul(t2, t2, f);
    p.frob(t2, t2, 2);                         // (f^(6u^2 + 1))^(p^2)
    p.cyc_pow(t1, t0, 6);                      // f^(6u)
    p.cyc_sqr(t0, t1);                         // f^(12u)
    p.mul(t1, t0, t1);                         // f^(18u)
    p.mul(t5, t3, t5);
    p.mul(t5, t5, t0);                         // f^(36u^3 + 18u^2 + 12u)
    p.conj(t5, t5);
    p.mul(t5, t5, f);
    p.frob(t5, t5, 1);                         // (f^l1)^p
    p.mul(t4, t3, t4);
    p.mul(t4, t4, t1);                         // f^(36u^3 + 30u^2 + 18u)
    p.cyc_sqr(t0, f);
    p.mul(t4, t4, t0);
    p.conj(t4, t4);                            // f^l0
    p.frob(t0, f, 3);
    p.mul(f, t0, t2);
    p.mul(f, f, t5);
    p.mul(f, f, t4);
  } else {
    // BLS12-381: with a = f^(u-1), b = a^(u-1), c = b^(u+p), d = c^(u^2 + p^2 - 1): d f^3
    pow_u(t0, f);
    p.conj(t1, f);
    p.mul(t0, t0, t1);                         // a
    pow_u(t2, t0);
    p.conj(t0, t0);
    p.mul(t0, t2, t0);                         // b
    pow_u(t2, t0);
    p.frob(t0, t0, 1);
    p.mul(t0, t2, t0);                         // c
    pow_u(t2, t0);
    pow_u(t3, t2);                             // c^(u^2)
    p.frob(t2, t0, 2);
    p.mul(t3, t3, t2);
    p.conj(t2, t0);
    p.mul(t3, t3, t2);                         // d
    p.cyc_sqr(t2, f);
    p.mul(t2, t2, f);                          // f^3
    p.mul(f, t3, t2);
  }
  return p;
}
template <class C>
struct PairingProgramOf {
  static constexpr PairingProgram value = make_pairing_program<C>();
  static_assert(value.n < PairingProgram::CAP, "the program outgrew its table");
};

// the host exchange: one lane after the other
struct HostLanes {
  template <class Fn>
  void each(int n, Fn fn) {
    for (int t = 0; t < n; ++t) fn(t);
  }
  static uint32_t uniform(uint32_t v) { return v; }
};

template <class C>
struct Tower {
  using F = typename C::Fp;
  using Fd = Field<F>;
  using E = Fe<F>;
  using E2 = Fp2<C>;
  using Sh = PairingShared<C>;
  using Tab = PairingTables<C>;
  static constexpr int N = F::N;
  static constexpr int NW = F::NW;
  // the non-zero coefficients of a line: 1, w, w^3 on a D twist; 1, w^2, w^3 on an M twist
  static constexpr uint32_t LINE_MASK = C::TWIST_D ? 0x0bu : 0x0du;
  static constexpr uint32_t FULL_MASK = 0x3fu;

  // ---- Fp2 ---------------------------------------------------------------------------------------------
  static KZG_HD E fe_const(const uint32_t* w) {
    E r;
#pragma unroll
    for (int j = 0; j < N; ++j) r.l[j] = w[j];
    return r;
  }
  static KZG_HD E2 const2(const uint32_t (&w)[2][N]) { E2 r; r.c0 = fe_const(w[0]); r.c1 = fe_const(w[1]); return r; }
  static KZG_HD E2 zero2() { E2 r; r.c0 = Fd::zero(); r.c1 = Fd::zero(); return r; }
  static KZG_HD E2 one2() { E2 r; r.c0 = Fd::one(); r.c1 = Fd::zero(); return r; }
  static KZG_HD E2 add2(const E2& a, const E2& b) { E2 r; r.c0 = Fd::add(a.c0, b.c0); r.c1 = Fd::add(a.c1, b.c1); return r; }
  static KZG_HD E2 sub2(const E2& a, const E2& b) { E2 r; r.c0 = Fd::sub(a.c0, b.c0); r.c1 = Fd::sub(a.c1, b.c1); return r; }
  static KZG_HD E2 dbl2(const E2& a) { return add2(a, a); }
  static KZG_HD E2 neg2(const E2& a) { E2 r; r.c0 = Fd::neg(a.c0); r.c1 = Fd::neg(a.c1); return r; }
  static KZG_HD E2 neg_weak2(const E2& a) { E2 r; r.c0 = Fd::neg_weak(a.c0); r.c1 = Fd::neg_weak(a.c1); return r; }
  static KZG_HD E2 conj2(const E2& a) { E2 r; r.c0 = a.c0; r.c1 = Fd::neg(a.c1); return r; }
  static KZG_HD E2 select2(bool c, const E2& a, const E2& b) {
    E2 r; r.c0 = Fd::select(c, a.c0, b.c0); r.c1 = Fd::select(c, a.c1, b.c1); return r;
  }
  // (a0 b0 - a1 b1) + (a0 b1 + a1 b0) i: two mul2 (the bounds are in the header of this file)
  static KZG_HD E2 mul2(const E2& a, const E2& b) {
    E2 r;
    r.c0 = Fd::mul2(a.c0, b.c0, Fd::neg_weak(a.c1), b.c1);
    r.c1 = Fd::mul2(a.c0, b.c1, a.c1, b.c0);
    return r;
  }
  // (a0 + a1)(a0 - a1) + 2 a0 a1 i
  static KZG_HD E2 sqr2(const E2& a) {
    E2 r;
    r.c0 = Fd::mul(Fd::add(a.c0, a.c1), Fd::sub(a.c0, a.c1));
    r.c1 = Fd::mul(Fd::dbl(a.c0), a.c1);
    return r;
  }
  static KZG_HD E2 mul_fp(const E2& a, const E& s) { E2 r; r.c0 = Fd::mul(a.c0, s); r.c1 = Fd::mul(a.c1, s); return r; }
  // a + b with limbs carried and no reduction: normalised limbs in and out, the VALUE is the sum of the values.  The
  // lazy sums of this file end in reduce_wide (normalised limbs, value below 2^(L N) = 128p / 512p at the least).
  static KZG_HD E lz_add(const E& a, const E& b) { return Fd::carry(Fd::add_lazy(a, b)); }
  // a xi = (XI_RE a0 - a1) + (XI_RE a1 + a0) i for weak-normal a.  XI_RE = 9: lazily, 9 a0 + (2p - a1) and 9 a1 + a0
  // (neg_weak(a1) = 2p - a1 is normalised and at most 2p), values at most 20p, one reduce_wide each: canonical out.
  static KZG_HD E2 mul_xi(const E2& a) {
    static_assert(C::XI_RE == 1 || C::XI_RE == 9, "xi is 1 + i or 9 + i");
    E2 r;
    if (C::XI_RE == 9) {
      const E a0x2 = lz_add(a.c0, a.c0), a0x4 = lz_add(a0x2, a0x2), a0x8 = lz_add(a0x4, a0x4);
      const E a1x2 = lz_add(a.c1, a.c1), a1x4 = lz_add(a1x2, a1x2), a1x8 = lz_add(a1x4, a1x4);
      r.c0 = Fd::reduce_wide(lz_add(lz_add(a0x8, a.c0), Fd::neg_weak(a.c1)));
      r.c1 = Fd::reduce_wide(lz_add(lz_add(a1x8, a.c1), a.c0));
    } else {
      r.c0 = Fd::sub(a.c0, a.c1);
      r.c1 = Fd::add(a.c0, a.c1);
    }
    return r;
  }
  // conj(a) / (a0^2 + a1^2): one inversion in Fp; inv2(0) = 0
  static KZG_HD E2 inv2(const E2& a) {
    const E d = Fd::inv(Fd::add(Fd::sqr(a.c0), Fd::sqr(a.c1)));
    E2 r;
    r.c0 = Fd::mul(a.c0, d);
    r.c1 = Fd::mul(Fd::neg(a.c1), d);
    return r;
  }
  static KZG_HD bool is_zero2(const E2& a) { return Fd::is_zero(a.c0) && Fd::is_zero(a.c1); }
  static KZG_HD bool eq2(const E2& a, const E2& b) { return is_zero2(sub2(a, b)); }

  // ---- the interpreter ---------------------------------------------------------------------------------------------
  static KZG_HD int slot_of(uint16_t ref, int pair, int reg) {
    const int base = ref >> 12, idx = ref & 0xfff;
    return base == BASE_PAIR ? S_PAIR + pair * PS_COUNT + idx : base == BASE_ABS ? idx : 6 * reg + idx;
  }
  // the six coefficients r_t = sum_(i+j = t) + xi sum_(i+j = t+6) of the products prod[6i + j], j in mask.  Lane t adds
  // the products with i <= t, then those with i > t, into ONE lazy accumulator: acc <- carry(add_lazy(acc, s)) keeps
  // the limbs normalised (a normalised limb plus a limb of a weak-normal value is below 2^(L+1), no 32-bit wrap) and
  // lets the value grow to at most 6 * 2p = 12p, whose top limb is below 2^26 in both fields -- inside reduce_wide's
  // domain (normalised limbs, value below 2^(L N)), which brings each of the two sums to [0, p) once.
  static KZG_HD E2 reduce12(const E2* prod, int t, uint32_t mask) {
    E2 acc = zero2(), lo = zero2();
#pragma unroll 1
    for (int i = 0; i < 6; ++i) {
      if (i == t + 1) { lo = acc; acc = zero2(); }
      const int j = i > t ? t + 6 - i : t - i;
      if ((mask >> j) & 1u) {
        const E2 s = prod[i * 6 + j];
        acc.c0 = Fd::carry(Fd::add_lazy(acc.c0, s.c0));
        acc.c1 = Fd::carry(Fd::add_lazy(acc.c1, s.c1));
      }
    }
    E2 hi = acc;
    if (t == 5) { lo = acc; hi = zero2(); }
    lo.c0 = Fd::reduce_wide(lo.c0); lo.c1 = Fd::reduce_wide(lo.c1);
    hi.c0 = Fd::reduce_wide(hi.c0); hi.c1 = Fd::reduce_wide(hi.c1);
    return add2(lo, mul_xi(hi));
  }
  // a^2 for a in the cyclotomic subgroup (Granger-Scott): with the pairs (c0, c3), (c1, c4), (c2, c5) as elements
  // x + y s of Fp4 = Fp2[s]/(s^2 - xi), s = w^3, and T = (x^2 + xi y^2) + (2 x y) s the square of each pair (products
  // x^2, y^2, x y of pair q at prod[3q ..]):  c0' = 3 T0.e - 2 c0, c3' = 3 T0.o + 2 c3, c1' = 3 xi T2.o + 2 c1,
  // c4' = 3 T2.e - 2 c4, c2' = 3 T1.e - 2 c2, c5' = 3 T1.o + 2 c5.
  static KZG_HD E2 cyc_finish(const E2* prod, const E2& c, int t) {
    const int pair = t == 0 || t == 3 ? 0 : t == 2 || t == 5 ? 1 : 2;
    const int kind = t == 1 ? 2 : t >= 3 && t != 4 ? 1 : 0;                // 0: even part, 1: odd part, 2: xi * odd part
    const E2 ev = add2(prod[3 * pair], mul_xi(prod[3 * pair + 1]));
    const E2 od = dbl2(prod[3 * pair + 2]);
    const E2 T = select2(kind == 0, ev, select2(kind == 1, od, mul_xi(od)));
    // 3T + 2d with d = c or 2p - c (neg_weak), lazily: T and c are weak-normal, the sum is at most 10p
    const E2 d = select2(kind == 0, neg_weak2(c), c);
    E2 r;
    r.c0 = Fd::reduce_wide(lz_add(lz_add(lz_add(lz_add(T.c0, T.c0), T.c0), d.c0), d.c0));
    r.c1 = Fd::reduce_wide(lz_add(lz_add(lz_add(lz_add(T.c1, T.c1), T.c1), d.c1), d.c1));
    return r;
  }

  // Runs `n` instructions on the slots of sh for an equation of k pairs.  Wave-uniform throughout: the program counter,
  // the current pair and the skip flags are the same on every lane.
  template <class X>
  static KZG_HD void run(X& x, Sh* sh, const Ins* prog, int n, int k) {
    E2* v = sh->v;
    int pc = 0, pair = 0;
    while (pc < n) {
      const Ins in = prog[pc];
      const int op = in.op, rr = in.r, ra = in.a, rb = in.b;
      if (op == OP_PAIRS_BEGIN || op == OP_PAIRS_END) {
        int nxt = op == OP_PAIRS_BEGIN ? 0 : pair + 1;
        while (nxt < k && x.uniform(sh->skip[nxt])) ++nxt;
        if (nxt < k) { pair = nxt; pc = op == OP_PAIRS_BEGIN ? pc + 1 : pc - ra; }
        else pc = op == OP_PAIRS_BEGIN ? pc + ra + 2 : pc + 1;
        continue;
      }
      if (op <= OP_PROD_LAST) {
        const JobTable* tab = &Tab::TAB[op == OP_PRODTAB ? ra : 0];
        const int jobs = tab->jobs;
        const int lanes = op == OP_PROD12 || op == OP_PRODLINE ? 36 : op == OP_PRODCYC ? 9 : op == OP_PRODFROB ? 6 :
                          tab->per_pair ? k * jobs : jobs;
        const int cur = pair;
        x.each(lanes, [=](int t) {
          int d = 0, a = 0, b = 0;
          bool live = true;
          if (op == OP_PROD12 || op == OP_PRODLINE) {
            const int i = t / 6, j = t % 6;
            d = S_PROD + t;
            a = 6 * ra + i;
            if (op == OP_PROD12) {
              b = 6 * rb + j;
            } else {
              live = (LINE_MASK >> j) & 1u;
              b = S_PAIR + cur * PS_COUNT + PS_LN + (j == 0 ? 0 : j == 3 ? 2 : 1);
            }
          } else if (op == OP_PRODCYC) {
            const int q = t / 3, s = t % 3;
            d = S_PROD + t;
            a = 6 * ra + (s == 1 ? q + 3 : q);
            b = 6 * ra + (s == 0 ? q : q + 3);
          } else if (op == OP_PRODFROB) {
            d = 6 * rr + t;
            a = 6 * ra + t;
            b = S_FROB + 6 * (rb - 1) + t;
          } else {
            const int p = tab->per_pair ? t / jobs : 0;
            const Job job = tab->job[tab->per_pair ? t % jobs : t];
            live = !(tab->per_pair && sh->skip[p]);
            d = slot_of(job.dst, p, rb);
            a = slot_of(job.a, p, rb);
            b = slot_of(job.b, p, rb);
          }
          if (live) v[d] = mul2(v[a], v[b]);          // THE multiplication of the pairing
        });
        ++pc;
        continue;
      }
      switch (op) {
        case OP_RED12:
          x.each(6, [=](int t) { v[6 * rr + t] = reduce12(v + S_PROD, t, rb ? LINE_MASK : FULL_MASK); });
          break;
        case OP_CYCFIN:
          x.each(6, [=](int t) { v[6 * rr + t] = cyc_finish(v + S_PROD, v[6 * ra + t], t); });
          break;
        case OP_CONJ:
          x.each(6, [=](int t) { v[6 * rr + t] = select2((t & 1) != 0, neg2(v[6 * ra + t]), v[6 * ra + t]); });
          break;
        case OP_CONJ2:
          x.each(6, [=](int t) { v[6 * rr + t] = conj2(v[6 * ra + t]); });
          break;
        case OP_COPY:
          x.each(6, [=](int t) { v[6 * rr + t] = v[6 * ra + t]; });
          break;
        case OP_ONE:
          x.each(6, [=](int t) { v[6 * rr + t] = select2(t == 0, one2(), zero2()); });
          break;
        case OP_DBL_C1:
          x.each(k, [=](int t) {
            if (sh->skip[t]) return;
            E2* s = v + S_PAIR + t * PS_COUNT;
            const E2 Ee = s[Tab::T2], B = s[Tab::T1], Ff = add2(dbl2(Ee), Ee);
            s[Tab::T5] = Ff;
            s[Tab::T3] = dbl2(s[Tab::T3]);
            s[Tab::T6] = sub2(B, Ff);
            s[Tab::T7] = add2(B, Ff);
            s[Tab::LN_F] = sub2(Ee, B);
          });
          break;
        case OP_DBL_C2:
          x.each(k, [=](int t) {
            if (sh->skip[t]) return;
            E2* s = v + S_PAIR + t * PS_COUNT;
            const E2 e2 = s[Tab::T2], e6 = dbl2(add2(dbl2(e2), e2));
            s[PS_X] = dbl2(s[PS_X]);
            s[PS_Y] = sub2(s[Tab::T7], dbl2(e6));
            s[PS_Z] = dbl2(dbl2(s[PS_Z]));
            s[Tab::LN_Y] = neg2(s[Tab::T5]);
            s[Tab::LN_X] = add2(dbl2(s[Tab::T4]), s[Tab::T4]);
          });
          break;
        case OP_ADD_C1:
          x.each(k, [=](int t) {
            if (sh->skip[t]) return;
            E2* s = v + S_PAIR + t * PS_COUNT;
            s[Tab::T0] = sub2(s[PS_Y], s[Tab::T0]);
            s[Tab::T1] = sub2(s[PS_X], s[Tab::T1]);
          });
          break;
        case OP_ADD_C2:
          x.each(k, [=](int t) {
            if (sh->skip[t]) return;
            E2* s = v + S_PAIR + t * PS_COUNT;
            const E2 g = s[Tab::T8], h = sub2(add2(s[Tab::T6], s[Tab::T7]), dbl2(g));
            s[Tab::T2] = h;
            s[Tab::T3] = sub2(g, h);
            s[Tab::LN_F] = sub2(s[Tab::T4], s[Tab::T5]);
          });
          break;
        case OP_ADD_C3:
          x.each(k, [=](int t) {
            if (sh->skip[t]) return;
            E2* s = v + S_PAIR + t * PS_COUNT;
            s[PS_Y] = sub2(s[Tab::T4], s[Tab::T5]);
            s[Tab::LN_X] = neg2(s[Tab::T7]);
          });
          break;
        case OP_QPREP:
          x.each(k, [=](int t) {
            if (sh->skip[t]) return;
            E2* s = v + S_PAIR + t * PS_COUNT;
            s[PS_QA] = select2(ra == 1, conj2(s[PS_QX]), s[PS_QX]);
            s[PS_QB] = select2(ra == 1, conj2(s[PS_QY]), s[PS_QY]);
          });
          break;
        case OP_INV_C1:
          x.each(3, [=](int t) {
            const E2* q = v + S_PROD;
            v[S_PROD + 6 + t] = t == 0 ? sub2(q[0], mul_xi(q[1])) : t == 1 ? sub2(mul_xi(q[2]), q[3]) : sub2(q[4], q[5]);
          });
          break;
        case OP_INV_C2:
          x.each(1, [=](int) {
            const E2* q = v + S_PROD;
            v[S_PROD + 12] = inv2(add2(q[9], mul_xi(add2(q[10], q[11]))));
          });
          break;
        default:
          break;
      }
      ++pc;
    }
  }

  // ---- points in --------------------------------------------------------------------------------------------------
  // THE rule "canonical words -> a point of the twist": the four coordinates words (x.c0, x.c1, y.c0, y.c1) below p
  // and y^2 = x^3 + b'
  static KZG_HD bool import_g2(const uint32_t* w, E2& qx, E2& qy) {
    const bool below = words_below_p<F>(w) && words_below_p<F>(w + NW) && words_below_p<F>(w + 2 * NW) &&
                       words_below_p<F>(w + 3 * NW);
    qx.c0 = Fd::reduce(Fd::to_mont(Fd::from_words(w)));
    qx.c1 = Fd::reduce(Fd::to_mont(Fd::from_words(w + NW)));
    qy.c0 = Fd::reduce(Fd::to_mont(Fd::from_words(w + 2 * NW)));
    qy.c1 = Fd::reduce(Fd::to_mont(Fd::from_words(w + 3 * NW)));
    return below && eq2(sqr2(qy), add2(mul2(sqr2(qx), qx), const2(C::TWIST_B)));
  }

  // the constants a program reads from slots
  template <class X>
  static KZG_HD void load_constants(X& x, Sh* sh) {
    E2* v = sh->v;
    x.each(19, [=](int t) { v[S_FROB + t] = t < 18 ? const2(C::FROB[t / 6][t % 6]) : const2(C::TWIST_B3); });
  }

  // One equation: status 0 (the product of the k pairings is 1), 1 (it is not) or 2 (a finite point with a coordinate
  // >= p, off its curve or off its twist), the same value on every lane.  g1: k points x | y of NW words, g2: k points
  // of 4 NW words, flags may be null.  out_gt (may be null): the product to the power GT_MULTIPLE, 12 NW canonical
  // words, zeros for status 2.  Work is fixed but for three wave-uniform decisions: a pair with an infinity flag is
  // skipped, a malformed point ends the equation, and an equation with every pair skipped has the product 1.
  template <class X>
  static KZG_HD int equation(X& x, Sh* sh, const uint32_t* g1, const uint8_t* g1_inf, const uint32_t* g2,
                             const uint8_t* g2_inf, int k, uint32_t* out_gt) {
    E2* v = sh->v;
    load_constants(x, sh);
    x.each(k, [=](int t) {
      const bool inf1 = g1_inf && g1_inf[t], inf2 = g2_inf && g2_inf[t];
      E2* s = v + S_PAIR + t * PS_COUNT;
      bool ok = true;
      if (!inf1) {
        E px, py;
        ok = import_affine<C>(g1 + t * 2 * NW, g1 + t * 2 * NW + NW, px, py);
        s[PS_PX].c0 = px; s[PS_PX].c1 = Fd::zero();
        s[PS_PY].c0 = py; s[PS_PY].c1 = Fd::zero();
      }
      if (!inf2) {
        E2 qx, qy;
        ok = import_g2(g2 + t * 4 * NW, qx, qy) && ok;
        s[PS_QX] = qx; s[PS_QY] = qy;
        s[PS_X] = qx; s[PS_Y] = qy; s[PS_Z] = one2();
      }
      sh->skip[t] = inf1 || inf2 ? 1u : 0u;
      sh->flag[t] = ok ? 0u : 1u;
    });
    uint32_t bad = 0, live = 0;
    for (int p = 0; p < k; ++p) { bad |= sh->flag[p]; live |= sh->skip[p] ^ 1u; }
    bad = x.uniform(bad);
    live = x.uniform(live);
    if (bad) {
      if (out_gt) x.each(6, [=](int t) { for (int j = 0; j < 2 * NW; ++j) out_gt[t * 2 * NW + j] = 0; });
      return 2;
    }
    if (live) {
      run(x, sh, PairingProgramOf<C>::value.ins, PairingProgramOf<C>::value.n, k);
    } else {
      x.each(6, [=](int t) { v[6 * R_F + t] = select2(t == 0, one2(), zero2()); });
    }
    x.each(6, [=](int t) {
      const E2 c = v[6 * R_F + t];
      sh->flag[t] = eq2(c, select2(t == 0, one2(), zero2())) ? 0u : 1u;
      if (out_gt) {
        Fd::to_words(Fd::from_mont(c.c0), out_gt + t * 2 * NW);
        Fd::to_words(Fd::from_mont(c.c1), out_gt + t * 2 * NW + NW);
      }
    });
    uint32_t differs = 0;
    for (int t = 0; t < 6; ++t) differs |= sh->flag[t];
    return x.uniform(differs) ? 1 : 0;
  }
};

}  // namespace kzg
