// lagrange.hip -- evaluation-form KZG on gfx950: commitment keys in the Lagrange basis of a domain
// H = {w^i, i < n}, n = 2^log_n, and openings computed from values f[i] = p(w^i) (natural order).
//
//   key from tau      L_i(tau) = (tau^n - 1)/n * w^i / (tau - w^i)   (e_m when tau = w^m), then the fixed-base
//                     table of srs_generate_kernel (msm.hip) with the scalar taken from that vector
//   key from a key    L_i = n^-1 sum_j w^(-ij) P_j over the first n window-0 records of a monomial key: an inverse
//                     NTT over G1 in XYZZ, radix 2, decimation in time: a bit-reversed load (g1_intt_load_kernel),
//                     the levels of domain.hip's transform (launch_levels: one vector, root w^-1, natural output),
//                     and n^-1 applied once, in the pass that writes the affine records (g1_intt_finish_kernel).
//   open from values  P = sum_j xi^(j+1) f_j (kzg.py:148-150, fr_vec_lincomb), d_i = z - w^i inverted as a batch
//                     (fr_vec_inverse, 0 -> 0), then ONE reduction pass for three sums over i with d_i != 0
//                       S = sum P_i w^i / d_i     T = sum w^i / d_i     E = P_m (the i with d_i = 0, if any)
//                     y = (z^n - 1)/n * S + E (barycentric; the first term vanishes for z in H), and the quotient on
//                     H: q_i = (P_i - y)/(w^i - z); for z = w^m, q_m = sum_(i != m) (P_i - y) w^i / (z (z - w^i))
//                     = (S - y T)/z (EIP-4844 compute_quotient_eval_within_domain).  The proof is the commit of q
//                     against the Lagrange key, y riding in the pipeline's slot like kzg_open_device_async's S_0.
// The Fr kernels run beside a commit's accumulate kernel in the pipelined form: <= 128 VGPRs, tiny LDS, no scratch.
#include <cstring>
#include <algorithm>
#include <vector>
#include "internal.h"
#include "fr_util.h"
#include "g1_util.h"
#include "msm.h"
#include "srs_rec.h"

namespace kzg {

namespace {

constexpr int LG_FRN = 9;         // both scalar fields: 9 x 29-bit limbs
struct LgWords {                  // one Fr element as canonical words (a scalar multiplier)
  uint32_t w[8];
};
constexpr uint32_t SUM_TB = 128;  // threads per workgroup of the reduction pass
// its workgroups at most: every thread is a serial chain of products, so the pass wants many waves (256 workgroups,
// 32 elements per thread at 2^20: 115 us; 2048: 4 per thread)
constexpr uint32_t SUM_MAXG = 2048;

// ---- Fr passes ------------------------------------------------------------------------------------

// out[i] = w^i (canonical words); w in Montgomery form
template <class F>
__global__ __launch_bounds__(256) void lagr_wpow_kernel(uint32_t n, FrArg w, uint32_t* out) {
  using Fd = Field<F>;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fe<F> b = arg_fe<F>(w), acc = Fd::one();
  for (uint32_t bits = i; bits; bits >>= 1) {
    if (bits & 1u) acc = Fd::mul(acc, b);
    b = Fd::sqr(b);
  }
  store_words<F>(out + (size_t)i * 8, Fd::from_mont(acc));
}

// tab <- the two-level power table of `base` (fr_util.h: POW_TAB entries, Montgomery words); base_hi = base^POW_TLO
template <class F>
__global__ __launch_bounds__(256) void fr_pow_table_kernel(FrArg base, FrArg base_hi, uint32_t* tab) {
  using Fd = Field<F>;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= POW_TAB) return;
  Fe<F> b = arg_fe<F>(i < POW_TLO ? base : base_hi), acc = Fd::one();
  for (uint32_t bits = i < POW_TLO ? i : i - POW_TLO; bits; bits >>= 1) {
    if (bits & 1u) acc = Fd::mul(acc, b);
    b = Fd::sqr(b);
  }
  store_words<F>(tab + (size_t)i * 8, acc);
}

template <class F>
int pow_table_t(Ctx* c, const FrArg& base, uint32_t* d_tab) {
  Fe<F> hi;
  memcpy(hi.l, base.l, sizeof(hi.l));
  for (uint32_t q = 0; q < POW_TLOG; ++q) hi = Field<F>::sqr(hi);
  hipLaunchKernelGGL(fr_pow_table_kernel<F>, dim3((POW_TAB + 255) / 256), dim3(256), 0, c->stream, base, fr_arg<F>(hi),
                     d_tab);
  KZG_HIP(c, hipGetLastError());
  return KZG_OK;
}

// d[i] = z - w^i (z in standard form: the difference of two standard values is one)
template <class F>
__global__ __launch_bounds__(256) void lagr_denom_kernel(uint32_t n, const uint32_t* wpow, FrArg z, uint32_t* d) {
  using Fd = Field<F>;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  store_words<F>(d + (size_t)i * 8, Fd::sub(arg_fe<F>(z), load_words<F>(wpow + (size_t)i * 8)));
}

// L_i(tau) from the inverted denominators: inv_i = 0 marks tau = w^i (scalar 1; cz = 0 then zeroes the others)
template <class F>
__global__ __launch_bounds__(256) void lagr_basis_scalars_kernel(uint32_t n, const uint32_t* wpow,
                                                                 const uint32_t* inv, FrArg cz, uint32_t* out) {
  using Fd = Field<F>;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fe<F> iv = load_words<F>(inv + (size_t)i * 8);
  Fe<F> r;
  if (Fd::is_zero(iv)) r = Fd::raw_one();
  else r = Fd::mul(Fd::mul(arg_fe<F>(cz), Fd::to_mont(load_words<F>(wpow + (size_t)i * 8))), iv);   // standard form
  store_words<F>(out + (size_t)i * 8, r);
}

// Per workgroup: S = sum P_i w^i inv_i, T = sum w^i inv_i over inv_i != 0, E = sum P_i over inv_i = 0 (P_i = 0 for
// i >= plen).  Montgomery limbs, [3][9] words per workgroup.
template <class F>
__global__ __launch_bounds__(SUM_TB) void lagr_sums_kernel(uint32_t n, uint32_t plen, const uint32_t* P,
                                                           const uint32_t* wpow, const uint32_t* inv, uint32_t* part) {
  using Fd = Field<F>;
  __shared__ uint32_t red[SUM_TB / 64][3 * LG_FRN];
  Fe<F> S = Fd::zero(), T = Fd::zero(), E = Fd::zero();
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const Fe<F> iv = load_words<F>(inv + (size_t)i * 8);
    const Fe<F> p = i < plen ? Fd::to_mont(load_words<F>(P + (size_t)i * 8)) : Fd::zero();
    if (Fd::is_zero(iv)) {
      E = Fd::add(E, p);
    } else {
      const Fe<F> u = Fd::mul(Fd::to_mont(load_words<F>(wpow + (size_t)i * 8)), Fd::to_mont(iv));
      T = Fd::add(T, u);
      S = Fd::add(S, Fd::mul(p, u));
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    S = Fd::add(S, shfl_xor_fe<F>(S, m));
    T = Fd::add(T, shfl_xor_fe<F>(T, m));
    E = Fd::add(E, shfl_xor_fe<F>(E, m));
  }
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0) {
    store_limbs<F>(&red[wave][0], S);
    store_limbs<F>(&red[wave][LG_FRN], T);
    store_limbs<F>(&red[wave][2 * LG_FRN], E);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t q = 1; q < SUM_TB / 64; ++q) {
      S = Fd::add(S, load_limbs<F>(&red[q][0]));
      T = Fd::add(T, load_limbs<F>(&red[q][LG_FRN]));
      E = Fd::add(E, load_limbs<F>(&red[q][2 * LG_FRN]));
    }
    uint32_t* o = part + (size_t)blockIdx.x * 3 * LG_FRN;
    store_limbs<F>(o, S);
    store_limbs<F>(o + LG_FRN, T);
    store_limbs<F>(o + 2 * LG_FRN, E);
  }
}

// One wave: y = cz S + E, q_m = zinv (S - y T).  out: y as canonical words [8], y (Montgomery) [9], q_m [9]
template <class F>
__global__ __launch_bounds__(64) void lagr_value_kernel(uint32_t groups, const uint32_t* part, FrArg cz, FrArg zinv,
                                                        uint32_t* out) {
  using Fd = Field<F>;
  Fe<F> S = Fd::zero(), T = Fd::zero(), E = Fd::zero();
  for (uint32_t g = threadIdx.x; g < groups; g += 64) {
    const uint32_t* q = part + (size_t)g * 3 * LG_FRN;
    S = Fd::add(S, load_limbs<F>(q));
    T = Fd::add(T, load_limbs<F>(q + LG_FRN));
    E = Fd::add(E, load_limbs<F>(q + 2 * LG_FRN));
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    S = Fd::add(S, shfl_xor_fe<F>(S, m));
    T = Fd::add(T, shfl_xor_fe<F>(T, m));
    E = Fd::add(E, shfl_xor_fe<F>(E, m));
  }
  if (threadIdx.x != 0) return;
  const Fe<F> y = Fd::reduce(Fd::add(Fd::mul(arg_fe<F>(cz), S), E));
  const Fe<F> qm = Fd::reduce(Fd::mul(arg_fe<F>(zinv), Fd::sub(S, Fd::mul(y, T))));
  store_words<F>(out, Fd::from_mont(y));
  store_limbs<F>(out + 8, y);
  store_limbs<F>(out + 8 + LG_FRN, qm);
}

// q_i = (y - P_i) inv_i = (P_i - y)/(w^i - z); q_m (inv_m = 0, z = w^m) from lagr_value_kernel
template <class F>
__global__ __launch_bounds__(256) void lagr_quotient_kernel(uint32_t n, const uint32_t* P, const uint32_t* inv,
                                                            const uint32_t* val, uint32_t* q) {
  using Fd = Field<F>;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fe<F> iv = load_words<F>(inv + (size_t)i * 8);
  Fe<F> r;
  if (Fd::is_zero(iv)) {
    r = Fd::from_mont(load_limbs<F>(val + 8 + LG_FRN));
  } else {
    const Fe<F> d = Fd::sub(load_limbs<F>(val + 8), Fd::to_mont(load_words<F>(P + (size_t)i * 8)));   // Montgomery
    r = Fd::mul(d, iv);                                                                           // standard
  }
  store_words<F>(q + (size_t)i * 8, r);
}

// ---- batched evaluation: b vectors over one domain, vector j at its own point ------------------------------------

constexpr uint32_t BATCH_MAXG = 32;   // workgroups per vector of the batched reduction pass

// d[j n + i] = z_j - w^i over the whole block of cb vectors (z_j canonical words, standard form)
template <class F>
__global__ __launch_bounds__(256) void lagr_batch_denom_kernel(uint32_t log_n, size_t total, const uint32_t* wpow,
                                                               const uint32_t* z, uint32_t* d) {
  using Fd = Field<F>;
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const size_t j = e >> log_n, i = e & (((size_t)1 << log_n) - 1);
  store_words<F>(d + e * 8, Fd::sub(load_words<F>(z + j * 8), load_words<F>(wpow + i * 8)));
}

// lagr_sums_kernel with the vector index in the grid (blockIdx.y), without T (only the quotient needs it):
// part[j][g] = [S | E] of workgroup g over vector j, Montgomery limbs
template <class F>
__global__ __launch_bounds__(SUM_TB) void lagr_batch_sums_kernel(uint32_t n, size_t stride, const uint32_t* lens,
                                                                 const uint32_t* vals, const uint32_t* wpow,
                                                                 const uint32_t* inv, uint32_t* part) {
  using Fd = Field<F>;
  __shared__ uint32_t red[SUM_TB / 64][2 * LG_FRN];
  const uint32_t j = blockIdx.y, plen = lens[j];
  const uint32_t* P = vals + (size_t)j * stride * 8;
  const uint32_t* iv_j = inv + (size_t)j * n * 8;
  Fe<F> S = Fd::zero(), E = Fd::zero();
  const uint32_t step = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < plen; i += step) {    // P_i = 0 from plen on
    const Fe<F> iv = load_words<F>(iv_j + (size_t)i * 8);
    const Fe<F> p = Fd::to_mont(load_words<F>(P + (size_t)i * 8));
    if (Fd::is_zero(iv)) {
      E = Fd::add(E, p);
    } else {
      const Fe<F> u = Fd::mul(Fd::to_mont(load_words<F>(wpow + (size_t)i * 8)), Fd::to_mont(iv));
      S = Fd::add(S, Fd::mul(p, u));
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    S = Fd::add(S, shfl_xor_fe<F>(S, m));
    E = Fd::add(E, shfl_xor_fe<F>(E, m));
  }
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0) {
    store_limbs<F>(&red[wave][0], S);
    store_limbs<F>(&red[wave][LG_FRN], E);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t q = 1; q < SUM_TB / 64; ++q) {
      S = Fd::add(S, load_limbs<F>(&red[q][0]));
      E = Fd::add(E, load_limbs<F>(&red[q][LG_FRN]));
    }
    uint32_t* o = part + ((size_t)j * gridDim.x + blockIdx.x) * 2 * LG_FRN;
    store_limbs<F>(o, S);
    store_limbs<F>(o + LG_FRN, E);
  }
}

// One wave per vector: out[j] = (z_j^n - 1)/n * S + E, canonical words; ninv = n^-1 (Montgomery)
template <class F>
__global__ __launch_bounds__(64) void lagr_batch_value_kernel(uint32_t log_n, uint32_t groups, const uint32_t* part,
                                                              const uint32_t* z, FrArg ninv, uint32_t* out) {
  using Fd = Field<F>;
  const uint32_t j = blockIdx.x;
  Fe<F> S = Fd::zero(), E = Fd::zero();
  for (uint32_t g = threadIdx.x; g < groups; g += 64) {
    const uint32_t* q = part + ((size_t)j * groups + g) * 2 * LG_FRN;
    S = Fd::add(S, load_limbs<F>(q));
    E = Fd::add(E, load_limbs<F>(q + LG_FRN));
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    S = Fd::add(S, shfl_xor_fe<F>(S, m));
    E = Fd::add(E, shfl_xor_fe<F>(E, m));
  }
  if (threadIdx.x != 0) return;
  Fe<F> zn = Fd::to_mont(load_words<F>(z + (size_t)j * 8));
  for (uint32_t q = 0; q < log_n; ++q) zn = Fd::sqr(zn);
  const Fe<F> cz = Fd::mul(Fd::sub(zn, Fd::one()), arg_fe<F>(ninv));
  store_words<F>(out + (size_t)j * 8, Fd::from_mont(Fd::reduce(Fd::add(Fd::mul(cz, S), E))));
}

// ---- G1 inverse NTT -------------------------------------------------------------------------------

// buf[bitrev(i)] = record i of window 0
template <class C>
__global__ __launch_bounds__(128) void g1_intt_load_kernel(const uint32_t* recs, uint32_t n, uint32_t log_n,
                                                           uint32_t* buf) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Affine<C> a;
  a.inf = load_rec<C>(recs, i, a.x, a.y) & 1u;
  st_point<C>(buf, __brev(i) >> (32 - log_n), Ec<C>::from_affine(a));
}

// record i = n^-1 * buf[i], affine canonical (window 0 of the Lagrange key)
template <class C>
__global__ __launch_bounds__(64) void g1_intt_finish_kernel(const uint32_t* buf, uint32_t n, LgWords ninv,
                                                            uint32_t* recs) {
  using Fd = Field<typename C::Fp>;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const XYZZ<C> p = g1_mul_words<C>(ld_point<C>(buf, i), ninv.w);
  const Affine<C> a = Ec<C>::to_affine(p);
  store_rec<C>(recs, i, Fd::reduce(a.x), Fd::reduce(a.y), a.inf);
}

// ---- host side --------------------------------------------------------------------------------------

// (z^n - 1)/n (Montgomery) and whether z^n = 1 (z in H)
template <class F>
Fe<F> vanishing_over_n(const Fe<F>& z_mont, uint32_t log_n, bool* in_domain) {
  using Fd = Field<F>;
  Fe<F> zn = z_mont;
  for (uint32_t q = 0; q < log_n; ++q) zn = Fd::sqr(zn);
  const Fe<F> num = Fd::sub(zn, Fd::one());
  *in_domain = Fd::is_zero(num);
  return Fd::reduce(Fd::mul(num, inv_pow2<F>(log_n)));
}

constexpr int LG_MAX_LOG = 24;

template <class F>
int launch_wpow(Ctx* c, uint32_t n, const uint32_t* w_words, uint32_t* out) {
  const Fe<F> w = mont_from_words<F>(w_words);
  hipLaunchKernelGGL(lagr_wpow_kernel<F>, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, fr_arg<F>(w), out);
  KZG_HIP(c, hipGetLastError());
  return KZG_OK;
}

// The value pass shared by the opening and the evaluation: from P (plen values, zero above), the table w^i and z,
// leaves d_val = [y words (8) | y Montgomery (9) | q_m (9)] and, when d_q != null, the quotient q over H.
// d_den, d_inv: n elements of scratch each (d_q may alias d_den).
template <class F>
int value_pass(Ctx* c, uint32_t log_n, uint32_t plen, const uint32_t* d_P, const uint32_t* d_wpow,
               const uint32_t* z_words, uint32_t* d_den, uint32_t* d_inv, uint32_t* d_part, uint32_t* d_val,
               uint32_t* d_q) {
  using Fd = Field<F>;
  const uint32_t n = 1u << log_n;
  const Fe<F> zs = Fd::from_words(z_words);
  const Fe<F> zm = Fd::to_mont(zs);
  bool in_domain = false;
  const Fe<F> cz = vanishing_over_n<F>(zm, log_n, &in_domain);
  const Fe<F> zinv = in_domain ? Fd::reduce(Fd::inv(zm)) : Fd::zero();
  const uint32_t grid = (n + 255) / 256;
  hipLaunchKernelGGL(lagr_denom_kernel<F>, dim3(grid), dim3(256), 0, c->stream, n, d_wpow, fr_arg<F>(zs), d_den);
  KZG_HIP(c, hipGetLastError());
  int rc = fr_vec_inverse(c, n, d_den, d_inv);
  if (rc) return rc;
  const uint32_t groups = std::min<uint32_t>(SUM_MAXG, (n + SUM_TB - 1) / SUM_TB);
  hipLaunchKernelGGL(lagr_sums_kernel<F>, dim3(groups), dim3(SUM_TB), 0, c->stream, n, plen, d_P, d_wpow, d_inv,
                     d_part);
  hipLaunchKernelGGL(lagr_value_kernel<F>, dim3(1), dim3(64), 0, c->stream, groups, d_part, fr_arg<F>(cz),
                     fr_arg<F>(zinv), d_val);
  KZG_HIP(c, hipGetLastError());
  if (d_q) {
    hipLaunchKernelGGL(lagr_quotient_kernel<F>, dim3(grid), dim3(256), 0, c->stream, n, d_P, d_inv, d_val, d_q);
    KZG_HIP(c, hipGetLastError());
  }
  return KZG_OK;
}

template <class C>
int srs_generate_lagrange_t(Ctx* c, const uint32_t* tau_words, uint32_t log_n, const uint32_t* w_words, Srs** out) {
  using F = typename C::Fr;
  using Fd = Field<F>;
  if (log_n < 1 || log_n > LG_MAX_LOG) return set_err(c, KZG_ERR_ARG, "Lagrange key: log_n must be in [1, 24]");
  if (!primitive_root<F>(mont_from_words<F>(w_words), log_n))
    return set_err(c, KZG_ERR_ARG, "Lagrange key: w is not a primitive root");
  const uint32_t n = 1u << log_n;
  ProfScope ps(c, "srs_lagrange");
  DevTmp<uint32_t> d_wpow, d_tmp;
  if (d_wpow.alloc((size_t)n * 32) != hipSuccess || d_tmp.alloc((size_t)n * 3 * 32) != hipSuccess)
    return set_err(c, KZG_ERR_ALLOC, "hipMalloc(Lagrange key)");
  uint32_t *d_den = d_tmp, *d_inv = d_tmp + (size_t)n * 8, *d_sc = d_tmp + (size_t)n * 16;
  int rc = launch_wpow<F>(c, n, w_words, d_wpow);
  if (rc) return rc;
  const Fe<F> ts = Fd::from_words(tau_words);
  bool in_domain = false;
  const Fe<F> cz = vanishing_over_n<F>(Fd::to_mont(ts), log_n, &in_domain);
  const uint32_t grid = (n + 255) / 256;
  hipLaunchKernelGGL(lagr_denom_kernel<F>, dim3(grid), dim3(256), 0, c->stream, n, d_wpow.get(), fr_arg<F>(ts), d_den);
  if ((rc = fr_vec_inverse(c, n, d_den, d_inv))) return rc;
  hipLaunchKernelGGL(lagr_basis_scalars_kernel<F>, dim3(grid), dim3(256), 0, c->stream, n, d_wpow.get(), d_inv,
                     fr_arg<F>(cz), d_sc);
  KZG_HIP(c, hipGetLastError());
  Srs* s = nullptr;
  if ((rc = srs_generate_scalars(c, d_sc, n, &s))) return rc;   // synchronises
  s->basis = SRS_LAGRANGE;
  s->log_n = log_n;
  memcpy(s->w, w_words, 32);
  s->d_wpow = d_wpow.release();
  *out = s;
  return KZG_OK;
}

template <class C>
int srs_lagrange_t(Ctx* c, const Srs* mono, uint32_t log_n, const uint32_t* w_words, Srs** out) {
  using F = typename C::Fr;
  using Fd = Field<F>;
  if (mono->curve != c->curve) return set_err(c, KZG_ERR_ARG, "SRS belongs to another curve");
  if (mono->basis != SRS_MONOMIAL) return set_err(c, KZG_ERR_ARG, "kzg_srs_lagrange: the source key must be monomial");
  if (log_n < 1 || log_n > LG_MAX_LOG) return set_err(c, KZG_ERR_ARG, "Lagrange key: log_n must be in [1, 24]");
  const uint32_t n = 1u << log_n;
  if (mono->n < n) return set_err(c, KZG_ERR_ARG, "kzg_srs_lagrange: monomial key shorter than the domain");
  if (!primitive_root<F>(mont_from_words<F>(w_words), log_n))
    return set_err(c, KZG_ERR_ARG, "Lagrange key: w is not a primitive root");
  SrsPtr s;
  int rc = srs_create(c, n, &s);
  if (rc) return rc;
  {
    DevTmp<uint32_t> d_buf;
    if (hipMalloc(reinterpret_cast<void**>(&s->d_wpow), (size_t)n * 32) != hipSuccess ||
        d_buf.alloc((size_t)n * 4 * C::Fp::N * 4) != hipSuccess)
      return set_err(c, KZG_ERR_ALLOC, "hipMalloc(Lagrange key)");
    {
      ProfScope ps(c, "srs_lagrange");
      if ((rc = launch_wpow<F>(c, n, w_words, s->d_wpow))) return rc;
      const Fe<F> winv = Fd::inv(mont_from_words<F>(w_words));
      LgWords ninv;
      words_from_mont<F>(inv_pow2<F>(log_n), ninv.w);
      hipLaunchKernelGGL(g1_intt_load_kernel<C>, dim3((n + 127) / 128), dim3(128), 0, c->stream, mono->recs, n, log_n,
                         d_buf.get());
      if ((rc = launch_levels(c, d_buf, 1, log_n, fr_arg<F>(winv)))) return rc;
      hipLaunchKernelGGL(g1_intt_finish_kernel<C>, dim3((n + 63) / 64), dim3(64), 0, c->stream, d_buf.get(), n, ninv,
                         s->recs);
      KZG_HIP(c, hipGetLastError());
    }
    KZG_HIP(c, hipStreamSynchronize(c->stream));
  }                                                      // the transform's buffer goes before the windows are built
  s->basis = SRS_LAGRANGE;
  s->log_n = log_n;
  memcpy(s->w, w_words, 32);
  if ((rc = srs_finish_windows(c, s.get()))) return rc;
  *out = s.release();
  return KZG_OK;
}

template <class F>
int open_evals_t(Ctx* c, const Srs* s, const uint32_t* d_vals, const size_t* lens, size_t k, size_t stride,
                 const uint32_t* z_words, const uint32_t* xi_words, uint64_t* out_xy, uint8_t* out_inf,
                 uint64_t* eval_out, bool sync) {
  using Fd = Field<F>;
  if (s->curve != c->curve) return set_err(c, KZG_ERR_ARG, "SRS belongs to another curve");
  if (s->basis != SRS_LAGRANGE) return set_err(c, KZG_ERR_ARG, "kzg_open_evals: the key is not a Lagrange key");
  if (k > 64) return set_err(c, KZG_ERR_ARG, "kzg_open_evals: more than 64 vectors");
  const size_t n = s->n;
  for (size_t j = 0; j < k; ++j) {
    if (lens[j] > n) return set_err(c, KZG_ERR_DEGREE, "value vector longer than the domain");
    if (lens[j] > stride) return set_err(c, KZG_ERR_ARG, "kzg_open_evals: lens[j] > stride");
  }
  const uint32_t groups = std::min<uint32_t>(SUM_MAXG, (uint32_t)((n + SUM_TB - 1) / SUM_TB));
  // [P | den = q | inv] n elements each, then the partial sums and the value block
  int rc = ensure_buf(c, c->lagr_tmp, n * 3 * 32 + (size_t)groups * 3 * LG_FRN * 4 + 128);
  if (rc) return rc;
  uint32_t* d_P = static_cast<uint32_t*>(c->lagr_tmp.p);
  uint32_t* d_den = d_P + n * 8;
  uint32_t* d_inv = d_den + n * 8;
  uint32_t* d_val = d_inv + n * 8;                       // 32-byte aligned: y words first
  uint32_t* d_part = d_val + 32;
  {
    ProfScope ps(c, "open_evals_poly");
    std::vector<const uint32_t*> ptrs(k);
    std::vector<uint32_t> xw(std::max<size_t>(k, 1) * 8);
    const Fe<F> xi = mont_from_words<F>(xi_words);
    Fe<F> xp = Fd::one();
    for (size_t j = 0; j < k; ++j) {
      ptrs[j] = d_vals + j * stride * 8;
      xp = Fd::mul(xp, xi);                                // xi^(j+1): kzg.py:148-150
      words_from_mont<F>(xp, &xw[j * 8]);
    }
    if ((rc = fr_vec_lincomb(c, n, k, ptrs.data(), lens, xw.data(), d_P))) return rc;
    if ((rc = value_pass<F>(c, s->log_n, (uint32_t)n, d_P, s->d_wpow, z_words, d_den, d_inv, d_part, d_val, d_den)))
      return rc;
  }
  const size_t qlen = n;
  if (!sync) return commit_device(c, s, d_den, &qlen, 1, n, out_xy, out_inf, /*drain=*/false, d_val, eval_out);
  if (eval_out) KZG_HIP(c, hipMemcpyAsync(eval_out, d_val, 32, hipMemcpyDeviceToHost, c->stream));
  rc = commit_device(c, s, d_den, &qlen, 1, n, out_xy, out_inf);
  if (rc) return rc;
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  return KZG_OK;
}

template <class F>
int fr_eval_lagrange_t(Ctx* c, uint32_t log_n, const uint32_t* w_words, size_t len, const uint32_t* d_vals,
                       const uint32_t* z_words, uint64_t* out) {
  memset(out, 0, 32);
  if (log_n < 1 || log_n > LG_MAX_LOG) return set_err(c, KZG_ERR_ARG, "kzg_fr_eval_lagrange: log_n must be in [1, 24]");
  if (!primitive_root<F>(mont_from_words<F>(w_words), log_n))
    return set_err(c, KZG_ERR_ARG, "kzg_fr_eval_lagrange: w is not a primitive root");
  const size_t n = (size_t)1 << log_n;
  if (len > n) return set_err(c, KZG_ERR_DEGREE, "value vector longer than the domain");
  if (len == 0) return KZG_OK;
  const uint32_t groups = std::min<uint32_t>(SUM_MAXG, (uint32_t)((n + SUM_TB - 1) / SUM_TB));
  int rc = ensure_buf(c, c->lagr_tmp, n * 3 * 32 + (size_t)groups * 3 * LG_FRN * 4 + 128);
  if (rc) return rc;
  uint32_t* d_wpow = static_cast<uint32_t*>(c->lagr_tmp.p);
  uint32_t* d_den = d_wpow + n * 8;
  uint32_t* d_inv = d_den + n * 8;
  uint32_t* d_val = d_inv + n * 8;
  uint32_t* d_part = d_val + 32;
  if ((rc = launch_wpow<F>(c, (uint32_t)n, w_words, d_wpow))) return rc;
  if ((rc = value_pass<F>(c, log_n, (uint32_t)len, d_vals, d_wpow, z_words, d_den, d_inv, d_part, d_val, nullptr)))
    return rc;
  KZG_HIP(c, hipMemcpyAsync(out, d_val, 32, hipMemcpyDeviceToHost, c->stream));
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  return KZG_OK;
}

constexpr size_t BATCH_SCRATCH_BYTES = (size_t)1 << 30;   // denominators and inverses of one chunk of vectors
constexpr size_t BATCH_MAX_CHUNK = 65535;                 // the vector index is blockIdx.y

template <class F>
int fr_eval_lagrange_batch_t(Ctx* c, uint32_t log_n, const uint32_t* w_words, const uint32_t* d_vals,
                             const size_t* lens, size_t b, size_t stride, const uint32_t* d_z, uint32_t* d_out) {
  if (log_n < 1 || log_n > LG_MAX_LOG)
    return set_err(c, KZG_ERR_ARG, "kzg_fr_eval_lagrange_batch: log_n must be in [1, 24]");
  if (!primitive_root<F>(mont_from_words<F>(w_words), log_n))
    return set_err(c, KZG_ERR_ARG, "kzg_fr_eval_lagrange_batch: w is not a primitive root");
  const size_t n = (size_t)1 << log_n;
  for (size_t j = 0; j < b; ++j) {
    if (lens[j] > n) return set_err(c, KZG_ERR_DEGREE, "value vector longer than the domain");
    if (lens[j] > stride) return set_err(c, KZG_ERR_ARG, "kzg_fr_eval_lagrange_batch: lens[j] > stride");
  }
  if (b == 0) return KZG_OK;
  if (((reinterpret_cast<uintptr_t>(d_vals) | reinterpret_cast<uintptr_t>(d_z) | reinterpret_cast<uintptr_t>(d_out)) & 31u))
    return set_err(c, KZG_ERR_ARG, "kzg_fr_eval_lagrange_batch: misaligned device pointer");
  size_t chunk = c->tune_eval_batch_chunk > 0 ? (size_t)c->tune_eval_batch_chunk
                                              : std::max<size_t>(1, BATCH_SCRATCH_BYTES / (n * 64));
  chunk = std::min<size_t>({chunk, b, BATCH_MAX_CHUNK});
  const uint32_t groups = std::min<uint32_t>(BATCH_MAXG, (uint32_t)((n + SUM_TB - 1) / SUM_TB));
  // [w^i: n | den: chunk n | inv: chunk n | partial sums | lens: b]
  const size_t part_bytes = (chunk * groups * 2 * LG_FRN * 4 + 31) / 32 * 32;
  int rc = ensure_buf(c, c->lagr_tmp, n * 32 + chunk * n * 64 + part_bytes + b * 4);
  if (rc) return rc;
  uint32_t* d_wpow = static_cast<uint32_t*>(c->lagr_tmp.p);
  uint32_t* d_den = d_wpow + n * 8;
  uint32_t* d_inv = d_den + chunk * n * 8;
  uint32_t* d_part = d_inv + chunk * n * 8;
  uint32_t* d_lens = d_part + part_bytes / 4;
  // the lengths: through the context's pinned array (an earlier call's copy out of it has to be over first)
  if (c->eval_lens_ev) KZG_HIP(c, hipEventSynchronize(c->eval_lens_ev));
  else KZG_HIP(c, hipEventCreateWithFlags(&c->eval_lens_ev, hipEventDisableTiming));
  if (c->eval_lens_cap < b) {
    if (c->eval_lens_pin) KZG_HIP(c, hipHostFree(c->eval_lens_pin));
    c->eval_lens_pin = nullptr;
    c->eval_lens_cap = 0;
    KZG_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&c->eval_lens_pin), b * 4, hipHostMallocDefault));
    c->eval_lens_cap = b;
  }
  for (size_t j = 0; j < b; ++j) c->eval_lens_pin[j] = (uint32_t)lens[j];
  ProfScope ps(c, "eval_lagrange_batch");
  KZG_HIP(c, hipMemcpyAsync(d_lens, c->eval_lens_pin, b * 4, hipMemcpyHostToDevice, c->stream));
  KZG_HIP(c, hipEventRecord(c->eval_lens_ev, c->stream));
  if ((rc = launch_wpow<F>(c, (uint32_t)n, w_words, d_wpow))) return rc;
  const FrArg ninv = fr_arg<F>(Field<F>::reduce(inv_pow2<F>(log_n)));
  for (size_t j0 = 0; j0 < b; j0 += chunk) {
    const size_t cb = std::min(chunk, b - j0), total = cb * n;
    hipLaunchKernelGGL(lagr_batch_denom_kernel<F>, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, c->stream, log_n,
                       total, d_wpow, d_z + j0 * 8, d_den);
    KZG_HIP(c, hipGetLastError());
    if ((rc = fr_vec_inverse(c, total, d_den, d_inv))) return rc;
    hipLaunchKernelGGL(lagr_batch_sums_kernel<F>, dim3(groups, (uint32_t)cb), dim3(SUM_TB), 0, c->stream, (uint32_t)n,
                       stride, d_lens + j0, d_vals + j0 * stride * 8, d_wpow, d_inv, d_part);
    hipLaunchKernelGGL(lagr_batch_value_kernel<F>, dim3((uint32_t)cb), dim3(64), 0, c->stream, log_n, groups, d_part,
                       d_z + j0 * 8, ninv, d_out + j0 * 8);
    KZG_HIP(c, hipGetLastError());
  }
  return KZG_OK;
}

}  // namespace

int fr_pow_table(Ctx* c, const FrArg& base, uint32_t* d_tab) { return KZG_BY_FR(c, pow_table_t, c, base, d_tab); }
int srs_generate_lagrange(Ctx* c, const uint32_t* tau_words, uint32_t log_n, const uint32_t* w_words, Srs** out) {
  return KZG_BY_CURVE(c, srs_generate_lagrange_t, c, tau_words, log_n, w_words, out);
}
int srs_lagrange(Ctx* c, const Srs* mono, uint32_t log_n, const uint32_t* w_words, Srs** out) {
  return KZG_BY_CURVE(c, srs_lagrange_t, c, mono, log_n, w_words, out);
}
int open_evals_device(Ctx* c, const Srs* s, const uint32_t* d_vals, const size_t* lens, size_t k, size_t stride,
                      const uint32_t* z_words, const uint32_t* xi_words, uint64_t* out_xy, uint8_t* out_inf,
                      uint64_t* eval_out, bool sync) {
  return KZG_BY_FR(c, open_evals_t, c, s, d_vals, lens, k, stride, z_words, xi_words, out_xy, out_inf, eval_out, sync);
}
int fr_eval_lagrange(Ctx* c, uint32_t log_n, const uint32_t* w_words, size_t len, const uint32_t* d_vals,
                     const uint32_t* z_words, uint64_t* out) {
  return KZG_BY_FR(c, fr_eval_lagrange_t, c, log_n, w_words, len, d_vals, z_words, out);
}
int fr_eval_lagrange_batch(Ctx* c, uint32_t log_n, const uint32_t* w_words, const uint32_t* d_vals, const size_t* lens,
                           size_t b, size_t stride, const uint32_t* d_z, uint32_t* d_out) {
  return KZG_BY_FR(c, fr_eval_lagrange_batch_t, c, log_n, w_words, d_vals, lens, b, stride, d_z, d_out);
}

}  // namespace kzg
