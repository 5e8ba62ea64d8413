// recover.hip -- coset recovery on gfx950: b polynomials of degree < n back from their values on any K >= n/l of the
// C = N/l cosets of {w^t, t < N} (recover_cells_and_kzg_proofs of EIP-7594 without the proofs).
//
// u = w^l, coset i is the root set of X^l - u^i, M the missing cosets, s the field's multiplicative generator:
//   1  V(Y) = prod_(i in M) (Y - u^i);  Z(X) = V(X^l) vanishes on the missing cosets;  Z(w^t) = DFT_C(V)[t mod C]
//   2  E = the given values, 0 where missing:  E Z = p Z on the whole domain, deg(p Z) < N  ->  p Z = IDFT_N(E Z)
//   3  (p Z)(s w^t) = DFT_N(coefficient t times s^t);  Z(s w^t) = DFT_C(V_j s^(lj))[t mod C], never zero
//   4  p(s w^t) = (p Z)(s w^t) / Z(s w^t);  IDFT_N, coefficient t times s^-t: p
//   5  the values lie on a polynomial of degree < n iff coefficients n .. N-1 are all zero (exact)
//
// V is a product tree (once per call, shared by the batch).  The host knows M, hence every node's degree:
//   leaves   rec_leaf_kernel: one workgroup multiplies out up to REC_LEAF = 64 linear factors in LDS (schoolbook,
//            Montgomery form), the roots from a two-level power table of w (fr_pow_table); a leaf without roots is the constant 1
//   level    nodes of capacity d are multiplied in pairs at transform size T = 2d: forward transform of both
//            (ntt_run_device, batch = nodes), rec_pair_mul_kernel, inverse transform.  Only two FULL monic nodes
//            reach degree T: their leading 1 wraps onto position 0, and rec_expand_kernel -- which lays the products
//            out in slots of 2T for the next level -- subtracts it there and writes it at position T.
//   Only nodes that hold roots are processed (an odd one out is paired with the constant 1); |M| <= 64 has no level.
// Per chunk of polynomials, on one [chunk][N] buffer in place: rec_scatter_kernel (E Z, zeros included), IDFT_N,
// rec_shift_kernel (s^t from a two-level table, batched), DFT_N, rec_divide_kernel (period C), IDFT_N,
// rec_finish_kernel (s^-t on the first n coefficients, one flag per polynomial for a non-zero tail).
// Every kernel: plain vector stores, no scratch, <= 128 VGPRs; elements travel as 8 canonical words.
#include <algorithm>
#include <cstring>
#include <vector>
#include "internal.h"
#include "fr_util.h"

namespace kzg {

namespace {

constexpr uint32_t REC_LEAF_LOG = 6;
constexpr uint32_t REC_LEAF = 1u << REC_LEAF_LOG;               // linear factors per leaf
constexpr uint32_t REC_MISSING = 0xffffffffu;                   // pos[] entry of a coset that was not given
constexpr size_t REC_SCRATCH_BYTES = (size_t)2 << 30;           // chunks of polynomials stay below this
constexpr uint32_t REC_MAX_CHUNK = 1024;

// Leaf q = blockIdx.x: prod (Y - u^i) over the missing cosets miss[q REC_LEAF .. ), at most REC_LEAF of them, written
// as standard-form coefficients into out[q][0 .. slot) (zero above the degree).  slot > the degree: the host passes
// 2 REC_LEAF for a tree with levels and C > |M| for a single leaf.
template <class F>
__global__ __launch_bounds__(128) void rec_leaf_kernel(uint32_t m, const uint32_t* miss, uint32_t log_l,
                                                       const uint32_t* wtab, uint32_t slot, uint32_t* out) {
  using Fd = Field<F>;
  __shared__ uint32_t coef[(REC_LEAF + 1) * F::N];
  __shared__ uint32_t root[REC_LEAF * F::N];
  const uint32_t q = blockIdx.x, tid = threadIdx.x;
  const uint32_t first = q << REC_LEAF_LOG;
  const uint32_t deg = first >= m ? 0u : min(m - first, REC_LEAF);
  if (tid < deg) store_limbs<F>(root + tid * F::N, fr_pow_lookup<F>(wtab, miss[first + tid] << log_l));   // u^i = w^(i l)
  if (tid <= REC_LEAF) store_limbs<F>(coef + tid * F::N, tid == 0 ? Fd::one() : Fd::zero());
  __syncthreads();
  for (uint32_t j = 0; j < deg; ++j) {                  // times (Y - r): c_i <- c_(i-1) - r c_i, i <= j + 1
    Fe<F> v = Fd::zero();
    const bool mine = tid <= j + 1;
    if (mine) {
      const Fe<F> lower = tid ? load_limbs<F>(coef + (tid - 1) * F::N) : Fd::zero();
      v = Fd::sub(lower, Fd::mul(load_limbs<F>(root + j * F::N), load_limbs<F>(coef + tid * F::N)));
    }
    __syncthreads();
    if (mine) store_limbs<F>(coef + tid * F::N, v);
    __syncthreads();
  }
  for (uint32_t i = tid; i < slot; i += 128) {
    const Fe<F> v = i <= deg ? Fd::from_mont(load_limbs<F>(coef + i * F::N)) : Fd::zero();
    store_words<F>(out + ((size_t)q * slot + i) * 8, v);
  }
}

// prod[j][i] = in[2j][i] * in[2j + 1][i], i < T = 2^log_t (transforms of a pair of nodes)
template <class F>
__global__ __launch_bounds__(256) void rec_pair_mul_kernel(const uint32_t* in, uint32_t nn, uint32_t log_t,
                                                           uint32_t* prod) {
  using Fd = Field<F>;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ((size_t)nn << log_t)) return;
  const size_t j = g >> log_t, i = g & (((size_t)1 << log_t) - 1);
  const uint32_t* a = in + (((2 * j) << log_t) + i) * 8;
  store_words<F>(prod + g * 8, Fd::mul(Fd::to_mont(load_words<F>(a)), load_words<F>(a + ((size_t)8 << log_t))));
}

// The products of a level (prod: [nn][T] cyclic products, node q of degree min(max(m - q T, 0), T)) laid out for the
// next one: out[q][0 .. slot), q < nslots, slot > T.  A node of degree T is the product of two full monic nodes: its
// leading 1 wrapped onto position 0.  Nodes q >= nn hold no roots: the constant 1.
template <class F>
__global__ __launch_bounds__(256) void rec_expand_kernel(const uint32_t* prod, uint32_t nn, uint32_t log_t, uint32_t m,
                                                         uint32_t log_slot, uint32_t nslots, uint32_t* out) {
  using Fd = Field<F>;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ((size_t)nslots << log_slot)) return;
  const uint32_t q = (uint32_t)(g >> log_slot), i = (uint32_t)(g & (((size_t)1 << log_slot) - 1));
  const uint32_t T = 1u << log_t;
  const uint64_t first = (uint64_t)q << log_t;
  const bool full = first + T <= m;
  Fe<F> v = Fd::zero();
  if (q >= nn) {
    if (i == 0) v = Fd::raw_one();
  } else if (i < T) {
    v = load_words<F>(prod + (((size_t)q << log_t) + i) * 8);
    if (full && i == 0) v = Fd::sub(v, Fd::raw_one());
  } else if (i == T && full) {
    v = Fd::raw_one();
  }
  store_words<F>(out + g * 8, v);
}

// in place: x[i] <- x[i] R (the Montgomery form, kept as words) for the two period-C factor vectors
template <class F>
__global__ __launch_bounds__(256) void rec_to_mont_kernel(uint32_t* a, uint32_t* b, uint32_t count) {
  using Fd = Field<F>;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * count) return;
  uint32_t* p = (i < count ? a : b) + (size_t)(i < count ? i : i - count) * 8;
  store_words<F>(p, Fd::to_mont(load_words<F>(p)));
}

// x[j][t] = E_j[t] Z(w^t): t = i + k C is value k of coset i; pos[i] = the cell that holds coset i, or REC_MISSING
// (then 0).  vals: [nvec][K][l] canonical words, zw: [C] Montgomery words.
template <class F>
__global__ __launch_bounds__(256) void rec_scatter_kernel(const uint32_t* vals, const uint32_t* pos, const uint32_t* zw,
                                                          uint32_t nvec, uint32_t K, uint32_t log_N, uint32_t log_l,
                                                          uint32_t* x) {
  using Fd = Field<F>;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ((size_t)nvec << log_N)) return;
  const uint32_t log_c = log_N - log_l;
  const size_t j = g >> log_N;
  const uint32_t t = (uint32_t)(g & (((size_t)1 << log_N) - 1)), i = t & ((1u << log_c) - 1), k = t >> log_c;
  const uint32_t cell = pos[i];
  Fe<F> v = Fd::zero();
  if (cell != REC_MISSING)
    v = Fd::mul(load_words<F>(vals + (((j * K + cell) << log_l) + k) * 8), load_words<F>(zw + (size_t)i * 8));
  store_words<F>(x + g * 8, v);
}

// x[j][t] <- x[j][t] s^t (tab: the two-level table of s), every vector of the chunk in one launch
template <class F>
__global__ __launch_bounds__(256) void rec_shift_kernel(uint32_t* x, uint32_t nvec, uint32_t log_N,
                                                        const uint32_t* tab) {
  using Fd = Field<F>;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ((size_t)nvec << log_N)) return;
  const uint32_t t = (uint32_t)(g & (((size_t)1 << log_N) - 1));
  store_words<F>(x + g * 8, Fd::mul(load_words<F>(x + g * 8), fr_pow_lookup<F>(tab, t)));
}

// x[j][t] <- x[j][t] zinv[t mod C] (zinv: Montgomery words)
template <class F>
__global__ __launch_bounds__(256) void rec_divide_kernel(uint32_t* x, uint32_t nvec, uint32_t log_N, uint32_t log_c,
                                                         const uint32_t* zinv) {
  using Fd = Field<F>;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ((size_t)nvec << log_N)) return;
  const size_t i = g & (((size_t)1 << log_c) - 1);
  store_words<F>(x + g * 8, Fd::mul(load_words<F>(x + g * 8), load_words<F>(zinv + i * 8)));
}

// coeffs[j][t] = x[j][t] s^-t for t < n; a non-zero x[j][t], t >= n, raises flag[j] (any_nonzero_kernel's pattern:
// x s^-t is zero exactly where x is)
template <class F>
__global__ __launch_bounds__(256) void rec_finish_kernel(const uint32_t* x, uint32_t nvec, uint32_t log_N,
                                                         uint32_t log_n, const uint32_t* sitab, uint32_t* coeffs,
                                                         uint32_t* flag) {
  using Fd = Field<F>;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ((size_t)nvec << log_N)) return;
  const size_t j = g >> log_N;
  const uint32_t t = (uint32_t)(g & (((size_t)1 << log_N) - 1));
  if (t < (1u << log_n)) {
    store_words<F>(coeffs + ((j << log_n) + t) * 8, Fd::mul(load_words<F>(x + g * 8), fr_pow_lookup<F>(sitab, t)));
  } else {
    const uint4* p = reinterpret_cast<const uint4*>(x + g * 8);
    const uint4 lo = p[0], hi = p[1];
    if (lo.x | lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w) atomicOr(flag + j, 1u);
  }
}

// ---- host side --------------------------------------------------------------------------------------

struct RecLevel {
  uint32_t log_t;      // transform size T = twice the capacity of the nodes it multiplies
  uint32_t nn;         // pairs
};

inline dim3 rec_grid(size_t threads) { return dim3((uint32_t)((threads + 255) / 256)); }

template <class Cv>
int recover_t(Ctx* c, uint32_t log_n, uint32_t log_N, uint32_t log_l, const uint32_t* w_words,
              const uint32_t* coset_idx, size_t K, const uint32_t* values, bool host, size_t b, uint32_t* coeffs,
              uint8_t* out_consistent) {
  using F = typename Cv::Fr;
  using Fd = Field<F>;
  if (log_l > 12 || log_l > log_n || log_n > log_N || log_N > 21 || log_l >= log_N)
    return set_err(c, KZG_ERR_ARG, "kzg_recover_cosets: need 0 <= log_l <= 12, log_l <= log_n <= log_N <= 21 and log_l < log_N");
  const uint32_t log_c = log_N - log_l;
  const size_t C = (size_t)1 << log_c, N = (size_t)1 << log_N, n = (size_t)1 << log_n;
  if (b < 1) return set_err(c, KZG_ERR_ARG, "kzg_recover_cosets: need b >= 1");
  if (K > C) return set_err(c, KZG_ERR_ARG, "kzg_recover_cosets: more cells than cosets");
  if ((K << log_l) < n) return set_err(c, KZG_ERR_ARG, "kzg_recover_cosets: K * l < n, too few cells for degree < n");
  std::vector<uint32_t> pos(C, REC_MISSING), miss;
  for (size_t k = 0; k < K; ++k) {
    if (coset_idx[k] >= C) return set_err(c, KZG_ERR_ARG, "kzg_recover_cosets: coset index out of range");
    if (pos[coset_idx[k]] != REC_MISSING) return set_err(c, KZG_ERR_ARG, "kzg_recover_cosets: a coset index is repeated");
    pos[coset_idx[k]] = (uint32_t)k;
  }
  const Fe<F> w = mont_from_words<F>(w_words);
  if (!primitive_root<F>(w, log_N))
    return set_err(c, KZG_ERR_ARG, "kzg_recover_cosets: w is not a primitive N-th root of unity");
  if (!host && ((reinterpret_cast<uintptr_t>(values) | reinterpret_cast<uintptr_t>(coeffs)) & 31))
    return set_err(c, KZG_ERR_ARG, "kzg_recover_cosets_device: device pointers must be 32-byte aligned");
  miss.reserve(C - K);
  for (size_t i = 0; i < C; ++i)
    if (pos[i] == REC_MISSING) miss.push_back((uint32_t)i);
  const uint32_t m = (uint32_t)miss.size();              // |M| <= C - n/l < C

  // the tree: leaves that hold roots, then pairs until one node is left
  std::vector<RecLevel> levels;
  size_t cap_a = 0, cap_b = 0;
  {
    uint32_t active = std::max<uint32_t>(1, (m + REC_LEAF - 1) >> REC_LEAF_LOG), log_d = REC_LEAF_LOG;
    while (active > 1) {
      const uint32_t nn = (active + 1) / 2;
      levels.push_back({log_d + 1, nn});
      cap_a = std::max(cap_a, (size_t)2 * nn << (log_d + 1));
      cap_b = std::max(cap_b, (size_t)nn << (log_d + 1));
      active = nn;
      ++log_d;
    }
  }

  const size_t cells = K << log_l;
  const size_t per_vec = N * 32 + (host ? (cells + n) * 32 : 0);
  size_t chunk = c->tune_recover_chunk > 0 ? (size_t)c->tune_recover_chunk
                                           : std::max<size_t>(1, REC_SCRATCH_BYTES / per_vec);
  chunk = std::min<size_t>({chunk, b, REC_MAX_CHUNK});
  uint32_t *d_wtab, *d_stab, *d_sitab, *d_miss, *d_pos, *d_a, *d_b, *d_v, *d_zw, *d_zinv, *d_flag, *d_x, *d_vals, *d_out;
  int rc = carve(c, c->rec_tmp, [&](Carve& ws) {
    d_wtab = ws.take((size_t)POW_TAB * 32);  d_stab = ws.take((size_t)POW_TAB * 32);
    d_sitab = ws.take((size_t)POW_TAB * 32);  d_miss = ws.take((size_t)m * 4);  d_pos = ws.take(C * 4);
    d_a = ws.take(cap_a * 32);  d_b = ws.take(cap_b * 32);  d_v = ws.take(C * 32);
    d_zw = ws.take(2 * C * 32);                                  // Z on the domain, then (d_zs) on its shift
    d_zinv = ws.take(C * 32);  d_flag = ws.take(b * 4);  d_x = ws.take(chunk * N * 32);
    d_vals = ws.take_if<uint32_t>(host, chunk * cells * 32);  d_out = ws.take_if<uint32_t>(host, chunk * n * 32);
  });
  if (rc) return rc;
  uint32_t* d_zs = d_zw + C * 8;

  const Fe<F> s = fr_generator<Cv>(), s_inv = Fd::inv(s);                      // the multiplicative generator: s^N != 1
  Fe<F> s_l = s;
  for (uint32_t q = 0; q < log_l; ++q) s_l = Fd::sqr(s_l);
  uint32_t sl_words[8], one_words[8] = {1, 0, 0, 0, 0, 0, 0, 0}, u_words[8];
  words_from_mont<F>(s_l, sl_words);
  std::vector<Fe<F>> w_pow(log_N + 1);                   // w_pow[k] = w^(N / 2^k): the root of a size-2^k transform
  w_pow[log_N] = w;
  for (uint32_t k = log_N; k-- > 0;) w_pow[k] = Fd::sqr(w_pow[k + 1]);
  words_from_mont<F>(w_pow[log_c], u_words);

  ProfScope ps(c, "recover_cosets");
  hipStream_t st = c->stream;
  if (m) KZG_HIP(c, hipMemcpyAsync(d_miss, miss.data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
  KZG_HIP(c, hipMemcpyAsync(d_pos, pos.data(), C * 4, hipMemcpyHostToDevice, st));
  KZG_HIP(c, hipMemsetAsync(d_flag, 0, b * 4, st));
  if ((rc = fr_pow_table(c, fr_arg<F>(w), d_wtab))) return rc;
  if ((rc = fr_pow_table(c, fr_arg<F>(s), d_stab))) return rc;
  if ((rc = fr_pow_table(c, fr_arg<F>(s_inv), d_sitab))) return rc;

  // ---- V: leaves, then one level per doubling
  if (levels.empty()) {
    hipLaunchKernelGGL(rec_leaf_kernel<F>, dim3(1), dim3(128), 0, st, m, d_miss, log_l, d_wtab, (uint32_t)C, d_v);
  } else {
    hipLaunchKernelGGL(rec_leaf_kernel<F>, dim3(2 * levels[0].nn), dim3(128), 0, st, m, d_miss, log_l, d_wtab,
                       2 * REC_LEAF, d_a);
  }
  KZG_HIP(c, hipGetLastError());
  for (size_t lv = 0; lv < levels.size(); ++lv) {
    const uint32_t log_t = levels[lv].log_t, nn = levels[lv].nn;
    uint32_t root_words[8];
    words_from_mont<F>(w_pow[log_t], root_words);               // log_t <= log_c: T <= C whenever a level exists
    if ((rc = ntt_run_device(c, d_a, log_t, root_words, 0, 2 * nn))) return rc;
    hipLaunchKernelGGL(rec_pair_mul_kernel<F>, rec_grid((size_t)nn << log_t), dim3(256), 0, st, d_a, nn, log_t, d_b);
    KZG_HIP(c, hipGetLastError());
    if ((rc = ntt_run_device(c, d_b, log_t, root_words, 1, nn))) return rc;
    const bool last = lv + 1 == levels.size();
    const uint32_t log_slot = last ? log_c : log_t + 1, nslots = last ? 1u : 2 * levels[lv + 1].nn;
    hipLaunchKernelGGL(rec_expand_kernel<F>, rec_grid((size_t)nslots << log_slot), dim3(256), 0, st, d_b, nn, log_t, m,
                       log_slot, nslots, last ? d_v : d_a);
    KZG_HIP(c, hipGetLastError());
  }

  // ---- Z on the domain and on its shift; the inverses of the latter
  KZG_HIP(c, hipMemcpyAsync(d_zw, d_v, C * 32, hipMemcpyDeviceToDevice, st));
  if ((rc = fr_vec_mul_powers(c, C, d_v, sl_words, one_words, d_zs))) return rc;
  if ((rc = ntt_run_device(c, d_zw, log_c, u_words, 0, 2))) return rc;
  if ((rc = fr_vec_inverse(c, C, d_zs, d_zinv))) return rc;
  hipLaunchKernelGGL(rec_to_mont_kernel<F>, rec_grid(2 * C), dim3(256), 0, st, d_zw, d_zinv, (uint32_t)C);
  KZG_HIP(c, hipGetLastError());

  // ---- the polynomials, chunk by chunk
  for (size_t j0 = 0; j0 < b; j0 += chunk) {
    const uint32_t mv = (uint32_t)std::min(chunk, b - j0);
    const size_t elems = (size_t)mv << log_N;
    const uint32_t* src = values + j0 * cells * 8;
    uint32_t* dst = coeffs + j0 * n * 8;
    if (host) {
      KZG_HIP(c, hipMemcpyAsync(d_vals, src, (size_t)mv * cells * 32, hipMemcpyHostToDevice, st));
      src = d_vals;
    }
    hipLaunchKernelGGL(rec_scatter_kernel<F>, rec_grid(elems), dim3(256), 0, st, src, d_pos, d_zw, mv, (uint32_t)K,
                       log_N, log_l, d_x);
    KZG_HIP(c, hipGetLastError());
    if ((rc = ntt_run_device(c, d_x, log_N, w_words, 1, mv))) return rc;
    hipLaunchKernelGGL(rec_shift_kernel<F>, rec_grid(elems), dim3(256), 0, st, d_x, mv, log_N, d_stab);
    KZG_HIP(c, hipGetLastError());
    if ((rc = ntt_run_device(c, d_x, log_N, w_words, 0, mv))) return rc;
    hipLaunchKernelGGL(rec_divide_kernel<F>, rec_grid(elems), dim3(256), 0, st, d_x, mv, log_N, log_c, d_zinv);
    KZG_HIP(c, hipGetLastError());
    if ((rc = ntt_run_device(c, d_x, log_N, w_words, 1, mv))) return rc;
    hipLaunchKernelGGL(rec_finish_kernel<F>, rec_grid(elems), dim3(256), 0, st, d_x, mv, log_N, log_n, d_sitab,
                       host ? d_out : dst, d_flag + j0);
    KZG_HIP(c, hipGetLastError());
    if (host) {
      KZG_HIP(c, hipMemcpyAsync(dst, d_out, (size_t)mv * n * 32, hipMemcpyDeviceToHost, st));
      // the next chunk overwrites the staging buffers the copies use
      KZG_HIP(c, hipStreamSynchronize(st));
    }
  }
  std::vector<uint32_t> flags(b);
  KZG_HIP(c, hipMemcpyAsync(flags.data(), d_flag, b * 4, hipMemcpyDeviceToHost, st));
  KZG_HIP(c, hipStreamSynchronize(st));
  for (size_t j = 0; j < b; ++j) out_consistent[j] = flags[j] ? 0 : 1;
  return KZG_OK;
}

}  // namespace

uint32_t recover_leaf_width() { return REC_LEAF; }

int recover_cosets(Ctx* c, uint32_t log_n, uint32_t log_N, uint32_t log_l, const uint32_t* w_words,
                   const uint32_t* coset_idx, size_t K, const uint32_t* values, bool host_ptrs, size_t b,
                   uint32_t* coeffs, uint8_t* out_consistent) {
  return KZG_BY_CURVE(c, recover_t, c, log_n, log_N, log_l, w_words, coset_idx, K, values, host_ptrs, b, coeffs,
                      out_consistent);
}

}  // namespace kzg
