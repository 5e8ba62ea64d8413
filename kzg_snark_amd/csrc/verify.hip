// verify.hip -- bulk verification on gfx950: K coset claims folded into the two G1 points of ONE pairing equation.
//
// Claim k: the polynomial of commitment C[c_k] takes the l values y_k[t] at w^(i_k + t N/l), proof pi_k.  With
// h_k = w^(i_k), a_k = h_k^l, zeta = w^(N/l), the remainder I_k(X) = sum_j rho_kj X^j,
// rho_kj = h_k^-j l^-1 sum_t y_k[t] zeta^(-jt), and the weights r_k = rho^(k+1):
//     L = sum_j (sum_(k: c_k = j) r_k) C[j]  -  [T(tau)] G1  +  sum_k (r_k a_k) pi_k,     T_j = sum_k r_k rho_kj
//     R = sum_k r_k pi_k                           accept iff e(L, G2) = e(R, [tau^l] G2)       
//
//   powers    w^e (e < N <= 2^21) and rho^e (e <= K <= 2^21) come from two-level tables x^e = lo[e & 2047] hi[e >> 11]
//             (fr_pow_table, 3073 entries each): one product per power, no per-cell exponentiation
//   weights   r_k and s_k = r_k a_k as canonical scalars (ver_weights_kernel); the per-commitment sums of r_k over the
//             cells grouped by commitment (a counting sort of the small indices on the host, ver_commsum_kernel)
//   values    ver_cell_kernel: tiles of max(l, 256) elements in LDS, a decimation-in-frequency inverse transform per
//             cell (twiddles from the w table), then r_k l^-1 h_k^-j applied on the way back to memory;
//             ver_colsum_kernel / ver_colsum_final_kernel add the cells up: T.  kzg_verify_cosets_bytes brings them as
//             32-byte big-endian elements: uploaded once behind the pinned layout, written into the
//             value array by the intake kernel of blob.hip; an element >= r is a verdict and nothing is folded
//   proofs    imported as window-0 records (g1_import: coordinates < p, on the curve) of a key that holds NO
//             other window; every scalar is cut into slices of win_bits - 1 bits (ver_slice_kernel) and each slice
//             vector goes through the commit pipeline as one polynomial: a slice yields one digit, in window 0, without
//             a carry.  sum_s 2^(s (win_bits - 1)) P_s is finished on the host.
//   short     [T(tau)] is a commit of l scalars against the monomial key, the commitment term a commit of n_comm
//             scalars against a key loaded from the commitments.
//   plan      tile size and count, the grid cap, the threads of the column sum, the shares of a commitment sum and the
//             slices are decided in one place, VerPlan (ver_layout.h), which the host tests read through their shim.
// Fr kernels: <= 128 VGPRs, no scratch; elements travel as 8 canonical words (values in standard form, table entries
// and factors in Montgomery form, so a product of the two is in standard form again).
#include <cstring>
#include <algorithm>
#include <vector>
#include "internal.h"
#include "fr_util.h"
#include "g1_util.h"
#include "msm.h"
#include "g1_words.h"
#include "ver_layout.h"

namespace kzg {

namespace {

// r_k = rho^(k+1) and s_k = r_k w^(i_k l), canonical words
template <class F>
__global__ __launch_bounds__(256) void ver_weights_kernel(uint32_t K, uint32_t log_l, const uint32_t* coset_idx,
                                                          const uint32_t* wtab, const uint32_t* rtab, uint32_t* r_out,
                                                          uint32_t* s_out) {
  using Fd = Field<F>;
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const Fe<F> r = fr_pow_lookup<F>(rtab, k + 1);
  const Fe<F> s = Fd::mul(r, fr_pow_lookup<F>(wtab, coset_idx[k] << log_l));     // i_k < N/l: the exponent is below N
  store_words<F>(r_out + (size_t)k * 8, Fd::from_mont(r));
  store_words<F>(s_out + (size_t)k * 8, Fd::from_mont(s));
}

template <class F>
__device__ __forceinline__ Fe<F> ver_lds_load(const uint32_t* tile, uint32_t pos) {
  return load_words<F>(tile + (size_t)pos * 8);
}

// vals[k][j] <- r_k l^-1 h_k^-j sum_t vals[k][t] zeta^(-jt), in place.  A workgroup takes tiles of E = 2^log_e =
// max(l, 256) consecutive elements (whole cells): decimation in frequency in LDS, natural order in, bit-reversed out,
// the output j of a cell read from position bitrev(j).  Dynamic LDS: E x 32 bytes.
template <class F>
__global__ __launch_bounds__(256) void ver_cell_kernel(uint32_t K, uint32_t log_l, uint32_t log_N, uint32_t log_e,
                                                       const uint32_t* coset_idx, const uint32_t* wtab,
                                                       const uint32_t* rtab, FrArg linv, uint32_t* vals) {
  using Fd = Field<F>;
  extern __shared__ __attribute__((aligned(16))) uint32_t ver_tile[];
  const uint32_t E = 1u << log_e, l = 1u << log_l, N = 1u << log_N, tid = threadIdx.x;
  const size_t M = (size_t)K << log_l;
  const size_t ntiles = (M + E - 1) >> log_e;
  for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const size_t base = t << log_e;
    for (uint32_t p = tid; p < E; p += 256) {
      uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
      if (base + p < M) {
        const uint4* g = reinterpret_cast<const uint4*>(vals + (base + p) * 8);
        lo = g[0];
        hi = g[1];
      }
      uint4* s = reinterpret_cast<uint4*>(ver_tile + (size_t)p * 8);
      s[0] = lo;
      s[1] = hi;
    }
    __syncthreads();
    for (uint32_t ll = log_l; ll >= 1; --ll) {         // blocks of 2^ll elements, never across a cell
      const uint32_t half = 1u << (ll - 1);
      for (uint32_t b = tid; b < E / 2; b += 256) {
        const uint32_t i = b & (half - 1);
        const uint32_t pos = ((b >> (ll - 1)) << ll) + i;
        const Fe<F> u = ver_lds_load<F>(ver_tile, pos), v = ver_lds_load<F>(ver_tile, pos + half);
        const uint32_t ex = (N - (N >> ll) * i) & (N - 1);             // (zeta^-1)^(i l / 2^ll) = w^(-i N / 2^ll)
        store_words<F>(ver_tile + (size_t)pos * 8, Fd::add(u, v));
        store_words<F>(ver_tile + (size_t)(pos + half) * 8, Fd::mul(Fd::sub(u, v), fr_pow_lookup<F>(wtab, ex)));
      }
      __syncthreads();
    }
    for (uint32_t p = tid; p < E; p += 256) {
      if (base + p >= M) continue;
      const uint32_t k = (uint32_t)((base + p) >> log_l), j = p & (l - 1);
      const Fe<F> x = ver_lds_load<F>(ver_tile, (p & ~(l - 1)) + bitrev(j, log_l));
      const uint32_t ex = (N - (uint32_t)(((uint64_t)coset_idx[k] * j) & (N - 1))) & (N - 1);   // h_k^-j
      const Fe<F> f = Fd::mul(Fd::mul(fr_pow_lookup<F>(rtab, k + 1), arg_fe<F>(linv)), fr_pow_lookup<F>(wtab, ex));
      store_words<F>(vals + (base + p) * 8, Fd::mul(x, f));
    }
    __syncthreads();
  }
}

// part[t] = sum of vals[e], e = t mod (number of threads): the thread count is a multiple of l, so every thread stays
// in one column j = t mod l
template <class F>
__global__ __launch_bounds__(256) void ver_colsum_kernel(size_t M, const uint32_t* vals, uint32_t* part) {
  using Fd = Field<F>;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  Fe<F> acc = Fd::zero();
  for (size_t e = t; e < M; e += stride) acc = Fd::add(acc, load_words<F>(vals + e * 8));
  store_words<F>(part + t * 8, acc);
}

// out[j] = sum_(q < cnt) part[q * cols + j]: one wave per column
template <class F>
__global__ __launch_bounds__(64) void ver_colsum_final_kernel(uint32_t cols, uint32_t cnt, const uint32_t* part,
                                                              uint32_t* out) {
  using Fd = Field<F>;
  const uint32_t j = blockIdx.x;
  Fe<F> acc = Fd::zero();
  for (uint32_t q = threadIdx.x; q < cnt; q += 64) acc = Fd::add(acc, load_words<F>(part + ((size_t)q * cols + j) * 8));
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc = Fd::add(acc, shfl_xor_fe<F>(acc, m));
  if (threadIdx.x == 0) store_words<F>(out + (size_t)j * 8, acc);
}

// part[sp][j] = sum of r[perm[q]] over share sp of the cells of commitment j (perm: cells grouped by commitment,
// off[j] .. off[j + 1])
template <class F>
__global__ __launch_bounds__(256) void ver_commsum_kernel(const uint32_t* r, const uint32_t* perm, const uint32_t* off,
                                                          uint32_t n_comm, uint32_t* part) {
  using Fd = Field<F>;
  __shared__ uint32_t red[4][F::N];
  const uint32_t j = blockIdx.x, sp = blockIdx.y, nsp = gridDim.y;
  const uint32_t q0 = off[j], len = off[j + 1] - q0;
  const uint32_t a = q0 + (uint32_t)(((uint64_t)len * sp) / nsp), b = q0 + (uint32_t)(((uint64_t)len * (sp + 1)) / nsp);
  Fe<F> acc = Fd::zero();
  for (uint32_t q = a + threadIdx.x; q < b; q += 256) acc = Fd::add(acc, load_words<F>(r + (size_t)perm[q] * 8));
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc = Fd::add(acc, shfl_xor_fe<F>(acc, m));
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0) store_limbs<F>(red[wave], acc);
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t q = 1; q < 4; ++q) acc = Fd::add(acc, load_limbs<F>(red[q]));
    store_words<F>(part + ((size_t)sp * n_comm + j) * 8, acc);
  }
}

// out[k] = bits [bit, bit + bits) of the canonical scalar src[k], as a scalar of its own (bits <= 19)
__global__ __launch_bounds__(256) void ver_slice_kernel(uint32_t K, const uint32_t* src, uint32_t bit, uint32_t bits,
                                                        uint32_t* out) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const uint32_t idx = bit >> 5, sh = bit & 31u;
  const uint64_t lo = src[(size_t)k * 8 + idx], hi = idx + 1 < 8 ? src[(size_t)k * 8 + idx + 1] : 0u;
  const uint32_t d = (uint32_t)(((hi << 32) | lo) >> sh) & ((1u << bits) - 1);
  uint4* o = reinterpret_cast<uint4*>(out + (size_t)k * 8);
  o[0] = make_uint4(d, 0, 0, 0);
  o[1] = make_uint4(0, 0, 0, 0);
}

// ---- host side --------------------------------------------------------------------------------------

template <class C>
XYZZ<C> host_point(const uint64_t* xy, uint8_t inf) {
  return Ec<C>::from_affine(affine_from_words<C>(reinterpret_cast<const uint32_t*>(xy), inf != 0));
}

// sum_s 2^(s * sb) P_s over the slice results, from the top slice down
template <class C>
XYZZ<C> recombine_slices(const uint64_t* xy, const uint8_t* inf, uint32_t ns, uint32_t sb) {
  constexpr size_t PW64 = C::Fp::NW;                // 64-bit words per point (2 coordinates of NW / 2)
  XYZZ<C> acc = Ec<C>::infinity();
  for (uint32_t s = ns; s-- > 0;) {
    for (uint32_t d = 0; d < sb; ++d) acc = Ec<C>::dbl(acc);
    acc = Ec<C>::add(acc, host_point<C>(xy + (size_t)s * PW64, inf[s]));
  }
  return acc;
}

// The values of the K claims, one of two forms: canonical limbs in natural order, or cells of 32-byte big-endian
// elements that the intake kernel of blob.hip turns into the former on the device (status: their verdict)
struct VerClaims {
  const uint64_t* limbs;
  const uint8_t* cells;
  int bit_reversed;
  uint8_t* status;
};

template <class C>
int verify_cosets_t(Ctx* c, const Srs* mono, uint32_t log_N, uint32_t log_l, const uint32_t* w_words,
                    const uint64_t* comm_xy, const uint8_t* comm_inf, size_t n_comm, const uint32_t* comm_idx,
                    const uint32_t* coset_idx, const VerClaims& claims, const uint64_t* proof_xy,
                    const uint8_t* proof_inf, size_t K, const uint32_t* rho_words, uint64_t* out_xy, uint8_t* out_inf) {
  using F = typename C::Fr;
  using Fd = Field<F>;
  using Fp = typename C::Fp;
  constexpr size_t PW64 = Fp::NW;                   // 64-bit words per affine point
  constexpr size_t PT_BYTES = 2 * Fp::NW * 4;
  if (mono->curve != c->curve) return set_err(c, KZG_ERR_ARG, "SRS belongs to another curve");
  if (mono->basis != SRS_MONOMIAL) return set_err(c, KZG_ERR_ARG, "kzg_verify_cosets: the key must be monomial");
  if (log_l > 12 || log_N <= log_l || log_N > 21)
    return set_err(c, KZG_ERR_ARG, "kzg_verify_cosets: need 0 <= log_l <= 12 and log_l < log_N <= 21");
  if (K > ((size_t)1 << 21) || (K << log_l) > ((size_t)1 << 24))
    return set_err(c, KZG_ERR_ARG, "kzg_verify_cosets: need K <= 2^21 and K * l <= 2^24");
  if (n_comm < 1 || n_comm > ((size_t)1 << 16)) return set_err(c, KZG_ERR_ARG, "kzg_verify_cosets: need 1 <= n_comm <= 2^16");
  const size_t l = (size_t)1 << log_l;
  if (mono->n < l) return set_err(c, KZG_ERR_ARG, "kzg_verify_cosets: the key has fewer than l points");
  const Fe<F> w = mont_from_words<F>(w_words);
  if (!primitive_root<F>(w, log_N))
    return set_err(c, KZG_ERR_ARG, "kzg_verify_cosets: w is not a primitive N-th root of unity");
  memset(out_xy, 0, 2 * PT_BYTES);
  out_inf[0] = out_inf[1] = 1;
  if (claims.status) *claims.status = 0;
  if (K == 0) return KZG_OK;
  // the cells grouped by commitment: a counting sort of the indices (and their range check, cell by cell)
  const uint32_t n_cosets = 1u << (log_N - log_l);
  std::vector<uint32_t> off, perm;
  const size_t k_bad = group_by_index(comm_idx, K, n_comm, off, perm);
  for (size_t k = 0; k < k_bad; ++k)
    if (coset_idx[k] >= n_cosets) return set_err(c, KZG_ERR_ARG, "kzg_verify_cosets: coset index out of range");
  if (k_bad < K) return set_err(c, KZG_ERR_ARG, "kzg_verify_cosets: commitment index out of range");

  Srs pv;                                            // the proofs as a key of one window; its records after the carve
  srs_window0_view(c, nullptr, K, &pv);
  const VerPlan plan(K, log_l, n_comm, (uint32_t)pv.win_bits, F::BITS);
  const size_t M = plan.M, rb = srs_rec_bytes(c->curve);
  VerifyWs d;
  uint32_t* d_cells = nullptr;                       // the cells as bytes and their verdict, behind the pinned layout
  uint8_t* d_status = nullptr;
  size_t total = 0;
  int rc = carve(c, c->ver_tmp, [&](Carve& ws) {
    d.layout(ws, K, n_comm, l, proof_inf != nullptr, comm_inf != nullptr, PT_BYTES, rb, POW_TAB, plan.sum_threads,
             plan.shares);
    d_cells = ws.take_if<uint32_t>(claims.cells != nullptr, M * 32);
    d_status = ws.take_if(claims.cells != nullptr, K);
  }, &total);
  if (rc) return rc;
  pv.recs = d.recs;

  SrsPtr cs;                                         // the commitments as a key of their own (all windows)
  if ((rc = srs_create(c, n_comm, &cs))) return rc;
  c->ver_last_bytes = total + (size_t)cs->nwin * n_comm * rb;

  ProfScope ps(c, "verify_cosets");
  hipStream_t st = c->stream;
  KZG_HIP(c, hipMemcpyAsync(d.pxy, proof_xy, K * PT_BYTES, hipMemcpyHostToDevice, st));
  if (proof_inf) KZG_HIP(c, hipMemcpyAsync(d.pinf, proof_inf, K, hipMemcpyHostToDevice, st));
  KZG_HIP(c, hipMemcpyAsync(d.cxy, comm_xy, n_comm * PT_BYTES, hipMemcpyHostToDevice, st));
  if (comm_inf) KZG_HIP(c, hipMemcpyAsync(d.cinf, comm_inf, n_comm, hipMemcpyHostToDevice, st));
  KZG_HIP(c, hipMemsetAsync(d.bad, 0, 4, st));
  if ((rc = g1_import(c, d.pxy, d.pinf, K, /*range=*/true, d.recs, d.bad))) return rc;
  if ((rc = g1_import(c, d.cxy, d.cinf, n_comm, /*range=*/true, cs->recs, d.bad))) return rc;
  uint32_t bad = 0;
  KZG_HIP(c, hipMemcpyAsync(&bad, d.bad, 4, hipMemcpyDeviceToHost, st));
  // the claims travel while the points are checked
  std::vector<uint8_t> status(claims.cells ? K : 0);  // per cell, as the intake writes them
  if (claims.cells) {
    KZG_HIP(c, hipMemcpyAsync(d_cells, claims.cells, M * 32, hipMemcpyHostToDevice, st));
    if ((rc = blob_intake_launch(c, log_l, d_cells, K, claims.bit_reversed, d.vals, d_status))) return rc;
    KZG_HIP(c, hipMemcpyAsync(status.data(), d_status, K, hipMemcpyDeviceToHost, st));
  } else {
    KZG_HIP(c, hipMemcpyAsync(d.vals, claims.limbs, M * 32, hipMemcpyHostToDevice, st));
  }
  KZG_HIP(c, hipMemcpyAsync(d.cidx, coset_idx, K * 4, hipMemcpyHostToDevice, st));
  KZG_HIP(c, hipMemcpyAsync(d.perm, perm.data(), K * 4, hipMemcpyHostToDevice, st));
  KZG_HIP(c, hipMemcpyAsync(d.off, off.data(), (n_comm + 1) * 4, hipMemcpyHostToDevice, st));
  KZG_HIP(c, hipStreamSynchronize(st));
  if (bad) return set_err(c, KZG_ERR_ARG, "kzg_verify_cosets: a proof or commitment has a coordinate >= p or is not on the curve");
  if (std::find(status.begin(), status.end(), 1) != status.end()) {   // an element >= r: a verdict, nothing is folded
    *claims.status = 1;
    return KZG_OK;
  }
  if ((rc = srs_finish_windows(c, cs.get()))) return rc;

  // ---- weights and the fold of the values
  const Fe<F> rho = mont_from_words<F>(rho_words);
  const dim3 k_grid((uint32_t)((K + 255) / 256));
  if ((rc = fr_pow_table(c, fr_arg<F>(w), d.wtab))) return rc;
  if ((rc = fr_pow_table(c, fr_arg<F>(rho), d.rtab))) return rc;
  hipLaunchKernelGGL(ver_weights_kernel<F>, k_grid, dim3(256), 0, st, (uint32_t)K, log_l, d.cidx, d.wtab, d.rtab, d.r,
                     d.s);
  KZG_HIP(c, hipGetLastError());
  if (plan.lds_bytes > 64 * 1024 && !c->ver_lds_attr_set) {   // > 64 KiB of dynamic LDS (gfx950: 160 KiB per CU); per device
    KZG_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(ver_cell_kernel<F>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    c->ver_lds_attr_set = 1;
  }
  hipLaunchKernelGGL(ver_cell_kernel<F>, dim3(plan.cell_grid), dim3(256), plan.lds_bytes, st, (uint32_t)K, log_l, log_N,
                     plan.log_e, d.cidx, d.wtab, d.rtab, fr_arg<F>(Fd::reduce(inv_pow2<F>(log_l))), d.vals);
  hipLaunchKernelGGL(ver_colsum_kernel<F>, dim3(plan.sum_threads / 256), dim3(256), 0, st, M, d.vals, d.part);
  hipLaunchKernelGGL(ver_colsum_final_kernel<F>, dim3((uint32_t)l), dim3(64), 0, st, (uint32_t)l, plan.sum_cnt, d.part,
                     d.T);
  KZG_HIP(c, hipGetLastError());
  if ((rc = ver_commitment_sums(c, d.r, d.perm, d.off, n_comm, d.cpart, d.coef))) return rc;

  // ---- the MSMs: 2 x ns slice vectors over the proofs, T over the key, the weights over the commitments
  const uint32_t sb = plan.slice_bits, ns = plan.slices;
  std::vector<uint64_t> h_xy((size_t)(2 * ns + 2) * PW64);
  std::vector<uint8_t> h_inf(2 * ns + 2);
  for (uint32_t v = 0; v < 2 && rc == KZG_OK; ++v) {
    for (uint32_t s = 0; s < ns && rc == KZG_OK; ++s) {
      hipLaunchKernelGGL(ver_slice_kernel, k_grid, dim3(256), 0, st, (uint32_t)K, v ? d.s : d.r, s * sb, sb, d.slice);
      // the pipeline takes its own copy of the scalars in stream order (or holds the stream until they are consumed):
      // the next slice may overwrite d.slice
      const size_t idx = (size_t)v * ns + s;
      rc = commit_device(c, &pv, d.slice, &K, 1, K, h_xy.data() + idx * PW64, h_inf.data() + idx, /*drain=*/false);
    }
  }
  if (rc == KZG_OK)
    rc = commit_device(c, mono, d.T, &l, 1, l, h_xy.data() + (size_t)2 * ns * PW64, h_inf.data() + 2 * ns, false);
  if (rc == KZG_OK)
    rc = commit_device(c, cs.get(), d.coef, &n_comm, 1, n_comm, h_xy.data() + (size_t)(2 * ns + 1) * PW64,
                       h_inf.data() + 2 * ns + 1, false);
  const int rc2 = commit_flush(c);                    // also on an error: nothing may point at h_xy afterwards
  if (rc == KZG_OK) rc = rc2;
  if (rc) return rc;

  const XYZZ<C> R = recombine_slices<C>(h_xy.data(), h_inf.data(), ns, sb);
  const XYZZ<C> S = recombine_slices<C>(h_xy.data() + (size_t)ns * PW64, h_inf.data() + ns, ns, sb);
  XYZZ<C> Tp = host_point<C>(h_xy.data() + (size_t)2 * ns * PW64, h_inf[2 * ns]);
  Tp.y = Field<Fp>::neg(Tp.y);                        // -O = O: y = 0 stays 0
  const XYZZ<C> Cc = host_point<C>(h_xy.data() + (size_t)(2 * ns + 1) * PW64, h_inf[2 * ns + 1]);
  out_inf[0] = affine_to_words<C>(Ec<C>::to_affine(Ec<C>::add(Ec<C>::add(Cc, Tp), S)), reinterpret_cast<uint32_t*>(out_xy));
  out_inf[1] = affine_to_words<C>(Ec<C>::to_affine(R), reinterpret_cast<uint32_t*>(out_xy + PW64));
  return KZG_OK;
}

template <class F>
int commitment_sums_t(Ctx* c, const uint32_t* d_r, const uint32_t* d_perm, const uint32_t* d_off, size_t n_comm,
                      uint32_t* d_cpart, uint32_t* d_coef) {
  const uint32_t nsp = (uint32_t)ver_commsum_shares(n_comm);
  hipLaunchKernelGGL(ver_commsum_kernel<F>, dim3((uint32_t)n_comm, nsp), dim3(256), 0, c->stream, d_r, d_perm, d_off,
                     (uint32_t)n_comm, d_cpart);
  hipLaunchKernelGGL(ver_colsum_final_kernel<F>, dim3((uint32_t)n_comm), dim3(64), 0, c->stream, (uint32_t)n_comm, nsp,
                     d_cpart, d_coef);
  KZG_HIP(c, hipGetLastError());
  return KZG_OK;
}

template <class F>
int column_sums_t(Ctx* c, uint32_t cols, uint32_t cnt, const uint32_t* d_part, uint32_t* d_out) {
  hipLaunchKernelGGL(ver_colsum_final_kernel<F>, dim3(cols), dim3(64), 0, c->stream, cols, cnt, d_part, d_out);
  KZG_HIP(c, hipGetLastError());
  return KZG_OK;
}

}  // namespace

size_t ver_commsum_shares(size_t n_comm) { return ver_shares(n_comm); }
int ver_commitment_sums(Ctx* c, const uint32_t* d_r, const uint32_t* d_perm, const uint32_t* d_off, size_t n_comm,
                        uint32_t* d_cpart, uint32_t* d_coef) {
  return KZG_BY_FR(c, commitment_sums_t, c, d_r, d_perm, d_off, n_comm, d_cpart, d_coef);
}
int ver_column_sums(Ctx* c, uint32_t cols, uint32_t cnt, const uint32_t* d_part, uint32_t* d_out) {
  return KZG_BY_FR(c, column_sums_t, c, cols, cnt, d_part, d_out);
}

int verify_cosets(Ctx* c, const Srs* mono, uint32_t log_N, uint32_t log_l, const uint32_t* w_words,
                  const uint64_t* comm_xy, const uint8_t* comm_inf, size_t n_comm, const uint32_t* comm_idx,
                  const uint32_t* coset_idx, const uint64_t* values, const uint64_t* proof_xy, const uint8_t* proof_inf,
                  size_t K, const uint32_t* rho_words, uint64_t* out_xy, uint8_t* out_inf) {
  const VerClaims claims{values, nullptr, 0, nullptr};
  return KZG_BY_CURVE(c, verify_cosets_t, c, mono, log_N, log_l, w_words, comm_xy, comm_inf, n_comm, comm_idx, coset_idx,
                      claims, proof_xy, proof_inf, K, rho_words, out_xy, out_inf);
}
int verify_cosets_bytes(Ctx* c, const Srs* mono, uint32_t log_N, uint32_t log_l, const uint32_t* w_words,
                        const uint64_t* comm_xy, const uint8_t* comm_inf, size_t n_comm, const uint32_t* comm_idx,
                        const uint32_t* coset_idx, const uint8_t* cells, int bit_reversed, const uint64_t* proof_xy,
                        const uint8_t* proof_inf, size_t K, const uint32_t* rho_words, uint64_t* out_xy,
                        uint8_t* out_inf, uint8_t* out_status) {
  const VerClaims claims{nullptr, cells, bit_reversed, out_status};
  return KZG_BY_CURVE(c, verify_cosets_t, c, mono, log_N, log_l, w_words, comm_xy, comm_inf, n_comm, comm_idx, coset_idx,
                      claims, proof_xy, proof_inf, K, rho_words, out_xy, out_inf);
}

}  // namespace kzg
