// domain.hip -- all n KZG proofs on a domain H = {w^i, i < n} at once (Feist-Khovratovich, "Fast amortized KZG
// proofs", 2020: FK20), n = 2^log_n, on gfx950.  Each proof equals kzg_open's at z = w^i (kzg.py:122-159).
//
// For p(X) = sum_(j<n) c_j X^j and the monomial key s_t = [tau^t] G1, the quotient at z is sum_(m<n) z^m Q_m(X) with
//     pi(z) = sum_(m<n) h_m z^m,    h_m = sum_(j=m+1)^(n-1) c_j s_(j-m-1)    (h_(n-1) = 0),
// so pi(w^k), k < n, is the forward G1 DFT of h with the caller's root w.  h is a Toeplitz product, taken as a
// circular convolution of size N = 2n with the library's primitive N-th root omega (g^((r-1)/N), g the smallest
// primitive root of Fr -- any primitive root gives the same h):
//   table (once per key and n)   s^_u = s_(n-2-u) for u <= n-2, O above;  S = DFT_G1,N(s^)  ->  N compact affine points
//   per polynomial               c^ = DFT_Fr,N(c zero-padded)           (ntt_run_device, batched)
//                                u^_i = (c^_i / N) * S_i                 (one scalar times one fixed affine point)
//                                u = DFT_G1,N(u^) with omega^-1          (no 1/N: it rode on the scalars)
//                                h_m = u_(n-1+m), m <= n-2; h_(n-1) = O  (the linear convolution has 2n-2 < N terms)
//                                pi = DFT_G1,n(h) with w, natural order
// The G1 DFTs are radix 2, decimation in time, in XYZZ: a bit-reversed load (folded into the Hadamard pass and the
// extraction), one launch per level over every vector of the batch (g1_level_kernel, launch_levels: also the
// transform of lagrange.hip's key from a key), a pass to affine.  Butterfly t of a vector takes twiddle index
// k = t / (len / 2h): the lanes of a wave share a twiddle wherever >= 64 butterflies do, so the double-and-add
// branches are wave-uniform on all but the last six levels, and twiddle index 0 only adds and subtracts.
// Every kernel: vector stores only, no scratch, <= 256 VGPRs, one instantiation per curve.
#include <algorithm>
#include "internal.h"
#include "fr_util.h"
#include "g1_util.h"
#include "msm.h"
#include "srs_rec.h"
#include "g1_words.h"

namespace kzg {

namespace {

// compact affine record of the table: x[NW] y[NW] canonical words, flag word (bit 0: infinity), pad to 16 bytes
template <class C>
struct Tbl {
  static constexpr int NW = C::Fp::NW;
  static constexpr int WORDS = 2 * NW + 4;       // 20 (BN254) / 28 (BLS12-381) words
};

// the table point as XYZZ (Montgomery)
template <class C>
__device__ __forceinline__ XYZZ<C> ld_tbl(const uint32_t* tbl, size_t idx) {
  using Fd = Field<typename C::Fp>;
  constexpr int NW = C::Fp::NW;
  uint32_t w[Tbl<C>::WORDS];
  ld_words<Tbl<C>::WORDS>(tbl + idx * Tbl<C>::WORDS, w);
  Affine<C> a;
  a.inf = (w[2 * NW] & 1u) != 0;
  a.x = Fd::to_mont(Fd::from_words(w));
  a.y = Fd::to_mont(Fd::from_words(w + NW));
  return Ec<C>::from_affine(a);
}

template <class C>
__device__ __forceinline__ void st_tbl(uint32_t* tbl, size_t idx, const Affine<C>& a) {
  constexpr int NW = C::Fp::NW;
  uint32_t w[Tbl<C>::WORDS];
  w[2 * NW] = affine_to_words<C>(a, w) ? 1u : 0u;
#pragma unroll
  for (int q = 2 * NW + 1; q < Tbl<C>::WORDS; ++q) w[q] = 0;
  st_words<Tbl<C>::WORDS>(tbl + idx * Tbl<C>::WORDS, w);
}

// ---- kernels -----------------------------------------------------------------------------------------------------

// table input of sub-table j < l (l = 2^log_l, m = n/l, 2m = 2^log_mm): buf[j][bitrev_2m(u)] = s_((m-2-u) l + j)
// (window-0 record of the monomial key) for u <= m-2, O for u >= m-1.  l = 1 is open_domain's single table.
template <class C>
__global__ __launch_bounds__(128) void dom_load_key_kernel(const uint32_t* recs, uint32_t m, uint32_t log_l,
                                                           uint32_t log_mm, uint32_t* buf) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (1u << (log_l + log_mm))) return;
  const uint32_t j = g >> log_mm, u = g & ((1u << log_mm) - 1);
  Affine<C> a;
  if (u + 2 <= m) {
    a.inf = load_rec<C>(recs, ((size_t)(m - 2 - u) << log_l) + j, a.x, a.y) & 1u;
  } else {
    a.inf = true;
  }
  st_point<C>(buf, ((size_t)j << log_mm) + bitrev(u, log_mm), Ec<C>::from_affine(a));
}

// one radix-2 level of half-size h = 2^s over `nvec` vectors of 2^log_len points each (vector j at j << log_len):
// butterfly t pairs i0 = b*2h + k and i0 + h with twiddle root^(k * len/(2h)), k = t / (len/(2h)), b = t mod
// (len/(2h)).  root in Montgomery form.
template <class C>
__global__ __launch_bounds__(64) void g1_level_kernel(uint32_t* buf, uint32_t nvec, uint32_t log_len, uint32_t s,
                                                       FrArg root) {
  using Fr = typename C::Fr;
  using Frd = Field<Fr>;
  using Fd = Field<typename C::Fp>;
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lh = log_len - 1;
  if (g >= (nvec << lh)) return;
  const uint32_t j = g >> lh, t = g & ((1u << lh) - 1);
  const uint32_t lnb = lh - s;                            // log2 of the butterflies per twiddle
  const uint32_t k = t >> lnb, b = t & ((1u << lnb) - 1);
  const size_t base = (size_t)j << log_len;
  const size_t i0 = base + ((size_t)b << (s + 1)) + k, i1 = i0 + ((size_t)1 << s);
  XYZZ<C> B = ld_point<C>(buf, i1);
  if (k) {
    Fe<Fr> pw = arg_fe<Fr>(root), acc = Frd::one();
    for (uint32_t bits = k << lnb; bits; bits >>= 1) {
      if (bits & 1u) acc = Frd::mul(acc, pw);
      pw = Frd::sqr(pw);
    }
    uint32_t e[8];
    Frd::to_words(Frd::from_mont(acc), e);
    B = g1_mul_words<C>(B, e);
  }
  const XYZZ<C> A = ld_point<C>(buf, i0);
  st_point<C>(buf, i0, Ec<C>::add(A, B));
  B.y = Fd::neg(B.y);
  st_point<C>(buf, i1, Ec<C>::add(A, B));
}

// Hadamard step: buf[j][bitrev_N(i)] = (chat_j[i] * N^-1) * S_i -- chat: [nvec][N] canonical Fr words (the forward
// transform of the zero-padded coefficients), S: the table's points.  Double-and-add from the top bit (ec.h: exact
// for every input); the scalars differ per lane, so unlike the levels' twiddles the branches diverge.
template <class C>
__global__ __launch_bounds__(64) void dom_hadamard_kernel(const uint32_t* chat, const uint32_t* tbl, uint32_t nvec,
                                                          uint32_t log_nn, FrArg ninv, uint32_t* buf) {
  using Fr = typename C::Fr;
  using Frd = Field<Fr>;
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (nvec << log_nn)) return;
  const uint32_t j = g >> log_nn, i = g & ((1u << log_nn) - 1);
  const XYZZ<C> P = ld_tbl<C>(tbl, i);
  uint32_t e[8];                                                                      // standard * Montgomery
  Frd::to_words(Frd::reduce(Frd::mul(load_words<Fr>(chat + (size_t)g * 8), arg_fe<Fr>(ninv))), e);
  st_point<C>(buf, ((size_t)j << log_nn) + bitrev(i, log_nn), g1_mul_words<C>(P, e));
}

// extraction into the bit-reversed input of the final transform: dst[j][bitrev(u)] = src[j][m-1+u] for u <= m-2, O
// for m-1 <= u < 2^log_dst (src: [nvec][2^log_src], dst: [nvec][2^log_dst]).  open_domain: m = n, src 2n, dst n;
// open_cosets: m = n/l, src 2m, dst N/l >= m (O-padded).
template <class C>
__global__ __launch_bounds__(64) void dom_extract_kernel(const uint32_t* src, uint32_t nvec, uint32_t log_src,
                                                         uint32_t m, uint32_t log_dst, uint32_t* dst) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (nvec << log_dst)) return;
  const uint32_t j = g >> log_dst, u = g & ((1u << log_dst) - 1);
  const XYZZ<C> v = u + 2 <= m ? ld_point<C>(src, ((size_t)j << log_src) + m - 1 + u) : Ec<C>::infinity();
  st_point<C>(dst, ((size_t)j << log_dst) + bitrev(u, log_dst), v);
}

// ---- coset openings (open_cosets) ---------------------------------------------------------------------------------

// de-interleave: dst[v][j][s] = src[v][s l + j] for s < m, 0 for m <= s < 2m (src: [nvec][n] zero-padded canonical
// words, dst: [nvec][l][2m]) -- the inputs a^(j) of the l size-2m transforms
__global__ __launch_bounds__(256) void dom_deinterleave_kernel(const uint32_t* src, uint32_t nvec, uint32_t log_l,
                                                               uint32_t log_mm, uint32_t* dst) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t log_nn = log_l + log_mm;                  // l * 2m = 2n
  if (g >= (nvec << log_nn)) return;
  const uint32_t v = g >> log_nn, j = (g >> log_mm) & ((1u << log_l) - 1), s = g & ((1u << log_mm) - 1);
  uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
  if (s < (1u << (log_mm - 1))) {
    const uint4* p = reinterpret_cast<const uint4*>(src + (((size_t)v << (log_nn - 1)) + ((size_t)s << log_l) + j) * 8);
    lo = p[0];
    hi = p[1];
  }
  uint4* q = reinterpret_cast<uint4*>(dst + (size_t)g * 8);
  q[0] = lo;
  q[1] = hi;
}

// in place: x[i] <- x[i] * 2m^-1 (canonical words; ninv Montgomery) -- the scalars of the Hadamard sum
template <class F>
__global__ __launch_bounds__(256) void dom_scale_kernel(uint32_t* x, uint32_t count, FrArg ninv) {
  using Fd = Field<F>;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  uint32_t* p = x + (size_t)i * 8;
  store_words<F>(p, Fd::mul(load_words<F>(p), arg_fe<F>(ninv)));      // standard * Montgomery
}

// Hadamard sum over one group of G = 2^log_g sub-tables, Straus style (one doubling chain for the G terms):
//   r = sum_(jj < G) e_(j0 + jj) * S^(j0 + jj)_i,   j0 = grp G,   e_j = chat[v][j][i] (already scaled by 2m^-1)
// Thread (v, grp, i), i fastest.  With one group (G = l) r is u^_i itself and goes to dst[v][bitrev_2m(i)];
// otherwise to part[v][i][grp] for dom_group_sum_kernel.  A scalar word is re-read per bit (L1 hits: four lanes share
// a line) and a table point per addition, so the chain holds one accumulator and one addend; the bits differ per
// lane, so, as in dom_hadamard_kernel, the addition runs almost always.
template <class C>
__global__ __launch_bounds__(64) void dom_hadsum_kernel(const uint32_t* chat, const uint32_t* tbl, uint32_t nvec,
                                                        uint32_t log_l, uint32_t log_mm, uint32_t log_g,
                                                        uint32_t* dst) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t log_ng = log_l - log_g;
  if (g >= (nvec << (log_mm + log_ng))) return;
  const uint32_t i = g & ((1u << log_mm) - 1), grp = (g >> log_mm) & ((1u << log_ng) - 1), v = g >> (log_mm + log_ng);
  const uint32_t G = 1u << log_g, j0 = grp << log_g;
  const uint32_t* e0 = chat + (((((size_t)v << log_l) + j0) << log_mm) + i) * 8;     // e_j0; e_(j0+jj): + jj 2m
  const size_t estep = (size_t)8 << log_mm;
  const size_t t0 = ((size_t)j0 << log_mm) + i;                                    // S^(j0)_i; S^(j0+jj)_i: + jj 2m
  XYZZ<C> r = Ec<C>::infinity();
#pragma unroll 1
  for (int q = 7; q >= 0; --q) {
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
      r = Ec<C>::dbl(r);
#pragma unroll 1
      for (uint32_t jj = 0; jj < G; ++jj) {
        const uint32_t word = e0[jj * estep + q];
        if ((word >> bit) & 1u) r = Ec<C>::add(r, ld_tbl<C>(tbl, t0 + ((size_t)jj << log_mm)));
      }
    }
  }
  if (log_ng == 0)
    st_point<C>(dst, ((size_t)v << log_mm) + bitrev(i, log_mm), r);
  else
    st_point<C>(dst, ((((size_t)v << log_mm) + i) << log_ng) + grp, r);
}

// u^[v][bitrev_2m(i)] = sum_grp part[v][i][grp]
template <class C>
__global__ __launch_bounds__(64) void dom_group_sum_kernel(const uint32_t* part, uint32_t nvec, uint32_t log_mm,
                                                           uint32_t log_ng, uint32_t* dst) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (nvec << log_mm)) return;
  const uint32_t v = g >> log_mm, i = g & ((1u << log_mm) - 1);
  const size_t base = (size_t)g << log_ng;
  XYZZ<C> r = ld_point<C>(part, base);
#pragma unroll 1
  for (uint32_t k = 1; k < (1u << log_ng); ++k) r = Ec<C>::add(r, ld_point<C>(part, base + k));
  st_point<C>(dst, ((size_t)v << log_mm) + bitrev(i, log_mm), r);
}

// the values of every coset: dst[v][i][k] = src[v][i + k N/l] (src: [nvec][N] = DFT_N(p) with w, dst: [nvec][N/l][l])
__global__ __launch_bounds__(256) void dom_coset_values_kernel(const uint32_t* src, uint32_t nvec, uint32_t log_nn,
                                                               uint32_t log_l, uint32_t* dst) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (nvec << log_nn)) return;
  const uint32_t v = g >> log_nn, i = (g & ((1u << log_nn) - 1)) >> log_l, k = g & ((1u << log_l) - 1);
  const uint4* p =
      reinterpret_cast<const uint4*>(src + (((size_t)v << log_nn) + i + ((size_t)k << (log_nn - log_l))) * 8);
  uint4* q = reinterpret_cast<uint4*>(dst + (size_t)g * 8);
  q[0] = p[0];
  q[1] = p[1];
}

// table record i = buf[i] as compact affine
template <class C>
__global__ __launch_bounds__(64) void dom_finish_table_kernel(const uint32_t* buf, uint32_t count, uint32_t* tbl) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  st_tbl<C>(tbl, i, Ec<C>::to_affine(ld_point<C>(buf, i)));
}

// proofs: buf[i] as canonical affine words x[NW] y[NW] (kzg_open's point format) and a flag byte
template <class C>
__global__ __launch_bounds__(64) void dom_finish_proofs_kernel(const uint32_t* buf, uint32_t count, uint32_t* out_xy,
                                                               uint8_t* out_inf) {
  constexpr int NW = C::Fp::NW;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  uint32_t w[2 * NW];
  out_inf[i] = affine_to_words<C>(Ec<C>::to_affine(ld_point<C>(buf, i)), w) ? 1 : 0;
  st_words<2 * NW>(out_xy + (size_t)i * 2 * NW, w);
}

// ---- host side --------------------------------------------------------------------------------------------------

constexpr uint32_t DOM_MAX_LOG = 20;
// scratch of one call: chunks of vectors are sized to stay below this (kzg_ctx_set_tuning "open_domain_chunk" forces
// the chunk instead)
constexpr size_t DOM_SCRATCH_BYTES = (size_t)2 << 30;
constexpr uint32_t DOM_MAX_CHUNK = 1024;       // keeps every launch below 2^31 threads (N <= 2^21)

template <class F>
Fe<F> fr_pow_words(const Fe<F>& base, const uint32_t* e) {
  using Fd = Field<F>;
  Fe<F> acc = Fd::one();
  for (int k = 7; k >= 0; --k)
    for (int b = 31; b >= 0; --b) {
      acc = Fd::sqr(acc);
      if ((e[k] >> b) & 1u) acc = Fd::mul(acc, base);
    }
  return acc;
}

// the library's primitive 2^log_len-th root: g^((r-1) / 2^log_len), g = fr_generator (fr_util.h), Montgomery
template <class C>
Fe<typename C::Fr> dom_omega(uint32_t log_len) {
  using F = typename C::Fr;
  uint32_t e[8];
  for (int k = 0; k < 8; ++k) e[k] = F::PW[k];
  e[0] -= 1;                                           // r - 1 (r is odd)
  for (int k = 0; k < 8; ++k) {                        // >> log_len (< 32)
    const uint32_t hi = k + 1 < 8 ? e[k + 1] : 0u;
    e[k] = (e[k] >> log_len) | (log_len ? hi << (32 - log_len) : 0u);
  }
  return fr_pow_words<F>(fr_generator<C>(), e);
}

template <class C>
size_t xyzz_bytes() { return (size_t)4 * C::Fp::N * 4; }

// d_dst[j] = vector j of polys (lens[j] coefficients, `stride` elements apart) zero-padded to `len` elements, j < m
int stage_polys(Ctx* c, uint32_t* d_dst, size_t len, const uint32_t* polys, hipMemcpyKind kind, const size_t* lens,
                size_t stride, uint32_t m) {
  KZG_HIP(c, hipMemsetAsync(d_dst, 0, (size_t)m * len * 32, c->stream));
  for (uint32_t j = 0; j < m; ++j)
    if (lens[j])
      KZG_HIP(c, hipMemcpyAsync(d_dst + (size_t)j * len * 8, polys + j * stride * 8, lens[j] * 32, kind, c->stream));
  return KZG_OK;
}

// The tail of a chunk of `nvec` vectors: h from u = d_big (dom_extract_kernel), pi = DFT_G1(h) with `root` in d_small,
// the 2^log_dst proofs per vector as affine words in d_oxy / d_oinf and on their way to the host (vector 0 of the
// chunk is vector j0 of the call).
template <class C>
int finish_proofs(Ctx* c, const uint32_t* d_big, uint32_t nvec, uint32_t log_src, uint32_t m, uint32_t log_dst,
                  uint32_t* d_small, const Fe<typename C::Fr>& root, uint32_t* d_oxy, uint8_t* d_oinf, size_t j0,
                  uint64_t* out_xy, uint8_t* out_inf) {
  const size_t count = (size_t)nvec << log_dst, pt_words = 2 * C::Fp::NW;
  const uint32_t blocks = (uint32_t)((count + 63) / 64);
  hipLaunchKernelGGL(dom_extract_kernel<C>, dim3(blocks), dim3(64), 0, c->stream, d_big, nvec, log_src, m, log_dst,
                     d_small);
  KZG_HIP(c, hipGetLastError());
  int rc = launch_levels(c, d_small, nvec, log_dst, fr_arg<typename C::Fr>(root));
  if (rc) return rc;
  hipLaunchKernelGGL(dom_finish_proofs_kernel<C>, dim3(blocks), dim3(64), 0, c->stream, d_small, (uint32_t)count,
                     d_oxy, d_oinf);
  KZG_HIP(c, hipGetLastError());
  KZG_HIP(c, hipMemcpyAsync(out_xy + (j0 << log_dst) * pt_words / 2, d_oxy, count * pt_words * 4,
                            hipMemcpyDeviceToHost, c->stream));
  KZG_HIP(c, hipMemcpyAsync(out_inf + (j0 << log_dst), d_oinf, count, hipMemcpyDeviceToHost, c->stream));
  return KZG_OK;
}

}  // namespace

// A table of one monomial key, one domain size n and one coset size l = 2^log_l (1 for kzg_domain_table_create):
// l sub-tables [l][2m], m = n/l, of compact affine points S^(j) = DFT_G1,2m(s^(j)) with root omega_2m -- 2n points
// for every l.
struct DomainTable {
  int curve = 0;
  uint32_t log_n = 0;
  uint32_t log_l = 0;
  size_t n = 0;
  uint32_t* d_tbl = nullptr;
};

namespace {

template <class C>
int domain_table_t(Ctx* c, const Srs* mono, uint32_t log_n, uint32_t log_l, const char* fn, const char* span,
                   DomainTable** out) {
  using F = typename C::Fr;
  if (mono->curve != c->curve) return set_err(c, KZG_ERR_ARG, "SRS belongs to another curve");
  if (mono->basis != SRS_MONOMIAL) return set_err(c, KZG_ERR_ARG, (std::string(fn) + ": the key must be monomial").c_str());
  if (log_n < 1 || log_n > DOM_MAX_LOG) return set_err(c, KZG_ERR_ARG, (std::string(fn) + ": log_n must be in [1, 20]").c_str());
  if (log_l >= log_n) return set_err(c, KZG_ERR_ARG, (std::string(fn) + ": log_l must be in [0, log_n - 1]").c_str());
  const uint32_t n = 1u << log_n, nn = 2 * n;
  const uint32_t m = n >> log_l, log_mm = log_n - log_l + 1;
  if (mono->n < n) return set_err(c, KZG_ERR_ARG, (std::string(fn) + ": monomial key shorter than the domain").c_str());
  const Fe<F> omega = dom_omega<C>(log_mm);
  if (!primitive_root<F>(omega, log_mm)) return set_err(c, KZG_ERR_ARG, (std::string(fn) + ": no 2m-th root").c_str());
  DomainTablePtr t(new DomainTable());
  t->curve = c->curve;
  t->log_n = log_n;
  t->log_l = log_l;
  t->n = n;
  DevTmp<uint32_t> d_buf;
  if (hipMalloc(reinterpret_cast<void**>(&t->d_tbl), (size_t)nn * Tbl<C>::WORDS * 4) != hipSuccess ||
      d_buf.alloc((size_t)nn * xyzz_bytes<C>()) != hipSuccess)
    return set_err(c, KZG_ERR_ALLOC, "hipMalloc(domain table)");
  {
    ProfScope ps(c, span);
    hipLaunchKernelGGL(dom_load_key_kernel<C>, dim3((nn + 127) / 128), dim3(128), 0, c->stream, mono->recs, m, log_l,
                       log_mm, d_buf.get());
    if (int rc = launch_levels(c, d_buf, 1u << log_l, log_mm, fr_arg<F>(omega))) return rc;
    hipLaunchKernelGGL(dom_finish_table_kernel<C>, dim3((nn + 63) / 64), dim3(64), 0, c->stream, d_buf.get(), nn,
                       t->d_tbl);
    KZG_HIP(c, hipGetLastError());
  }
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  *out = t.release();
  return KZG_OK;
}

// polys: device coefficient vectors (host_polys: host memory, staged per vector); outputs in host memory
template <class C>
int open_domain_t(Ctx* c, const DomainTable* t, const uint32_t* polys, bool host_polys, const size_t* lens, size_t b,
                  size_t stride, const uint32_t* w_words, uint64_t* out_xy, uint8_t* out_inf, uint64_t* eval_out) {
  using F = typename C::Fr;
  using Fd = Field<F>;
  using Fp = typename C::Fp;
  if (t->curve != c->curve) return set_err(c, KZG_ERR_ARG, "domain table belongs to another curve");
  if (t->log_l) return set_err(c, KZG_ERR_ARG, "kzg_open_domain: a coset table (l > 1) needs kzg_open_cosets");
  const uint32_t log_n = t->log_n, log_nn = log_n + 1;
  const size_t n = t->n, nn = 2 * n;
  if (!primitive_root<F>(mont_from_words<F>(w_words), log_n))
    return set_err(c, KZG_ERR_ARG, "kzg_open_domain: w is not a primitive n-th root of unity");
  for (size_t j = 0; j < b; ++j) {
    if (lens[j] > n) return set_err(c, KZG_ERR_DEGREE, "polynomial longer than the domain");
    if (lens[j] > stride) return set_err(c, KZG_ERR_ARG, "kzg_open_domain: lens[j] > stride");
  }
  if (b == 0) return KZG_OK;
  // per vector: the size-N XYZZ buffer (later the proofs' output), the size-n XYZZ buffer, N Fr elements
  const size_t per_vec = nn * xyzz_bytes<C>() + n * xyzz_bytes<C>() + nn * 32;
  size_t chunk = c->tune_open_domain_chunk > 0 ? (size_t)c->tune_open_domain_chunk
                                               : std::max<size_t>(1, DOM_SCRATCH_BYTES / per_vec);
  chunk = std::min<size_t>({chunk, b, DOM_MAX_CHUNK});
  int rc = ensure_buf(c, c->dom_tmp, chunk * per_vec);
  if (rc) return rc;
  uint32_t* d_big = static_cast<uint32_t*>(c->dom_tmp.p);                              // [chunk][N] XYZZ
  uint32_t* d_small = d_big + chunk * nn * 4 * Fp::N;                                  // [chunk][n] XYZZ
  uint32_t* d_fr = d_small + chunk * n * 4 * Fp::N;                                    // [chunk][N] Fr words
  uint32_t* d_oxy = d_big;                                                             // [chunk][n][2 NW] words
  uint8_t* d_oinf = reinterpret_cast<uint8_t*>(d_big + chunk * n * 2 * Fp::NW);        // [chunk][n] flags

  const Fe<F> omega = dom_omega<C>(log_nn);
  const Fe<F> omega_inv = Fd::inv(omega);
  uint32_t omega_words[8];
  words_from_mont<F>(omega, omega_words);
  const Fe<F> ninv = Fd::reduce(inv_pow2<F>(log_nn));
  const Fe<F> w = mont_from_words<F>(w_words);
  const hipMemcpyKind kind = host_polys ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;

  ProfScope ps(c, "open_domain");
  for (size_t j0 = 0; j0 < b; j0 += chunk) {
    const uint32_t m = (uint32_t)std::min(chunk, b - j0);
    // c^ = DFT_N(c), zero-padded
    if ((rc = stage_polys(c, d_fr, nn, polys + j0 * stride * 8, kind, lens + j0, stride, m))) return rc;
    if ((rc = ntt_run_device(c, d_fr, log_nn, omega_words, 0, m))) return rc;
    const size_t big = (size_t)m * nn, small = (size_t)m * n;
    hipLaunchKernelGGL(dom_hadamard_kernel<C>, dim3((uint32_t)((big + 63) / 64)), dim3(64), 0, c->stream, d_fr,
                       t->d_tbl, m, log_nn, fr_arg<F>(ninv), d_big);
    KZG_HIP(c, hipGetLastError());
    if ((rc = launch_levels(c, d_big, m, log_nn, fr_arg<F>(omega_inv)))) return rc;
    if ((rc = finish_proofs<C>(c, d_big, m, log_nn, (uint32_t)n, log_n, d_small, w, d_oxy, d_oinf, j0, out_xy,
                               out_inf)))
      return rc;
    if (eval_out) {   // y = DFT_n(c) with w, in the Fr buffer the Hadamard step has consumed
      if ((rc = stage_polys(c, d_fr, n, polys + j0 * stride * 8, kind, lens + j0, stride, m))) return rc;
      if ((rc = ntt_run_device(c, d_fr, log_n, w_words, 0, m))) return rc;
      KZG_HIP(c, hipMemcpyAsync(eval_out + j0 * n * 4, d_fr, small * 32, hipMemcpyDeviceToHost, c->stream));
    }
    // the next chunk overwrites the buffers the copies read
    KZG_HIP(c, hipStreamSynchronize(c->stream));
  }
  return KZG_OK;
}

// Coset FK20: N/l proofs per vector, coset i = {w^(i + k N/l), k < l}.  The l Toeplitz products of size m = n/l are
// summed before one inverse G1 DFT (the sum of the Hadamard products is the transform of the sum):
//   c^(j) = DFT_Fr,2m(a^(j)),  a^(j)_s = c_(s l + j)          one batched NTT over l vectors per polynomial
//   u^_i  = sum_j (c^(j)_i / 2m) S^(j)_i                      dom_hadsum_kernel (+ dom_group_sum_kernel)
//   u     = DFT_G1,2m(u^) with omega^-1;  h_u = u_(m-1+u) (u <= m-2), O up to N/l
//   pi    = DFT_G1,N/l(h) with w^l
// Buffers of one chunk of vectors (every region a multiple of 32 bytes per vector):
//   big [2m] XYZZ, part [2m][l/G] XYZZ (only when G < l), small [N/l] XYZZ, fr [l][2m] Fr, stage [n] Fr,
//   (values) val [N] Fr, valt [N] Fr, (proofs) oxy [N/l][2 NW] words, oinf [N/l] bytes.
template <class C>
int open_cosets_t(Ctx* c, const DomainTable* t, const uint32_t* polys, bool host_polys, const size_t* lens, size_t b,
                  size_t stride, uint32_t log_N, const uint32_t* w_words, uint64_t* out_xy, uint8_t* out_inf,
                  uint64_t* eval_out) {
  using F = typename C::Fr;
  using Fd = Field<F>;
  using Fp = typename C::Fp;
  if (t->curve != c->curve) return set_err(c, KZG_ERR_ARG, "domain table belongs to another curve");
  const uint32_t log_n = t->log_n, log_l = t->log_l;
  if (log_N < log_n || log_N > std::min<uint32_t>(log_n + 2, DOM_MAX_LOG + 1))
    return set_err(c, KZG_ERR_ARG, "kzg_open_cosets: log_N must be in [log_n, min(log_n + 2, 21)]");
  if (!primitive_root<F>(mont_from_words<F>(w_words), log_N))
    return set_err(c, KZG_ERR_ARG, "kzg_open_cosets: w is not a primitive N-th root of unity");
  const size_t n = t->n;
  for (size_t j = 0; j < b; ++j) {
    if (lens[j] > n) return set_err(c, KZG_ERR_DEGREE, "polynomial longer than the domain table");
    if (lens[j] > stride) return set_err(c, KZG_ERR_ARG, "kzg_open_cosets: lens[j] > stride");
  }
  if (b == 0) return KZG_OK;
  const uint32_t m = (uint32_t)(n >> log_l), log_mm = log_n - log_l + 1, mm = 2 * m;
  const uint32_t log_L = log_N - log_l;                      // N/l proofs per vector
  const size_t L = (size_t)1 << log_L, NN = (size_t)1 << log_N;
  // Straus group: G = min(l, 16) terms share a doubling chain, fewer while that would leave < 2^16 threads busy
  // (kzg_ctx_set_tuning "open_cosets_group" fixes log_g = value - 1 instead, clipped to log_l)
  uint32_t log_g = std::min<uint32_t>(log_l, 4);
  if (c->tune_open_cosets_group > 0)
    log_g = std::min<uint32_t>(log_l, (uint32_t)c->tune_open_cosets_group - 1);
  else
    while (log_g && ((std::min<size_t>(b, 64) * 2 * n) >> log_g) < ((size_t)1 << 16)) --log_g;
  const uint32_t log_ng = log_l - log_g;
  const size_t xb = xyzz_bytes<C>(), pt_words = 2 * Fp::NW;
  const size_t part_pts = log_ng ? (size_t)mm << log_ng : 0;
  const size_t oxy_bytes = (L * pt_words * 4 + 31) / 32 * 32, oinf_bytes = (L + 31) / 32 * 32;
  const size_t per_vec = (mm + part_pts + L) * xb + (2 * n + n) * 32 + (eval_out ? 2 * NN * 32 : 0) + oxy_bytes +
                         oinf_bytes;
  size_t chunk = c->tune_open_cosets_chunk > 0 ? (size_t)c->tune_open_cosets_chunk
                                               : std::max<size_t>(1, DOM_SCRATCH_BYTES / per_vec);
  chunk = std::min<size_t>({chunk, b, DOM_MAX_CHUNK});
  int rc = ensure_buf(c, c->dom_tmp, chunk * per_vec + 9 * 256);
  if (rc) return rc;
  uint8_t* base = static_cast<uint8_t*>(c->dom_tmp.p);
  auto region = [&](size_t per) { uint8_t* p = base; base += (chunk * per + 255) / 256 * 256; return p; };
  uint32_t* d_big = reinterpret_cast<uint32_t*>(region(mm * xb));                 // [chunk][2m] XYZZ
  uint32_t* d_part = reinterpret_cast<uint32_t*>(region(part_pts * xb));          // [chunk][2m][l/G] XYZZ
  uint32_t* d_small = reinterpret_cast<uint32_t*>(region(L * xb));                // [chunk][N/l] XYZZ
  uint32_t* d_fr = reinterpret_cast<uint32_t*>(region(2 * n * 32));               // [chunk][l][2m] Fr
  uint32_t* d_stage = reinterpret_cast<uint32_t*>(region(n * 32));                // [chunk][n] Fr
  uint32_t* d_val = reinterpret_cast<uint32_t*>(region(eval_out ? NN * 32 : 0));  // [chunk][N] Fr
  uint32_t* d_valt = reinterpret_cast<uint32_t*>(region(eval_out ? NN * 32 : 0)); // [chunk][N/l][l] Fr
  uint32_t* d_oxy = reinterpret_cast<uint32_t*>(region(oxy_bytes));               // [chunk][N/l][2 NW] words
  uint8_t* d_oinf = region(oinf_bytes);                                           // [chunk][N/l] flags

  const Fe<F> omega = dom_omega<C>(log_mm);
  const Fe<F> omega_inv = Fd::inv(omega);
  uint32_t omega_words[8];
  words_from_mont<F>(omega, omega_words);
  const Fe<F> mminv = Fd::reduce(inv_pow2<F>(log_mm));
  Fe<F> wl = mont_from_words<F>(w_words);                                         // w^l: the final transform's root
  for (uint32_t q = 0; q < log_l; ++q) wl = Fd::sqr(wl);
  const hipMemcpyKind kind = host_polys ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;

  ProfScope ps(c, "open_cosets");
  for (size_t j0 = 0; j0 < b; j0 += chunk) {
    const uint32_t mv = (uint32_t)std::min(chunk, b - j0);
    // the coefficients, zero-padded to n, then de-interleaved into the l zero-padded transforms of size 2m
    if ((rc = stage_polys(c, d_stage, n, polys + j0 * stride * 8, kind, lens + j0, stride, mv))) return rc;
    const size_t frs = (size_t)mv * 2 * n;
    hipLaunchKernelGGL(dom_deinterleave_kernel, dim3((uint32_t)((frs + 255) / 256)), dim3(256), 0, c->stream, d_stage,
                       mv, log_l, log_mm, d_fr);
    KZG_HIP(c, hipGetLastError());
    if ((rc = ntt_run_device(c, d_fr, log_mm, omega_words, 0, mv << log_l))) return rc;
    hipLaunchKernelGGL(dom_scale_kernel<F>, dim3((uint32_t)((frs + 255) / 256)), dim3(256), 0, c->stream, d_fr,
                       (uint32_t)frs, fr_arg<F>(mminv));
    KZG_HIP(c, hipGetLastError());
    const size_t hs = (size_t)mv * mm << log_ng, big = (size_t)mv * mm;
    hipLaunchKernelGGL(dom_hadsum_kernel<C>, dim3((uint32_t)((hs + 63) / 64)), dim3(64), 0, c->stream, d_fr,
                       t->d_tbl, mv, log_l, log_mm, log_g, log_ng ? d_part : d_big);
    KZG_HIP(c, hipGetLastError());
    if (log_ng) {
      hipLaunchKernelGGL(dom_group_sum_kernel<C>, dim3((uint32_t)((big + 63) / 64)), dim3(64), 0, c->stream, d_part,
                         mv, log_mm, log_ng, d_big);
      KZG_HIP(c, hipGetLastError());
    }
    if ((rc = launch_levels(c, d_big, mv, log_mm, fr_arg<F>(omega_inv)))) return rc;
    if ((rc = finish_proofs<C>(c, d_big, mv, log_mm, m, log_L, d_small, wl, d_oxy, d_oinf, j0, out_xy, out_inf)))
      return rc;
    if (eval_out) {   // y = DFT_N(c) with w, regrouped per coset
      KZG_HIP(c, hipMemsetAsync(d_val, 0, (size_t)mv * NN * 32, c->stream));
      KZG_HIP(c, hipMemcpy2DAsync(d_val, NN * 32, d_stage, n * 32, n * 32, mv, hipMemcpyDeviceToDevice, c->stream));
      if ((rc = ntt_run_device(c, d_val, log_N, w_words, 0, mv))) return rc;
      const size_t vals = (size_t)mv * NN;
      hipLaunchKernelGGL(dom_coset_values_kernel, dim3((uint32_t)((vals + 255) / 256)), dim3(256), 0, c->stream, d_val,
                         mv, log_N, log_l, d_valt);
      KZG_HIP(c, hipGetLastError());
      KZG_HIP(c, hipMemcpyAsync(eval_out + j0 * NN * 4, d_valt, vals * 32, hipMemcpyDeviceToHost, c->stream));
    }
    // the next chunk overwrites the buffers the copies read
    KZG_HIP(c, hipStreamSynchronize(c->stream));
  }
  return KZG_OK;
}

}  // namespace

// every level of the transform of `nvec` vectors of 2^log_len points (bit-reversed in, natural out), root Montgomery
int launch_levels(Ctx* c, uint32_t* buf, uint32_t nvec, uint32_t log_len, const FrArg& root) {
  const size_t threads = (size_t)nvec << (log_len - 1);
  const dim3 blocks((uint32_t)((threads + 63) / 64));
  for (uint32_t lv = 0; lv < log_len; ++lv) {
    if (c->curve == 0)
      hipLaunchKernelGGL(g1_level_kernel<Bn254>, blocks, dim3(64), 0, c->stream, buf, nvec, log_len, lv, root);
    else
      hipLaunchKernelGGL(g1_level_kernel<Bls12_381>, blocks, dim3(64), 0, c->stream, buf, nvec, log_len, lv, root);
  }
  KZG_HIP(c, hipGetLastError());
  return KZG_OK;
}
int domain_table_create(Ctx* c, const Srs* mono, uint32_t log_n, DomainTable** out) {
  return KZG_BY_CURVE(c, domain_table_t, c, mono, log_n, 0, "kzg_domain_table_create", "domain_table", out);
}
int coset_table_create(Ctx* c, const Srs* mono, uint32_t log_n, uint32_t log_l, DomainTable** out) {
  return KZG_BY_CURVE(c, domain_table_t, c, mono, log_n, log_l, "kzg_coset_table_create", "coset_table", out);
}
void domain_table_free(DomainTable* t) {
  if (!t) return;
  hipFree(t->d_tbl);
  delete t;
}
size_t domain_table_size(const DomainTable* t) { return t ? t->n : 0; }
int open_domain(Ctx* c, const DomainTable* t, const uint32_t* polys, bool host_polys, const size_t* lens, size_t b,
                size_t stride, const uint32_t* w_words, uint64_t* out_xy, uint8_t* out_inf, uint64_t* eval_out) {
  return KZG_BY_CURVE(c, open_domain_t, c, t, polys, host_polys, lens, b, stride, w_words, out_xy, out_inf, eval_out);
}
int open_cosets(Ctx* c, const DomainTable* t, const uint32_t* polys, bool host_polys, const size_t* lens, size_t b,
                size_t stride, uint32_t log_N, const uint32_t* w_words, uint64_t* out_xy, uint8_t* out_inf,
                uint64_t* eval_out) {
  return KZG_BY_CURVE(c, open_cosets_t, c, t, polys, host_polys, lens, b, stride, log_N, w_words, out_xy, out_inf,
                      eval_out);
}

}  // namespace kzg
