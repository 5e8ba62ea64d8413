// verify_points.hip -- bulk verification at arbitrary points on gfx950: K single-point claims folded into the two G1
// points of ONE pairing equation, on a kernel of its own instead of the commit pipeline.
//
// Claim k: the polynomial of commitment C[c_k] takes the value y_k at z_k (any element of Fr), proof pi_k.  With the
// weights r_k = rho^(k+1):
//     L = sum_j (sum_(k: c_k = j) r_k) C[j]  -  (sum_k r_k y_k) G1  +  sum_k (r_k z_k) pi_k
//     R = sum_k r_k pi_k                           accept iff e(L, G2) = e(R, [tau] G2)
//
//   weights   rho^e from the two-level table of fr_util.h; vpt_weights_kernel writes r_k and s_k = r_k z_k as
//             canonical scalars and per-thread partial sums of -r_k y_k, which verify.hip's column sum folds into the
//             scalar of one extra "commitment", the generator; the per-commitment sums of r_k are verify.hip's
//             (a counting sort of the indices on the host, ver_commitment_sums)
//   ladder    vpt_ladder_kernel: ONE lane per (point, scalar) pair -- r_k pi_k, s_k pi_k and coef_j C_j for the
//             n_comm + 1 short terms.  A lane first writes 1P .. 8P (XYZZ) into its column of a table in the call's
//             scratch buffer, [multiple][16-byte piece][lane] so that the loads of a wave's lanes with equal digits
//             fall into the same lines.  The scalar plus 0x88..8 read nibble by nibble is its signed radix-16 form
//             (digit = nibble - 8 in [-8, 7], one more digit 0 / 1 from the carry): 64 windows of four doublings and at
//             most one full addition of +-|d| P.  Lanes differ only in the digit (its sign, d = 0) and in infinity.
//   sum       the workgroup adds its 256 results through LDS with Ec::add (two lanes may hold P and P, P and -P,
//             or O) and writes one partial point; a segment of the grid (a multiple of 256 lanes) feeds one output, so
//             a workgroup never mixes two.  vpt_fold_kernel adds the partial points of each of the three outputs; the
//             host adds the commitment term to the s-term and converts to affine, as verify_cosets_t ends.
// Launches cover at most VPT_LAUNCH_BLOCKS workgroups each (the workgroups split evenly over the fewest such launches),
// which bounds the table (1664 bytes per lane on BLS12-381).
#include <cstring>
#include <algorithm>
#include <vector>
#include "internal.h"
#include "fr_util.h"
#include "g1_util.h"
#include "msm.h"
#include "g1_words.h"
#include "srs_rec.h"
#include "ver_layout.h"

namespace kzg {

namespace {

constexpr uint32_t VPT_TB = 256;                         // lanes per workgroup of the ladder and of the fold
constexpr uint32_t VPT_LAUNCH_BLOCKS = 512;              // workgroups per ladder launch: two per CU
constexpr uint32_t VPT_WEIGHT_THREADS = 1u << 14;        // vpt_weights_kernel: threads, one partial sum each
constexpr int VPT_TABLE = 8;                             // multiples 1P .. 8P per lane

// r_k = rho^(k+1), s_k = r_k z_k (canonical words) and ypart[t] = -sum of r_k y_k over the claims of thread t
template <class F>
__global__ __launch_bounds__(256) void vpt_weights_kernel(uint32_t K, const uint32_t* rtab, const uint32_t* z,
                                                          const uint32_t* y, uint32_t* r_out, uint32_t* s_out,
                                                          uint32_t* ypart) {
  using Fd = Field<F>;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
  Fe<F> acc = Fd::zero();
  for (uint32_t k = t; k < K; k += step) {
    const Fe<F> r = fr_pow_lookup<F>(rtab, k + 1);                        // Montgomery: a product with a standard
    store_words<F>(r_out + (size_t)k * 8, Fd::from_mont(r));              // value is in standard form
    store_words<F>(s_out + (size_t)k * 8, Fd::mul(r, load_words<F>(z + (size_t)k * 8)));
    acc = Fd::sub(acc, Fd::mul(r, load_words<F>(y + (size_t)k * 8)));
  }
  store_words<F>(ypart + (size_t)t * 8, acc);
}

// the lanes of the ladder: blocks [0, nb) the pairs (r_k, pi_k), [nb, 2 nb) the pairs (s_k, pi_k), the rest the short
// terms (coef_j, C_j), j < n_short
struct VptGrid {
  uint32_t K, nb, n_short;
};

// piece q (16 bytes) of multiple e of the lane `slot`: a wave's lanes are adjacent
__device__ __forceinline__ size_t vpt_tab_at(int pieces, uint32_t slots, int e, int q, uint32_t slot) {
  return ((size_t)(e * pieces + q)) * slots + slot;
}
template <class C>
__device__ __forceinline__ void vpt_tab_store(uint4* tab, uint32_t slots, uint32_t slot, int e, const XYZZ<C>& v) {
  constexpr int N = C::Fp::N;
  uint32_t w[4 * N];
#pragma unroll
  for (int j = 0; j < N; ++j) { w[j] = v.x.l[j]; w[N + j] = v.y.l[j]; w[2 * N + j] = v.zz.l[j]; w[3 * N + j] = v.zzz.l[j]; }
#pragma unroll
  for (int q = 0; q < N; ++q)
    tab[vpt_tab_at(N, slots, e, q, slot)] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
}
template <class C>
__device__ __forceinline__ XYZZ<C> vpt_tab_load(const uint4* tab, uint32_t slots, uint32_t slot, int e) {
  constexpr int N = C::Fp::N;
  uint32_t w[4 * N];
#pragma unroll
  for (int q = 0; q < N; ++q) {
    const uint4 v = tab[vpt_tab_at(N, slots, e, q, slot)];
    w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
  }
  XYZZ<C> r;
#pragma unroll
  for (int j = 0; j < N; ++j) { r.x.l[j] = w[j]; r.y.l[j] = w[N + j]; r.zz.l[j] = w[2 * N + j]; r.zzz.l[j] = w[3 * N + j]; }
  return r;
}

// the sum of the workgroup's 256 points in thread 0: in every round s = 128 .. 1 the upper half of the live lanes
// (s <= t < 2s) parks its points in LDS ([limb][lane], 128 lanes) and lane t - s adds them.  The full addition: the two
// lanes of a pair may hold P and P, P and -P, or O.
template <class C>
__device__ __forceinline__ XYZZ<C> vpt_block_sum(XYZZ<C> acc, uint32_t* sh) {
  constexpr int N = C::Fp::N;
  const uint32_t tid = threadIdx.x;
#pragma unroll 1
  for (uint32_t s = VPT_TB / 2; s >= 1; s >>= 1) {
    if (tid >= s && tid < 2 * s) {
      uint32_t* p = sh + (tid - s);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        p[(size_t)j * (VPT_TB / 2)] = acc.x.l[j];
        p[(size_t)(N + j) * (VPT_TB / 2)] = acc.y.l[j];
        p[(size_t)(2 * N + j) * (VPT_TB / 2)] = acc.zz.l[j];
        p[(size_t)(3 * N + j) * (VPT_TB / 2)] = acc.zzz.l[j];
      }
    }
    __syncthreads();
    if (tid < s) {
      const uint32_t* p = sh + tid;
      XYZZ<C> o;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        o.x.l[j] = p[(size_t)j * (VPT_TB / 2)];
        o.y.l[j] = p[(size_t)(N + j) * (VPT_TB / 2)];
        o.zz.l[j] = p[(size_t)(2 * N + j) * (VPT_TB / 2)];
        o.zzz.l[j] = p[(size_t)(3 * N + j) * (VPT_TB / 2)];
      }
      acc = Ec<C>::add(acc, o);
    }
    __syncthreads();
  }
  return acc;
}

// word k of e[8] for a k only known at run time: a chain of selects, no indexed register array
__device__ __forceinline__ uint32_t vpt_word(const uint32_t* e, int k) {
  uint32_t w = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) w = k == j ? e[j] : w;
  return w;
}

// partial[block0 + blockIdx.x] = the sum over the workgroup's lanes of scalar * point.  tab: VPT_TABLE * N pieces of
// `slots` = gridDim.x * 256 uint4 each.
template <class C>
__global__ __launch_bounds__(VPT_TB) void vpt_ladder_kernel(VptGrid g, uint32_t block0, const uint32_t* proof_recs,
                                                            const uint32_t* short_recs, const uint32_t* r,
                                                            const uint32_t* s, const uint32_t* coef, uint4* tab,
                                                            uint32_t* partial) {
  using Fd = Field<typename C::Fp>;
  constexpr int N = C::Fp::N;
  __shared__ uint32_t sh[4 * N * (VPT_TB / 2)];
  const uint32_t b = block0 + blockIdx.x, slots = gridDim.x * VPT_TB, slot = blockIdx.x * VPT_TB + threadIdx.x;
  const uint32_t seg = b < g.nb ? 0u : b < 2 * g.nb ? 1u : 2u;
  const uint32_t idx = (b - seg * g.nb) * VPT_TB + threadIdx.x;
  const bool live = idx < (seg == 2 ? g.n_short : g.K);
  XYZZ<C> acc = Ec<C>::infinity();
  if (live) {
    Affine<C> a;
    a.inf = load_rec<C>(seg == 2 ? short_recs : proof_recs, idx, a.x, a.y) & 1u;
    uint32_t e[8];
    ld_words<8>((seg == 0 ? r : seg == 1 ? s : coef) + (size_t)idx * 8, e);
    // 1P .. 8P: one doubling and six additions.  The full addition, not madd: with madd's affine doubling inlined in
    // this loop the register allocator spills (thousands of bytes of scratch), and six additions weigh nothing
    // beside the ladder.
    XYZZ<C> m = Ec<C>::from_affine(a);
    vpt_tab_store<C>(tab, slots, slot, 0, m);
    if (!a.inf) m = Ec<C>::dbl_affine(a.x, a.y);
    vpt_tab_store<C>(tab, slots, slot, 1, m);
#pragma unroll 1
    for (int q = 2; q < VPT_TABLE; ++q) {
      m = Ec<C>::add(m, Ec<C>::from_affine(a));
      vpt_tab_store<C>(tab, slots, slot, q, m);
    }
    // e + 0x88..8: nibble w of the sum minus 8 is the signed digit of window w; the carry out is digit 64 (0 or 1)
    uint32_t carry = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint64_t t = (uint64_t)e[k] + 0x88888888u + carry;
      e[k] = (uint32_t)t;
      carry = (uint32_t)(t >> 32);
    }
    if (carry) acc = Ec<C>::from_affine(a);
#pragma unroll 1
    for (int w = 63; w >= 0; --w) {
#pragma unroll 1
      for (int d = 0; d < 4; ++d) acc = Ec<C>::dbl(acc);
      const int digit = (int)((vpt_word(e, w >> 3) >> ((w & 7) * 4)) & 15u) - 8;
      if (digit != 0) {
        XYZZ<C> t = vpt_tab_load<C>(tab, slots, slot, (digit < 0 ? -digit : digit) - 1);
        if (digit < 0) t.y = Fd::neg(t.y);                   // -O = O: y = 0 stays 0
        acc = Ec<C>::add(acc, t);
      }
    }
  }
  acc = vpt_block_sum<C>(acc, sh);
  if (threadIdx.x == 0) st_point<C>(partial, b, acc);
}

// out[o] = the sum of the partial points of output o: blocks [0, nb), [nb, 2 nb), [2 nb, 2 nb + nc)
template <class C>
__global__ __launch_bounds__(VPT_TB) void vpt_fold_kernel(uint32_t nb, uint32_t nc, const uint32_t* partial,
                                                          uint32_t* out) {
  constexpr int N = C::Fp::N;
  __shared__ uint32_t sh[4 * N * (VPT_TB / 2)];
  const uint32_t o = blockIdx.x, lo = o * nb, hi = o == 2 ? 2 * nb + nc : lo + nb;
  XYZZ<C> acc = Ec<C>::infinity();
#pragma unroll 1
  for (uint32_t b = lo + threadIdx.x; b < hi; b += VPT_TB) acc = Ec<C>::add(acc, ld_point<C>(partial, b));
  acc = vpt_block_sum<C>(acc, sh);
  if (threadIdx.x == 0) st_point<C>(out, o, acc);
}

// ---- host side --------------------------------------------------------------------------------------

template <class C>
XYZZ<C> point_from_limbs(const uint32_t* w) {
  constexpr int N = C::Fp::N;
  XYZZ<C> r;
  for (int j = 0; j < N; ++j) { r.x.l[j] = w[j]; r.y.l[j] = w[N + j]; r.zz.l[j] = w[2 * N + j]; r.zzz.l[j] = w[3 * N + j]; }
  return r;
}

template <class C>
int verify_points_t(Ctx* c, const uint64_t* comm_xy, const uint8_t* comm_inf, size_t n_comm, const uint32_t* comm_idx,
                    const uint64_t* z, const uint64_t* y, const uint64_t* proof_xy, const uint8_t* proof_inf, size_t K,
                    const uint32_t* rho_words, uint64_t* out_xy, uint8_t* out_inf) {
  using F = typename C::Fr;
  using Fp = typename C::Fp;
  constexpr size_t PW64 = Fp::NW;                   // 64-bit words per affine point
  constexpr size_t PT_BYTES = 2 * Fp::NW * 4;
  constexpr size_t XYZZ_BYTES = 4 * Fp::N * 4;
  if (K > ((size_t)1 << 21)) return set_err(c, KZG_ERR_ARG, "kzg_verify_points: need K <= 2^21");
  if (n_comm < 1 || n_comm > ((size_t)1 << 16)) return set_err(c, KZG_ERR_ARG, "kzg_verify_points: need 1 <= n_comm <= 2^16");
  memset(out_xy, 0, 2 * PT_BYTES);
  out_inf[0] = out_inf[1] = 1;
  if (K == 0) return KZG_OK;
  // the claims grouped by commitment: a counting sort of the indices (and their range check)
  std::vector<uint32_t> off, perm;
  if (group_by_index(comm_idx, K, n_comm, off, perm) < K)
    return set_err(c, KZG_ERR_ARG, "kzg_verify_points: commitment index out of range");

  const size_t n_short = n_comm + 1;
  const uint32_t nb = (uint32_t)((K + VPT_TB - 1) / VPT_TB), nc = (uint32_t)((n_short + VPT_TB - 1) / VPT_TB);
  // the workgroups split evenly over the fewest launches of at most VPT_LAUNCH_BLOCKS: no launch of a few workgroups
  // trails behind a full one with a whole ladder's latency of its own
  const uint32_t blocks = 2 * nb + nc, launches = (blocks + VPT_LAUNCH_BLOCKS - 1) / VPT_LAUNCH_BLOCKS;
  const uint32_t launch_blocks = (blocks + launches - 1) / launches;
  VerifyPointsWs d;
  int rc = carve(c, c->vpt_tmp, [&](Carve& ws) {
    d.layout(ws, K, n_comm, proof_inf != nullptr, comm_inf != nullptr, PT_BYTES, srs_rec_bytes(c->curve), POW_TAB,
             VPT_WEIGHT_THREADS, ver_commsum_shares(n_comm), blocks, XYZZ_BYTES,
             (size_t)VPT_TABLE * XYZZ_BYTES * launch_blocks * VPT_TB);
  }, &c->vpt_last_bytes);
  if (rc) return rc;

  ProfScope ps(c, "verify_points");
  hipStream_t st = c->stream;
  KZG_HIP(c, hipMemcpyAsync(d.pxy, proof_xy, K * PT_BYTES, hipMemcpyHostToDevice, st));
  if (proof_inf) KZG_HIP(c, hipMemcpyAsync(d.pinf, proof_inf, K, hipMemcpyHostToDevice, st));
  // the commitments, then the generator as one more: its scalar is -sum r_k y_k
  KZG_HIP(c, hipMemcpyAsync(d.cxy, comm_xy, n_comm * PT_BYTES, hipMemcpyHostToDevice, st));
  KZG_HIP(c, hipMemcpyAsync(reinterpret_cast<uint8_t*>(d.cxy) + n_comm * PT_BYTES, g1_generator_limbs(c->curve),
                            PT_BYTES, hipMemcpyHostToDevice, st));
  if (comm_inf) {
    KZG_HIP(c, hipMemcpyAsync(d.cinf, comm_inf, n_comm, hipMemcpyHostToDevice, st));
    KZG_HIP(c, hipMemsetAsync(d.cinf + n_comm, 0, 1, st));
  }
  KZG_HIP(c, hipMemsetAsync(d.bad, 0, 4, st));
  if ((rc = g1_import(c, d.pxy, d.pinf, K, /*range=*/true, d.precs, d.bad))) return rc;
  if ((rc = g1_import(c, d.cxy, d.cinf, n_short, /*range=*/true, d.crecs, d.bad))) return rc;
  uint32_t bad = 0;
  KZG_HIP(c, hipMemcpyAsync(&bad, d.bad, 4, hipMemcpyDeviceToHost, st));
  // the claims travel while the points are checked
  KZG_HIP(c, hipMemcpyAsync(d.z, z, K * 32, hipMemcpyHostToDevice, st));
  KZG_HIP(c, hipMemcpyAsync(d.y, y, K * 32, hipMemcpyHostToDevice, st));
  KZG_HIP(c, hipMemcpyAsync(d.perm, perm.data(), K * 4, hipMemcpyHostToDevice, st));
  KZG_HIP(c, hipMemcpyAsync(d.off, off.data(), (n_comm + 1) * 4, hipMemcpyHostToDevice, st));
  KZG_HIP(c, hipStreamSynchronize(st));
  if (bad) return set_err(c, KZG_ERR_ARG, "kzg_verify_points: a proof or commitment has a coordinate >= p or is not on the curve");

  // ---- weights: r, s, the per-commitment sums and -sum r_k y_k as scalar n_comm
  if ((rc = fr_pow_table(c, fr_arg<F>(mont_from_words<F>(rho_words)), d.rtab))) return rc;
  hipLaunchKernelGGL(vpt_weights_kernel<F>, dim3(VPT_WEIGHT_THREADS / 256), dim3(256), 0, st, (uint32_t)K, d.rtab, d.z,
                     d.y, d.r, d.s, d.ypart);
  KZG_HIP(c, hipGetLastError());
  if ((rc = ver_commitment_sums(c, d.r, d.perm, d.off, n_comm, d.cpart, d.coef))) return rc;
  if ((rc = ver_column_sums(c, 1, VPT_WEIGHT_THREADS, d.ypart, d.coef + n_comm * 8))) return rc;

  // ---- the ladders, VPT_LAUNCH_BLOCKS workgroups at a time over one table, and the fold of their partial points
  const VptGrid g{(uint32_t)K, nb, (uint32_t)n_short};
  for (uint32_t b0 = 0; b0 < blocks; b0 += launch_blocks) {
    hipLaunchKernelGGL(vpt_ladder_kernel<C>, dim3(std::min(launch_blocks, blocks - b0)), dim3(VPT_TB), 0, st, g, b0,
                       d.precs, d.crecs, d.r, d.s, d.coef, static_cast<uint4*>(d.tab), d.partial);
    KZG_HIP(c, hipGetLastError());
  }
  hipLaunchKernelGGL(vpt_fold_kernel<C>, dim3(3), dim3(VPT_TB), 0, st, nb, nc, d.partial, d.out);
  KZG_HIP(c, hipGetLastError());
  uint32_t h_out[3 * 4 * Fp::N];
  KZG_HIP(c, hipMemcpyAsync(h_out, d.out, sizeof(h_out), hipMemcpyDeviceToHost, st));
  KZG_HIP(c, hipStreamSynchronize(st));

  const XYZZ<C> R = point_from_limbs<C>(h_out), S = point_from_limbs<C>(h_out + 4 * Fp::N),
                Cc = point_from_limbs<C>(h_out + 8 * Fp::N);
  out_inf[0] = affine_to_words<C>(Ec<C>::to_affine(Ec<C>::add(Cc, S)), reinterpret_cast<uint32_t*>(out_xy));
  out_inf[1] = affine_to_words<C>(Ec<C>::to_affine(R), reinterpret_cast<uint32_t*>(out_xy + PW64));
  return KZG_OK;
}

}  // namespace

int verify_points(Ctx* c, const uint64_t* comm_xy, const uint8_t* comm_inf, size_t n_comm, const uint32_t* comm_idx,
                  const uint64_t* z, const uint64_t* y, const uint64_t* proof_xy, const uint8_t* proof_inf, size_t K,
                  const uint32_t* rho_words, uint64_t* out_xy, uint8_t* out_inf) {
  return KZG_BY_CURVE(c, verify_points_t, c, comm_xy, comm_inf, n_comm, comm_idx, z, y, proof_xy, proof_inf, K,
                      rho_words, out_xy, out_inf);
}

}  // namespace kzg
