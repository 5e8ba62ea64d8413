// poly.hip -- the polynomial half of KZG.open (kzg.py:122-159) on gfx950:
//
//   combined(X) = sum_i xi^(i+1) * p_i(X)                     kzg.py:147-150
//   witness(X)  = (combined(X) - combined(z)) // (X - z)      kzg.py:153-154
//
// Division by (X - z) is synthetic division: with S_j = sum_{i>=j} c_i z^(i-j)
// (suffix Horner values, S_j = c_j + z*S_{j+1}) the quotient is q_{j-1} = S_j for
// j >= 1 and combined(z) = S_0.  The recurrence is evaluated in two tile passes (below,
// "The opening's scan as TWO tile passes"); kzg_fr_poly_eval is the first of them without its stores.
// The MSM of the quotient (msm.hip) dominates open() by far.
// These kernels are bound by dependent Horner chains and by memory latency, not by instruction issue: the chain pin of
// field.h (an asm volatile per multiply-add) would only keep the scheduler from hoisting the next loads.
#define KZG_NO_CHAIN_PIN 1
#include "internal.h"
#include "fr_util.h"
#include "msm.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

namespace kzg {

namespace {

constexpr uint32_t LC = 32;       // elements per thread of the vector primitives (batch inversion, powers, prefix product)
// Chunk of the suffix-Horner scans (open, poly_eval): what one thread walks serially, and the group of lanes whose
// products one DPP sum collapses (8 limbs of 29 bits stay below 2^32).
constexpr uint32_t SC_LOG = 3;
constexpr uint32_t SC = 1u << SC_LOG;
constexpr uint32_t MAXK = 64;     // polynomials per open()

constexpr int FRN = 9;            // both scalar fields: 9 x 29-bit limbs
struct LincombArgs {              // travels in the kernel arguments (2.6 KB): no staging copy, no host synchronisation
  const uint32_t* polys;     // k polynomials, `stride` elements apart, canonical words
  uint64_t stride;
  uint32_t k;
  uint32_t lens[MAXK];
  uint32_t xipow[MAXK * FRN];   // xi^(i+1), Montgomery form
};

// sum over up to DOT_G terms c_g * x_g with ONE Montgomery reduction (Field::dot): 81 multiply-adds per term plus 74
// for the group, against 155 per term for separate products -- the combination kernels are bound by exactly these
// multiply-adds (rocprofv3, profiles/r03_open_pmc.csv: 31 M VALU wave-instructions per 2^20 x 6 combination before).
constexpr uint32_t DOT_G = 6;
template <class F>
__device__ __forceinline__ Fe<F> dot_upto(uint32_t cnt, const Fe<F>* c, const Fe<F>* x) {
  using Fd = Field<F>;
  switch (cnt) {                                             // uniform over the launch
    case 1: return Fd::template dot<1>(c, x);
    case 2: return Fd::template dot<2>(c, x);
    case 3: return Fd::template dot<3>(c, x);
    case 4: return Fd::template dot<4>(c, x);
    case 5: return Fd::template dot<5>(c, x);
    default: return Fd::template dot<6>(c, x);
  }
}

// out[t] = sum_i xipow[i] * p_i[t]   (xipow in Montgomery form => result in standard form)
template <class F>
__global__ void lincomb_kernel(LincombArgs a, uint32_t* out, uint32_t n) {
  using Fd = Field<F>;
  static_assert(F::N == FRN, "scalar fields have 9 limbs");
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  Fe<F> acc = Fd::zero();
  for (uint32_t i0 = 0; i0 < a.k; i0 += DOT_G) {
    const uint32_t cnt = min(DOT_G, a.k - i0);
    Fe<F> c[DOT_G], x[DOT_G];
#pragma unroll
    for (uint32_t g = 0; g < DOT_G; ++g) {
      const uint32_t i = i0 + g;
      const bool on = g < cnt && t < a.lens[i];               // shorter polynomials read as zero-padded
      c[g] = on ? load_words<F>(a.polys + (a.stride * i + t) * 8) : Fd::zero();
      x[g] = load_limbs<F>(a.xipow + (g < cnt ? i : i0) * F::N);
    }
    const Fe<F> part = dot_upto<F>(cnt, c, x);
    acc = i0 ? Fd::add(acc, part) : part;
  }
  store_words<F>(out + (size_t)t * 8, acc);
}

__global__ void any_nonzero_kernel(const uint32_t* words, size_t from_elem, size_t to_elem, uint32_t* flag) {
  const size_t i = from_elem + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= to_elem) return;
  uint32_t acc = 0;
  for (int k = 0; k < 8; ++k) acc |= words[i * 8 + k];
  if (acc) atomicOr(flag, 1u);
}

// =====================================================================================
// The opening's scan as TWO tile passes (round 4; rounds 1-3 collapsed chunks of 8 level by level: thirteen launches
// for a 2^20 opening, eleven of them 7-9 us dependent chains on a handful of waves).
//
// A workgroup of TB threads owns a TILE of T = 8 TB consecutive coefficients c_(bT) .. c_(bT+T-1) (thread q owns the
// chunk of 8 at local offset 8q).  With z != 0 the suffix values S_j = sum_(i >= j) c_i z^(i-j) are plain suffix SUMS of
// scaled terms, S_j = z^-j sum_(i >= j) c_i z^i, and the scaling is applied hierarchically so that no power table is
// longer than a tile:
//
//   pass 1 (tile_combine_kernel): comb = sum_i xi^(i+1) p_i (kzg.py:148-150), coalesced (thread t takes the local
//     elements t, t + TB, ..); e = comb * z^(pos mod 8); the 8 products of a chunk are added across 8 adjacent lanes by
//     DPP (lazily: 8 limbs of 29 bits stay below 2^32) -> h_q = sum_(r<8) c_(8q+r) z^r; g_q = h_q z^(8q); the tile's
//     aggregate H_b = sum_q g_q = sum_(i<T) c_(bT+i) z^i.  Written: comb (32 B per coefficient), g (36 B per chunk),
//     H (36 B per tile).  Extra workgroups at the head of the grid build the two tables pass 2 reads: zinv[q] = z^(-8q)
//     (q <= TB) and W[k] = z^(T(k+1)), from a few generator powers the host passes in the kernel arguments.
//   pass 2 (tile_fill_kernel): every tile sums the aggregates ABOVE it itself, Q_b = z^T S_((b+1)T) = sum_(k>=0) H_(b+1+k) W[k]
//     -- one product per tile pair, 1.3 * 10^5 products at 2^20, spread over all workgroups: there is no serial chain
//     over the tiles and no launch per level; beyond 1024 tiles the aggregates of 64 tiles are first folded into one
//     (tile_group_kernel) so that a tile never sums more than 63 + ntiles/64 terms.  Inside the tile a wave-wide suffix
//     sum of the g_q (additions only) gives the carry into chunk q, S_(bT+8(q+1)) = zinv[q+1] (sum_(q'>q) g_q' + Q_b),
//     and each thread walks its 8 coefficients in LDS from there (S_j = c_j + z S_(j+1)); the suffix values leave
//     coalesced: S_0 = combined(z), S_j = quotient coefficient j-1 (kzg.py:153-154).
//
// Products per coefficient: the combination's k (one reduction, Field::dot) + 1 (e) + 1 (walk) + (2 + 1 + ~1)/8.
// Traffic: k + 1 reads of 32 B, 2 writes of 32 B per coefficient + 9 B per coefficient of g -> (k+3)/(k+1) of the
// algorithmic bytes, the floor of a combine-then-scan structure.  z = 0 has no inverse: then S_j = c_j, a copy.
// =====================================================================================
constexpr uint32_t SG_LOG = 6, SG = 1u << SG_LOG;      // tiles per group of the two-level aggregate sum
constexpr uint32_t TILE_MAXK = 16;                     // polynomials per tile_combine launch (more: combined first)
constexpr uint32_t TILE_GW = 22;                       // generator powers z^(T 2^s) for the W table: 2^22 tiles
constexpr uint32_t TILE_DIRECT_MAX = 1024;             // up to this many tiles every tile sums all aggregates above it
#ifndef KZG_TILE_ITER
#define KZG_TILE_ITER 4
#endif
// Issue priority of the two tile kernels.  Beside an accumulate kernel they hold a wave slot and ~110 VGPRs per SIMD
// that the reduce stage's 168-VGPR waves then cannot get: at priority 0 the combination of opening p + 1 sat there for
// 1.4 ms and rc1 / rc2 / prep_binsort stretched 4-17x (profiles/r04_open_async_timeline_prio0.txt); raised, it is gone after 0.48 ms:
// 448 vs 430 pipelined opens/s, same box, alternating (profiles/r04_open_async_ab.txt).
#ifndef KZG_TILE_PRIO
#define KZG_TILE_PRIO 3
#endif
constexpr uint32_t TILE_ITER = KZG_TILE_ITER;          // coefficients per thread of the combination (tile_combine_kernel)

struct TileLincomb {
  const uint32_t* polys;
  uint64_t stride;
  uint32_t k;
  uint32_t lens[TILE_MAXK];
  uint32_t xipow[TILE_MAXK * FRN];    // xi^(i+1), Montgomery form
};
struct TileScanArgs {                 // all Montgomery form; 2.5 KB of the 4 KB kernel-argument limit with TileLincomb
  uint32_t zs[SC * FRN];              // z^r, r < 8
  uint32_t zq_lo[16 * FRN];           // z^(8c), c < 16         z^(8q) = zq_lo[q & 15] * zq_hi[q >> 4]
  uint32_t zq_hi[16 * FRN];           // z^(128c), c < 16
  uint32_t ginv[9 * FRN];             // z^(-8 * 2^s), s <= 8   -> zinv[q], q <= 256
  uint32_t gw[TILE_GW * FRN];         // z^(T * 2^s)            -> W[k] = z^(T(k+1))
};

// sum over the 8 lanes of an aligned group (every lane of the group ends with the total): two quad permutes and a
// half-row mirror, no LDS
__device__ __forceinline__ uint32_t lane8_sum(uint32_t x) {
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xF, 0xF, true);     // quad_perm:[1,0,3,2]
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xF, 0xF, true);     // quad_perm:[2,3,0,1]
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x141, 0xF, 0xF, true);    // row_half_mirror
  return x;
}
// 8 weak-normal values -> their canonical sum (8 * 2p < 2^261, limbs < 2^32), in every lane of the group
template <class F>
__device__ __forceinline__ Fe<F> lane8_sum_reduced(const Fe<F>& v) {
  Fe<F> s;
#pragma unroll
  for (int j = 0; j < F::N; ++j) s.l[j] = lane8_sum(v.l[j]);
  return Field<F>::reduce_wide(Field<F>::carry(s));
}
// Sum of one weak-normal value per thread over the workgroup (all threads call it); valid in thread 0 only.
// red: (TB / 8 + TB / 64) elements of LDS.
template <class F, uint32_t TB>
__device__ __forceinline__ Fe<F> block_sum(const Fe<F>& v, uint32_t* red) {
  using Fd = Field<F>;
  const uint32_t tid = threadIdx.x;
  const Fe<F> s1 = lane8_sum_reduced<F>(v);
  if ((tid & 7) == 0) store_limbs<F>(red + (tid >> 3) * F::N, s1);
  __syncthreads();
  const Fe<F> x = tid < TB / 8 ? load_limbs<F>(red + tid * F::N) : Fd::zero();
  const Fe<F> s2 = lane8_sum_reduced<F>(x);
  if ((tid & 7) == 0 && tid < TB / 8) store_limbs<F>(red + (TB / 8 + (tid >> 3)) * F::N, s2);
  __syncthreads();
  Fe<F> r = Fd::zero();
  if (tid == 0)
    for (uint32_t u = 0; u < TB / 64; ++u) r = Fd::add(r, load_limbs<F>(red + (TB / 8 + u) * F::N));
  return r;
}
// product of the generators g[s] over the set bits s of e (Montgomery form)
template <class F>
__device__ __forceinline__ Fe<F> pow_from_generators(const uint32_t* g, uint32_t e) {
  Fe<F> p = Field<F>::one();
  for (uint32_t s = 0; (e >> s) != 0; ++s)
    if ((e >> s) & 1u) p = Field<F>::mul(p, load_limbs<F>(g + s * F::N));
  return p;
}

// The steps of pass 1 that are the same for one point (tile_combine_kernel) and for several (tile_combine_multi_kernel,
// below), per point.
// Entry t of the two tables pass 2 reads: zinv[t] = z^(-8t) (t <= TB; ZINV = false: not wanted) and W[t] = z^(T(t+1))
// (t < ntiles), each a chain of <= 20 products over the host's generator powers.
template <class F, uint32_t TB, bool ZINV = true>
__device__ __forceinline__ void tile_table_entry(uint32_t t, uint32_t ntiles, const uint32_t* ginv, const uint32_t* gw,
                                                 uint32_t* zinv, uint32_t* W) {
  if (ZINV && t <= TB) store_limbs<F>(zinv + (size_t)t * F::N, pow_from_generators<F>(ginv, t));
  if (t < ntiles) store_limbs<F>(W + (size_t)t * F::N, pow_from_generators<F>(gw, t + 1));
}
// A coefficient's term of its chunk sum, c z^(pos mod 8) (0 beyond the end), added across the chunk's 8 lanes; the
// sum stays in lazy limbs (8 limbs of 29 bits are below 2^32) and goes to h, the chunk's place in LDS.
template <class F>
__device__ __forceinline__ void tile_chunk_sum(const Fe<F>& cf, const Fe<F>& zr, uint32_t* h) {
  const Fe<F> e = Field<F>::mul(cf, zr);
  Fe<F> s;
#pragma unroll
  for (int j = 0; j < F::N; ++j) s.l[j] = lane8_sum(e.l[j]);
  if ((threadIdx.x & 7) == 0) store_limbs<F>(h, s);
}
// The chunk sums hs of tile b (complete in LDS) -> g_q = h_q z^(8q), to G[b TB + q] if STORE, and their sum, the
// tile's aggregate, to Hb.  All TK threads of the workgroup call it; red as for block_sum<TK>.
template <class F, uint32_t TB, uint32_t TK, bool STORE>
__device__ __forceinline__ void tile_aggregate(const uint32_t* hs, const uint32_t* zq_lo, const uint32_t* zq_hi,
                                               uint32_t b, uint32_t* G, uint32_t* Hb, uint32_t* red) {
  using Fd = Field<F>;
  const uint32_t tid = threadIdx.x;
  Fe<F> g = Fd::zero();
  if (tid < TB) {                                                             // whole waves: TB is a multiple of 64
    const Fe<F> hq = Fd::reduce_wide(Fd::carry(load_limbs<F>(hs + tid * F::N)));
    const Fe<F> zq = Fd::mul(load_limbs<F>(zq_lo + (tid & 15) * F::N), load_limbs<F>(zq_hi + (tid >> 4) * F::N));
    g = Fd::mul(hq, zq);
    if (STORE) store_limbs<F>(G + ((size_t)b * TB + tid) * F::N, g);
  }
  const Fe<F> hb = block_sum<F, TK>(g, red);
  if (tid == 0) store_limbs<F>(Hb, hb);
}

// TB chunks (T = 8 TB coefficients) per tile, TK = T / ITER threads per workgroup: the kernel waits for memory, so the
// coefficients of a tile are spread over MORE threads than the fill uses (2 waves per SIMD at one thread per chunk:
// 77 us for the 2^20 x 6 combination; profiles/r04a_open_kernel_stats.csv), each taking ITER strided elements.
// STORE = false: the aggregates alone (kzg_fr_poly_eval: nothing but H and the tables is written).
template <class F, uint32_t TB, uint32_t ITER, bool STORE = true>
__global__ __launch_bounds__(TB * SC / ITER) void tile_combine_kernel(TileLincomb a, TileScanArgs ts, uint32_t* comb,
                                                                      uint32_t n, uint32_t ntiles, uint32_t* G,
                                                                      uint32_t* H, uint32_t* zinv, uint32_t* W) {
  using Fd = Field<F>;
  constexpr uint32_t T = TB * SC, TK = T / ITER;
  static_assert(F::N == FRN && SC == 8 && TB % 64 == 0 && TB <= 256 && TK % 64 == 0 && TK >= TB && TK <= 1024, "tile layout");
  __shared__ uint32_t hs[TB * FRN];                         // chunk sums (lazy limbs)
  __shared__ uint32_t zsh[SC * FRN];
  __shared__ uint32_t red[(TK / 8 + TK / 64) * FRN];
  const uint32_t tid = threadIdx.x;
#if KZG_TILE_PRIO
  __builtin_amdgcn_s_setprio(KZG_TILE_PRIO);
#endif
  const uint32_t ntab = gridDim.x - ntiles;
  if (blockIdx.x < ntab) {       // table workgroups (nothing of pass 1 reads these): FIRST in the grid, so that their
    tile_table_entry<F, TB>(blockIdx.x * TK + tid, ntiles, ts.ginv, ts.gw, zinv, W);      // chains start at once and end early
    return;
  }
  const uint32_t b = blockIdx.x - ntab, base = b * T;
  if (tid < SC * FRN) zsh[tid] = ts.zs[tid];
  __syncthreads();
  const Fe<F> zr = load_limbs<F>(zsh + (tid & (SC - 1)) * F::N);
#pragma unroll 1
  for (uint32_t it = 0; it < ITER; ++it) {
    const uint32_t i = it * TK + tid, t = base + i;
    Fe<F> acc = Fd::zero();
    if (t < n) {
      for (uint32_t i0 = 0; i0 < a.k; i0 += DOT_G) {
        const uint32_t cnt = min(DOT_G, a.k - i0);
        Fe<F> c[DOT_G], x[DOT_G];
#pragma unroll
        for (uint32_t g = 0; g < DOT_G; ++g) {
          const uint32_t p = i0 + g;
          const bool on = g < cnt && t < a.lens[g < cnt ? p : i0];           // shorter polynomials read as zero-padded
          c[g] = on ? load_words<F>(a.polys + (a.stride * p + t) * 8) : Fd::zero();
          x[g] = load_limbs<F>(a.xipow + (g < cnt ? p : i0) * F::N);
        }
        const Fe<F> part = dot_upto<F>(cnt, c, x);
        acc = i0 ? Fd::add(acc, part) : part;
      }
      if (STORE) store_words<F>(comb + (size_t)t * 8, acc);
    }
    tile_chunk_sum<F>(acc, zr, hs + (i >> 3) * F::N);
  }
  __syncthreads();
  tile_aggregate<F, TB, TK, STORE>(hs, ts.zq_lo, ts.zq_hi, b, G, H + (size_t)b * F::N, red);
}

// A[s] = sum_(i < 64) H[64 s + i] z^(T i): one wave per group of tiles
template <class F>
__global__ __launch_bounds__(64) void tile_group_kernel(const uint32_t* H, const uint32_t* W, uint32_t ntiles,
                                                        uint32_t* A) {
  using Fd = Field<F>;
  static_assert(SG == 64, "one wave per group");
  const uint32_t s = blockIdx.x, i = threadIdx.x, bt = s * SG + i;
  Fe<F> v = Fd::zero();
  if (bt < ntiles) {
    v = load_limbs<F>(H + (size_t)bt * F::N);
    if (i) v = Fd::mul(v, load_limbs<F>(W + (size_t)(i - 1) * F::N));
  }
  const Fe<F> x = lane8_sum_reduced<F>(v);
  Fe<F> r = x;
#pragma unroll 1
  for (uint32_t u = 1; u < 8; ++u) {
    Fe<F> t;
#pragma unroll
    for (int j = 0; j < F::N; ++j) t.l[j] = (uint32_t)__shfl((int)x.l[j], (int)(u * 8));
    r = Fd::add(r, t);
  }
  if (i == 0) store_limbs<F>(A + (size_t)s * F::N, r);
}

// Q_b = sum over everything above tile b, each term once: tiles of b's own group, then whole groups (A != null), then
// the caller's carry as the aggregate of a virtual tile `ntiles` (sharded open).  All threads call; valid in thread 0.
template <class F, uint32_t TB>
__device__ __forceinline__ Fe<F> tile_carry_sum(uint32_t b, uint32_t ntiles, const uint32_t* H, const uint32_t* A,
                                                uint32_t nsuper, const FrArg& hv, uint32_t has_hv, const uint32_t* W,
                                                uint32_t* red) {
  using Fd = Field<F>;
  const uint32_t tid = threadIdx.x;
  Fe<F> acc = Fd::zero();
  if (!A) {
    for (uint32_t bp = b + 1 + tid; bp < ntiles; bp += TB)
      acc = Fd::add(acc, Fd::mul(load_limbs<F>(H + (size_t)bp * F::N), load_limbs<F>(W + (size_t)(bp - b - 1) * F::N)));
  } else {
    const uint32_t s = b >> SG_LOG, gend = min((s + 1) << SG_LOG, ntiles);
    for (uint32_t bp = b + 1 + tid; bp < gend; bp += TB)
      acc = Fd::add(acc, Fd::mul(load_limbs<F>(H + (size_t)bp * F::N), load_limbs<F>(W + (size_t)(bp - b - 1) * F::N)));
    for (uint32_t sp = s + 1 + tid; sp < nsuper; sp += TB)
      acc = Fd::add(acc, Fd::mul(load_limbs<F>(A + (size_t)sp * F::N),
                                 load_limbs<F>(W + (size_t)((sp << SG_LOG) - b - 1) * F::N)));
  }
  if (has_hv && tid == TB - 1)
    acc = Fd::add(acc, Fd::mul(arg_fe<F>(hv), load_limbs<F>(W + (size_t)(ntiles - b - 1) * F::N)));
  return block_sum<F, TB>(acc, red);
}

// Pass 2 for one point: out (S_0, S_1, ..: n elements) = the suffix values of comb at z, or, with `add`, what `out`
// holds plus them (kzg_open_points: the points of a call follow each other on the stream, so that their sum needs
// neither a buffer per point nor a pass of its own).  has_hv: hv is the aggregate of a virtual tile above the last one
// (sharded open).  zero: z = 0, the suffix values are comb itself and no table is read.
template <class F, uint32_t TB>
__global__ __launch_bounds__(TB) void tile_fill_kernel(const uint32_t* comb, uint32_t n, uint32_t ntiles,
                                                       const uint32_t* G, const uint32_t* H, const uint32_t* A,
                                                       uint32_t nsuper, FrArg hv, uint32_t has_hv, FrArg zarg,
                                                       uint32_t zero, const uint32_t* zinv, const uint32_t* W,
                                                       uint32_t add, uint32_t* out) {
  using Fd = Field<F>;
  constexpr uint32_t T = TB * SC, NWAVE = TB / 64;
  __shared__ uint4 st[T * 2 + TB];                          // 32 B per coefficient + one pad quad per chunk
  __shared__ uint32_t red[(TB / 8 + TB / 64) * FRN];
  __shared__ uint32_t wsum[NWAVE * FRN];
  __shared__ uint32_t qsh[FRN];
#if KZG_TILE_PRIO
  __builtin_amdgcn_s_setprio(KZG_TILE_PRIO);
#endif
  const uint32_t tid = threadIdx.x, b = blockIdx.x, e0 = b * T;
  const uint4* gin = reinterpret_cast<const uint4*>(comb);
  for (uint32_t i = tid; i < T * 2; i += TB) {
    const uint32_t e = i >> 1;
    if (e0 + e < n) st[i + (e >> SC_LOG)] = gin[(size_t)(e0 + e) * 2 + (i & 1)];
  }
  if (!zero) {
    const Fe<F> q0 = tile_carry_sum<F, TB>(b, ntiles, H, A, nsuper, hv, has_hv, W, red);
    if (tid == 0) store_limbs<F>(qsh, q0);
    // suffix sums of the tile's scaled chunk values: inclusive inside the wave by shuffles, the waves above from LDS
    const uint32_t lane = tid & 63, wave = tid >> 6;
    Fe<F> incl = load_limbs<F>(G + ((size_t)b * TB + tid) * F::N);
#pragma unroll 1
    for (uint32_t d = 1; d < 64; d <<= 1) {
      Fe<F> t;
#pragma unroll
      for (int j = 0; j < F::N; ++j) t.l[j] = (uint32_t)__shfl_down((int)incl.l[j], d);
      const Fe<F> s = Fd::add(incl, t);
      incl = Fd::select(lane + d < 64, s, incl);
    }
    if (lane == 0) store_limbs<F>(wsum + wave * F::N, incl);
    Fe<F> ex;                                               // sum over the chunks after this one
#pragma unroll
    for (int j = 0; j < F::N; ++j) {
      const uint32_t t = (uint32_t)__shfl_down((int)incl.l[j], 1);
      ex.l[j] = lane == 63 ? 0u : t;
    }
    __syncthreads();                                        // st, qsh, wsum complete
    for (uint32_t w = wave + 1; w < NWAVE; ++w) ex = Fd::add(ex, load_limbs<F>(wsum + w * F::N));
    Fe<F> acc = Fd::mul(Fd::add(ex, load_limbs<F>(qsh)), load_limbs<F>(zinv + (size_t)(tid + 1) * F::N));
    const uint32_t j0 = e0 + tid * SC;
    if (j0 < n) {
      const Fe<F> z = arg_fe<F>(zarg);
      for (uint32_t j = j0 + SC; j-- > j0;) {
        if (j >= n) {                                       // the chunk that holds the end: zero coefficients above it,
          if (has_hv) acc = Fd::mul(acc, z);                // and acc is zero up there without a carry
          continue;
        }
        const uint32_t q = (j - e0) * 2 + tid;              // (j - e0) >> SC_LOG == tid
        const uint4 lo = st[q], hi = st[q + 1];
        const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        acc = Fd::add(Fd::from_words(w), Fd::mul(acc, z));
        uint32_t o[8];
        Fd::to_words(Fd::reduce(acc), o);
        st[q] = make_uint4(o[0], o[1], o[2], o[3]);
        st[q + 1] = make_uint4(o[4], o[5], o[6], o[7]);
      }
    }
  }
  __syncthreads();
  uint4* gout = reinterpret_cast<uint4*>(out);
  if (!add) {
    for (uint32_t i = tid; i < T * 2; i += TB) {
      const uint32_t e = i >> 1;
      if (e0 + e < n) gout[(size_t)(e0 + e) * 2 + (i & 1)] = st[i + (e >> SC_LOG)];
    }
    return;
  }
  // whole elements, 32 contiguous bytes per lane: the tile's part of `out` was written by the launch before this one
#pragma unroll 2
  for (uint32_t e = tid; e < T; e += TB) {
    if (e0 + e >= n) break;
    const size_t o = (size_t)(e0 + e) * 2;
    const uint4 lo = st[e * 2 + (e >> SC_LOG)], hi = st[e * 2 + 1 + (e >> SC_LOG)], plo = gout[o], phi = gout[o + 1];
    const uint32_t x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const uint32_t y[8] = {plo.x, plo.y, plo.z, plo.w, phi.x, phi.y, phi.z, phi.w};
    uint32_t r[8];
    Fd::to_words(Fd::reduce(Fd::add(Fd::from_words(x), Fd::from_words(y))), r);
    gout[o] = make_uint4(r[0], r[1], r[2], r[3]);
    gout[o + 1] = make_uint4(r[4], r[5], r[6], r[7]);
  }
}

// S_0 = H_0 + sum_k H_(1+k) W[k] from the aggregates of pass 1, to out_words; all TB threads of the workgroup call it
template <class F, uint32_t TB>
__device__ __forceinline__ void tile_store_s0(uint32_t ntiles, const uint32_t* H, const uint32_t* A, uint32_t nsuper,
                                              const uint32_t* W, uint32_t* red, uint32_t* out_words) {
  FrArg none{};
  const Fe<F> q0 = tile_carry_sum<F, TB>(0, ntiles, H, A, nsuper, none, 0, W, red);
  if (threadIdx.x == 0) store_words<F>(out_words, Field<F>::add(q0, load_limbs<F>(H)));
}

// S_0 alone (the slice evaluation of a sharded open)
template <class F, uint32_t TB>
__global__ __launch_bounds__(TB) void tile_eval_kernel(uint32_t ntiles, const uint32_t* H, const uint32_t* A,
                                                       uint32_t nsuper, const uint32_t* W, uint32_t* out_words) {
  __shared__ uint32_t red[(TB / 8 + TB / 64) * FRN];
  tile_store_s0<F, TB>(ntiles, H, A, nsuper, W, red, out_words);
}

// =====================================================================================
// The two passes for SEVERAL points at once (kzg_open_points, kzg_fr_poly_eval_batch):
//   Q = sum_j Q_(z_j)[ sum_i w_ij p_i ],  Q_z[p] = (p - p(z)) / (X - z): the suffix values of the combination
//   comb_j = sum_i w_ij p_i at z_j, added up over the points.
// A launch takes up to MP points.  Pass 1 (tile_combine_multi_kernel) differs from tile_combine_kernel in its
// combination alone: it loads the (up to TILE_MAXK) coefficients of a position ONCE and forms every comb_j from them;
// the tables, the chunk sums and the tile aggregates are the steps above (tile_table_entry, tile_chunk_sum,
// tile_aggregate), taken per point.  Pass 2 is tile_fill_kernel itself, one launch per point, one after the other on
// the stream: each but the call's first ADDS its point's suffix values into the one output vector in place.  (A loop
// over the points inside one kernel was built first: every address derived from the thread index became loop-invariant
// and stayed in registers across the body, 98-118 VGPRs against tile_fill_kernel's 71-84.)
// The per-point tables (TileScanArgs, weights, z) do not fit the kernel arguments: they travel in a device buffer.
// z_j = 0: the suffix values are comb_j itself; the point takes no part in the scan (tile_fill_kernel's `zero`).
// =====================================================================================
constexpr uint32_t MP = 3;            // points per launch: 9 VGPRs of combination and 9 KiB of chunk sums each (a
                                      // fourth takes the BLS12-381 kernel past 128 VGPRs: 3 waves per SIMD for 4)
struct MultiPoint {                   // one point of one launch, Montgomery form
  TileScanArgs ts;
  uint32_t w[TILE_MAXK * FRN];        // weight of the launch's polynomial i at this point
  uint32_t z[FRN];
  uint32_t groups;                    // bit g: a polynomial of the g-th group of DOT_G has a non-zero weight here
  uint32_t zero;                      // z = 0
};
struct MultiPolys {                   // the launch's polynomials: rows row[i] of the caller's array (a zero weight
  const uint32_t* polys;              // everywhere drops a row before it gets here)
  uint64_t stride;
  uint32_t k;
  uint32_t lens[TILE_MAXK];
  uint32_t row[TILE_MAXK];
};
struct MultiCarve {                   // the scan buffers of a launch's points as the kernel takes them: from the
                                      // points' TileShapes (launch_tile_combine_multi)
  uint32_t *G[MP], *H[MP], *A[MP], *zinv[MP], *W[MP];
};

// fn(integral_constant j) for j < MP: the points of a launch by constant index, so that acc[j] stays in registers
template <class Fn, uint32_t... J>
__device__ __forceinline__ void for_points(Fn&& fn, std::integer_sequence<uint32_t, J...>) {
  (fn(std::integral_constant<uint32_t, J>{}), ...);
}
template <class Fn>
__device__ __forceinline__ void for_points(Fn&& fn) {
  for_points(fn, std::make_integer_sequence<uint32_t, MP>{});
}
// an element at an address that is the same in every lane, into scalar registers
template <class F>
__device__ __forceinline__ Fe<F> load_limbs_uniform(const uint32_t* p) {
  Fe<F> r;
#pragma unroll
  for (int j = 0; j < F::N; ++j) r.l[j] = (uint32_t)__builtin_amdgcn_readfirstlane((int)p[j]);
  return r;
}

// STORE = true (opening): the grid is one-dimensional, the k polynomials are combined per point.
// STORE = false (batched evaluation): blockIdx.y is ONE polynomial, taken as it is for every point; only the tile
// aggregates H[(poly0 + y) * hstride + b] and the W tables are written.
template <class F, uint32_t TB, uint32_t ITER, bool STORE>
__global__ __launch_bounds__(TB * SC / ITER) void tile_combine_multi_kernel(MultiPolys a, const MultiPoint* __restrict__ pts,
                                                                            uint32_t np, MultiCarve cv, uint32_t* comb,
                                                                            uint64_t comb_stride, uint32_t n,
                                                                            uint32_t ntiles, uint32_t poly0,
                                                                            uint32_t hstride) {
  using Fd = Field<F>;
  constexpr uint32_t T = TB * SC, TK = T / ITER;
  static_assert(F::N == FRN && SC == 8 && TB % 64 == 0 && TB <= 256 && TK % 64 == 0 && TK >= TB && TK <= 1024, "tile layout");
  __shared__ uint32_t hs[MP * TB * FRN];                    // chunk sums (lazy limbs), per point
  __shared__ uint32_t zsh[MP * SC * FRN];
  __shared__ uint32_t red[(TK / 8 + TK / 64) * FRN];
  const uint32_t tid = threadIdx.x;
#if KZG_TILE_PRIO
  __builtin_amdgcn_s_setprio(KZG_TILE_PRIO);
#endif
  const uint32_t ntab = gridDim.x - ntiles;
  if (blockIdx.x < ntab) {                                  // table workgroups, for every point that is scanned
    if (blockIdx.y) return;
#pragma unroll 1
    for (uint32_t j = 0; j < np; ++j)
      if (!pts[j].zero)
        tile_table_entry<F, TB, STORE>(blockIdx.x * TK + tid, ntiles, pts[j].ts.ginv, pts[j].ts.gw, cv.zinv[j], cv.W[j]);
    return;
  }
  const uint32_t b = blockIdx.x - ntab, base = b * T;
  const uint32_t len = STORE ? n : a.lens[blockIdx.y];
  if (base >= len) return;                                  // a tile above this polynomial's end (evaluation form)
  const uint32_t* src = a.polys + a.stride * a.row[blockIdx.y] * 8;
  for (uint32_t u = tid; u < np * SC * FRN; u += TK) zsh[u] = pts[u / (SC * FRN)].ts.zs[u % (SC * FRN)];
  __syncthreads();
#pragma unroll 1
  for (uint32_t it = 0; it < ITER; ++it) {
    const uint32_t i = it * TK + tid, t = base + i;
    Fe<F> acc[MP];
#pragma unroll
    for (uint32_t j = 0; j < MP; ++j) acc[j] = Fd::zero();
    if (t < len) {
      if (STORE) {
        for (uint32_t i0 = 0, grp = 0; i0 < a.k; i0 += DOT_G, ++grp) {
          const uint32_t cnt = min(DOT_G, a.k - i0);
          Fe<F> c[DOT_G];
#pragma unroll
          for (uint32_t g = 0; g < DOT_G; ++g) {
            const uint32_t p = i0 + g;
            const bool on = g < cnt && t < a.lens[g < cnt ? p : i0];         // shorter polynomials read as zero-padded
            c[g] = on ? load_words<F>(a.polys + (a.stride * a.row[g < cnt ? p : i0] + t) * 8) : Fd::zero();
          }
          for_points([&](auto jc) {
            constexpr uint32_t j = decltype(jc)::value;
            if (j >= np || !((pts[j].groups >> grp) & 1u)) return;           // uniform: no weight of this group here
            Fe<F> x[DOT_G];
#pragma unroll
            for (uint32_t g = 0; g < DOT_G; ++g) x[g] = load_limbs_uniform<F>(pts[j].w + (g < cnt ? i0 + g : i0) * F::N);
            acc[j] = Fd::add(acc[j], dot_upto<F>(cnt, c, x));
          });
        }
        for_points([&](auto jc) {
          constexpr uint32_t j = decltype(jc)::value;
          if (j < np) store_words<F>(comb + (comb_stride * j + t) * 8, acc[j]);
        });
      } else {
        const Fe<F> cf = load_words<F>(src + (size_t)t * 8);
#pragma unroll
        for (uint32_t j = 0; j < MP; ++j) acc[j] = cf;
      }
    }
    for_points([&](auto jc) {
      constexpr uint32_t j = decltype(jc)::value;
      if (j >= np || pts[j].zero) return;
      tile_chunk_sum<F>(acc[j], load_limbs<F>(zsh + (j * SC + (tid & (SC - 1))) * F::N), hs + (j * TB + (i >> 3)) * F::N);
    });
  }
  __syncthreads();
#pragma unroll 1
  for (uint32_t j = 0; j < np; ++j)
    if (!pts[j].zero)
      tile_aggregate<F, TB, TK, STORE>(hs + j * TB * F::N, pts[j].ts.zq_lo, pts[j].ts.zq_hi, b, cv.G[j],
                                       cv.H[j] + ((size_t)(poly0 + blockIdx.y) * hstride + b) * F::N, red);
}

// The values of a batched evaluation from the aggregates of pass 1: one workgroup per (polynomial, point).
struct EvalBatchArgs {
  const uint32_t* polys;
  uint64_t stride;
  uint32_t lens[MAXK];
  uint32_t slot[MAXK];                // the point's place among the non-zero points, MAXK for z = 0
};
template <class F, uint32_t TB>
__global__ __launch_bounds__(TB) void tile_eval_batch_kernel(EvalBatchArgs a, uint32_t k, const uint32_t* H,
                                                             uint32_t hstride, const uint32_t* W, uint32_t wstride,
                                                             uint32_t npts, uint32_t* out_words) {
  __shared__ uint32_t red[(TB / 8 + TB / 64) * FRN];
  const uint32_t i = blockIdx.x, j = blockIdx.y, len = a.lens[i], slot = a.slot[j];
  uint32_t* o = out_words + ((size_t)i * npts + j) * 8;
  if (len <= 1 || slot == MAXK) {                           // nothing, or the constant coefficient (poly_eval_t)
    if (threadIdx.x < 8) o[threadIdx.x] = len ? a.polys[a.stride * i * 8 + threadIdx.x] : 0u;
    return;
  }
  const uint32_t ntiles = (len + TB * SC - 1) / (TB * SC);
  const uint32_t* Hij = H + ((size_t)slot * k + i) * hstride * F::N;
  tile_store_s0<F, TB>(ntiles, Hij, nullptr, 0, W + (size_t)slot * wstride * F::N, red, o);
}

// Buffer layout of poly_tmp[0] (canonical words, 8 per element), cap = n + 1:
//   comb[0 .. cap)   combined polynomial
//   eval             S_0
//   quot[0 .. cap)   S_1, S_2, ...        => [eval, quot...] is the contiguous vector S_0, S_1, ...
// scan_tmp: g (9 words per chunk), H (per tile, + 1), A (per group of 64 tiles), zinv (TB + 1), W (per tile).
// A plan is the TileShape (internal.h: all that a fill or eval launch needs, and what the sharded opening keeps from
// begin to finish) and what pass 1 alone needs:
struct TilePass1 {
  uint32_t ntab = 0;                                          // table workgroups at the head of the grid
  TileScanArgs ts;
};

// The two buffers hold one opening at a time.  Every opening but kzg_open_shard_finish takes them through here, and
// that ends the slice a kzg_open_shard_begin holds in them: finish then refuses.
struct OpenBufs { DevBuf &vec, &scan; };
static OpenBufs claim_open_bufs(Ctx* c) {
  if (c->open_slice.state == OpenSlice::HELD) c->open_slice.state = OpenSlice::LOST;
  return {c->poly_tmp[0], c->scan_tmp};
}
// vec sized for n coefficients, by the layout above: the combination, and S_0 with the quotient behind it
static int open_vectors(Ctx* c, DevBuf& vec, size_t n, uint32_t** d_comb, uint32_t** d_eval) {
  if (int rc = ensure_buf(c, vec, (2 * (n + 1) + 1) * 32)) return rc;
  *d_comb = static_cast<uint32_t*>(vec.p);
  *d_eval = *d_comb + (n + 1) * 8;
  return KZG_OK;
}

static bool words_are_zero(const uint32_t* w) {
  uint32_t acc = 0;
  for (int i = 0; i < 8; ++i) acc |= w[i];
  return acc == 0;
}

// fn(std::integral_constant<uint32_t, TB>) for the tile width tb, one of 128 and 256
template <class Fn>
static int by_tile_width(uint32_t tb, Fn&& fn) {
  return tb == 128 ? fn(std::integral_constant<uint32_t, 128>{}) : fn(std::integral_constant<uint32_t, 256>{});
}

// Tile width: 256 threads (2048 coefficients, 65 KiB of LDS in the fill) when the GPU is the opening's; 128 threads
// (33 KiB) while an accumulate kernel of the commit pipeline holds 114 of a CU's 160 KiB, so that the fill still gets
// a workgroup onto every CU (the transform makes the same choice, ntt.hip).  c->tune_open_tb fixes it (tests).
static uint32_t open_tile_threads(Ctx* c) {
  if (c->tune_open_tb == 128 || c->tune_open_tb == 256) return (uint32_t)c->tune_open_tb;
  static const int fixed = [] { const char* e = getenv("KZG_OPEN_TB"); return e ? atoi(e) : 0; }();      // experiments
  if (fixed == 128 || fixed == 256) return (uint32_t)fixed;
  return msm_accumulate_in_flight(c) ? 128u : 256u;
}

// the counts of a scan over n coefficients in tiles of tb threads
static void tile_counts(Ctx* c, size_t n, uint32_t tb, TileShape* s, uint32_t* ntab) {
  const uint32_t T = tb * SC, tk = T / TILE_ITER;
  s->tb = tb, s->n = n;
  s->ntiles = (uint32_t)((n + T - 1) / T);
  *ntab = (std::max(tb + 1, s->ntiles) + tk - 1) / tk;
  const uint32_t direct_max = c->tune_open_direct_max > 0 ? (uint32_t)c->tune_open_direct_max : TILE_DIRECT_MAX;
  s->nsuper = s->ntiles > direct_max ? (s->ntiles + SG - 1) / SG : 0;
}
// the powers of z != 0 that the two passes take from the host (one inversion), for tiles of tb threads
template <class F>
void tile_powers(const uint32_t* z_words, uint32_t tb, TileShape* s, TileScanArgs* ts) {
  using Fd = Field<F>;
  const Fe<F> z = Fd::to_mont(Fd::from_words(z_words));
  memcpy(s->z, z.l, F::N * 4);
  Fe<F> zj = Fd::one();
  for (uint32_t j = 0; j < SC; ++j) { memcpy(&ts->zs[j * F::N], zj.l, F::N * 4); zj = Fd::mul(zj, z); }
  const Fe<F> z8 = zj;
  zj = Fd::one();
  for (uint32_t j = 0; j < 16; ++j) { memcpy(&ts->zq_lo[j * F::N], zj.l, F::N * 4); zj = Fd::mul(zj, z8); }
  const Fe<F> z128 = zj;
  zj = Fd::one();
  for (uint32_t j = 0; j < 16; ++j) { memcpy(&ts->zq_hi[j * F::N], zj.l, F::N * 4); zj = Fd::mul(zj, z128); }
  Fe<F> g = z128;                                             // z^(8 * 16) -> z^(8 * tb) = z^T
  for (uint32_t q = 16; q < tb; q <<= 1) g = Fd::mul(g, g);
  for (uint32_t q = 0; q < TILE_GW; ++q) { memcpy(&ts->gw[q * F::N], g.l, F::N * 4); g = Fd::mul(g, g); }
  g = Fd::inv(z);
  memcpy(s->z_inv, g.l, F::N * 4);
  for (uint32_t q = 0; q < SC_LOG; ++q) g = Fd::mul(g, g);    // z^-8
  for (uint32_t q = 0; q < 9; ++q) { memcpy(&ts->ginv[q * F::N], g.l, F::N * 4); g = Fd::mul(g, g); }
}
// the carve of one scan's buffer at `base` (null: measure only); returns its words (with_chunks = false: no g)
static size_t tile_carve(TileShape* s, uint32_t* base, bool with_chunks) {
  const size_t chunk_words = with_chunks ? (size_t)s->ntiles * s->tb : 0;
  s->G = base;
  s->H = s->G + chunk_words * FRN;
  s->A = s->H + (size_t)(s->ntiles + 1) * FRN;
  s->zinv = s->A + (size_t)(s->nsuper + 1) * FRN;
  s->W = s->zinv + (size_t)(s->tb + 1) * FRN;
  return (chunk_words + (s->ntiles + 1) + (s->nsuper + 1) + (s->tb + 1) + s->ntiles) * FRN;
}

// the plan of a scan over n coefficients at z != 0 in tiles of tb threads, carved out of buf (with_chunks = false: no g)
template <class F>
int tile_plan(Ctx* c, size_t n, const uint32_t* z_words, uint32_t tb, DevBuf& buf, TileShape* s, TilePass1* p,
              bool with_chunks = true) {
  tile_counts(c, n, tb, s, &p->ntab);
  tile_powers<F>(z_words, tb, s, &p->ts);
  int rc = ensure_buf(c, buf, tile_carve(s, nullptr, with_chunks) * 4);
  if (rc) return rc;
  tile_carve(s, static_cast<uint32_t*>(buf.p), with_chunks);
  return KZG_OK;
}

// the weights xi^(i+1) (kzg.py:148-150) and the lengths of k polynomials, into a LincombArgs or a TileLincomb
template <class F, class Args>
Args lincomb_args(const uint32_t* d_polys, const size_t* lens, size_t k, size_t stride, const uint32_t* xi_words) {
  using Fd = Field<F>;
  Args la{};
  la.polys = d_polys; la.stride = stride; la.k = (uint32_t)k;
  const Fe<F> xi = Fd::to_mont(Fd::from_words(xi_words));
  Fe<F> xp = Fd::one();
  for (size_t i = 0; i < k; ++i) {
    xp = Fd::mul(xp, xi);
    memcpy(&la.xipow[i * F::N], xp.l, F::N * 4);
    la.lens[i] = (uint32_t)lens[i];
  }
  return la;
}
// weight one over a single vector of n elements
template <class F>
TileLincomb lincomb_of_one(const uint32_t* d_vec, size_t n) {
  TileLincomb la{};
  la.polys = d_vec; la.stride = n; la.k = 1; la.lens[0] = (uint32_t)n;
  const Fe<F> one = Field<F>::one();
  memcpy(&la.xipow[0], one.l, F::N * 4);
  return la;
}

// plain combination: out[t] = sum_i xi^(i+1) p_i[t]  (any k <= 64)
template <class F>
int launch_lincomb(Ctx* c, const uint32_t* d_polys, const size_t* lens, size_t k, size_t stride,
                   const uint32_t* xi_words, uint32_t* d_out, size_t n) {
  hipLaunchKernelGGL(lincomb_kernel<F>, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, c->stream,
                     (lincomb_args<F, LincombArgs>(d_polys, lens, k, stride, xi_words)), d_out, (uint32_t)n);
  return KZG_HIP_RC(c, hipGetLastError());
}

// the aggregates of groups of 64 tiles, where the scan sums in two levels (after pass 1: reads H and W)
template <class F>
int launch_tile_group(Ctx* c, const TileShape& s) {
  if (s.nsuper) hipLaunchKernelGGL(tile_group_kernel<F>, dim3(s.nsuper), dim3(64), 0, c->stream, s.H, s.W, s.ntiles, s.A);
  return KZG_HIP_RC(c, hipGetLastError());
}
// pass 1: combination + chunk / tile aggregates + tables.  STORE = false: the aggregates and tables alone.
template <class F, uint32_t TB, bool STORE = true>
int launch_tile_combine(Ctx* c, const TileShape& s, const TilePass1& p, const TileLincomb& la, uint32_t* d_comb) {
  hipLaunchKernelGGL((tile_combine_kernel<F, TB, TILE_ITER, STORE>), dim3(s.ntiles + p.ntab),
                     dim3(TB * SC / TILE_ITER), 0, c->stream, la, p.ts, d_comb, (uint32_t)s.n, s.ntiles,
                     STORE ? s.G : (uint32_t*)nullptr, s.H, s.zinv, s.W);
  KZG_HIP(c, hipGetLastError());
  return launch_tile_group<F>(c, s);
}
// pass 1 of an opening.  More than TILE_MAXK polynomials are combined first and pass 1 then runs over the combination
// itself (weight one).
template <class F, uint32_t TB>
int launch_open_combine(Ctx* c, const TileShape& s, const TilePass1& p, const uint32_t* d_polys, const size_t* lens,
                        size_t k, size_t stride, const uint32_t* xi_words, uint32_t* d_comb) {
  if (k <= TILE_MAXK)
    return launch_tile_combine<F, TB>(c, s, p, lincomb_args<F, TileLincomb>(d_polys, lens, k, stride, xi_words), d_comb);
  int rc = launch_lincomb<F>(c, d_polys, lens, k, stride, xi_words, d_comb, s.n);
  return rc ? rc : launch_tile_combine<F, TB>(c, s, p, lincomb_of_one<F>(d_comb, s.n), d_comb);
}

// pass 2.  hv: the aggregate of a virtual tile above the last one (sharded open), or null.  zero: s.z is 0 and d_S
// takes d_comb as it is; add: d_S keeps what it holds and the suffix values are added to it (kzg_open_points).
template <class F, uint32_t TB>
int launch_tile_fill(Ctx* c, const TileShape& s, const uint32_t* d_comb, const FrArg* hv, uint32_t* d_S,
                     bool zero = false, bool add = false) {
  FrArg none{}, z;
  memcpy(z.l, s.z, sizeof(z.l));
  hipLaunchKernelGGL((tile_fill_kernel<F, TB>), dim3(s.ntiles), dim3(TB), 0, c->stream, d_comb, (uint32_t)s.n, s.ntiles,
                     s.G, s.H, s.nsuper ? s.A : (const uint32_t*)nullptr, s.nsuper, hv ? *hv : none, hv ? 1u : 0u, z,
                     zero ? 1u : 0u, s.zinv, s.W, add ? 1u : 0u, d_S);
  return KZG_HIP_RC(c, hipGetLastError());
}

// S_0 alone from the aggregates of pass 1
template <class F, uint32_t TB>
int launch_tile_eval(Ctx* c, const TileShape& s, uint32_t* d_out) {
  hipLaunchKernelGGL((tile_eval_kernel<F, TB>), dim3(1), dim3(TB), 0, c->stream, s.ntiles, s.H,
                     s.nsuper ? s.A : (const uint32_t*)nullptr, s.nsuper, s.W, d_out);
  return KZG_HIP_RC(c, hipGetLastError());
}

template <class F>
int check_open_args(Ctx* c, const size_t* lens, size_t k, size_t stride, size_t* n_out) {
  if (k > MAXK) return set_err(c, KZG_ERR_ARG, "kzg_open: more than 64 polynomials");
  size_t n = 0;
  for (size_t i = 0; i < k; ++i) {
    if (lens[i] > stride) return set_err(c, KZG_ERR_ARG, "kzg_open: lens[i] > stride");
    n = std::max(n, lens[i]);
  }
  if (n >= (1ull << 31) - 1) return set_err(c, KZG_ERR_ARG, "kzg_open: polynomial too long");
  *n_out = n;
  return KZG_OK;
}

// witness of kzg.py:153-154: eval <- S_0, quotient coefficient j-1 <- S_j.  ONE "open_poly" span per opening.
// eval_out: host memory that receives S_0 when `sync` (the call then waits for the stream); otherwise nothing is
// copied and nothing waits -- the pipelined open fetches the 32 bytes below the quotient itself (msm.hip).
template <class F>
int open_quotient_t(Ctx* c, const uint32_t* d_polys, const size_t* lens, size_t k, size_t stride,
                    const uint32_t* z_words, const uint32_t* xi_words, uint32_t** d_quot_out, size_t* quot_len,
                    uint64_t* eval_out, bool sync) {
  if (eval_out) memset(eval_out, 0, 32);
  *quot_len = 0;
  *d_quot_out = nullptr;
  size_t n = 0;
  int rc = check_open_args<F>(c, lens, k, stride, &n);
  if (rc) return rc;
  if (n == 0) return KZG_OK;     // all polynomials zero: witness 0, evaluation 0
  const OpenBufs bufs = claim_open_bufs(c);
  uint32_t *d_comb, *d_eval;
  if ((rc = open_vectors(c, bufs.vec, n, &d_comb, &d_eval))) return rc;
  {
    ProfScope ps(c, "open_poly");
    if (words_are_zero(z_words)) {         // S_j = c_j: the combination IS the vector of suffix values
      if ((rc = launch_lincomb<F>(c, d_polys, lens, k, stride, xi_words, d_eval, n))) return rc;
    } else {
      TileShape s;
      TilePass1 p;
      if ((rc = tile_plan<F>(c, n, z_words, open_tile_threads(c), bufs.scan, &s, &p))) return rc;
      rc = by_tile_width(s.tb, [&](auto w) {
        return launch_open_combine<F, w>(c, s, p, d_polys, lens, k, stride, xi_words, d_comb);
      });
      if (!rc) rc = by_tile_width(s.tb, [&](auto w) { return launch_tile_fill<F, w>(c, s, d_comb, nullptr, d_eval); });
      if (rc) return rc;
    }
  }
  if (sync && eval_out) {
    KZG_HIP(c, hipMemcpyAsync(eval_out, d_eval, 32, hipMemcpyDeviceToHost, c->stream));
    KZG_HIP(c, hipStreamSynchronize(c->stream));
  }
  *d_quot_out = d_eval + 8;
  *quot_len = n - 1;
  return KZG_OK;
}

// Sharded open, step 1: combine this rank's coefficient slices and evaluate the slice polynomial (local indexing)
// at z.  The combination, its chunk values and tile aggregates stay on the device for step 2.
template <class F>
int open_shard_begin_t(Ctx* c, const uint32_t* d_polys, const size_t* lens, size_t k, size_t stride,
                       const uint32_t* z_words, const uint32_t* xi_words, uint64_t* chunk_eval_out) {
  memset(chunk_eval_out, 0, 32);
  const OpenBufs bufs = claim_open_bufs(c);      // first: a begin that fails leaves no slice
  size_t n = 0;
  int rc = check_open_args<F>(c, lens, k, stride, &n);
  if (rc) return rc;
  OpenSlice held;                                // shape.tb = 0: the empty slice, or z = 0
  held.state = OpenSlice::HELD;
  held.shape.n = n;
  memcpy(held.z_words, z_words, 32);
  uint32_t *d_comb = nullptr, *d_eval = nullptr;
  if (n && (rc = open_vectors(c, bufs.vec, n, &d_comb, &d_eval))) return rc;
  if (n) {
    ProfScope ps(c, "open_shard_poly");
    if (words_are_zero(z_words)) {         // slice(0) = its constant coefficient
      if ((rc = launch_lincomb<F>(c, d_polys, lens, k, stride, xi_words, d_comb, n))) return rc;
      d_eval = d_comb;
    } else {
      TilePass1 p;
      if ((rc = tile_plan<F>(c, n, z_words, open_tile_threads(c), bufs.scan, &held.shape, &p))) return rc;
      rc = by_tile_width(held.shape.tb, [&](auto w) {
        int r = launch_open_combine<F, w>(c, held.shape, p, d_polys, lens, k, stride, xi_words, d_comb);
        return r ? r : launch_tile_eval<F, w>(c, held.shape, d_eval);
      });
      if (rc) return rc;
    }
    KZG_HIP(c, hipMemcpyAsync(chunk_eval_out, d_eval, 32, hipMemcpyDeviceToHost, c->stream));
  }
  if (n) KZG_HIP(c, hipStreamSynchronize(c->stream));
  c->open_slice = held;
  return KZG_OK;
}

// step 2: the carry S_hi of the ranks above enters the fill as the aggregate of a virtual tile above the slice
// (exact: S_j of the slice depends on what lies above only through S_hi).  Returns the vector to commit.
template <class F>
int open_shard_finish_t(Ctx* c, const uint32_t* z_words, const uint32_t* carry_words, int first_rank,
                        uint32_t** d_vec_out, size_t* vec_len, uint64_t* eval_out) {
  using Fd = Field<F>;
  memset(eval_out, 0, 32);
  *d_vec_out = nullptr;
  *vec_len = 0;
  // the slice is trusted as begin left it: no plan is made here, and the tuning of the moment has no say
  const OpenSlice& held = c->open_slice;
  if (held.state == OpenSlice::NEVER) return set_err(c, KZG_ERR_ARG, "kzg_open_shard_finish without kzg_open_shard_begin");
  if (held.state == OpenSlice::LOST)
    return set_err(c, KZG_ERR_ARG, "kzg_open_shard_finish: another opening has used the context since kzg_open_shard_begin");
  if (memcmp(z_words, held.z_words, 32))
    return set_err(c, KZG_ERR_ARG, "kzg_open_shard_finish: z differs from the z of kzg_open_shard_begin");
  const TileShape& s = held.shape;
  const size_t n = s.n;
  if (n == 0) return KZG_OK;
  uint32_t *d_comb, *d_eval;
  int rc = open_vectors(c, c->poly_tmp[0], n, &d_comb, &d_eval);      // as begin sized it: nothing is allocated
  if (rc) return rc;
  {
    ProfScope ps(c, "open_shard_poly");
    if (s.tb == 0) {                       // z = 0: S_j = c_j for every j below the slice's end
      KZG_HIP(c, hipMemcpyAsync(d_eval, d_comb, n * 32, hipMemcpyDeviceToDevice, c->stream));
    } else {
      // virtual tile `ntiles`: its aggregate is S at index ntiles * T, i.e. carry * z^-(ntiles * T - n)
      const size_t gap = (size_t)s.ntiles * s.tb * SC - n;
      Fe<F> hv = Fd::from_words(carry_words), zi;
      memcpy(zi.l, s.z_inv, F::N * 4);
      for (size_t e = gap; e; e >>= 1) {
        if (e & 1) hv = Fd::mul(hv, zi);
        zi = Fd::mul(zi, zi);
      }
      const FrArg hva = fr_arg<F>(hv);
      if ((rc = by_tile_width(s.tb, [&](auto w) { return launch_tile_fill<F, w>(c, s, d_comb, &hva, d_eval); }))) return rc;
    }
  }
  KZG_HIP(c, hipMemcpyAsync(eval_out, d_eval, 32, hipMemcpyDeviceToHost, c->stream));
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  // first rank: S_0 is the evaluation, the quotient slice is S_1 .. S_(n-1); otherwise S_lo is the quotient
  // coefficient lo-1: commit S_lo .. S_(hi-1)
  *d_vec_out = d_eval + (first_rank ? 8 : 0);
  *vec_len = n - (first_rank ? 1 : 0);
  return KZG_OK;
}

// pass 1 for the np <= MP points whose scan buffers are shapes[0 .. np) and whose tables are d_pts[0 .. np): the
// opening's form (STORE: d_comb takes the np combinations, comb_stride elements apart) or the evaluation's (one
// polynomial per blockIdx.y; its aggregates to H[(poly0 + y) * hstride ..]).  ntab = 0: the tables are there already.
template <class F, uint32_t TB, bool STORE>
int launch_tile_combine_multi(Ctx* c, const TileShape* shapes, uint32_t np, uint32_t ntab, const MultiPolys& polys,
                              const MultiPoint* d_pts, uint32_t* d_comb, size_t comb_stride, uint32_t poly0,
                              uint32_t hstride) {
  MultiCarve cv{};
  for (uint32_t q = 0; q < np; ++q) {
    const TileShape& s = shapes[q];
    cv.G[q] = s.G, cv.H[q] = s.H, cv.A[q] = s.A, cv.zinv[q] = s.zinv, cv.W[q] = s.W;
  }
  hipLaunchKernelGGL((tile_combine_multi_kernel<F, TB, TILE_ITER, STORE>), dim3(shapes[0].ntiles + ntab, STORE ? 1 : polys.k),
                     dim3(TB * SC / TILE_ITER), 0, c->stream, polys, d_pts, np, cv, d_comb, (uint64_t)comb_stride,
                     (uint32_t)shapes[0].n, shapes[0].ntiles, poly0, hstride);
  return KZG_HIP_RC(c, hipGetLastError());
}

// a point's tables (z != 0) for tiles of tb threads; weights and groups are the launch's to fill
template <class F>
MultiPoint multi_point(const uint32_t* z_words, uint32_t tb) {
  MultiPoint m{};
  m.zero = words_are_zero(z_words);
  if (!m.zero) {
    TileShape s;
    tile_powers<F>(z_words, tb, &s, &m.ts);
    memcpy(m.z, s.z, sizeof(m.z));
  }
  return m;
}

// Q = sum_j Q_(z_j)[ sum_i w_ij p_i ]: the vector S (n elements; Q's n - 1 coefficients are S_1 ..) in poly_tmp[0],
// with the launch's MP combinations behind it; MP carves of scan_tmp; the launches' point tables in poly_tmp[1].
// Polynomials that carry no weight and points whose weights are all zero never reach a launch.  More than TILE_MAXK
// polynomials or MP points are further launches: the output is linear in both, so each pair of passes adds its part
// to S in place.  ONE "open_points_poly" span per call.
template <class F>
int open_points_quotient_t(Ctx* c, const uint32_t* d_polys, const size_t* lens, size_t k, size_t stride,
                           const uint32_t* points, size_t t, const uint32_t* weights, uint32_t** d_quot_out,
                           size_t* quot_len) {
  using Fd = Field<F>;
  *d_quot_out = nullptr;
  *quot_len = 0;
  if (t > MAXK) return set_err(c, KZG_ERR_ARG, "kzg_open_points: more than 64 points");
  size_t n = 0;
  int rc = check_open_args<F>(c, lens, k, stride, &n);
  if (rc) return rc;
  if (n <= 1) return KZG_OK;                     // a constant has the quotient 0 at every point
  auto weight = [&](size_t i, size_t j) { return weights + (i * t + j) * 8; };
  std::vector<uint32_t> pi, pj;
  for (size_t i = 0; i < k; ++i) {
    bool any = false;
    for (size_t j = 0; j < t && !any; ++j) any = !words_are_zero(weight(i, j));
    if (any && lens[i]) pi.push_back((uint32_t)i);
  }
  for (size_t j = 0; j < t; ++j) {
    bool any = false;
    for (size_t q = 0; q < pi.size() && !any; ++q) any = !words_are_zero(weight(pi[q], j));
    if (any) pj.push_back((uint32_t)j);
  }
  const OpenBufs bufs = claim_open_bufs(c);
  const uint32_t tb = open_tile_threads(c);
  TileShape shapes[MP];                          // the scan of a launch's q-th point; its z is the launch's to fill
  uint32_t ntab = 0;
  tile_counts(c, n, tb, &shapes[0], &ntab);
  const size_t cap = n + 1, scan_words = tile_carve(&shapes[0], nullptr, true);
  if ((rc = ensure_buf(c, bufs.vec, (MP + 1) * cap * 32))) return rc;
  if ((rc = ensure_buf(c, bufs.scan, MP * scan_words * 4))) return rc;
  uint32_t* d_S = static_cast<uint32_t*>(bufs.vec.p);
  uint32_t* d_comb = d_S + cap * 8;
  for (uint32_t q = 0; q < MP; ++q) {
    shapes[q] = shapes[0];
    tile_carve(&shapes[q], static_cast<uint32_t*>(bufs.scan.p) + q * scan_words, true);
  }
  std::vector<MultiPoint> proto;
  for (uint32_t j : pj) proto.push_back(multi_point<F>(points + (size_t)j * 8, tb));
  struct Launch { MultiPolys polys; size_t first; uint32_t np; };
  std::vector<Launch> launches;
  std::vector<MultiPoint> table;
  for (size_t i0 = 0; i0 < pi.size(); i0 += TILE_MAXK) {
    const uint32_t kc = (uint32_t)std::min<size_t>(TILE_MAXK, pi.size() - i0);
    for (size_t j0 = 0; j0 < pj.size(); j0 += MP) {
      Launch L{};
      L.polys.polys = d_polys, L.polys.stride = stride, L.polys.k = kc;
      for (uint32_t q = 0; q < kc; ++q) L.polys.row[q] = pi[i0 + q], L.polys.lens[q] = (uint32_t)lens[pi[i0 + q]];
      L.first = table.size();
      for (size_t jj = j0; jj < std::min<size_t>(j0 + MP, pj.size()); ++jj) {
        MultiPoint m = proto[jj];
        for (uint32_t q = 0; q < kc; ++q) {
          const uint32_t* w = weight(pi[i0 + q], pj[jj]);
          if (words_are_zero(w)) continue;
          m.groups |= 1u << (q / DOT_G);
          const Fe<F> wm = Fd::to_mont(Fd::from_words(w));
          memcpy(&m.w[q * F::N], wm.l, F::N * 4);
        }
        if (m.groups) table.push_back(m), ++L.np;
      }
      if (L.np) launches.push_back(L);
    }
  }
  if (launches.empty()) {
    KZG_HIP(c, hipMemsetAsync(d_S, 0, n * 32, c->stream));
  } else {
    if ((rc = ensure_buf(c, c->poly_tmp[1], table.size() * sizeof(MultiPoint)))) return rc;
    const MultiPoint* d_table = static_cast<const MultiPoint*>(c->poly_tmp[1].p);
    KZG_HIP(c, hipMemcpyAsync(c->poly_tmp[1].p, table.data(), table.size() * sizeof(MultiPoint), hipMemcpyHostToDevice,
                              c->stream));
    ProfScope ps(c, "open_points_poly");
    for (size_t l = 0; l < launches.size() && !rc; ++l) {
      const Launch& L = launches[l];
      const MultiPoint* pts = &table[L.first];
      rc = by_tile_width(tb, [&](auto w) {
        int r = launch_tile_combine_multi<F, w, true>(c, shapes, L.np, ntab, L.polys, d_table + L.first, d_comb, cap, 0, 0);
        for (uint32_t q = 0; q < L.np && !r; ++q)
          if (!pts[q].zero) r = launch_tile_group<F>(c, shapes[q]);
        for (uint32_t q = 0; q < L.np && !r; ++q) {      // one after the other: each adds to what the one before left
          memcpy(shapes[q].z, pts[q].z, sizeof(pts[q].z));
          r = launch_tile_fill<F, w>(c, shapes[q], d_comb + q * cap * 8, nullptr, d_S, pts[q].zero, l || q);
        }
        return r;
      });
    }
    if (rc) return rc;
  }
  KZG_HIP(c, hipStreamSynchronize(c->stream));    // `table` has left the host
  *d_quot_out = d_S + 8;
  *quot_len = n - 1;
  return KZG_OK;
}

// =====================================================================================
// Coset opening: division by Z = X^l - a, a = h^l (l = 2^log_l).  With S_t = c_t + a S_(t+l) (zero beyond the end)
// the quotient is q_t = S_(t+l) and the remainder rho_j = S_j (j < l).  Read as rows of l coefficients (row s holds
// c_(s l) .. c_(s l + l - 1)) that is l independent suffix-Horner chains down the rows, all with the multiplier a --
// the opening's scan with the stride l -- run as a blocked scan over tiles of CS_R rows:
//   coset_tile_kernel  A[b][j] = sum_(r < R) x[bR + r][j] a^r             (the tile's aggregate, one thread per (b, j))
//   the same on A with a^R, recursively, until one tile holds every row  (log_R(rows) levels: 5 at 2^20, l = 1)
//   coset_fill_kernel  x[row][j] <- S, walking the tile's rows down from the carry S at row (b+1)R = A[b+1][j] (now a
//                      suffix value of the level above), top level first
// Every launch spreads over ceil(rows / R) * l threads; no host round trip, no power table.  R = 16: a 2^20 scan
// starts at 2^16 threads.
// =====================================================================================
constexpr uint32_t CS_R = 16;
constexpr uint32_t CS_MAX_LOG_L = 12;

template <class F>
__global__ __launch_bounds__(256) void coset_tile_kernel(const uint32_t* x, uint32_t rows, uint32_t log_l, FrArg a,
                                                         uint32_t* agg) {
  using Fd = Field<F>;
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t tiles = (rows + CS_R - 1) / CS_R;
  if (g >= (tiles << log_l)) return;
  const uint32_t j = g & ((1u << log_l) - 1), b = g >> log_l;
  const Fe<F> am = arg_fe<F>(a);
  Fe<F> acc = Fd::zero();
#pragma unroll 1
  for (int r = CS_R - 1; r >= 0; --r) {
    const uint32_t row = b * CS_R + r;
    if (row < rows) acc = Fd::add(load_words<F>(x + (((size_t)row << log_l) + j) * 8), Fd::mul(acc, am));
  }
  store_words<F>(agg + (size_t)g * 8, acc);
}

// upper: the suffix values of the level above (rows `upper_rows`), null at the top level
template <class F>
__global__ __launch_bounds__(256) void coset_fill_kernel(uint32_t* x, uint32_t rows, uint32_t log_l, FrArg a,
                                                         const uint32_t* upper, uint32_t upper_rows) {
  using Fd = Field<F>;
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t tiles = (rows + CS_R - 1) / CS_R;
  if (g >= (tiles << log_l)) return;
  const uint32_t j = g & ((1u << log_l) - 1), b = g >> log_l;
  const Fe<F> am = arg_fe<F>(a);
  Fe<F> acc = upper && b + 1 < upper_rows ? load_words<F>(upper + ((((size_t)b + 1) << log_l) + j) * 8) : Fd::zero();
#pragma unroll 1
  for (int r = CS_R - 1; r >= 0; --r) {
    const uint32_t row = b * CS_R + r;
    if (row < rows) {
      uint32_t* p = x + (((size_t)row << log_l) + j) * 8;
      acc = Fd::add(load_words<F>(p), Fd::mul(acc, am));
      store_words<F>(p, acc);
    }
  }
}

// level `lv` of the blocked scan over x (rows x l), multiplier a (Montgomery); tmp: the aggregates of every level
template <class F>
int coset_scan_level(Ctx* c, uint32_t* x, uint32_t rows, uint32_t log_l, const Fe<F>& a, uint32_t* tmp) {
  using Fd = Field<F>;
  const uint32_t tiles = (rows + CS_R - 1) / CS_R;
  const uint32_t threads = tiles << log_l;
  const FrArg aa = fr_arg<F>(a);
  if (tiles == 1) {
    hipLaunchKernelGGL(coset_fill_kernel<F>, dim3((threads + 255) / 256), dim3(256), 0, c->stream, x, rows, log_l, aa,
                       (const uint32_t*)nullptr, 0u);
    KZG_HIP(c, hipGetLastError());
    return KZG_OK;
  }
  hipLaunchKernelGGL(coset_tile_kernel<F>, dim3((threads + 255) / 256), dim3(256), 0, c->stream, x, rows, log_l, aa,
                     tmp);
  KZG_HIP(c, hipGetLastError());
  Fe<F> aR = a;
  for (uint32_t r = 1; r < CS_R; r <<= 1) aR = Fd::sqr(aR);                  // a^R
  int rc = coset_scan_level<F>(c, tmp, tiles, log_l, aR, tmp + ((size_t)tiles << log_l) * 8);
  if (rc) return rc;
  hipLaunchKernelGGL(coset_fill_kernel<F>, dim3((threads + 255) / 256), dim3(256), 0, c->stream, x, rows, log_l, aa,
                     (const uint32_t*)tmp, tiles);
  KZG_HIP(c, hipGetLastError());
  return KZG_OK;
}

template <class F>
int open_coset_check_t(Ctx* c, const size_t* lens, size_t k, size_t stride, uint32_t log_l, const uint32_t* h_words,
                       const uint32_t* zeta_words, size_t key_n, size_t* n_out) {
  using Fd = Field<F>;
  if (log_l > CS_MAX_LOG_L) return set_err(c, KZG_ERR_ARG, "kzg_open_coset: log_l must be in [0, 12]");
  if (words_are_zero(h_words)) return set_err(c, KZG_ERR_ARG, "kzg_open_coset: h must be non-zero");
  const Fe<F> zeta = mont_from_words<F>(zeta_words);
  if (log_l == 0) {
    if (!Fd::eq(zeta, Fd::one())) return set_err(c, KZG_ERR_ARG, "kzg_open_coset: zeta must be 1 for l = 1");
  } else if (!primitive_root<F>(zeta, log_l)) {
    return set_err(c, KZG_ERR_ARG, "kzg_open_coset: zeta is not a primitive l-th root of unity");
  }
  int rc = check_open_args<F>(c, lens, k, stride, n_out);
  if (rc) return rc;
  if (*n_out > key_n) return set_err(c, KZG_ERR_DEGREE, "polynomial longer than the commitment key");
  return KZG_OK;
}

// The combination (kzg_open's xi rule), its remainder mod X^l - h^l and quotient.  d_quot receives max(n - l, 0)
// coefficients (canonical words); eval_out ([l][4], may be null) the values at h zeta^k: y = DFT_l(rho_j h^j) with
// zeta, on the host.  ONE "open_coset_poly" span per call; synchronises (the l remainder coefficients come back).
template <class F>
int open_coset_quotient_t(Ctx* c, const uint32_t* d_polys, const size_t* lens, size_t k, size_t stride,
                          uint32_t log_l, const uint32_t* h_words, const uint32_t* zeta_words, const uint32_t* xi_words,
                          size_t key_n, uint32_t** d_quot_out, size_t* quot_len, uint64_t* eval_out) {
  using Fd = Field<F>;
  *quot_len = 0;
  *d_quot_out = nullptr;
  size_t n = 0;
  int rc = open_coset_check_t<F>(c, lens, k, stride, log_l, h_words, zeta_words, key_n, &n);
  if (rc) return rc;
  const size_t l = (size_t)1 << log_l;
  if (eval_out) memset(eval_out, 0, l * 32);
  if (n == 0) return KZG_OK;     // all polynomials zero: quotient 0, every value 0
  const uint32_t rows = (uint32_t)((n + l - 1) >> log_l);
  const size_t padded = (size_t)rows << log_l;
  const OpenBufs bufs = claim_open_bufs(c);
  if ((rc = ensure_buf(c, bufs.vec, padded * 32))) return rc;
  size_t agg = 0;                                             // aggregates of every level of the blocked scan
  for (uint32_t r = rows; r > 1; r = (r + CS_R - 1) / CS_R) agg += (size_t)((r + CS_R - 1) / CS_R) << log_l;
  if ((rc = ensure_buf(c, bufs.scan, (agg + 1) * 32))) return rc;
  uint32_t* d_S = static_cast<uint32_t*>(bufs.vec.p);
  const Fe<F> h = Fd::to_mont(Fd::from_words(h_words));
  Fe<F> a = h;
  for (uint32_t q = 0; q < log_l; ++q) a = Fd::sqr(a);        // a = h^l
  std::vector<uint32_t> rho(l * 8, 0u);
  {
    ProfScope ps(c, "open_coset_poly");
    if ((rc = launch_lincomb<F>(c, d_polys, lens, k, stride, xi_words, d_S, padded))) return rc;   // zero-padded rows
    if ((rc = coset_scan_level<F>(c, d_S, rows, log_l, a, static_cast<uint32_t*>(bufs.scan.p)))) return rc;
    KZG_HIP(c, hipMemcpyAsync(rho.data(), d_S, std::min(l, n) * 32, hipMemcpyDeviceToHost, c->stream));
  }
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  if (eval_out) {     // y_k = sum_j rho_j h^j zeta^(jk): radix-2 DFT of size l on the host
    std::vector<Fe<F>> v(l);
    Fe<F> hp = Fd::one();
    for (size_t j = 0; j < l; ++j) {
      v[j] = Fd::mul(Fd::to_mont(Fd::from_words(&rho[j * 8])), hp);
      hp = Fd::mul(hp, h);
    }
    for (size_t i = 1, j = 0; i < l; ++i) {                   // bit-reversed order
      size_t bit = l >> 1;
      for (; j & bit; bit >>= 1) j ^= bit;
      j ^= bit;
      if (i < j) std::swap(v[i], v[j]);
    }
    const Fe<F> zeta = Fd::to_mont(Fd::from_words(zeta_words));
    for (size_t len = 2; len <= l; len <<= 1) {
      Fe<F> wl = zeta;                                        // zeta^(l / len)
      for (size_t e = len; e < l; e <<= 1) wl = Fd::sqr(wl);
      for (size_t i = 0; i < l; i += len) {
        Fe<F> wp = Fd::one();
        for (size_t j = 0; j < len / 2; ++j) {
          const Fe<F> u = v[i + j], t = Fd::mul(v[i + j + len / 2], wp);
          v[i + j] = Fd::add(u, t);
          v[i + j + len / 2] = Fd::sub(u, t);
          wp = Fd::mul(wp, wl);
        }
      }
    }
    for (size_t q = 0; q < l; ++q) words_from_mont<F>(v[q], reinterpret_cast<uint32_t*>(eval_out + q * 4));
  }
  if (n > l) {
    *d_quot_out = d_S + l * 8;
    *quot_len = n - l;
  }
  return KZG_OK;
}

}  // namespace

int open_quotient_device(Ctx* c, const uint32_t* d_polys, const size_t* lens, size_t k, size_t stride,
                         const uint32_t* z_words, const uint32_t* xi_words, uint32_t** d_quot_out, size_t* quot_len,
                         uint64_t* eval_out, bool sync) {
  return KZG_BY_FR(c, open_quotient_t, c, d_polys, lens, k, stride, z_words, xi_words, d_quot_out, quot_len, eval_out,
                   sync);
}

int open_shard_begin_device(Ctx* c, const uint32_t* d_polys, const size_t* lens, size_t k, size_t stride,
                            const uint32_t* z_words, const uint32_t* xi_words, uint64_t* chunk_eval_out) {
  return KZG_BY_FR(c, open_shard_begin_t, c, d_polys, lens, k, stride, z_words, xi_words, chunk_eval_out);
}
int open_shard_finish_device(Ctx* c, const uint32_t* z_words, const uint32_t* carry_words, int first_rank,
                             uint32_t** d_vec_out, size_t* vec_len, uint64_t* eval_out) {
  return KZG_BY_FR(c, open_shard_finish_t, c, z_words, carry_words, first_rank, d_vec_out, vec_len, eval_out);
}

int open_points_quotient_device(Ctx* c, const uint32_t* d_polys, const size_t* lens, size_t k, size_t stride,
                                const uint32_t* points, size_t t, const uint32_t* weights, uint32_t** d_quot_out,
                                size_t* quot_len) {
  return KZG_BY_FR(c, open_points_quotient_t, c, d_polys, lens, k, stride, points, t, weights, d_quot_out, quot_len);
}

int open_coset_check(Ctx* c, const size_t* lens, size_t k, size_t stride, uint32_t log_l, const uint32_t* h_words,
                     const uint32_t* zeta_words, size_t key_n) {
  size_t n = 0;
  return KZG_BY_FR(c, open_coset_check_t, c, lens, k, stride, log_l, h_words, zeta_words, key_n, &n);
}
int open_coset_quotient_device(Ctx* c, const uint32_t* d_polys, const size_t* lens, size_t k, size_t stride,
                               uint32_t log_l, const uint32_t* h_words, const uint32_t* zeta_words,
                               const uint32_t* xi_words, size_t key_n, uint32_t** d_quot_out, size_t* quot_len,
                               uint64_t* eval_out) {
  return KZG_BY_FR(c, open_coset_quotient_t, c, d_polys, lens, k, stride, log_l, h_words, zeta_words, xi_words, key_n,
                   d_quot_out, quot_len, eval_out);
}

// true iff any of the elements [from, to) of a canonical-word array is non-zero
int device_any_nonzero(Ctx* c, const uint32_t* d_words, size_t from, size_t to, bool* out) {
  *out = false;
  if (from >= to) return KZG_OK;
  DevTmp<uint32_t> d_flag;
  KZG_HIP(c, d_flag.alloc(4));
  KZG_HIP(c, hipMemsetAsync(d_flag, 0, 4, c->stream));
  hipLaunchKernelGGL(any_nonzero_kernel, dim3((uint32_t)((to - from + 255) / 256)), dim3(256), 0, c->stream, d_words,
                     from, to, d_flag.get());
  KZG_HIP(c, hipGetLastError());
  uint32_t f = 0;
  KZG_HIP(c, hipMemcpyAsync(&f, d_flag, 4, hipMemcpyDeviceToHost, c->stream));
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  *out = f != 0;
  return KZG_OK;
}

}  // namespace kzg

// =====================================================================================
// Device polynomial / vector primitives over Fr (include/kzg_mi355x.h "kzg_fr_*").  What the
// reference's callers get from Sage's dense polynomial arithmetic (plonk/prover.py:243-316:
// accumulator ratios, products, division by Z_H on a coset) expressed as data-parallel passes
// over device-resident coefficient / evaluation vectors.
// =====================================================================================
namespace kzg {
namespace {

enum : int { VEC_ADD = 0, VEC_SUB = 1, VEC_MUL = 2 };

template <class F>
__global__ void vec_binary_kernel(int op, size_t n, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  using Fd = Field<F>;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fe<F> x = load_words<F>(a + i * 8), y = load_words<F>(b + i * 8);
  Fe<F> r;
  if (op == VEC_ADD) r = Fd::add(x, y);
  else if (op == VEC_SUB) r = Fd::sub(x, y);
  else r = Fd::mul(Fd::to_mont(x), y);          // (xR)*y/R = x*y
  store_words<F>(out + i * 8, r);
}

// Everything a lincomb launch needs travels in the kernel arguments (3.1 KB of the 4 KB limit): no
// staging copy, no host synchronisation, so a chain of vector operations is enqueued without stalls.
constexpr int FR_LIMBS = 9;       // both scalar fields: 9 x 29-bit limbs
struct ScalarLincombArgs {
  const uint32_t* ptr[MAXK];
  uint32_t len[MAXK];
  uint32_t scal[MAXK * FR_LIMBS];   // s_j, Montgomery form
  uint32_t k;
};
// out[i] = sum_j s_j * p_j[i]  (s_j in Montgomery form; p_j shorter than n count as zero-padded); groups of DOT_G
// terms share one Montgomery reduction
template <class F>
__global__ void vec_lincomb_kernel(ScalarLincombArgs a, uint32_t* out, uint32_t n) {
  using Fd = Field<F>;
  static_assert(F::N == FR_LIMBS, "scalar fields have 9 limbs");
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  Fe<F> acc = Fd::zero();
  for (uint32_t j0 = 0; j0 < a.k; j0 += DOT_G) {
    const uint32_t cnt = min(DOT_G, a.k - j0);
    Fe<F> c[DOT_G], x[DOT_G];
#pragma unroll
    for (uint32_t g = 0; g < DOT_G; ++g) {
      const uint32_t j = j0 + g;
      const bool on = g < cnt && t < a.len[j];
      c[g] = on ? load_words<F>(a.ptr[j] + (size_t)t * 8) : Fd::zero();
      x[g] = load_limbs<F>(a.scal + (g < cnt ? j : j0) * F::N);
    }
    const Fe<F> part = dot_upto<F>(cnt, c, x);
    acc = j0 ? Fd::add(acc, part) : part;
  }
  store_words<F>(out + (size_t)t * 8, acc);
}

// out[i] = a[i] * c * s^i : thread handles LC consecutive i (one pow per chunk, then a running product)
struct PowArgs {
  uint32_t s[FR_LIMBS], c[FR_LIMBS];   // Montgomery form, in the kernel arguments
  uint32_t step[FR_LIMBS];             // s^(threads of the launch)
};
// Thread t takes the elements t, t + T, t + 2T, .. (T = threads of the launch): consecutive lanes touch consecutive
// 32-byte elements (round 2 gave a thread LC consecutive elements -- a 1 KB lane stride, four times the bytes through
// the memory system and 0.5 ms per 2^22 elements in the prover's coset shifts).  p = c * s^t by square-and-multiply
// once, then p *= s^T per element (sc.step, computed by the host).
template <class F>
__global__ void vec_mul_powers_kernel(size_t n, const uint32_t* a, PowArgs sc, uint32_t* out) {
  using Fd = Field<F>;
  static_assert(F::N == FR_LIMBS, "scalar fields have 9 limbs");
  const size_t T = (size_t)gridDim.x * blockDim.x;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  Fe<F> b = load_limbs<F>(sc.s), p = load_limbs<F>(sc.c);   // p = c (Montgomery)
  for (size_t bits = t; bits; bits >>= 1) {                 // p = c * s^t
    if (bits & 1u) p = Fd::mul(p, b);
    b = Fd::mul(b, b);
  }
  const Fe<F> step = load_limbs<F>(sc.step);
  for (size_t i = t; i < n; i += T) {
    store_words<F>(out + i * 8, Fd::mul(load_words<F>(a + i * 8), p));
    p = Fd::mul(p, step);
  }
}

// out[i] = a[i]^-1 (0 -> 0), Fermat: one exponentiation per element.  Used when out aliases a.
template <class F>
__global__ void vec_inverse_fermat_kernel(size_t n, const uint32_t* a, uint32_t* out) {
  using Fd = Field<F>;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fe<F> x = Fd::to_mont(load_words<F>(a + i * 8));
  store_words<F>(out + i * 8, Fd::from_mont(Fd::inv(x)));
}
// The same by batch inversion (Montgomery's trick) over LC elements per thread -- the elements t, t + T, t + 2T, ..
// (T = threads of the launch), so that consecutive lanes touch consecutive elements (round 2 batched LC CONSECUTIVE
// elements: a 1 KB lane stride).  The output buffer first receives the running products of the non-zero elements
// (Montgomery form), one exponentiation inverts the batch product, and the backward sweep peels the inverses off:
// 5 multiplications per element + 1/LC of an exponentiation instead of a whole one (~380).
template <class F>
__global__ void vec_inverse_kernel(size_t n, const uint32_t* a, uint32_t* out) {
  using Fd = Field<F>;
  const size_t T = (size_t)gridDim.x * blockDim.x;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  Fe<F> acc = Fd::one();
  size_t last = t;
  for (size_t i = t; i < n; i += T) {
    store_words<F>(out + i * 8, acc);                       // product of the non-zero elements of the batch before i
    const Fe<F> x = Fd::to_mont(load_words<F>(a + i * 8));
    if (!Fd::is_zero(x)) acc = Fd::mul(acc, x);
    last = i;
  }
  Fe<F> inv = Fd::inv(acc);                                 // acc is a product of non-zero elements (or one)
  for (size_t i = last;; i -= T) {
    const Fe<F> x = Fd::to_mont(load_words<F>(a + i * 8));
    if (Fd::is_zero(x)) {
      store_words<F>(out + i * 8, Fd::zero());
    } else {
      const Fe<F> pre = load_words<F>(out + i * 8);
      store_words<F>(out + i * 8, Fd::from_mont(Fd::mul(inv, pre)));
      inv = Fd::mul(inv, x);
    }
    if (i == t) break;
  }
}

// Exclusive prefix product out[i] = prod_{j<i} a[j], three steps with chunks of LC:
//   1 chunk products (and level-up while more than LC chunks remain), 2 serial scan of the top,
//   3 refill.  Values travel in Montgomery form between the steps.
template <class F, bool WORDS_IN>
__global__ void chunk_prod_kernel(const uint32_t* in, uint32_t m, uint32_t* prod) {
  using Fd = Field<F>;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t j0 = t * LC;
  if (j0 >= m) return;
  const uint32_t j1 = min(j0 + LC, m);
  Fe<F> acc = Fd::one();
  for (uint32_t j = j0; j < j1; ++j)
    acc = Fd::mul(acc, WORDS_IN ? Fd::to_mont(load_words<F>(in + (size_t)j * 8)) : load_limbs<F>(in + (size_t)j * F::N));
  store_limbs<F>(prod + (size_t)t * F::N, acc);
}
template <class F>
__global__ void top_prefix_kernel(const uint32_t* in, uint32_t m, uint32_t* pre) {   // pre[j] = prod_{i<j} in[i]
  using Fd = Field<F>;
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  Fe<F> acc = Fd::one();
  for (uint32_t j = 0; j < m; ++j) {
    store_limbs<F>(pre + (size_t)j * F::N, acc);
    acc = Fd::mul(acc, load_limbs<F>(in + (size_t)j * F::N));
  }
}
// pre_out[j] for j in chunk t = pre_up[t] * prod_{chunk start <= i < j} in[i]
template <class F, bool FINAL>
__global__ void chunk_prefix_fill_kernel(const uint32_t* in, uint32_t m, const uint32_t* pre_up, uint32_t* pre_out) {
  using Fd = Field<F>;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t j0 = t * LC;
  if (j0 >= m) return;
  const uint32_t j1 = min(j0 + LC, m);
  Fe<F> acc = load_limbs<F>(pre_up + (size_t)t * F::N);
  for (uint32_t j = j0; j < j1; ++j) {
    if (FINAL) {
      store_words<F>(pre_out + (size_t)j * 8, Fd::from_mont(acc));
      acc = Fd::mul(acc, Fd::to_mont(load_words<F>(in + (size_t)j * 8)));
    } else {
      store_limbs<F>(pre_out + (size_t)j * F::N, acc);
      acc = Fd::mul(acc, load_limbs<F>(in + (size_t)j * F::N));
    }
  }
}

template <class F>
int vec_binary_t(Ctx* c, int op, size_t n, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  if (n == 0) return KZG_OK;
  hipLaunchKernelGGL(vec_binary_kernel<F>, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, c->stream, op, n, a, b, out);
  KZG_HIP(c, hipGetLastError());
  return KZG_OK;
}

template <class F>
int vec_lincomb_t(Ctx* c, size_t n, size_t k, const uint32_t* const* ptrs, const size_t* lens, const uint32_t* scalars,
                  uint32_t* out) {
  using Fd = Field<F>;
  if (k > MAXK) return set_err(c, KZG_ERR_ARG, "kzg_fr_vec_lincomb: more than 64 terms");
  if (n == 0) return KZG_OK;
  if (n >= (1ull << 32)) return set_err(c, KZG_ERR_ARG, "vector too long");
  ScalarLincombArgs la{};
  la.k = (uint32_t)k;
  for (size_t j = 0; j < k; ++j) {
    const Fe<F> s = Fd::to_mont(Fd::from_words(scalars + j * 8));
    memcpy(&la.scal[j * F::N], s.l, F::N * 4);
    la.ptr[j] = ptrs[j];
    la.len[j] = (uint32_t)std::min(lens[j], n);
  }
  hipLaunchKernelGGL(vec_lincomb_kernel<F>, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, c->stream, la, out,
                     (uint32_t)n);
  KZG_HIP(c, hipGetLastError());
  return KZG_OK;
}

template <class F>
int vec_mul_powers_t(Ctx* c, size_t n, const uint32_t* a, const uint32_t* s_words, const uint32_t* c_words,
                     uint32_t* out) {
  using Fd = Field<F>;
  if (n == 0) return KZG_OK;
  const Fe<F> s = Fd::to_mont(Fd::from_words(s_words)), cc = Fd::to_mont(Fd::from_words(c_words));
  PowArgs sc;
  memcpy(sc.s, s.l, F::N * 4);
  memcpy(sc.c, cc.l, F::N * 4);
  // LC elements per thread; the thread count is a power of two so that s^T is log2(T) squarings on the host
  uint32_t lt = 7;
  while (((size_t)LC << lt) < n && lt < 24) ++lt;
  const size_t T = (size_t)1 << lt;
  Fe<F> step = s;
  for (uint32_t q = 0; q < lt; ++q) step = Fd::mul(step, step);
  memcpy(sc.step, step.l, F::N * 4);
  hipLaunchKernelGGL(vec_mul_powers_kernel<F>, dim3((uint32_t)(T / 128)), dim3(128), 0, c->stream, n, a, sc, out);
  KZG_HIP(c, hipGetLastError());
  return KZG_OK;
}

template <class F>
int vec_inverse_t(Ctx* c, size_t n, const uint32_t* a, uint32_t* out) {
  if (n == 0) return KZG_OK;
  if (a == out) {     // in place: the batch kernel needs the output buffer as scratch next to the input
    hipLaunchKernelGGL(vec_inverse_fermat_kernel<F>, dim3((uint32_t)((n + 127) / 128)), dim3(128), 0, c->stream, n, a,
                       out);
  } else {
    const size_t chunks = (n + LC - 1) / LC;
    hipLaunchKernelGGL(vec_inverse_kernel<F>, dim3((uint32_t)((chunks + 63) / 64)), dim3(64), 0, c->stream, n, a, out);
  }
  KZG_HIP(c, hipGetLastError());
  return KZG_OK;
}

template <class F>
int vec_prefix_product_t(Ctx* c, size_t n, const uint32_t* a, uint32_t* out) {
  if (n == 0) return KZG_OK;
  if (n >= (1ull << 31)) return set_err(c, KZG_ERR_ARG, "vector too long");
  std::vector<uint32_t> m{(uint32_t)n};
  while (m.back() > LC) m.push_back((m.back() + LC - 1) / LC);
  const size_t nl = m.size();
  size_t total = 0;
  for (size_t l = 1; l < nl; ++l) total += m[l];
  int rc;
  if ((rc = ensure_buf(c, c->poly_tmp[2], (total + 1) * F::N * 4))) return rc;      // chunk products per level
  if ((rc = ensure_buf(c, c->poly_tmp[3], (total + LC + 1) * F::N * 4))) return rc; // prefixes per level
  uint32_t* d_p = static_cast<uint32_t*>(c->poly_tmp[2].p);
  uint32_t* d_q = static_cast<uint32_t*>(c->poly_tmp[3].p);
  std::vector<uint32_t*> pp(nl, nullptr), qq(nl, nullptr);
  {
    uint32_t* x = d_p; uint32_t* y = d_q;
    for (size_t l = 1; l < nl; ++l) { pp[l] = x; x += (size_t)m[l] * F::N; qq[l] = y; y += (size_t)m[l] * F::N; }
  }
  auto grid = [](uint32_t chunks) { return dim3((chunks + 127) / 128); };
  if (nl == 1) {
    // a single chunk: its incoming prefix is 1
    const Fe<F> one = Field<F>::one();
    KZG_HIP(c, hipMemcpyAsync(d_q, one.l, F::N * 4, hipMemcpyHostToDevice, c->stream));
    KZG_HIP(c, hipStreamSynchronize(c->stream));
    hipLaunchKernelGGL((chunk_prefix_fill_kernel<F, true>), dim3(1), dim3(64), 0, c->stream, a, m[0], d_q, out);
  } else {
    hipLaunchKernelGGL((chunk_prod_kernel<F, true>), grid(m[1]), dim3(128), 0, c->stream, a, m[0], pp[1]);
    for (size_t l = 1; l + 1 < nl; ++l)
      hipLaunchKernelGGL((chunk_prod_kernel<F, false>), grid(m[l + 1]), dim3(128), 0, c->stream, pp[l], m[l], pp[l + 1]);
    hipLaunchKernelGGL(top_prefix_kernel<F>, dim3(1), dim3(64), 0, c->stream, pp[nl - 1], m[nl - 1], qq[nl - 1]);
    for (size_t l = nl - 2; l >= 1; --l)
      hipLaunchKernelGGL((chunk_prefix_fill_kernel<F, false>), grid(m[l + 1]), dim3(128), 0, c->stream, pp[l], m[l],
                         qq[l + 1], qq[l]);
    hipLaunchKernelGGL((chunk_prefix_fill_kernel<F, true>), grid(m[1]), dim3(128), 0, c->stream, a, m[0], qq[1], out);
  }
  KZG_HIP(c, hipGetLastError());
  return KZG_OK;
}

// p(z) for a coefficient vector: pass 1 of the opening's scan without its stores (tile aggregates only), then the
// one-workgroup sum of the aggregates -- two launches (rounds 1-3 collapsed chunks of 8 level by level: seven)
template <class F>
int poly_eval_t(Ctx* c, size_t n, const uint32_t* a, const uint32_t* z_words, uint64_t* out) {
  memset(out, 0, 32);
  if (n == 0) return KZG_OK;
  if (n >= (1ull << 31) - 1) return set_err(c, KZG_ERR_ARG, "vector too long");
  if (n == 1 || words_are_zero(z_words)) {      // the constant coefficient
    KZG_HIP(c, hipMemcpyAsync(out, a, 32, hipMemcpyDeviceToHost, c->stream));
    KZG_HIP(c, hipStreamSynchronize(c->stream));
    return KZG_OK;
  }
  TileShape s;                                  // its own plan in its own buffers: an opening's slice stays
  TilePass1 p;
  int rc = tile_plan<F>(c, n, z_words, 256, c->poly_tmp[2], &s, &p, /*with_chunks=*/false);
  if (rc) return rc;
  if ((rc = ensure_buf(c, c->poly_tmp[3], 32))) return rc;
  uint32_t* d_val = static_cast<uint32_t*>(c->poly_tmp[3].p);
  if ((rc = launch_tile_combine<F, 256, false>(c, s, p, lincomb_of_one<F>(a, n), nullptr))) return rc;
  if ((rc = launch_tile_eval<F, 256>(c, s, d_val))) return rc;
  KZG_HIP(c, hipMemcpyAsync(out, d_val, 32, hipMemcpyDeviceToHost, c->stream));
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  return KZG_OK;
}

// p_i(z_j) for k polynomials at t points: pass 1 without its stores over MP points at a time (a polynomial is read
// once per launch, blockIdx.y picks it), then one workgroup per (polynomial, point) sums that pair's tile aggregates.
// Buffers of its own, as poly_eval_t: the tables, W per point and H per (point, polynomial) in poly_tmp[2], the
// values in poly_tmp[3].  n = 0, n = 1 and z = 0 as in poly_eval_t: nothing, or the constant coefficient.
template <class F>
int poly_eval_batch_t(Ctx* c, const uint32_t* d_polys, const size_t* lens, size_t k, size_t stride,
                      const uint32_t* points, size_t t, uint64_t* out) {
  constexpr uint32_t TB = 256;
  if (k > MAXK || t > MAXK) return set_err(c, KZG_ERR_ARG, "kzg_fr_poly_eval_batch: more than 64 polynomials or points");
  if (!k || !t) return KZG_OK;
  memset(out, 0, k * t * 32);
  size_t n = 0;
  EvalBatchArgs ea{};
  ea.polys = d_polys, ea.stride = stride;
  for (size_t i = 0; i < k; ++i) {
    if (lens[i] > stride) return set_err(c, KZG_ERR_ARG, "kzg_fr_poly_eval_batch: lens[i] > stride");
    n = std::max(n, lens[i]);
    ea.lens[i] = (uint32_t)lens[i];
  }
  if (n >= (1ull << 31) - 1) return set_err(c, KZG_ERR_ARG, "vector too long");
  if (n == 0) return KZG_OK;
  std::vector<MultiPoint> table;
  for (size_t j = 0; j < t; ++j) {
    const MultiPoint m = multi_point<F>(points + j * 8, TB);
    ea.slot[j] = m.zero ? MAXK : (uint32_t)table.size();
    if (!m.zero) table.push_back(m);
  }
  TileShape s0;
  uint32_t ntab = 0;
  tile_counts(c, n, TB, &s0, &ntab);
  const size_t nz = n > 1 ? table.size() : 0;        // points that need the scan
  const uint32_t hstride = s0.ntiles + 1, wstride = s0.ntiles;
  MultiPoint* d_table = nullptr;
  uint32_t *d_H = nullptr, *d_W = nullptr;
  int rc = carve(c, c->poly_tmp[2], [&](Carve& ws) {
    d_table = ws.take<MultiPoint>((nz + 1) * sizeof(MultiPoint));
    d_H = ws.take((nz * k * hstride + 1) * F::N * 4);
    d_W = ws.take((nz * wstride + 1) * F::N * 4);
  });
  if (rc) return rc;
  if ((rc = ensure_buf(c, c->poly_tmp[3], k * t * 32))) return rc;
  uint32_t* d_val = static_cast<uint32_t*>(c->poly_tmp[3].p);
  {
    ProfScope ps(c, "poly_eval_batch");
    if (nz) KZG_HIP(c, hipMemcpyAsync(d_table, table.data(), nz * sizeof(MultiPoint), hipMemcpyHostToDevice, c->stream));
    for (size_t j0 = 0; j0 < nz; j0 += MP) {
      const uint32_t np = (uint32_t)std::min<size_t>(MP, nz - j0);
      TileShape shapes[MP];                        // no chunk values, no groups: H per (point, polynomial), W per point
      for (uint32_t q = 0; q < np; ++q) {
        shapes[q] = s0;
        shapes[q].H = d_H + (j0 + q) * k * hstride * F::N;
        shapes[q].W = d_W + (j0 + q) * wstride * F::N;
      }
      for (size_t i0 = 0; i0 < k; i0 += TILE_MAXK) {
        MultiPolys mp{};
        mp.polys = d_polys, mp.stride = stride, mp.k = (uint32_t)std::min<size_t>(TILE_MAXK, k - i0);
        for (uint32_t q = 0; q < mp.k; ++q) mp.row[q] = (uint32_t)(i0 + q), mp.lens[q] = ea.lens[i0 + q];
        // the W tables come from the first launch of a group of points
        if ((rc = launch_tile_combine_multi<F, TB, false>(c, shapes, np, i0 ? 0 : ntab, mp, d_table + j0, nullptr, 0,
                                                          (uint32_t)i0, hstride)))
          return rc;
      }
    }
    hipLaunchKernelGGL((tile_eval_batch_kernel<F, TB>), dim3((uint32_t)k, (uint32_t)t), dim3(TB), 0, c->stream, ea,
                       (uint32_t)k, d_H, hstride, d_W, wstride, (uint32_t)t, d_val);
    KZG_HIP(c, hipGetLastError());
  }
  KZG_HIP(c, hipMemcpyAsync(out, d_val, k * t * 32, hipMemcpyDeviceToHost, c->stream));
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  return KZG_OK;
}

}  // namespace

int fr_poly_eval_batch(Ctx* c, const uint32_t* d_polys, const size_t* lens, size_t k, size_t stride,
                       const uint32_t* points, size_t t, uint64_t* out) {
  return KZG_BY_FR(c, poly_eval_batch_t, c, d_polys, lens, k, stride, points, t, out);
}

int fr_vec_binary(Ctx* c, int op, size_t n, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  return KZG_BY_FR(c, vec_binary_t, c, op, n, a, b, out);
}
int fr_vec_lincomb(Ctx* c, size_t n, size_t k, const uint32_t* const* ptrs, const size_t* lens, const uint32_t* scalars,
                   uint32_t* out) {
  return KZG_BY_FR(c, vec_lincomb_t, c, n, k, ptrs, lens, scalars, out);
}
int fr_vec_mul_powers(Ctx* c, size_t n, const uint32_t* a, const uint32_t* s, const uint32_t* cc, uint32_t* out) {
  return KZG_BY_FR(c, vec_mul_powers_t, c, n, a, s, cc, out);
}
int fr_vec_inverse(Ctx* c, size_t n, const uint32_t* a, uint32_t* out) { return KZG_BY_FR(c, vec_inverse_t, c, n, a, out); }
int fr_vec_prefix_product(Ctx* c, size_t n, const uint32_t* a, uint32_t* out) {
  return KZG_BY_FR(c, vec_prefix_product_t, c, n, a, out);
}
int fr_poly_eval(Ctx* c, size_t n, const uint32_t* a, const uint32_t* z, uint64_t* out) {
  return KZG_BY_FR(c, poly_eval_t, c, n, a, z, out);
}

}  // namespace kzg
