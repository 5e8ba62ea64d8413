// g2_lincomb.hip -- linear combinations on the twist on gfx950: out = sum_i [k_i] Q_i as ONE point of
// G2's curve, the sum that kzg_g2_mul_each leaves to its caller.  Behind kzg_g2_lincomb and kzg_g2_lincomb_powers.
//
//   points   canonical affine words x.c0 | x.c1 | y.c0 | y.c1 and an optional infinity flag, validated by import_g2's
//            rule; any point of the twist is legal, inside the subgroup or not
//   scalars  n x 8 words taken as the 256-bit integers they are, or c0 s^i mod r from the power table of fr_util.h
//   product  g2_lincomb_kernel: one lane per point runs g_mul.h's ladder over its column of the table
//            ([multiple][piece][lane], g_mul_dev.h) and keeps the Jacobian result: no inversion per lane
//   wave     the 64 lanes of a workgroup add their results through LDS ([limb][lane], half the lanes park, the other
//            half add) with the FULL addition of g2_lincomb.h, and lane 0 writes one partial sum
//   fold     g2_lincomb_fold_kernel: a workgroup adds GL_FOLD_SPAN points, four per lane and then the same wave sum;
//            the last level is one workgroup and ends in the call's only inversion
// GlPlan (g2_lincomb.h) cuts a call into launches of at most GL_LAUNCH_LANES lanes over one table and states the
// partial sums and the levels of the fold.
#include <algorithm>
#include <string>
#include <string.h>
#include "msm.h"
#include "g_mul_dev.h"
#include "g2_lincomb.h"

namespace kzg {

namespace {

// the sum of the workgroup's 64 points in lane 0: in every round s = 32 .. 1 the lanes s <= t < 2s park their points in
// LDS and lane t - s adds them.  A pair of lanes may hold P and P, P and -P, or O: the full addition.
template <class C>
__device__ __forceinline__ Jac2<C> gl_wave_sum(Jac2<C> acc, uint32_t* sh) {
  const uint32_t tid = threadIdx.x;
#pragma unroll 1
  for (uint32_t s = GL_TB / 2; s >= 1; s >>= 1) {
    if (tid >= s && tid < 2 * s) g2_put_limbs<C>(acc, sh + (tid - s), GL_TB / 2);
    __syncthreads();
    if (tid < s) g2_add_full<C>(acc, g2_get_limbs<C>(sh + tid, GL_TB / 2));
    __syncthreads();
  }
  return acc;
}

// partial[first / GL_TB + blockIdx.x] = the sum over the workgroup's lanes of [k_i] Q_i, i = first + the lane's index
// in the launch; a lane with i >= n, and a point that is refused (its index goes to *bad, the smallest wins), adds
// infinity.  tab: gridDim.x * GL_TB columns.
template <class C>
__global__ __launch_bounds__(GL_TB) void g2_lincomb_kernel(uint32_t n, uint32_t first, const uint32_t* xy,
                                                           const uint8_t* inf, GmScalars sc, uint2* tab,
                                                           uint32_t* partial, uint32_t* bad) {
  constexpr int NW = C::Fp::NW;
  __shared__ uint32_t sh[g2_point_limbs<C>() * (GL_TB / 2)];
  const uint32_t slot = blockIdx.x * GL_TB + threadIdx.x, i = first + slot;
  Jac2<C> acc = g2_infinity<C>();
  if (i < n) {
    uint32_t w[4 * NW];
    ld_words<4 * NW>(xy + (size_t)i * 4 * NW, w);
    const bool is_inf = inf && inf[i];
    Fp2<C> x = Tower<C>::zero2(), y = Tower<C>::zero2();
    if (is_inf || Tower<C>::import_g2(w, x, y)) {
      uint32_t k[8];
      gm_scalar<C>(sc, i, k);
      G2Tab<C> column;
      column.tab = tab; column.slots = gridDim.x * GL_TB; column.slot = slot;
      acc = g2_mul<C>(x, y, is_inf, k, column);
    } else {
      atomicMin(bad, i);
    }
  }
  acc = gl_wave_sum<C>(acc, sh);
  if (threadIdx.x == 0) g2_put_limbs<C>(acc, partial + (first / GL_TB + blockIdx.x) * g2_point_limbs<C>(), 1);
}

// workgroup b adds in[b * GL_FOLD_SPAN .. min(count, (b + 1) * GL_FOLD_SPAN)).  out_xy == null: the sum goes to out[b];
// else (one workgroup) it is the call's result: canonical words and the infinity flag, after one inversion.
template <class C>
__global__ __launch_bounds__(GL_FOLD_TB) void g2_lincomb_fold_kernel(uint32_t count, const uint32_t* in, uint32_t* out,
                                                                     uint32_t* out_xy, uint8_t* out_inf) {
  constexpr int NW = C::Fp::NW;
  static_assert(GL_FOLD_TB == GL_TB, "the fold shares the wave sum of the product stage");
  __shared__ uint32_t sh[g2_point_limbs<C>() * (GL_TB / 2)];
  const uint32_t lo = blockIdx.x * GL_FOLD_SPAN, hi = min(count, lo + GL_FOLD_SPAN);
  Jac2<C> acc = g2_infinity<C>();
#pragma unroll 1
  for (uint32_t b = lo + threadIdx.x; b < hi; b += GL_FOLD_TB)
    g2_add_full<C>(acc, g2_get_limbs<C>(in + b * g2_point_limbs<C>(), 1));
  acc = gl_wave_sum<C>(acc, sh);
  if (threadIdx.x != 0) return;
  if (out_xy) {
    uint32_t w[4 * NW];
    const bool flag = g2_to_words<C>(acc, w);
    st_words<4 * NW>(out_xy, w);
    *out_inf = flag ? 1 : 0;
  } else {
    g2_put_limbs<C>(acc, out + blockIdx.x * g2_point_limbs<C>(), 1);
  }
}

// ---- host side --------------------------------------------------------------------------------------

// what a call keeps in the context's buffer: the table, the first refused index, the power table (power form), the
// staged arrays, the partial sums of the product stage and of the fold's levels (alternating), the result
struct GlWs {
  uint2* tab; uint32_t* bad; uint32_t* ptab; uint32_t* xy; uint8_t* inf; uint32_t* k; uint32_t* part[2];
  uint32_t* out_xy; uint8_t* out_inf;
  void layout(Carve& ws, const GlPlan& plan, size_t table_bytes, bool powers, size_t n, size_t point_bytes, bool has_inf,
              size_t partial_bytes) {
    tab = ws.take<uint2>(table_bytes);
    bad = ws.take(4);
    ptab = ws.take_if<uint32_t>(powers, (size_t)POW_TAB * 32);
    xy = ws.take<uint32_t>(n * point_bytes);
    inf = ws.take_if<uint8_t>(has_inf, n);
    k = ws.take_if<uint32_t>(!powers, n * 32);
    part[0] = ws.take(plan.width[0] * partial_bytes);
    part[1] = ws.take((size_t)plan.width[1] * partial_bytes);
    out_xy = ws.take(point_bytes);
    out_inf = ws.take<uint8_t>(1);
  }
};

template <class C>
int g2_lincomb_t(Ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, const uint32_t* k, const uint32_t* s,
                 const uint32_t* c0, uint64_t* out_xy, uint8_t* out_inf, const char* who) {
  constexpr size_t PT_BYTES = 4 * C::Fp::NW * 4, PART_BYTES = g2_point_limbs<C>() * 4;
  const bool powers = s != nullptr;
  if (powers) {                                            // the power form's scalars are checked whatever n is
    if (int rc = check_scalar<C>(c, s, who, "s")) return rc;
    if (int rc = check_scalar<C>(c, c0, who, "c0")) return rc;
  }
  if (n == 0) {                                            // the empty sum
    memset(out_xy, 0, PT_BYTES);
    *out_inf = 1;
    return KZG_OK;
  }
  const GlPlan plan(n, gm_g2_pieces<C>(), g2_point_limbs<C>());
  if (!plan.ok) return set_err(c, KZG_ERR_ARG, "g2_lincomb: the plan of the call does not fit its 32-bit indices");
  GlWs d;
  int rc = carve(c, c->gmul_tmp, [&](Carve& ws) {
    d.layout(ws, plan, g2_column_bytes<C>() * GL_TB * plan.mul.launch_blocks, powers, n, PT_BYTES, inf != nullptr, PART_BYTES);
  });
  if (rc) return rc;
  GmScalars sc;
  if ((rc = scalars_of<C>(c, d.k, s, c0, d.ptab, who, &sc))) return rc;
  ProfScope ps(c, "g2_lincomb");
  hipStream_t st = c->stream;
  KZG_HIP(c, hipMemcpyAsync(d.xy, xy, n * PT_BYTES, hipMemcpyHostToDevice, st));
  if (inf) KZG_HIP(c, hipMemcpyAsync(d.inf, inf, n, hipMemcpyHostToDevice, st));
  if (!powers) KZG_HIP(c, hipMemcpyAsync(d.k, k, n * 32, hipMemcpyHostToDevice, st));
  KZG_HIP(c, hipMemsetAsync(d.bad, 0xff, 4, st));
  for (uint32_t b0 = 0; b0 < plan.mul.blocks; b0 += plan.mul.launch_blocks) {
    hipLaunchKernelGGL(g2_lincomb_kernel<C>, dim3(std::min(plan.mul.launch_blocks, plan.mul.blocks - b0)), dim3(GL_TB), 0,
                       st, (uint32_t)n, b0 * GL_TB, d.xy, d.inf, sc, d.tab, d.part[0], d.bad);
    KZG_HIP(c, hipGetLastError());
  }
  for (uint32_t l = 0; l < plan.levels; ++l) {
    const bool last = l + 1 == plan.levels;
    hipLaunchKernelGGL(g2_lincomb_fold_kernel<C>, dim3(plan.width[l + 1]), dim3(GL_FOLD_TB), 0, st, plan.width[l],
                       d.part[l & 1], d.part[(l + 1) & 1], last ? d.out_xy : nullptr, last ? d.out_inf : nullptr);
    KZG_HIP(c, hipGetLastError());
  }
  // the result waits on the host until the call is known to be good: a refusal writes nothing to the outputs
  uint32_t bad = GM_NONE, w[PT_BYTES / 4];
  uint8_t flag = 0;
  KZG_HIP(c, hipMemcpyAsync(&bad, d.bad, 4, hipMemcpyDeviceToHost, st));
  KZG_HIP(c, hipMemcpyAsync(w, d.out_xy, PT_BYTES, hipMemcpyDeviceToHost, st));
  KZG_HIP(c, hipMemcpyAsync(&flag, d.out_inf, 1, hipMemcpyDeviceToHost, st));
  KZG_HIP(c, hipStreamSynchronize(st));
  if (bad != GM_NONE) return refuse(c, who, bad, "twist");
  memcpy(out_xy, w, PT_BYTES);
  *out_inf = flag;
  return KZG_OK;
}

}  // namespace

int g2_lincomb(Ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, const uint32_t* k, const uint32_t* s,
               const uint32_t* c0, uint64_t* out_xy, uint8_t* out_inf) {
  const char* who = s ? "kzg_g2_lincomb_powers" : "kzg_g2_lincomb";
  if (int rc = size_check(c, n, who)) return rc;
  return KZG_BY_CURVE(c, g2_lincomb_t, c, xy, inf, n, k, s, c0, out_xy, out_inf, who);
}

}  // namespace kzg
