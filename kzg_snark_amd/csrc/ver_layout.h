// ver_layout.h -- the launch plan of kzg_verify_cosets and the workspaces of the two bulk verifications.  The plan
// decides which regime of the kernels a call reaches and kzg_prof_read reports the workspaces' totals, so both are
// pinned by tests; like devmem.h this compiles for the CPU, the sizes from device headers passed in.
#pragma once
#include "devmem.h"

namespace kzg {

// ---- the launches of kzg_verify_cosets (verify.hip; tests/test_verify_scalars_host.py through the shim) ------------
constexpr uint32_t VER_MIN_TILE_LOG = 8;                        // ver_cell_kernel: tile of max(l, 256) elements
constexpr uint32_t VER_CELL_GRID = 4096;                        // ver_cell_kernel: workgroups at most, tiles by stride
constexpr uint32_t VER_SUM_THREADS = 1u << 15;                  // ver_colsum_kernel: threads (a multiple of every l)
constexpr uint32_t VER_COMM_SPLIT = 64;                         // ver_commsum_kernel: workgroups per commitment when few

inline uint32_t ver_shares(size_t n_comm) { return n_comm >= VER_COMM_SPLIT ? 1 : VER_COMM_SPLIT; }

// K claims of 2^log_l values over n_comm commitments; the proofs as a key of win_bits-wide windows, scalars of fr_bits
struct VerPlan {
  size_t M;                  // values in all
  uint32_t log_e;            // ver_cell_kernel: a tile is 2^log_e elements, whole cells
  size_t ntiles, lds_bytes;  //   tiles (the last one may be short) and the dynamic LDS of a workgroup
  uint32_t cell_grid;        //   workgroups: above VER_CELL_GRID tiles a workgroup takes more than one
  uint32_t sum_threads;      // ver_colsum_kernel: threads, sum_cnt of them per column for ver_colsum_final_kernel
  uint32_t sum_cnt;
  uint32_t shares;           // ver_commsum_kernel: workgroups per commitment
  uint32_t slice_bits;       // ver_slice_kernel: a scalar is cut into `slices` pieces of slice_bits bits
  uint32_t slices;
  VerPlan(size_t K, uint32_t log_l, size_t n_comm, uint32_t win_bits, uint32_t fr_bits) {
    M = K << log_l;
    log_e = log_l > VER_MIN_TILE_LOG ? log_l : VER_MIN_TILE_LOG;
    ntiles = (M + ((size_t)1 << log_e) - 1) >> log_e;
    lds_bytes = (size_t)32 << log_e;
    cell_grid = (uint32_t)(ntiles < VER_CELL_GRID ? ntiles : VER_CELL_GRID);
    sum_threads = ((uint32_t)1 << log_l) > VER_SUM_THREADS ? (uint32_t)1 << log_l : VER_SUM_THREADS;
    sum_cnt = sum_threads >> log_l;
    shares = ver_shares(n_comm);
    slice_bits = win_bits - 1;
    slices = (fr_bits + slice_bits - 1) / slice_bits;
  }
};

// verify.hip, ver_tmp: K claims of l values over n_comm commitments; points of pt_bytes, key records of rb bytes
struct VerifyWs {
  uint32_t *pxy, *cxy, *recs, *vals, *r, *s, *slice, *cidx, *perm, *off, *wtab, *rtab, *part, *cpart, *T, *coef, *bad;
  uint8_t *pinf, *cinf;      // null: no flags given
  void layout(Carve& w, size_t K, size_t n_comm, size_t l, bool proof_flags, bool comm_flags, size_t pt_bytes,
              size_t rb, size_t pow_tab, size_t sum_threads, size_t nsp) {
    pxy = w.take(K * pt_bytes);       pinf = w.take_if(proof_flags, K);
    cxy = w.take(n_comm * pt_bytes);  cinf = w.take_if(comm_flags, n_comm);
    recs = w.take(K * rb);            vals = w.take(K * l * 32);
    r = w.take(K * 32);               s = w.take(K * 32);               slice = w.take(K * 32);
    cidx = w.take(K * 4);             perm = w.take(K * 4);             off = w.take((n_comm + 1) * 4);
    wtab = w.take(pow_tab * 32);      rtab = w.take(pow_tab * 32);      part = w.take(sum_threads * 32);
    cpart = w.take(n_comm * nsp * 32);  T = w.take(l * 32);             coef = w.take(n_comm * 32);
    bad = w.take(4);
  }
};

// verify_points.hip, vpt_tmp: K claims over n_comm commitments and the generator; `blocks` partial points of xyzz
// bytes and a table of tab_bytes for the ladders
struct VerifyPointsWs {
  uint32_t *pxy, *cxy, *precs, *crecs, *z, *y, *r, *s, *perm, *off, *rtab, *ypart, *cpart, *coef, *partial, *out, *bad;
  uint8_t *pinf, *cinf;      // null: no flags given
  void* tab;
  void layout(Carve& w, size_t K, size_t n_comm, bool proof_flags, bool comm_flags, size_t pt_bytes, size_t rb,
              size_t pow_tab, size_t weight_threads, size_t nsp, size_t blocks, size_t xyzz, size_t tab_bytes) {
    const size_t n_short = n_comm + 1;
    pxy = w.take(K * pt_bytes);         pinf = w.take_if(proof_flags, K);
    cxy = w.take(n_short * pt_bytes);   cinf = w.take_if(comm_flags, n_short);
    precs = w.take(K * rb);             crecs = w.take(n_short * rb);
    z = w.take(K * 32);                 y = w.take(K * 32);
    r = w.take(K * 32);                 s = w.take(K * 32);
    perm = w.take(K * 4);               off = w.take((n_comm + 1) * 4);
    rtab = w.take(pow_tab * 32);        ypart = w.take(weight_threads * 32);
    cpart = w.take(n_comm * nsp * 32);  coef = w.take(n_short * 32);
    partial = w.take(blocks * xyzz);    out = w.take(3 * xyzz);
    bad = w.take(4);                    tab = w.take<void>(tab_bytes);
  }
};

}  // namespace kzg
