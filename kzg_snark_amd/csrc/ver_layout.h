// ver_layout.h -- the workspaces of the two bulk verifications.  kzg_prof_read reports their totals, so order and
// sizes are pinned by tests; like devmem.h this compiles for the CPU, the sizes from device headers passed in.
#pragma once
#include "devmem.h"

namespace kzg {

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
