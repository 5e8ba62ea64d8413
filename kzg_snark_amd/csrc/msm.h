// msm.h -- library-private interface of msm.hip (SRS tables and the commit pipeline).
#pragma once
#include "internal.h"

namespace kzg {

// Device-resident commitment key: the reference's `ck` = [tau^i G1] (kzg.py:70-72),
// expanded to NWIN window multiples per point (layout: msm.hip header comment).
struct Srs {
  size_t n = 0;
  int curve = 0;
  int win_bits = 16;          // Pippenger window c: 20 for keys of >= 2^18 points, else 16
  int nwin = 16;              // ceil(256 / c) table windows
  uint32_t* recs = nullptr;   // [nwin][n] records of Curve::REC_WORDS words
  // basis of the key: monomial ([tau^i] G) or Lagrange over the domain {w^i} of n = 2^log_n points
  // ([L_i(tau)] G, lagrange.hip); a commit against a Lagrange key commits values
  int basis = 0;              // SRS_MONOMIAL | SRS_LAGRANGE
  uint32_t log_n = 0;         // Lagrange keys: domain size and root (canonical words)
  uint32_t w[8] = {0};
  uint32_t* d_wpow = nullptr; // Lagrange keys: w^i, i < n (canonical words, 32 B each)
};
constexpr int SRS_MONOMIAL = 0;
constexpr int SRS_LAGRANGE = 1;

void srs_free(Srs* s);
using SrsPtr = Owned<Srs, srs_free>;            // a key under construction: freed unless release()d to the caller
int srs_load(Ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, Srs** out);
// the same from points already on the device: canonical words x | y per point, flags or null (g1_bytes.hip)
int srs_load_device(Ctx* c, const uint32_t* d_xy, const uint8_t* d_inf, size_t n, Srs** out);
// run_len = 0: the contiguous range tau^(start + i); otherwise record i = tau^(start + (i / run_len) * outer_stride +
// (i % run_len) * inner_stride)
int srs_generate(Ctx* c, const uint64_t* tau, size_t start, size_t n, Srs** out, size_t run_len = 0,
                 size_t inner_stride = 1, size_t outer_stride = 0);
// canonical affine words (x | y per point, flags or null) -> window-0 records at d_recs; *d_bad counts the points that
// fail.  range = true: both coordinates below p and the curve equation (g1_words.h's import_affine: verification,
// compression).  range = false: the curve equation alone, coordinates taken modulo p (key loading).  Enqueue only.
__attribute__((visibility("hidden")))   // library-private: not in the exported symbol list
int g1_import(Ctx* c, const uint32_t* d_xy, const uint8_t* d_inf, size_t n, bool range, uint32_t* d_recs,
              uint32_t* d_bad);
int srs_export(Ctx* c, const Srs* s, size_t start, size_t count, uint64_t* xy, uint8_t* inf);
// record i = scalars[i] * G1 (device vector of n canonical scalars), windows built; synchronises
int srs_generate_scalars(Ctx* c, const uint32_t* d_scalars, size_t n, Srs** out);
// an n-point key whose window-0 records the caller fills, then srs_finish_windows (synchronises)
int srs_create(Ctx* c, size_t n, SrsPtr* out);
int srs_finish_windows(Ctx* c, Srs* s);
// `out` becomes a key of n points over caller-owned window-0 records and NO further window (nothing is allocated, the
// caller keeps `recs` alive and never calls srs_free on it): good for commits whose scalars are all below
// 2^(win_bits - 1), which yield one digit, in window 0 (verify.hip)
void srs_window0_view(const Ctx* c, uint32_t* recs, size_t n, Srs* out);
size_t srs_rec_bytes(int curve);

// lagrange.hip: evaluation-form keys and openings
int srs_lagrange(Ctx* c, const Srs* mono, uint32_t log_n, const uint32_t* w_words, Srs** out);
int srs_generate_lagrange(Ctx* c, const uint32_t* tau_words, uint32_t log_n, const uint32_t* w_words, Srs** out);
int open_evals_device(Ctx* c, const Srs* s, const uint32_t* d_vals, const size_t* lens, size_t k, size_t stride,
                      const uint32_t* z_words, const uint32_t* xi_words, uint64_t* out_xy, uint8_t* out_inf,
                      uint64_t* eval_out, bool sync);
int fr_eval_lagrange(Ctx* c, uint32_t log_n, const uint32_t* w_words, size_t len, const uint32_t* d_vals,
                     const uint32_t* z_words, uint64_t* out);
// b vectors over one domain, vector j (lens[j] values at d_vals + j * stride elements) at its own point d_z[j]:
// d_out[j] = fr_eval_lagrange's result.  Device pointers; a fixed number of launches per chunk, no wait for the call's
// own work (the host may wait for the previous call's copy of its lengths, and for a reallocation of the scratch).
int fr_eval_lagrange_batch(Ctx* c, uint32_t log_n, const uint32_t* w_words, const uint32_t* d_vals, const size_t* lens,
                           size_t b, size_t stride, const uint32_t* d_z, uint32_t* d_out);

// domain.hip: the radix-2 G1 transform in XYZZ, in place, one launch per level: `nvec` vectors of 2^log_len points
// (vector j at point j << log_len), bit-reversed in, natural out, unscaled; root a primitive 2^log_len-th root of
// unity in Montgomery form.  log_len <= 24 for one vector, nvec << log_len <= 2^31.
struct FrArg;   // fr_util.h
__attribute__((visibility("hidden")))   // library-private: not in the exported symbol list
int launch_levels(Ctx* c, uint32_t* d_buf, uint32_t nvec, uint32_t log_len, const FrArg& root);

// domain.hip: all n proofs on a domain (FK20).  A table holds DFT_G1,2n of the reversed monomial key.
struct DomainTable;
int domain_table_create(Ctx* c, const Srs* mono, uint32_t log_n, DomainTable** out);
void domain_table_free(DomainTable* t);
using DomainTablePtr = Owned<DomainTable, domain_table_free>;
size_t domain_table_size(const DomainTable* t);
int open_domain(Ctx* c, const DomainTable* t, const uint32_t* polys, bool host_polys, const size_t* lens, size_t b,
                size_t stride, const uint32_t* w_words, uint64_t* out_xy, uint8_t* out_inf, uint64_t* eval_out);
// Coset openings: a table of l sub-tables (l = 2^log_l; l = 1 is kzg_domain_table_create's) and N/l proofs per vector.
int coset_table_create(Ctx* c, const Srs* mono, uint32_t log_n, uint32_t log_l, DomainTable** out);
int open_cosets(Ctx* c, const DomainTable* t, const uint32_t* polys, bool host_polys, const size_t* lens, size_t b,
                size_t stride, uint32_t log_N, const uint32_t* w_words, uint64_t* out_xy, uint8_t* out_inf,
                uint64_t* eval_out);

// One MSM per polynomial; scalars device-resident, results to host memory (synchronises).
// drain = false leaves up to four polynomials in flight; their outputs are written when their
// slot is recycled by a later call or by commit_flush().
// d_eval / out_eval (pipelined open, n_polys == 1): 32 bytes at d_eval -- written by work already enqueued on the
// context's stream -- are delivered to out_eval when the polynomial's slot is retired, together with its point.
int commit_device(Ctx* c, const Srs* s, const uint32_t* d_scalars, const size_t* lens, size_t n_polys,
                  size_t stride, uint64_t* out_xy, uint8_t* out_inf, bool drain = true,
                  const uint32_t* d_eval = nullptr, uint64_t* out_eval = nullptr);
int commit_flush(Ctx* c);
void msm_free_work(Ctx* c);

// poly.hip: combined = sum_i xi^(i+1) p_i; quotient (combined - combined(z)) / (X - z).
// d_quot receives max_len-1 coefficients (canonical words); eval_out the value combined(z).
int open_quotient_device(Ctx* c, const uint32_t* d_polys, const size_t* lens, size_t k, size_t stride,
                         const uint32_t* z_words, const uint32_t* xi_words, uint32_t** d_quot_out,
                         size_t* quot_len, uint64_t* eval_out, bool sync = true);
// poly.hip: Q = sum_j Q_(z_j)[ sum_i w_ij p_i ].  points [t][8], weights [k][t][8] canonical words on
// the host.  d_quot_out: max_len-1 coefficients (null: nothing to commit, Q = 0).  Enqueues; the host tables it
// uploads have been copied when it returns.
int open_points_quotient_device(Ctx* c, const uint32_t* d_polys, const size_t* lens, size_t k, size_t stride,
                                const uint32_t* points, size_t t, const uint32_t* weights, uint32_t** d_quot_out,
                                size_t* quot_len);
// poly.hip: coset opening.  combined = sum_i xi^(i+1) p_i; quotient (combined - rho) / (X^l - h^l), rho the remainder.
// d_quot receives max(n - l, 0) coefficients; eval_out ([l][4], may be null) combined(h zeta^k).  Synchronises.
// open_coset_check: the argument checks alone (log_l <= 12, h != 0, zeta a primitive l-th root, lens, key length).
int open_coset_check(Ctx* c, const size_t* lens, size_t k, size_t stride, uint32_t log_l, const uint32_t* h_words,
                     const uint32_t* zeta_words, size_t key_n);
int open_coset_quotient_device(Ctx* c, const uint32_t* d_polys, const size_t* lens, size_t k, size_t stride,
                               uint32_t log_l, const uint32_t* h_words, const uint32_t* zeta_words,
                               const uint32_t* xi_words, size_t key_n, uint32_t** d_quot_out, size_t* quot_len,
                               uint64_t* eval_out);

// verify.hip: the two G1 points (L, R) of a random linear combination of K coset claims
int verify_cosets(Ctx* c, const Srs* mono, uint32_t log_N, uint32_t log_l, const uint32_t* w_words,
                  const uint64_t* comm_xy, const uint8_t* comm_inf, size_t n_comm, const uint32_t* comm_idx,
                  const uint32_t* coset_idx, const uint64_t* values, const uint64_t* proof_xy, const uint8_t* proof_inf,
                  size_t K, const uint32_t* rho_words, uint64_t* out_xy, uint8_t* out_inf);
// the same fold with the values as cells of 32-byte big-endian elements: an element >= r sets
// *out_status and leaves both points at infinity
int verify_cosets_bytes(Ctx* c, const Srs* mono, uint32_t log_N, uint32_t log_l, const uint32_t* w_words,
                        const uint64_t* comm_xy, const uint8_t* comm_inf, size_t n_comm, const uint32_t* comm_idx,
                        const uint32_t* coset_idx, const uint8_t* cells, int bit_reversed, const uint64_t* proof_xy,
                        const uint8_t* proof_inf, size_t K, const uint32_t* rho_words, uint64_t* out_xy,
                        uint8_t* out_inf, uint8_t* out_status);

// verify.hip: d_coef[j] = sum of d_r[d_perm[q]], q in [d_off[j], d_off[j + 1]): the per-commitment sums of the weights
// over the cells grouped by commitment.  d_cpart: n_comm * ver_commsum_shares(n_comm) elements of scratch.  Two launches.
__attribute__((visibility("hidden")))   // library-private: not in the exported symbol list
size_t ver_commsum_shares(size_t n_comm);
__attribute__((visibility("hidden")))   // library-private: not in the exported symbol list
int ver_commitment_sums(Ctx* c, const uint32_t* d_r, const uint32_t* d_perm, const uint32_t* d_off, size_t n_comm,
                        uint32_t* d_cpart, uint32_t* d_coef);
// d_out[j] = sum_(q < cnt) d_part[q * cols + j], j < cols (ver_colsum_final_kernel).  One launch.
__attribute__((visibility("hidden")))   // library-private: not in the exported symbol list
int ver_column_sums(Ctx* c, uint32_t cols, uint32_t cnt, const uint32_t* d_part, uint32_t* d_out);

// verify_points.hip: the two G1 points (L, R) of a random linear combination of K claims at arbitrary points
// 
int verify_points(Ctx* c, const uint64_t* comm_xy, const uint8_t* comm_inf, size_t n_comm, const uint32_t* comm_idx,
                  const uint64_t* z, const uint64_t* y, const uint64_t* proof_xy, const uint8_t* proof_inf, size_t K,
                  const uint32_t* rho_words, uint64_t* out_xy, uint8_t* out_inf);
// msm.hip: the curve's generator, canonical affine limbs x | y (what a generated key starts with)
__attribute__((visibility("hidden")))   // library-private: not in the exported symbol list
const uint64_t* g1_generator_limbs(int curve);

// recover.hip: b coefficient vectors of n elements from their values on K of the N/l cosets.
// coset_idx and out_consistent in host memory; values / coeffs in host (host_ptrs) or device memory.  Synchronises.
int recover_cosets(Ctx* c, uint32_t log_n, uint32_t log_N, uint32_t log_l, const uint32_t* w_words,
                   const uint32_t* coset_idx, size_t K, const uint32_t* values, bool host_ptrs, size_t b,
                   uint32_t* coeffs, uint8_t* out_consistent);
uint32_t recover_leaf_width();     // linear factors a leaf of the product tree multiplies out

// g1_bytes.hip: compressed points and subgroup checks; the contracts are those of the kzg_* entry
// points of the same names.  n = 0 does nothing; more than 2^24 points is KZG_ERR_ARG.
int g1_compress(Ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out_bytes);
int g1_decompress(Ctx* c, const uint8_t* bytes, size_t n, int check_subgroup, uint64_t* out_xy, uint8_t* out_inf,
                  uint8_t* out_status);
int g1_decompress_device(Ctx* c, const void* d_bytes, size_t n, int check_subgroup, void* d_xy, void* d_inf,
                         void* d_status);
int g1_check_subgroup(Ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out_status);
// g2_bytes.hip: the G2 forms (points are 4 * FP words: x.c0 | x.c1 | y.c0 | y.c1, kzg_pairing_check's layout)
int g2_compress(Ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out_bytes);
int g2_decompress(Ctx* c, const uint8_t* bytes, size_t n, int check_subgroup, uint64_t* out_xy, uint8_t* out_inf,
                  uint8_t* out_status);
int g2_decompress_device(Ctx* c, const void* d_bytes, size_t n, int check_subgroup, void* d_xy, void* d_inf,
                         void* d_status);
int g2_check_subgroup(Ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out_status);
// g_mul.hip: per-point scalar multiplication; the contracts are those of the kzg_* entry points.
// k: n x 8 words, or null for the power form c0 s^i (s, c0: 8 canonical words below r).  n = 0 does nothing.
int g1_mul_each(Ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, const uint32_t* k, const uint32_t* s,
                const uint32_t* c0, uint64_t* out_xy, uint8_t* out_inf);
int g2_mul_each(Ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, const uint32_t* k, const uint32_t* s,
                const uint32_t* c0, uint64_t* out_xy, uint8_t* out_inf);
int g1_mul_each_device(Ctx* c, const void* d_xy, const void* d_inf, size_t n, const void* d_k, void* d_out_xy,
                       void* d_out_inf);
int srs_mul_powers(Ctx* c, const Srs* in, const uint32_t* s, const uint32_t* c0, Srs** out);
// g2_lincomb.hip: the sum of the products on the twist as one point.  s == null: k is n x 8 words;
// else the power form c0 s^i.  n = 0 is infinity.
int g2_lincomb(Ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, const uint32_t* k, const uint32_t* s,
               const uint32_t* c0, uint64_t* out_xy, uint8_t* out_inf);
int srs_load_g1_compressed(Ctx* c, const uint8_t* bytes, size_t n, int check_subgroup, Srs** out);
int srs_export_compressed(Ctx* c, const Srs* s, size_t start, size_t count, uint8_t* out_bytes);

// blob.hip: EIP-4844 blobs as bytes; the contracts are those of the kzg_* entry points of the same
// names.  b = 0 does nothing; log_n outside [1, 24] or more than 2^26 elements is KZG_ERR_ARG.
int blob_to_fr(Ctx* c, uint32_t log_n, const uint8_t* blobs, size_t b, int bit_reversed, uint64_t* out_vals,
               uint8_t* out_status);
int blob_to_fr_device(Ctx* c, uint32_t log_n, const void* d_blobs, size_t b, int bit_reversed, void* d_vals,
                      void* d_status);
int fr_to_blob(Ctx* c, uint32_t log_n, const uint64_t* vals, size_t b, int bit_reversed, uint8_t* out_bytes,
               uint8_t* out_status);
int fr_to_blob_device(Ctx* c, uint32_t log_n, const void* d_vals, size_t b, int bit_reversed, void* d_bytes,
                      void* d_status);
// the intake kernel alone, enqueued on the context's stream: nothing checked, log_n >= 0 (verify.hip: cells as bytes)
__attribute__((visibility("hidden")))   // library-private: not in the exported symbol list
int blob_intake_launch(Ctx* c, uint32_t log_n, const uint32_t* d_blobs, size_t b, int bit_reversed, uint32_t* d_vals,
                       uint8_t* d_status);
int blob_challenges(Ctx* c, uint32_t log_n, const uint8_t* blobs, const uint8_t* commitments, size_t b,
                    uint64_t* out_z);
int blob_challenges_device(Ctx* c, uint32_t log_n, const void* d_blobs, const void* d_commitments, size_t b,
                           void* d_z);

// pairing.hip: m pairing-product equations of k pairs each; the contract is that of
// kzg_pairing_check (out_gt == nullptr) and kzg_pairing_product.  m = 0 does nothing.
int pairing_product(Ctx* c, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf,
                    size_t m, size_t k, uint64_t* out_gt, uint8_t* out_status);
int pairing_gt_multiple(int curve);

int open_shard_begin_device(Ctx* c, const uint32_t* d_polys, const size_t* lens, size_t k, size_t stride,
                            const uint32_t* z_words, const uint32_t* xi_words, uint64_t* chunk_eval_out);
int open_shard_finish_device(Ctx* c, const uint32_t* z_words, const uint32_t* carry_words, int first_rank,
                             uint32_t** d_vec_out, size_t* vec_len, uint64_t* eval_out);

}  // namespace kzg
