/*
 * kzg_mi355x.h -- C ABI of libkzg_mi355x.so, the MI355X (gfx950) engine behind the
 * hot path of swusjask/kzg-snark:
 *
 *     fft_ff / ifft_ff / fft_ff_interpolation        (reference fft_ff.py:3,39,60)
 *     KZG.commit / KZG.open                           (reference kzg.py:80,122)
 *     KZG.setup's [tau^i G1] table                    (reference kzg.py:56-78)
 *
 * The reference has no FFI of its own (it is pure Python on SageMath + py_ecc);
 * these entry points are what a ctypes binding placed inside those five
 * functions calls (INTEGRATION.md shows the stubs).  Plain pointers and sizes
 * only; no exceptions cross the boundary.
 *
 * Conventions
 *  - Every function returns 0 on success or a negative KZG_ERR_* code;
 *    kzg_last_error(ctx) gives the message of the last failure on that context.
 *  - Field elements cross the boundary in CANONICAL form (integers < modulus,
 *    not Montgomery), little-endian 64-bit limbs: 4 limbs (32 B) for the scalar
 *    field Fr of either curve and for BN254's Fp, 6 limbs (48 B) for BLS12-381's
 *    Fp.  Scalars and NTT data MUST be reduced (< r): the facade does
 *    int(x) % r exactly like the reference's int(coeff) / Fq(x) coercions.
 *  - G1 points cross as affine (x, y) = 2*FP_LIMBS limbs plus a separate
 *    infinity flag byte (the reference's Z1, kzg.py:43).
 *  - "host" entry points take host pointers, copy in/out and synchronise.
 *    "_device" entry points take device pointers (>= 32-byte aligned), enqueue on
 *    the context's stream and return without synchronising.
 *  - A context is bound to one GPU and one stream; it is not thread-safe (one
 *    context per thread).  The library owns all device memory behind handles.
 *  - There is NO CPU fallback: without a gfx950 device kzg_ctx_create fails
 *    with KZG_ERR_NODEV.
 */
#ifndef KZG_MI355X_H
#define KZG_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KZG_CURVE_BN254 0      /* reference default, kzg.py:18,26 */
#define KZG_CURVE_BLS12_381 1  /* kzg.py:31 */

#define KZG_OK 0
#define KZG_ERR_ARG (-1)
#define KZG_ERR_HIP (-2)
#define KZG_ERR_NODEV (-3)
#define KZG_ERR_DEGREE (-4) /* polynomial longer than the SRS: ValueError at kzg.py:103-106 */
#define KZG_ERR_ALLOC (-5)

typedef struct kzg_ctx kzg_ctx;
typedef struct kzg_srs kzg_srs;
typedef struct kzg_domain_table kzg_domain_table;

/* ABI version of this header (bumped on incompatible change). */
int kzg_abi_version(void);

/* Limbs (uint64) per base-field element for a curve: 4 (BN254) or 6 (BLS12-381); 0 if unknown.
 * Curve selection mirrors KZG.__init__ (kzg.py:26-37). */
int kzg_fp_limbs(int curve_id);

/* Create / destroy a context on HIP device `device_id`. */
int kzg_ctx_create(int curve_id, int device_id, kzg_ctx** out);
void kzg_ctx_destroy(kzg_ctx* ctx);
const char* kzg_last_error(const kzg_ctx* ctx);

/* Use an existing hipStream_t (e.g. torch's current stream) for all work of this context.
 * NULL restores the context's own (non-blocking) stream; to run on HIP's null stream -- torch's
 * default stream -- pass hipStreamLegacy.  A context that keeps its own stream is NOT ordered with
 * work the caller enqueues elsewhere: synchronise, or bind the producer's stream.
 * The handle must be a live hipStream_t of this process (or hipStreamLegacy / hipStreamPerThread): HIP has no way
 * to validate one, so only values that cannot be runtime objects (other small integers, misaligned values) are
 * refused with KZG_ERR_ARG; the stream must outlive its use by the context. */
int kzg_ctx_set_stream(kzg_ctx* ctx, void* hip_stream);
/* Block until everything enqueued on the context's stream has finished. */
int kzg_ctx_synchronize(kzg_ctx* ctx);
/* Fix a choice the library otherwise makes from what is resident on the GPU (tests and A/B timing; results never
 * depend on it).  value 0 restores the library's choice.  Keys:
 *   "ntt_tile_log"       log2 of the transform's LDS tile, 8..12 (default: 11 alone, 10 beside an accumulate kernel)
 *   "open_tile_threads"  threads per tile of the opening's scan, 128 | 256 (default: 256 alone, 128 beside one)
 *   "open_direct_tiles"  tile count up to which every tile sums all tile aggregates above it (default 1024)
 *   "open_domain_chunk"  vectors per chunk of kzg_open_domain*, 1..1024 (default: as many as ~2 GiB of scratch holds)
 *   "open_cosets_chunk"  vectors per chunk of kzg_open_cosets*, 1..1024 (default: as many as ~2 GiB of scratch holds)
 *   "open_cosets_group"  1 + log2 of the sub-tables that share one doubling chain in kzg_open_cosets*, 1..5, clipped to
 *                        the table's log_l (default: min(l, 16) sub-tables, fewer while < 2^16 threads would run)
 *   "recover_chunk"      vectors per chunk of kzg_recover_cosets*, 1..1024 (default: as many as ~2 GiB of scratch holds)
 *   "eval_batch_chunk"   vectors per chunk of kzg_fr_eval_lagrange_batch*, 1..65535, the most one launch indexes
 *                        (default: as many as ~1 GiB of scratch holds, at most 65535) */
int kzg_ctx_set_tuning(kzg_ctx* ctx, const char* key, int64_t value);

/* ---- NTT: replaces fft_ff (fft_ff.py:3-37) and ifft_ff (fft_ff.py:39-58) -------------
 * data: n = 2^log_n elements of Fr, natural order in and out, transformed in place.
 * w: the caller's root, exactly the `w` argument of fft_ff / ifft_ff.  The result is that
 * of the reference recursion for any w (primitive or not).  inverse != 0 => ifft_ff:
 * transform with w^-1, then scale by n^-1. */
int kzg_ntt(kzg_ctx* ctx, uint64_t* data, uint32_t log_n, const uint64_t w[4], int inverse);
/* Same on `batch` consecutive device-resident arrays of n elements each. */
int kzg_ntt_device(kzg_ctx* ctx, void* d_data, uint32_t log_n, const uint64_t w[4], int inverse,
                   uint32_t batch);

/* fft_ff / ifft_ff for ANY list length n >= 1 (fft_ff.py:3-58 never checks it): powers of two go
 * to the kernels above; other lengths reproduce the reference recursion level by level -- slices of
 * ceil(n/2) and floor(n/2) elements, n//2 butterflies, result[n-1] left at zero for odd n
 * (fft_ff.py:20-35) -- which is what marlin/prover.py:439-449 receives when it passes list(row_A)
 * with trailing zeros dropped.  inverse: root w^-1, scale by F(n)^-1 (fft_ff.py:53-58).
 * n = 0 is KZG_ERR_ARG (the reference recurses without end). */
int kzg_fft_ff_any(kzg_ctx* ctx, uint64_t* data, size_t n, const uint64_t w[4], int inverse);
int kzg_fft_ff_any_device(kzg_ctx* ctx, void* d_data, size_t n, const uint64_t w[4], int inverse);

/* The two local halves of the multi-GPU four-step transform of n = 2^log_n = N1*N2 elements
 * (N1 = 2^ceil(log_n/2)); kzg_snark_amd/sharding.py exchanges the data between them with
 * all-to-all transposes.  Requires log_n > 12.
 *   columns: d_data is an [N1][n_cols] row-major matrix holding global columns col_base ..
 *            col_base+n_cols-1 of the N1 x N2 view; transformed in place down the columns and
 *            multiplied by the twist w^(row * global column) -- and by n^-1 when inverse (the scale
 *            of fft_ff.py:57-58 rides on the twist; the two halves are only meaningful as a pair).
 *   rows:    d_data is an [n_rows][N2] matrix (n_rows rows of the twisted matrix); transformed in
 *            place along the rows, natural order.
 * n_cols / n_rows: powers of two. */
int kzg_ntt_columns_device(kzg_ctx* ctx, void* d_data, uint32_t log_n, const uint64_t w[4], int inverse,
                           uint64_t n_cols, uint64_t col_base);
int kzg_ntt_rows_device(kzg_ctx* ctx, void* d_data, uint32_t log_n, const uint64_t w[4], int inverse,
                        uint64_t n_rows);
/* The same transform taken the other way round: input in the TRANSPOSED layout (what the rows pass above leaves:
 * row rho of the [N1][N2] matrix holds the elements b*N1 + rho, b = 0..N2-1), output in natural order --
 *   rows_twist:    N2-point transforms along n_rows rows (global rows row_base ..), each output (rho, beta) multiplied
 *                  by w^(rho*beta) (and by n^-1 when inverse); in place;
 *   (all-to-all: rows -> whole columns)
 *   columns_plain: N1-point transforms down n_cols columns of an [N1][n_cols] matrix, no twist; element (alpha, beta)
 *                  is then X[alpha*N2 + beta]: an all-to-all back to rows gives every rank a contiguous range.
 * Two all-to-alls instead of the four that "bring the data into range order, then transform" costs.  Unlike the
 * passes above this pair relies on w^n = 1: w must be a primitive 2^log_n-th root of unity (KZG_ERR_ARG otherwise).
 * Requires log_n > 12. */
int kzg_ntt_rows_twist_device(kzg_ctx* ctx, void* d_data, uint32_t log_n, const uint64_t w[4], int inverse,
                              uint64_t n_rows, uint64_t row_base);
int kzg_ntt_columns_plain_device(kzg_ctx* ctx, void* d_data, uint32_t log_n, const uint64_t w[4], int inverse,
                                 uint64_t n_cols);
/* The rows half reading and writing the all-to-all buffers directly (no repacking copies):
 *   d_src  [world][n_rows][N2/world]  what the columns -> rows all-to-all delivers: block h holds
 *          columns h*N2/world .. of this rank's n_rows rows;
 *   d_dst  blocked_out != 0: [world][n_rows][N2/world] over the OUTPUT index b (block h = outputs
 *          h*N2/world ..), the send buffer of the all-to-all that restores natural order;
 *          blocked_out == 0: [n_rows][N2] plain rows -- the "transposed" result layout: row t of
 *          this rank holds result indices b*N1 + t, b = 0..N2-1 (commit against a key shard in the
 *          same order, kzg_srs_generate_strided; two all-to-alls per transform instead of three).
 * Out of place (d_src != d_dst); world: power of two dividing N2. */
int kzg_ntt_rows_exchange_device(kzg_ctx* ctx, const void* d_src, void* d_dst, uint32_t log_n, const uint64_t w[4],
                                 int inverse, uint64_t n_rows, uint32_t world, int blocked_out);

/* ---- commitment key: the `ck` list of KZG.setup / KZG.commit (kzg.py:56-78, 80) ------
 * kzg_srs_load_g1 uploads n affine G1 points (xy: n x 2*FP_LIMBS limbs; inf: n flag bytes or
 * NULL) and expands them into the engine's device table (msm.hip).  Points are checked to be
 * on the curve (KZG_ERR_ARG otherwise).  The handle replaces passing `ck` on every call. */
int kzg_srs_load_g1(kzg_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, kzg_srs** out);
/* kzg_srs_generate builds [tau^i * G1], i = 0..n-1, on the device: the G1 half of KZG.setup
 * (kzg.py:70-72) with the secret supplied by the caller (the reference samples it at :67). */
int kzg_srs_generate(kzg_ctx* ctx, const uint64_t tau[4], size_t n, kzg_srs** out);
/* The slice [tau^(start+i) * G1], i = 0..n-1: one rank's shard of a key partitioned by
 * coefficient range across GPUs. */
int kzg_srs_generate_range(kzg_ctx* ctx, const uint64_t tau[4], size_t start, size_t n, kzg_srs** out);
/* Key points in a strided order: point i = tau^e * G1 with
 *   e = start + (i / run_len) * outer_stride + (i % run_len) * inner_stride.
 * The shard a rank needs to commit the "transposed" output of the distributed inverse NTT without
 * reordering it: rows t0..t0+R-1 of N2 coefficients each, coefficient (t, b) having index b*N1 + t
 * => start = t0, run_len = N2, inner_stride = N1, outer_stride = 1, n = R*N2. */
int kzg_srs_generate_strided(kzg_ctx* ctx, const uint64_t tau[4], size_t start, size_t n, size_t run_len,
                             size_t inner_stride, size_t outer_stride, kzg_srs** out);
/* Read points [start, start+count) back as canonical affine coordinates. */
int kzg_srs_export(kzg_ctx* ctx, const kzg_srs* srs, size_t start, size_t count, uint64_t* xy, uint8_t* inf);
size_t kzg_srs_size(const kzg_srs* srs);
void kzg_srs_free(kzg_srs* srs);

/* ---- KZG.commit (kzg.py:80-120) --------------------------------------------------------
 * n_polys coefficient arrays, `stride` elements apart, polynomial p having lens[p] coefficients
 * (low to high).  One affine point per polynomial: out_xy[p] (2*FP_LIMBS limbs), out_inf[p] = 1
 * for the point at infinity (zero polynomial, kzg.py:109).  lens[p] > kzg_srs_size(srs) returns
 * KZG_ERR_DEGREE -- the ValueError of kzg.py:103-106 -- before any work is queued.  Zero coefficients
 * contribute nothing (kzg.py:113-114).  The scalars are in host memory: polynomial p + 1 is copied to
 * the device while polynomial p is being accumulated. */
int kzg_commit(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* scalars, const size_t* lens, size_t n_polys,
               size_t stride, uint64_t* out_xy, uint8_t* out_inf);
/* Same with device-resident scalars; results are still written to host memory (one point per
 * polynomial), so the call synchronises the stream. */
int kzg_commit_device(kzg_ctx* ctx, const kzg_srs* srs, const void* d_scalars, const size_t* lens, size_t n_polys,
                      size_t stride, uint64_t* out_xy, uint8_t* out_inf);

/* Pipelined form: returns after enqueueing; up to four polynomials stay in flight across calls.
 * The scalars are copied at enqueue, in the order of the context's stream: work queued on that
 * stream afterwards (the next transform into the same buffer, say) may overwrite them, anything
 * else must wait for the stream.  out_xy / out_inf stay valid until kzg_commit_flush() returns
 * (or until a later call on this context has recycled the slot); results are written by the host
 * thread inside those calls. */
int kzg_commit_device_async(kzg_ctx* ctx, const kzg_srs* srs, const void* d_scalars, const size_t* lens,
                            size_t n_polys, size_t stride, uint64_t* out_xy, uint8_t* out_inf);
int kzg_commit_flush(kzg_ctx* ctx);

/* ---- KZG.open (kzg.py:122-159) -----------------------------------------------------------
 * combined = sum_i xi^(i+1) * polys[i]  (first polynomial scaled by xi, kzg.py:148-150);
 * witness = (combined - combined(z)) // (X - z); the proof is commit(witness).
 * eval_out (optional, 4 limbs) receives combined(z).
 * The witness's DEGREE is checked against the key, as the reference does through the commit of the witness
 * (kzg.py:157 -> :103-106), not the lengths: with n = max lens the witness has n - 1 coefficients, and those from
 * index kzg_srs_size(srs) on may be there as long as every one of them is zero -- literal trailing zeros of the
 * inputs, or a combination whose high coefficients cancel exactly; they are then left out of the commitment.  One
 * non-zero coefficient among them is KZG_ERR_DEGREE.  Only when n - 1 > kzg_srs_size(srs) are they looked at, on
 * the device, which waits for the stream.  After KZG_ERR_DEGREE out_xy and out_inf are as the caller left them,
 * eval_out is unspecified, nothing of the call is pending, and the context serves the next call as after any other. */
int kzg_open(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* polys, const size_t* lens, size_t k, size_t stride,
             const uint64_t z[4], const uint64_t xi[4], uint64_t* out_xy, uint8_t* out_inf, uint64_t* eval_out);
int kzg_open_device(kzg_ctx* ctx, const kzg_srs* srs, const void* d_polys, const size_t* lens, size_t k,
                    size_t stride, const uint64_t z[4], const uint64_t xi[4], uint64_t* out_xy, uint8_t* out_inf,
                    uint64_t* eval_out);

/* Pipelined form of kzg_open_device: the combine / evaluate / divide kernels and the MSM of the witness are only
 * enqueued (the MSM shares the commit pipeline's slots with kzg_commit_device_async); out_xy, out_inf and eval_out
 * (required, 4 limbs) are written when kzg_commit_flush() returns or a later call recycles the slot.  The input
 * polynomials may be overwritten by later work on the context's stream as soon as the call has returned.
 * The degree rule is kzg_open's.  Its check (n - 1 > kzg_srs_size(srs) only) is the one thing that synchronises this
 * form: the call waits for the context's stream, not for the pipeline.  KZG_ERR_DEGREE is returned by the call
 * itself, before the MSM takes a slot: out_xy and out_inf are as the caller left them and are not written later
 * (no flush touches them), eval_out is unspecified, and openings and commits enqueued before and after the refused
 * call deliver their results as if it had not been made. */
int kzg_open_device_async(kzg_ctx* ctx, const kzg_srs* srs, const void* d_polys, const size_t* lens, size_t k,
                          size_t stride, const uint64_t z[4], const uint64_t xi[4], uint64_t* out_xy, uint8_t* out_inf,
                          uint64_t* eval_out);

/* ---- evaluation form: keys in the Lagrange basis, openings from values ----------------------------
 * Domain H = {w^i, i < n}, n = 2^log_n (1 <= log_n <= 24), w a primitive n-th root of unity given by the caller (the
 * `w` of fft_ff); w^(n/2) != -1 is KZG_ERR_ARG.  Values are in natural order: vals[i] = p(w^i).
 * A Lagrange key holds [L_i(tau)] G1, L_i the Lagrange polynomial of point w^i, so kzg_commit* on a Lagrange key
 * commits VALUES: the result equals the coefficient commitment of their interpolant.  kzg_srs_export, kzg_srs_size
 * and kzg_srs_free work on either basis.
 *   kzg_srs_generate_lagrange  from the secret: L_i(tau) = (tau^n - 1)/n * w^i / (tau - w^i) on the device, then the
 *                              fixed-base table of kzg_srs_generate
 *   kzg_srs_lagrange           from the first n points of a monomial key (generated, loaded or read from a file; no
 *                              tau needed): an inverse NTT over G1.  KZG_ERR_ARG for a key shorter than n or one that
 *                              is itself a Lagrange key. */
int kzg_srs_generate_lagrange(kzg_ctx* ctx, const uint64_t tau[4], uint32_t log_n, const uint64_t w[4],
                              kzg_srs** out);
int kzg_srs_lagrange(kzg_ctx* ctx, const kzg_srs* monomial, uint32_t log_n, const uint64_t w[4], kzg_srs** out);
/* KZG.open from values: k value vectors, `stride` elements apart, vector j having lens[j] <= n values (missing values
 * read as zero; lens[j] > n is KZG_ERR_DEGREE).  combined = sum_j xi^(j+1) vals_j, its value y at z by the
 * barycentric formula, the quotient (combined - y)/(X - z) on H -- z in H included (the within-domain formula of
 * EIP-4844) -- committed against the Lagrange key `srs` (a monomial key is KZG_ERR_ARG).  Parameters, outputs and the
 * pipelined form's slot rules are those of kzg_open / kzg_open_device / kzg_open_device_async; the proof equals
 * kzg_open's on the interpolants, and eval_out receives y. */
int kzg_open_evals(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* vals, const size_t* lens, size_t k, size_t stride,
                   const uint64_t z[4], const uint64_t xi[4], uint64_t* out_xy, uint8_t* out_inf, uint64_t* eval_out);
int kzg_open_evals_device(kzg_ctx* ctx, const kzg_srs* srs, const void* d_vals, const size_t* lens, size_t k,
                          size_t stride, const uint64_t z[4], const uint64_t xi[4], uint64_t* out_xy, uint8_t* out_inf,
                          uint64_t* eval_out);
int kzg_open_evals_device_async(kzg_ctx* ctx, const kzg_srs* srs, const void* d_vals, const size_t* lens, size_t k,
                                size_t stride, const uint64_t z[4], const uint64_t xi[4], uint64_t* out_xy,
                                uint8_t* out_inf, uint64_t* eval_out);
/* ---- every proof on a domain at once: FK20 (Feist-Khovratovich, "Fast amortized KZG proofs", 2020) -----------
 * For b coefficient vectors p_j of degree < n = 2^log_n (1 <= log_n <= 20) and a primitive n-th root w, all n proofs
 * pi_j[i] = kzg_open(p_j, z = w^i, xi = 1) (kzg.py:122-159) in O(n log n) group work and no MSM: the forward G1 DFT of
 * h_m = sum_(t>m) c_t [tau^(t-m-1)] G1, whose Toeplitz product runs as a circular convolution of size 2n against a
 * table built once per key and n.
 *   kzg_domain_table_create  the table from the first n points of a monomial key (KZG_ERR_ARG for a Lagrange key, a
 *                            key of another curve or shorter than n, log_n outside [1, 20]): 2n affine points.
 *   kzg_open_domain          vectors `stride` elements apart, vector j having lens[j] <= n coefficients (KZG_ERR_DEGREE
 *                            above n, KZG_ERR_ARG for lens[j] > stride or a w that is not a primitive n-th root).
 *                            out_xy / out_inf: [b][n] proofs in kzg_open's point format; eval_out ([b][n][4] limbs, may
 *                            be NULL) receives y_j[i] = p_j(w^i).  The vectors run in chunks that bound the scratch
 *                            (tuning key "open_domain_chunk").  Synchronises; the commit pipeline is not touched. */
int kzg_domain_table_create(kzg_ctx* ctx, const kzg_srs* monomial, uint32_t log_n, kzg_domain_table** out);
size_t kzg_domain_table_size(const kzg_domain_table* t);
void kzg_domain_table_free(kzg_domain_table* t);
int kzg_open_domain(kzg_ctx* ctx, const kzg_domain_table* t, const uint64_t* polys, const size_t* lens, size_t b,
                    size_t stride, const uint64_t w[4], uint64_t* out_xy, uint8_t* out_inf, uint64_t* eval_out);
int kzg_open_domain_device(kzg_ctx* ctx, const kzg_domain_table* t, const void* d_polys, const size_t* lens, size_t b,
                           size_t stride, const uint64_t w[4], uint64_t* out_xy, uint8_t* out_inf,
                           uint64_t* eval_out);
/* ---- coset openings: the values at l = 2^log_l points with ONE proof (FK20's multi-reveal) ----------------------
 * A coset (h, zeta): zeta a primitive l-th root of unity (zeta = 1 for l = 1), h != 0, the points x_k = h zeta^k
 * (k < l), vanishing polynomial Z = X^l - a with a = h^l.  For p(X) = sum_(t<n) c_t X^t the remainder is
 * rho = p mod Z, rho_j = sum_s c_(sl+j) a^s (j < l), the quotient q = (p - rho) / Z, and the proof pi = [q(tau)] G1
 * (l = 1: kzg_open at z = h).  Check: e([p(tau)] - [rho(tau)], G2) = e(pi, [tau^l] G2 - a G2); the verifier recovers
 * rho from the values y_k = p(x_k) as rho_j = h^-j l^-1 sum_k y_k zeta^(-jk).
 *   kzg_coset_table_create  the table of a monomial key for n = 2^log_n (1 <= log_n <= 20) and l = 2^log_l
 *                           (0 <= log_l <= log_n - 1): l sub-tables of 2m points, m = n/l -- 2n affine points for
 *                           every l.  KZG_ERR_ARG as for kzg_domain_table_create.  A table from
 *                           kzg_domain_table_create is the l = 1 table; kzg_domain_table_size / _free apply to both;
 *                           kzg_open_domain* refuses a table with l > 1 (KZG_ERR_ARG).
 *   kzg_open_cosets         every coset of a domain {w^t, t < N}, N = 2^log_N (log_n <= log_N <= min(log_n + 2, 21)),
 *                           w a primitive N-th root: coset i < N/l is (h = w^i, zeta = w^(N/l)), its value k is
 *                           p(w^(i + k N/l)).  Vectors `stride` elements apart, vector j having lens[j] <= n
 *                           coefficients (KZG_ERR_DEGREE above n; KZG_ERR_ARG for lens[j] > stride, a w that is not a
 *                           primitive N-th root, log_N out of range).  out_xy / out_inf: [b][N/l] proofs in
 *                           kzg_open's point format; eval_out ([b][N/l][l][4] limbs, may be NULL) the values.
 *                           The l Toeplitz products of size m are summed before one inverse G1 DFT of size 2m, and
 *                           the final G1 DFT has size N/l (root w^l).  Chunks bound the scratch (tuning key
 *                           "open_cosets_chunk").  Synchronises; the commit pipeline is not touched.
 *   kzg_open_coset          ONE coset (0 <= log_l <= 12) of the combination sum_j xi^(j+1) p_j of k <= 64 polynomials
 *                           (kzg_open's rule): the quotient by X^l - a on the device, then one MSM against a
 *                           monomial key (KZG_ERR_ARG for a Lagrange key, a zeta that is not a primitive l-th root or
 *                           h = 0; KZG_ERR_DEGREE for lens[j] above the key, before any work is queued).  eval_out
 *                           ([l][4] limbs, may be NULL) receives the combination's values at h zeta^k.  Synchronises
 *                           like kzg_open; pending kzg_commit_device_async results stay correct. */
int kzg_coset_table_create(kzg_ctx* ctx, const kzg_srs* monomial, uint32_t log_n, uint32_t log_l,
                           kzg_domain_table** out);
int kzg_open_cosets(kzg_ctx* ctx, const kzg_domain_table* t, const uint64_t* polys, const size_t* lens, size_t b,
                    size_t stride, uint32_t log_N, const uint64_t w[4], uint64_t* out_xy, uint8_t* out_inf,
                    uint64_t* eval_out);
int kzg_open_cosets_device(kzg_ctx* ctx, const kzg_domain_table* t, const void* d_polys, const size_t* lens, size_t b,
                           size_t stride, uint32_t log_N, const uint64_t w[4], uint64_t* out_xy, uint8_t* out_inf,
                           uint64_t* eval_out);
int kzg_open_coset(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* polys, const size_t* lens, size_t k,
                   size_t stride, uint32_t log_l, const uint64_t h[4], const uint64_t zeta[4], const uint64_t xi[4],
                   uint64_t* out_xy, uint8_t* out_inf, uint64_t* eval_out);
int kzg_open_coset_device(kzg_ctx* ctx, const kzg_srs* srs, const void* d_polys, const size_t* lens, size_t k,
                          size_t stride, uint32_t log_l, const uint64_t h[4], const uint64_t zeta[4],
                          const uint64_t xi[4], uint64_t* out_xy, uint8_t* out_inf, uint64_t* eval_out);
/* ---- bulk verification: any number of coset claims folded into ONE pairing equation ----------------------------
 * Claim k < K: the polynomial of commitment C[c_k] takes the l = 2^log_l values y_k[t] at w^(i_k + t N/l), t < l
 * (N = 2^log_N, coset (h_k = w^(i_k), zeta = w^(N/l)) in kzg_open_cosets' numbering), with proof pi_k.  With
 * a_k = h_k^l, the remainder I_k(X) = sum_j rho_kj X^j recovered from the values as above, and weights r_k = rho^(k+1)
 * (the rule of the facade's batch_check / batch_check_cosets; rho is the caller's random element):
 *     L = sum_j (sum_(k: c_k = j) r_k) C[j]  -  [(sum_k r_k I_k)(tau)] G1  +  sum_k (r_k a_k) pi_k
 *     R = sum_k r_k pi_k
 * and every claim holds (up to the soundness error of the random combination) iff e(L, G2) = e(R, [tau^l] G2).  The
 * library returns the two points (out_xy / out_inf: L, then R, kzg_open's point format); the caller does the two
 * pairings.  This is verify_cell_kzg_proof_batch of EIP-7594 in this library's conventions; l = 1 checks the proofs of
 * kzg_open_domain.
 *   monomial   the monomial key (>= l points; KZG_ERR_ARG for a Lagrange key, a key of another curve, a shorter one)
 *   comm_xy / comm_inf   n_comm commitments (1 <= n_comm <= 2^16), comm_idx[k] = c_k < n_comm
 *   coset_idx  i_k < N/l;  values [K][l][4] canonical limbs (reduced by the caller), natural order: what
 *              kzg_open_cosets' eval_out holds for that coset;  proof_xy / proof_inf: the K proofs
 * Layouts are those kzg_open_cosets / kzg_open_domain write: for one polynomial, coset_idx = 0 .. N/l - 1 and
 * comm_idx = 0.  Cells may repeat, come in any order and cover any subset.  Ranges: 0 <= log_l <= 12,
 * log_l < log_N <= 21, K <= 2^21, K * l <= 2^24; K = 0 is KZG_OK with both points at infinity.  KZG_ERR_ARG, before
 * any MSM is queued: sizes or an index out of range, a w that is not a primitive N-th root, a proof or commitment
 * with a coordinate >= p or off the curve.  Membership in the prime-order subgroup is not part of this call: a caller that
 * takes points from an untrusted party runs them through kzg_g1_check_subgroup first (the facade's verify_cosets /
 * verify_domain do so with check_subgroup=True), or decompresses them with kzg_g1_decompress(check_subgroup = 1).
 * The proofs are used once, so they are not expanded into a key's window multiples: they become window-0 records
 * only (one record per proof), each scalar is cut into slices of win_bits - 1 bits, and every slice vector runs
 * through the commit pipeline as one polynomial.  Host pointers in, host results out; synchronises.
 * Results of kzg_commit_device_async / kzg_open_device_async still pending are delivered as by a later commit. */
int kzg_verify_cosets(kzg_ctx* ctx, const kzg_srs* monomial, uint32_t log_N, uint32_t log_l, const uint64_t w[4],
                      const uint64_t* comm_xy, const uint8_t* comm_inf, size_t n_comm, const uint32_t* comm_idx,
                      const uint32_t* coset_idx, const uint64_t* values, const uint64_t* proof_xy,
                      const uint8_t* proof_inf, size_t K, const uint64_t rho[4], uint64_t* out_xy, uint8_t* out_inf);
/* The same fold with the values as they travel in EIP-7594: cells [K][l][32], every element 32
 * big-endian bytes in host memory.  bit_reversed != 0: element t of a cell is value bitrev_log_l(t) of its coset, the
 * order of a cell of the specification; 0: natural order, as `values`.  The bytes are uploaded once and
 * kzg_blob_to_fr's kernel writes them into the workspace's value array (log_n = log_l, b = K); from there the call IS
 * kzg_verify_cosets, arguments, ranges and errors included.  An element >= r is a verdict, not an error:
 * *out_status = 1, both points at infinity and KZG_OK (nothing is folded); otherwise *out_status = 0.
 * "verify_device_bytes" then counts the staged bytes and the cells' status bytes as well. */
int kzg_verify_cosets_bytes(kzg_ctx* ctx, const kzg_srs* monomial, uint32_t log_N, uint32_t log_l, const uint64_t w[4],
                            const uint64_t* comm_xy, const uint8_t* comm_inf, size_t n_comm, const uint32_t* comm_idx,
                            const uint32_t* coset_idx, const uint8_t* cells, int bit_reversed, const uint64_t* proof_xy,
                            const uint8_t* proof_inf, size_t K, const uint64_t rho[4], uint64_t* out_xy,
                            uint8_t* out_inf, uint8_t* out_status);
/* ---- bulk verification at arbitrary points: K single-point claims folded into ONE pairing equation
 * Claim k < K: the polynomial of commitment C[c_k] takes the value y_k at z_k -- ANY element of Fr, what kzg_open,
 * kzg_open_evals and an EIP-4844 blob proof open at -- with proof pi_k.  With weights r_k = rho^(k+1) (the rule of
 * kzg_verify_cosets and the facade's batch_check):
 *     L = sum_j (sum_(k: c_k = j) r_k) C[j]  -  (sum_k r_k y_k) G1  +  sum_k (r_k z_k) pi_k
 *     R = sum_k r_k pi_k
 * and every claim holds (up to the soundness error of the random combination) iff e(L, G2) = e(R, [tau] G2).  G1 is
 * the curve's generator, the point a generated key starts with: the call takes no key.  out_xy / out_inf: L, then R,
 * kzg_verify_cosets' output format; the caller does the two pairings.  This is the fold of
 * verify_blob_kzg_proof_batch (EIP-4844) once the blobs' values y_k are known (kzg_fr_eval_lagrange_batch).
 *   comm_xy / comm_inf   n_comm commitments (1 <= n_comm <= 2^16), comm_idx[k] = c_k < n_comm
 *   z, y       [K][4] canonical limbs each, reduced by the caller;  proof_xy / proof_inf: the K proofs
 * K <= 2^21; K = 0 is KZG_OK with both points at infinity.  KZG_ERR_ARG, before any scalar multiplication runs: a
 * size or an index out of range, a proof or commitment with a coordinate >= p or off the curve (kzg_verify_cosets'
 * rule).  Membership in the prime-order subgroup is not part of this call (kzg_g1_check_subgroup; the facade's
 * verify_points / verify_blobs with check_subgroup=True).
 * Every (point, scalar) pair is one lane of one kernel: a 4-bit fixed-window ladder over a per-lane table of the
 * point's multiples, the lanes of a workgroup summed in LDS, the workgroups' partial points by a second kernel.  The
 * call does NOT use the commit pipeline: results of kzg_commit_device_async / kzg_open_device_async still pending are
 * neither retired nor disturbed.  Host pointers in, host results out; synchronises the context's stream. */
int kzg_verify_points(kzg_ctx* ctx, const uint64_t* comm_xy, const uint8_t* comm_inf, size_t n_comm,
                      const uint32_t* comm_idx, const uint64_t* z, const uint64_t* y, const uint64_t* proof_xy,
                      const uint8_t* proof_inf, size_t K, const uint64_t rho[4], uint64_t* out_xy, uint8_t* out_inf);
/* ---- coset recovery: b polynomials of degree < n back from their values on any K >= n/l cosets ------------------
 * The domain {w^t, t < N}, N = 2^log_N, has C = N/l cosets of l = 2^log_l points in kzg_open_cosets' numbering
 * (coset i = {w^(i + k C), k < l}, the roots of X^l - u^i, u = w^l).  K distinct cosets are given, M are missing:
 *   V(Y) = prod_(i in M) (Y - u^i), Z(X) = V(X^l): zero exactly on the missing cosets; Z(w^t) = DFT_C(V)[t mod C]
 *   E = the given values, 0 where missing: E Z = p Z on the whole domain and deg(p Z) < N, so p Z = IDFT_N(E Z)
 *   on the shifted domain s w^t (s the field's generator, s^N != 1) Z has no zero: p(s w^t) = (p Z)(s w^t) / Z(s w^t)
 *   p = IDFT_N of that, coefficient t times s^-t; V is a product tree built on the device in O(C log^2 C)
 *   the values lie on a polynomial of degree < n iff coefficients n .. N-1 vanish (exact; always so for K l = n)
 * This is recover_cells_and_kzg_proofs of EIP-7594 up to the proofs, which kzg_open_cosets_device gives from d_coeffs.
 *   coset_idx  [K] host memory in both forms, cell k of every polynomial is coset coset_idx[k], in any order
 *   values     [b][K][l][4] canonical limbs (reduced by the caller): what kzg_open_cosets' eval_out holds per coset
 *   out_coeffs [b][n][4];  out_consistent [b], host memory: 1 if the tail is zero, else 0 (the n coefficients of
 *              the degree < N interpolant are written all the same)
 * The device form takes device pointers for values and coefficients (32-byte aligned, used on the context's stream)
 * and synchronises like the host form, because it returns the flags.  One index set serves the whole batch: V, two
 * size-C transforms and C inversions per call; three size-N transforms and four element-wise passes per polynomial,
 * in chunks that bound the scratch (tuning key "recover_chunk").
 * Ranges: 0 <= log_l <= 12, log_l <= log_n <= log_N <= 21, log_l < log_N, b >= 1, K <= C.  KZG_ERR_ARG, before
 * anything is queued: a range violation, K l < n, an index >= C, a repeated index, a w that is not a primitive N-th
 * root, a misaligned device pointer. */
int kzg_recover_cosets(kzg_ctx* ctx, uint32_t log_n, uint32_t log_N, uint32_t log_l, const uint64_t w[4],
                       const uint32_t* coset_idx, size_t K, const uint64_t* values, size_t b, uint64_t* out_coeffs,
                       uint8_t* out_consistent);
int kzg_recover_cosets_device(kzg_ctx* ctx, uint32_t log_n, uint32_t log_N, uint32_t log_l, const uint64_t w[4],
                              const uint32_t* coset_idx, size_t K, const void* d_values, size_t b, void* d_coeffs,
                              uint8_t* out_consistent);
/* ---- KZG.open on ONE polynomial set partitioned by coefficient range across GPUs ----------------
 * Rank g holds coefficients [lo_g, hi_g) of every polynomial (the same ranges for all) and a key
 * shard.  kzg_open_shard_begin combines the slices (sum xi^(i+1) p_i) and returns the slice
 * polynomial's value H_g = sum_j c_(lo_g+j) z^j.  The ranks exchange the H_g (one field element
 * each); rank g's carry is S_(hi_g) = sum_(g' > g) H_g' * z^(lo_g' - hi_g).  kzg_open_shard_finish
 * lets the carry enter the scan above the slice's top coefficient and commits the quotient slice:
 *   first_rank != 0: coefficients S_1 .. S_(hi-1) against key points 0 ..      (eval_out = P(z))
 *   otherwise      : coefficients S_lo .. S_(hi-1) against key points lo-1 ..   -- the caller's shard
 *                    must therefore START at global index lo_g - 1 (kzg_srs_generate_range).
 * The partial points of all ranks add up to the opening proof.
 * Between the two calls the context HOLDS the slice: one per context, the last _begin's (an empty slice, every
 * length 0, is one).  _finish continues from exactly what _begin left:
 *   - it must be given _begin's z; another z is KZG_ERR_ARG and the slice stays held;
 *   - tuning changed after _begin (kzg_ctx_set_tuning) has no effect on it;
 *   - it does not consume the slice: it may be repeated, with the same result for the same carry;
 *   - the slice's LENGTH is checked against the key shard, not its degree (a rank cannot know what the others hold):
 *     more coefficients to commit than kzg_srs_size(srs) -- the slice's length, less one on the first rank -- is
 *     KZG_ERR_DEGREE even when the top ones are zero.  The slice stays held: the call may be repeated with a shard
 *     that is long enough.
 * The slice is KEPT across commits (pipelined ones too), key generation, kzg_fr_poly_eval[_batch], the kzg_fr_vec_*
 * primitives and kzg_ctx_set_tuning.  It is DROPPED by kzg_open, kzg_open_device[_async], kzg_open_coset[_device],
 * kzg_open_points[_device] (they work in the same buffers; only an opening of nothing but empty polynomials leaves them alone) and by a
 * _begin that fails: _finish is then KZG_ERR_ARG ("another opening has used the context"), as it is, with its own
 * message, on a context that never began. */
int kzg_open_shard_begin(kzg_ctx* ctx, const void* d_polys, const size_t* lens, size_t k, size_t stride,
                         const uint64_t z[4], const uint64_t xi[4], uint64_t* chunk_eval_out);
int kzg_open_shard_finish(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t z[4], const uint64_t carry[4],
                          int first_rank, uint64_t* out_xy, uint8_t* out_inf, uint64_t* eval_out);

/* ---- weighted sum of single-point quotients: the two proof points of a Shplonk opening ----------
 * With Q_z[p] = (p - p(z)) / (X - z), the call commits
 *     Q = sum_j Q_(z_j)[ sum_i w_ij p_i ],   j < t points, i < k polynomials (k, t <= 64),
 * n = max lens coefficients wide: out_xy / out_inf = commit(Q), Q's n - 1 coefficients.  points: [t][4] canonical
 * limbs; weights: [k][t][4], row i belongs to polynomial i.  Polynomials, lens and stride are those of kzg_open_device;
 * KZG_ERR_DEGREE applies as it does there: the degree of Q decides, so coefficients of Q beyond the key may be
 * there when they are zero (a polynomial longer than the key that carries no weight, or a sum that cancels), and after
 * an error out_xy / out_inf are as the caller left them.  A zero weight skips its polynomial, a column of zero weights its point;
 * z_j = 0 is a legal point (Q_0[p] is p shifted down by one) and points may repeat.  k = 0, t = 0 or nothing but
 * empty polynomials give the point at infinity.
 * d_quot (device, nullable): receives the n - 1 coefficients of Q as canonical words, the zeros beyond the key
 * included.  It may be a row of the same strided array above the k rows read, so that a second call can take Q as a
 * further polynomial.  After an error (KZG_ERR_DEGREE too) what d_quot holds is unspecified.
 * The call works in the buffers of kzg_open_device: it DROPS a slice held for kzg_open_shard_finish exactly as a plain
 * opening does.  Synchronises.  kzg_open_points takes the polynomials from host memory (d_quot stays a device
 * pointer). */
int kzg_open_points_device(kzg_ctx* ctx, const kzg_srs* srs, const void* d_polys, const size_t* lens, size_t k,
                           size_t stride, const uint64_t* points, size_t t, const uint64_t* weights, void* d_quot,
                           uint64_t* out_xy, uint8_t* out_inf);
int kzg_open_points(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t* polys, const size_t* lens, size_t k,
                    size_t stride, const uint64_t* points, size_t t, const uint64_t* weights, void* d_quot,
                    uint64_t* out_xy, uint8_t* out_inf);

/* Sum of n affine G1 points, on the HOST (no context, no GPU): what every rank does with the partial commitments /
 * partial opening proofs the others computed over their coefficient ranges -- the group law is not an RCCL reduction
 * operator, so the partial points are all-gathered as 97-byte records and added here (one inversion per sum).
 * xy: n x 2*FP_LIMBS canonical limbs; inf: n flags or NULL; KZG_ERR_ARG for a coordinate >= p or a point off the
 * curve.  Replaces the running kzg.add of kzg.py:116 over the ranks' results. */
int kzg_g1_sum(int curve_id, const uint64_t* xy, const uint8_t* inf, size_t n, uint64_t* out_xy, uint8_t* out_inf);

/* ---- compressed G1 points and subgroup membership ---------------------------------------------------
 * Byte formats: big-endian x with flags in the top bits of byte 0.
 *   BLS12-381  48 bytes, ZCash: bit 7 = compressed (must be 1), bit 6 = infinity, bit 5 = y is the larger root
 *              (y > (p - 1) / 2); infinity = bit 6 set, bit 5 clear, every other bit zero (0xc0, then 47 zero bytes)
 *   BN254      32 bytes, gnark: top two bits 10 = finite with the smaller y, 11 = finite with the larger y,
 *              01 = infinity (the other 254 bits zero), 00 = not a compressed point
 * Status of a point, one byte each, first failure wins:
 *   0 ok   1 bad encoding (the flags, a malformed infinity, x >= p)   2 x^3 + b is not a square: no such point
 *   3 on the curve but outside the subgroup of prime order r (BLS12-381 only: BN254's cofactor is 1)
 * The subgroup test of BLS12-381 is phi(P) = -[u^2] P with phi(x, y) = (beta x, y): exact, 126 doublings and 10
 * additions per point instead of the ~255 and ~128 of [r] P.  Infinity passes.
 *   kzg_g1_compress        n affine points (kzg_srs_load_g1's layout) -> n blobs.  A coordinate >= p or a point off
 *                          the curve is KZG_ERR_ARG (kzg_verify_cosets' rule); nothing is written then.
 *   kzg_g1_decompress      n blobs -> affine points, infinity flags and statuses.  KZG_OK when it ran: the verdicts are
 *                          in out_status.  A failed point decompresses to zeros with the flag 0.  check_subgroup = 0
 *                          never reports 3.
 *   kzg_g1_decompress_device   the same on device pointers (16-byte aligned; d_xy n * 2*FP_LIMBS limbs, d_inf and
 *                          d_status n bytes), enqueued on the context's stream without synchronising.
 *   kzg_g1_check_subgroup  statuses of n affine points: 0, 2 (a coordinate >= p or a point off the curve) or 3.
 *   kzg_srs_load_g1_compressed   kzg_srs_load_g1 from n blobs: decompressed on the device and expanded there, no
 *                          round trip of the points through the host.  Any status other than 0 is KZG_ERR_ARG and
 *                          kzg_last_error names the first such index and its status.  n = 0 is KZG_ERR_ARG, as for
 *                          kzg_srs_load_g1.
 *   kzg_srs_export_compressed    points [start, start + count) of a key as blobs (kzg_srs_export's range rule).
 * n = 0 is KZG_OK with no work; more than 2^24 points per call is KZG_ERR_ARG.  Host pointers in and out and a
 * synchronised stream, except for the _device form. */
int kzg_g1_compress(kzg_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out_bytes);
int kzg_g1_decompress(kzg_ctx* ctx, const uint8_t* bytes, size_t n, int check_subgroup, uint64_t* out_xy,
                      uint8_t* out_inf, uint8_t* out_status);
int kzg_g1_decompress_device(kzg_ctx* ctx, const void* d_bytes, size_t n, int check_subgroup, void* d_xy, void* d_inf,
                             void* d_status);
int kzg_g1_check_subgroup(kzg_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out_status);
int kzg_srs_load_g1_compressed(kzg_ctx* ctx, const uint8_t* bytes, size_t n, int check_subgroup, kzg_srs** out);
int kzg_srs_export_compressed(kzg_ctx* ctx, const kzg_srs* srs, size_t start, size_t count, uint8_t* out_bytes);

/* ---- compressed G2 points and subgroup membership on the twist ---------------------------------------
 * The G2 forms of the calls above.  A point is 4 * FP_LIMBS limbs, x.c0 | x.c1 | y.c0 | y.c1 (kzg_pairing_check's
 * layout; x = x.c0 + x.c1 i).  Byte formats: big-endian x.c1 then x.c0, the flag bits of the G1 format in the top bits
 * of byte 0.
 *   BLS12-381  96 bytes, ZCash; infinity = 0xc0, then 95 zero bytes
 *   BN254      64 bytes, gnark; infinity = 0x40, then 63 zero bytes
 * "The larger y" is lexicographic, c1 first: y.c1 > (p - 1) / 2, or y.c1 = 0 and y.c0 > (p - 1) / 2.
 * Status of a point, one byte each, first failure wins:
 *   0 ok   1 bad encoding (the flags, a malformed infinity, x.c0 or x.c1 >= p)   2 x^3 + b' is not a square in Fp2
 *   3 on the twist but outside the subgroup of prime order r (BOTH curves: BN254's twist has a cofactor too)
 * The subgroup tests are exact and use the endomorphism psi (untwist, Frobenius, twist): psi(Q) = [u] Q on BLS12-381,
 * [u + 1] Q + psi([u] Q) + psi^2([u] Q) = psi^3([2u] Q) on BN254: one multiplication by the 64-bit u instead of one
 * by the 255-bit r.  Infinity passes.  A pairing check against a G2 point outside the subgroup proves nothing:
 * kzg_pairing_check does not test membership, a caller with keys from an untrusted source runs them through here.
 *   kzg_g2_compress        n affine points -> n blobs.  A coordinate >= p or a point off the twist is KZG_ERR_ARG;
 *                          nothing is written then.
 *   kzg_g2_decompress      n blobs -> affine points, infinity flags and statuses.  KZG_OK when it ran: the verdicts are
 *                          in out_status.  A failed point decompresses to zeros with the flag 0.  check_subgroup = 0
 *                          never reports 3.
 *   kzg_g2_decompress_device   the same on device pointers (16-byte aligned; d_xy n * 4*FP_LIMBS limbs, d_inf and
 *                          d_status n bytes), enqueued on the context's stream without synchronising.
 *   kzg_g2_check_subgroup  statuses of n affine points: 0, 2 (a coordinate >= p or a point off the twist) or 3.
 * n = 0 is KZG_OK with no work; more than 2^24 points per call is KZG_ERR_ARG.  Host pointers in and out and a
 * synchronised stream, except for the _device form.  Profiling spans: "g2_decompress" (ONE per kzg_g2_decompress*),
 * "g2_subgroup" (ONE per kzg_g2_check_subgroup). */
int kzg_g2_compress(kzg_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out_bytes);
int kzg_g2_decompress(kzg_ctx* ctx, const uint8_t* bytes, size_t n, int check_subgroup, uint64_t* out_xy,
                      uint8_t* out_inf, uint8_t* out_status);
int kzg_g2_decompress_device(kzg_ctx* ctx, const void* d_bytes, size_t n, int check_subgroup, void* d_xy, void* d_inf,
                             void* d_status);
int kzg_g2_check_subgroup(kzg_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out_status);

/* ---- per-point scalar multiplication in G1 and G2 -------------------------------------------------
 * out[i] = [k_i] P_i for n points, the products kept apart (kzg_commit* is their sum): what a participant of a
 * powers-of-tau ceremony does to every section of a setup, cofactor clearing, the G2 powers of a setup.
 * Points: canonical affine limbs and infinity flags (inf may be NULL: no point is infinity) -- G1 x | y (2*FP_LIMBS
 * limbs), G2 x.c0 | x.c1 | y.c0 | y.c1 (4*FP_LIMBS limbs, kzg_pairing_check's layout).  Any point of the curve or of
 * the twist is accepted, inside the prime-order subgroup or not.
 * Scalars: `scalars` is n * 4 limbs, scalar i the 256-bit integer at limbs 4i .. 4i + 3 AS IT STANDS: it is not
 * reduced modulo r ([r] Q is not infinity for Q outside the subgroup).  The _powers forms multiply point i by
 * c0 * s^i mod r instead, formed on the device; s and c0 must be below r.
 * The results are exact for every point and every scalar: the ladder's additions finish P + P, P + (-P) and infinite
 * operands, which points of small order and scalars near multiples of r reach.
 *   kzg_g1_mul_each / kzg_g2_mul_each      host pointers in and out, synchronised.
 *   kzg_g1_mul_powers / kzg_g2_mul_powers  the same with the scalars c0 * s^i.
 *   kzg_g1_mul_each_device  device pointers (16-byte aligned; d_inf may be NULL), enqueued on the context's stream
 *                          without synchronising (the call waits for the stream only when its table has to grow).
 *                          It cannot fail for a bad point: such a point's output is zeros with the flag 2.
 *   kzg_srs_mul_powers     key handle -> new key handle: point i of `srs` times c0 * s^i, never through the host.
 *                          `srs` may be a monomial or a Lagrange key; *out is a plain (monomial-tagged) key of the same
 *                          length, the caller's to free.  Synchronises.
 * A coordinate >= p, a point off its curve, or s or c0 >= r is KZG_ERR_ARG with the first offending index (or the
 * argument's name) in kzg_last_error, and nothing is written.  n = 0 is KZG_OK with no work; more than 2^21 points per
 * call is KZG_ERR_ARG.  Profiling spans: "g1_mul_each", "g2_mul_each" (ONE per call). */
int kzg_g1_mul_each(kzg_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, const uint64_t* scalars,
                    uint64_t* out_xy, uint8_t* out_inf);
int kzg_g1_mul_each_device(kzg_ctx* ctx, const void* d_xy, const void* d_inf, size_t n, const void* d_scalars,
                           void* d_out_xy, void* d_out_inf);
int kzg_g1_mul_powers(kzg_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, const uint64_t s[4],
                      const uint64_t c0[4], uint64_t* out_xy, uint8_t* out_inf);
int kzg_srs_mul_powers(kzg_ctx* ctx, const kzg_srs* srs, const uint64_t s[4], const uint64_t c0[4], kzg_srs** out);
int kzg_g2_mul_each(kzg_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, const uint64_t* scalars,
                    uint64_t* out_xy, uint8_t* out_inf);
int kzg_g2_mul_powers(kzg_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, const uint64_t s[4],
                      const uint64_t c0[4], uint64_t* out_xy, uint8_t* out_inf);

/* ---- linear combinations in G2 -----------------------------------------------------------------------
 * out = sum_i [k_i] Q_i for n points of the twist, as ONE point: a commitment in G2, a random linear combination of
 * verification keys, the two folds of a setup's G2 chain.  The products of kzg_g2_mul_each summed on the device: no
 * per-point inversion and no per-point result on the host.
 * Points and scalars: exactly those of kzg_g2_mul_each / kzg_g2_mul_powers -- canonical affine limbs
 * x.c0 | x.c1 | y.c0 | y.c1 with optional infinity flags, any point of the twist inside the prime-order subgroup or
 * not; `scalars` n * 4 limbs, each the 256-bit integer AS IT STANDS (not reduced modulo r), or -- _powers -- the
 * scalars c0 * s^i mod r formed on the device, s and c0 below r (s = 0 gives c0, 0, 0, ...).
 * The sum is exact for every input: every addition of the sum finishes P + P, P + (-P) and infinite operands, which
 * equal points with equal scalars, a point and its negative, and points of small order all reach.
 *   kzg_g2_lincomb         host pointers in and out, synchronised.  out_xy: 4*FP_LIMBS limbs, zeros when the sum is
 *                          infinity; *out_inf: 1 for infinity, else 0.
 *   kzg_g2_lincomb_powers  the same with the scalars c0 * s^i.
 * A coordinate >= p or a point off the twist is KZG_ERR_ARG with the smallest offending index in kzg_last_error; s or
 * c0 >= r is KZG_ERR_ARG naming the argument, before any work; more than 2^21 points per call is KZG_ERR_ARG.  A call
 * that fails writes nothing to out_xy and out_inf.  n = 0 is KZG_OK and the sum is infinity.  Profiling span:
 * "g2_lincomb" (ONE per call, copies in and out included). */
int kzg_g2_lincomb(kzg_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, const uint64_t* scalars,
                   uint64_t* out_xy, uint8_t* out_inf);
int kzg_g2_lincomb_powers(kzg_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, const uint64_t s[4],
                          const uint64_t c0[4], uint64_t* out_xy, uint8_t* out_inf);

/* ---- EIP-4844 blobs as bytes: device intake and SHA-256 challenges ---------------------------------
 * A blob is n = 2^log_n field elements of 32 big-endian bytes each; b blobs lie one after the other ([b][n][32]).
 *   kzg_blob_to_fr          every element checked < r and written as four canonical little-endian limbs:
 *                           out_vals[j][i] = element i of blob j, or out_vals[j][bitrev_log_n(i)] when bit_reversed != 0
 *                           (EIP-4844 keeps a blob in bit-reversed order over the domain: the output is then in natural
 *                           order, what kzg_commit / kzg_open_evals / kzg_fr_eval_lagrange_batch take against a Lagrange
 *                           key).  A non-canonical element is not an error of the call: the verdict is in out_status,
 *                           one byte per blob, 0 ok, 1 some element >= r (as with kzg_g1_decompress); such an element is
 *                           written as zeros.
 *   kzg_blob_challenges     out_z[j] = SHA-256("FSBLOBVERIFY_V1_" | n as 16 bytes big-endian | blob j | commitment j)
 *                           read as a 256-bit big-endian number mod r, canonical limbs: compute_challenge of EIP-4844.
 *                           commitments: [b][G] bytes, G the size of a compressed point (48 on BLS12-381, 32 on BN254;
 *                           BN254 has no standard for this hash: the same construction over its own r and point bytes).
 *                           The bytes are hashed as given: neither the elements' canonicity nor the commitment's
 *                           validity is looked at, the hash is defined on bytes.  One lane per blob, 64-byte blocks,
 *                           n/2 + 2 compressions per blob.
 *   kzg_fr_to_blob          the intake's inverse: out_bytes[j][i] = the 32 big-endian bytes of
 *                           vals[j][i], or of vals[j][bitrev_log_n(i)] when bit_reversed != 0.  vals: [b][n][4] limbs;
 *                           out_status[j] = 1 if some element of row j is >= r, and that element's bytes are zeros.
 *                           One row of N natural-order evaluations with bit_reversed != 0 gives the N/l cells of
 *                           EIP-7594 one after the other: cell c is the coset bitrev(c) of kzg_open_cosets, element t
 *                           of a cell its value bitrev_log_l(t).  _device: d_vals 32-byte, d_bytes 16-byte aligned.
 * Ranges: 1 <= log_n <= 24 and b * 2^log_n <= 2^26 elements per call, otherwise KZG_ERR_ARG; b = 0 is KZG_OK with no
 * work.  The host forms take host pointers and synchronise.  The _device forms take device pointers (16-byte aligned;
 * d_vals and d_z 32-byte aligned; d_status b bytes), enqueue on the context's stream and do not wait.  Both run on the
 * context's stream alone: results of kzg_commit_device_async / kzg_open_device_async still pending are neither retired
 * nor disturbed. */
int kzg_blob_to_fr(kzg_ctx* ctx, uint32_t log_n, const uint8_t* blobs, size_t b, int bit_reversed, uint64_t* out_vals,
                   uint8_t* out_status);
int kzg_blob_to_fr_device(kzg_ctx* ctx, uint32_t log_n, const void* d_blobs, size_t b, int bit_reversed, void* d_vals,
                          void* d_status);
int kzg_fr_to_blob(kzg_ctx* ctx, uint32_t log_n, const uint64_t* vals, size_t b, int bit_reversed, uint8_t* out_bytes,
                   uint8_t* out_status);
int kzg_fr_to_blob_device(kzg_ctx* ctx, uint32_t log_n, const void* d_vals, size_t b, int bit_reversed, void* d_bytes,
                          void* d_status);
int kzg_blob_challenges(kzg_ctx* ctx, uint32_t log_n, const uint8_t* blobs, const uint8_t* commitments, size_t b,
                        uint64_t* out_z);
int kzg_blob_challenges_device(kzg_ctx* ctx, uint32_t log_n, const void* d_blobs, const void* d_commitments, size_t b,
                               void* d_z);

/* ---- device vector / polynomial primitives over Fr ------------------------------------------------
 * What the reference's callers do with Sage's dense polynomials between the transforms and the
 * commitments (plonk/prover.py:243-316: accumulator ratios, products, division by Z_H on a coset),
 * as passes over device-resident vectors of canonical 32-byte elements.  All enqueue on the context's
 * stream; out may alias an input for the element-wise ones (vec_op, vec_lincomb, vec_mul_powers,
 * vec_inverse: the same pointer, not a partial overlap).  vec_prefix_product: out must not overlap d_a.
 *   vec_op          out[i] = a[i] (+ | - | *) b[i]            op: 0 add, 1 sub, 2 mul
 *   vec_lincomb     out[i] = sum_j scalars[j] * p_j[i]         (p_j of lens[j] < n read as zero-padded)
 *   vec_mul_powers  out[i] = a[i] * c0 * s^i                   (coset shift of a coefficient vector)
 *   vec_inverse     out[i] = a[i]^-1, 0 -> 0
 *   vec_prefix_product  out[i] = prod_(j<i) a[j]               (exclusive; out[0] = 1)
 *   poly_eval       out = sum_i a[i] z^i                       (synchronises) */
int kzg_fr_vec_op(kzg_ctx* ctx, int op, size_t n, const void* d_a, const void* d_b, void* d_out);
int kzg_fr_vec_lincomb(kzg_ctx* ctx, size_t n, size_t k, const void* const* d_ptrs, const size_t* lens,
                       const uint64_t* scalars, void* d_out);
int kzg_fr_vec_mul_powers(kzg_ctx* ctx, size_t n, const void* d_a, const uint64_t s[4], const uint64_t c0[4],
                          void* d_out);
int kzg_fr_vec_inverse(kzg_ctx* ctx, size_t n, const void* d_a, void* d_out);
int kzg_fr_vec_prefix_product(kzg_ctx* ctx, size_t n, const void* d_a, void* d_out);
int kzg_fr_poly_eval(kzg_ctx* ctx, size_t n, const void* d_a, const uint64_t z[4], uint64_t out[4]);
/* Every value p_i(z_j) of k device-resident polynomials (`stride` elements apart, lens[i] <= stride coefficients) at
 * t points ([t][4] canonical limbs): out[i][j], [k][t][4] limbs in host memory.  k, t <= 64.  Each polynomial is read
 * once for all points of a launch; one copy and one synchronisation end the call.  Works in buffers of its own (a
 * slice held for kzg_open_shard_finish stays). */
int kzg_fr_poly_eval_batch(kzg_ctx* ctx, const void* d_polys, const size_t* lens, size_t k, size_t stride,
                           const uint64_t* points, size_t t, uint64_t* out);

/* Barycentric evaluation of one value vector over H = {w^i} (len <= 2^log_n values, missing ones zero; longer is
 * KZG_ERR_DEGREE) at z, z in H included: p(z) of the interpolant.  Device-resident values; synchronises. */
int kzg_fr_eval_lagrange(kzg_ctx* ctx, uint32_t log_n, const uint64_t w[4], size_t len, const void* d_vals,
                         const uint64_t z[4], uint64_t out[4]);
/* The same for b value vectors over ONE domain, vector j at its own point z_j (z_j in H included): out[j] is
 * kzg_fr_eval_lagrange's result for vector j and z_j -- the claimed values of a batch of blobs at their challenges.
 *   vals   [b][stride][4] canonical limbs, vector j holds lens[j] <= 2^log_n values (missing ones zero)
 *   z, out [b][4] canonical limbs (z reduced by the caller)
 * KZG_ERR_DEGREE for a lens[j] above 2^log_n; KZG_ERR_ARG for lens[j] > stride, log_n outside [1, 24] or a w that is
 * not a primitive 2^log_n-th root.  b = 0 is KZG_OK with no work.  The launch count does not depend on b: per chunk
 * of vectors (tuning key "eval_batch_chunk") the denominators z_j - w^i of the whole block, one batch inversion, one
 * reduction pass and one finishing kernel that forms (z_j^n - 1)/n on the device.  The host form takes host pointers
 * and synchronises; the _device form takes device pointers (32-byte aligned), enqueues on the context's stream and
 * does not wait for its own work.  It is not free of host waits: the lengths travel through one pinned array of the
 * context, so a call first waits until the PREVIOUS call's copy of its lengths has left that array (and with it for
 * whatever was queued on the stream before that copy), and a call that needs more scratch than any before it
 * reallocates, which synchronises the device. */
int kzg_fr_eval_lagrange_batch(kzg_ctx* ctx, uint32_t log_n, const uint64_t w[4], const uint64_t* vals,
                               const size_t* lens, size_t b, size_t stride, const uint64_t* z, uint64_t* out);
int kzg_fr_eval_lagrange_batch_device(kzg_ctx* ctx, uint32_t log_n, const uint64_t w[4], const void* d_vals,
                                      const size_t* lens, size_t b, size_t stride, const void* d_z, void* d_out);
/* ---- pairing-product checks: the verdict on the device -------------------------------------------
 * m equations of k pairs each, row-major [m][k]: is the product over i < k of e(P_i, Q_i) one?  e is the optimal-ate
 * pairing of the context's curve.  A G1 point is laid out as everywhere else (x | y, FP_LIMBS canonical limbs each,
 * with an infinity byte; g1_inf may be NULL: no point is infinity); a G2 point is x.c0, x.c1, y.c0, y.c1 (a
 * coordinate is c0 + c1 i), FP_LIMBS canonical limbs each, with an infinity byte (g2_inf may be NULL likewise).
 * An infinity byte wins over the coordinates beside it and drops its pair from the product.
 * out_status[e], a verdict and not an error (as kzg_blob_to_fr's):
 *   0  the product is one      1  it is not
 *   2  a finite point of the equation has a coordinate >= p, is off the curve (G1) or off the twist (G2)
 * An equation whose points are all infinity has the product one.  Membership in the prime-order subgroups is NOT part
 * of these calls: kzg_g1_check_subgroup tests G1 points and kzg_g2_check_subgroup G2 points (the verification keys of
 * a setup that arrived as bytes).  Input outside the subgroups yields status 0 or 1, no error.
 *   kzg_pairing_check        the statuses alone: what a verifier needs after kzg_verify_cosets / kzg_verify_points,
 *                            one equation [(L, G2), (-R, [tau] G2)].
 *   kzg_pairing_product      also the value of every product raised to c = kzg_pairing_gt_multiple(curve) (the final
 *                            exponentiation computes c (p^12 - 1) / r; c = 1 on BN254, 3 on BLS12-381; r does not
 *                            divide c, so "is one" is unchanged): out_gt[e] is the six Fp2 coefficients of
 *                            1, w, ..., w^5 in Fp12 = Fp2[w]/(w^6 - xi), xi = 9 + i (BN254) or 1 + i (BLS12-381),
 *                            each c0 | c1 in FP_LIMBS canonical limbs -- [m][12][FP_LIMBS]; zeros for status 2.
 * 1 <= k <= 16 and m <= 2^20, otherwise KZG_ERR_ARG before anything is queued; m = 0 is KZG_OK with no work.  Host
 * pointers in and out; the calls synchronise the context's stream.  They do not touch the commit pipeline: results
 * pending from kzg_commit_device_async / kzg_open_device_async stay pending and undisturbed. */
int kzg_pairing_check(kzg_ctx* ctx, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy,
                      const uint8_t* g2_inf, size_t m, size_t k, uint8_t* out_status);
int kzg_pairing_product(kzg_ctx* ctx, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy,
                        const uint8_t* g2_inf, size_t m, size_t k, uint64_t* out_gt, uint8_t* out_status);
int kzg_pairing_gt_multiple(int curve);

/* ---- measurement hooks (bench.py) -----------------------------------------------------------
 * When enabled, the library brackets its kernels with HIP events on the stream each one runs on.
 * Span names: "ntt_pass", "msm_partition1", "msm_partition2", "msm_order", "msm_accumulate",
 * "msm_finalize", "msm_reduce", "open_poly" (ONE span per kzg_open*: combination, scan and division),
 * "open_points_poly" (ONE per kzg_open_points*: the polynomial stage alone, not the MSM), "poly_eval_batch" (ONE per
 * kzg_fr_poly_eval_batch),
 * "open_shard_poly" (one per kzg_open_shard_begin and one per _finish), "srs_lagrange" (one per Lagrange key
 * built), "open_evals_poly" (ONE per kzg_open_evals*: combination, value and quotient), "domain_table" (one per
 * kzg_domain_table_create), "open_domain" (ONE per kzg_open_domain*: every chunk, transform and copy), "coset_table"
 * (one per kzg_coset_table_create), "open_cosets" (ONE per kzg_open_cosets*), "open_coset_poly" (ONE per
 * kzg_open_coset*: combination, division and remainder), "verify_cosets" (ONE per kzg_verify_cosets: the whole call on
 * the context's stream; its MSMs also report under the msm_* names), "recover_cosets" (ONE per kzg_recover_cosets*:
 * the product tree and every chunk), "g1_decompress" (ONE per kzg_g1_decompress*, and one per
 * kzg_srs_load_g1_compressed: the decoding, with the subgroup test when asked for), "g1_subgroup" (ONE per
 * kzg_g1_check_subgroup), "g2_decompress" (ONE per kzg_g2_decompress*), "g2_subgroup" (ONE per
 * kzg_g2_check_subgroup), "verify_points" (ONE per kzg_verify_points: the whole call), "eval_lagrange_batch" (ONE per
 * kzg_fr_eval_lagrange_batch*: every chunk), "blob_intake" (ONE per kzg_blob_to_fr*), "blob_output" (ONE per kzg_fr_to_blob*), "blob_challenge" (ONE per
 * kzg_blob_challenges*) and "pairing" (ONE per kzg_pairing_check / kzg_pairing_product: copies and kernel).  kzg_prof_read synchronises the
 * stream and returns the accumulated milliseconds and span count of one name since the last kzg_prof_reset.
 * Two names are not spans: "msm_accumulate_shader_mhz" and "ntt_pass_shader_mhz" return (in *total_ms) the shader
 * clock in MHz the accumulate / NTT kernel ran at since the last reset -- s_memtime over s_memrealtime ticks of its
 * first wave -- and *count = 1 when a launch has reported, 0 otherwise; "ntt_tile_log" returns log2 of the LDS
 * tile the last two-pass transform took; "verify_device_bytes" the bytes of device memory the last kzg_verify_cosets
 * asked for (commit-pipeline slots not included); "verify_points_device_bytes" the bytes the last kzg_verify_points
 * carved out of its scratch buffer; "recover_leaf" the number of linear factors one leaf of
 * kzg_recover_cosets' product tree multiplies out; "msm_accumulate_tail_us" and "msm_accumulate_exit_spread_us"
 * return, in microseconds averaged over the *count accumulate launches since the last reset, how long after the
 * MEAN exit of its waves the last wave of a launch left (the time its SIMDs stand half empty or idle) and how long
 * after the FIRST -- for launches of one grid size that do not overlap (those of one context never do). */
int kzg_prof_enable(kzg_ctx* ctx, int on);
int kzg_prof_reset(kzg_ctx* ctx);
int kzg_prof_read(kzg_ctx* ctx, const char* name, double* total_ms, uint64_t* count);

#ifdef __cplusplus
}
#endif
#endif /* KZG_MI355X_H */
