// blob.hip -- EIP-4844 blobs as bytes on the device: three kernels around the single-blob
// functions of blob.h, and the host drivers behind kzg_blob_to_fr*, kzg_fr_to_blob* and kzg_blob_challenges*.
//
//   intake      blob_intake_kernel: one lane per field element.  Two 16-byte loads, the byte swap into canonical
//               little-endian words, the comparison with r and two 16-byte stores, to the element's own place or to
//               the bit-reversed one.  An element >= r is stored as zeros and sets its blob's status byte: every such
//               lane stores the same 1, so a plain store serves and the status bytes are zeroed first on the stream.
//   output      blob_output_kernel: the intake's inverse, one lane per field element.  Two 16-byte loads from the
//               element's own place or the bit-reversed one, the comparison with r, the byte swap and two 16-byte
//               stores.  An element >= r leaves zero bytes and sets its row's status byte, as in the intake.
//   challenge   blob_challenge_kernel: one lane per blob (the hash is sequential within a blob, independent across
//               blobs).  The lanes of a wave read addresses a whole blob apart, so every block is a gather of four
//               16-byte pieces per lane; blob.h asks for the pieces of the next block before it compresses this one.
//               State, two message windows and the temporaries stay in registers: no scratch, no LDS.
// All run on the context's stream alone: pending results of the commit pipeline are neither retired nor disturbed.
#include <algorithm>
#include <string>
#include "internal.h"
#include "msm.h"
#include "g1_util.h"
#include "g1_bytes.h"
#include "blob.h"

namespace kzg {

namespace {

constexpr uint32_t BLOB_MAX_LOG_N = 24;
constexpr size_t BLOB_MAX_ELEMS = (size_t)1 << 26;       // elements per call
constexpr uint32_t CHALLENGE_TB = 64;                    // one wave per workgroup: the few lanes spread over the CUs

// vals[j][i or bitrev(i)] = element i of blob j, canonical words; status[j] = 1 if one of its elements is >= r
template <class F>
__global__ __launch_bounds__(256) void blob_intake_kernel(const uint32_t* blobs, size_t total, uint32_t log_n,
                                                          int bit_reversed, uint32_t* vals, uint8_t* status) {
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += step) {
    const size_t j = idx >> log_n;
    const uint32_t i = (uint32_t)(idx & (((size_t)1 << log_n) - 1));
    uint32_t raw[8], w[8];
    ld_words<8>(blobs + idx * 8, raw);
    const bool ok = blob_element<F>(raw, w);
    const uint32_t at = bit_reversed ? bitrev(i, log_n) : i;
    st_words<8>(vals + ((j << log_n) + at) * 8, w);
    if (!ok) status[j] = 1;
  }
}

// out[j][i] = the 32 big-endian bytes of vals[j][i or bitrev(i)]; status[j] = 1 if one of row j's elements is >= r
template <class F>
__global__ __launch_bounds__(256) void blob_output_kernel(const uint32_t* vals, size_t total, uint32_t log_n,
                                                          int bit_reversed, uint32_t* out, uint8_t* status) {
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += step) {
    const size_t j = idx >> log_n;
    const uint32_t i = (uint32_t)(idx & (((size_t)1 << log_n) - 1));
    const uint32_t at = bit_reversed ? bitrev(i, log_n) : i;
    uint32_t w[8], raw[8];
    ld_words<8>(vals + ((j << log_n) + at) * 8, w);
    const bool ok = blob_output_element<F>(w, raw);
    st_words<8>(out + idx * 8, raw);
    if (!ok) status[j] = 1;
  }
}

// the 16-byte pieces of one blob in global memory
struct BlobPieces {
  const uint4* base;
  KZG_HD void operator()(uint32_t q, uint32_t* out) const {
    const uint4 v = base[q];
    out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
  }
};

// z[j] = the challenge of blob j and commitment j, canonical words
template <class C>
__global__ __launch_bounds__(CHALLENGE_TB) void blob_challenge_kernel(const uint32_t* blobs, const uint32_t* comms,
                                                                      uint32_t b, uint32_t log_n, uint32_t* z) {
  constexpr int G = G1Bytes<C>::SIZE;
  const uint32_t j = blockIdx.x * CHALLENGE_TB + threadIdx.x;
  if (j >= b) return;
  uint32_t comm[G / 4];
  ld_words<G / 4>(comms + (size_t)j * (G / 4), comm);
  const BlobPieces pieces{reinterpret_cast<const uint4*>(blobs) + ((size_t)j << (log_n + 1))};
  uint64_t limbs[4];
  blob_challenge<typename C::Fr, G>(log_n, pieces, comm, limbs);
  uint32_t w[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) { w[2 * k] = (uint32_t)limbs[k]; w[2 * k + 1] = (uint32_t)(limbs[k] >> 32); }
  st_words<8>(z + (size_t)j * 8, w);
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// enqueue only
template <class F>
int intake_launch(Ctx* c, uint32_t log_n, const uint32_t* d_blobs, size_t b, int bit_reversed, uint32_t* d_vals,
                  uint8_t* d_status) {
  const size_t total = b << log_n;
  const uint32_t blocks = (uint32_t)std::min<size_t>((total + 255) / 256, 8192);
  KZG_HIP(c, hipMemsetAsync(d_status, 0, b, c->stream));
  hipLaunchKernelGGL(blob_intake_kernel<F>, dim3(blocks), dim3(256), 0, c->stream, d_blobs, total, log_n, bit_reversed,
                     d_vals, d_status);
  KZG_HIP(c, hipGetLastError());
  return KZG_OK;
}
template <class F>
int output_launch(Ctx* c, uint32_t log_n, const uint32_t* d_vals, size_t b, int bit_reversed, uint32_t* d_out,
                  uint8_t* d_status) {
  const size_t total = b << log_n;
  const uint32_t blocks = (uint32_t)std::min<size_t>((total + 255) / 256, 8192);
  KZG_HIP(c, hipMemsetAsync(d_status, 0, b, c->stream));
  hipLaunchKernelGGL(blob_output_kernel<F>, dim3(blocks), dim3(256), 0, c->stream, d_vals, total, log_n, bit_reversed,
                     d_out, d_status);
  KZG_HIP(c, hipGetLastError());
  return KZG_OK;
}
template <class C>
int challenge_launch(Ctx* c, uint32_t log_n, const uint32_t* d_blobs, const uint32_t* d_comms, size_t b, uint32_t* d_z) {
  hipLaunchKernelGGL(blob_challenge_kernel<C>, dim3((uint32_t)((b + CHALLENGE_TB - 1) / CHALLENGE_TB)),
                     dim3(CHALLENGE_TB), 0, c->stream, d_blobs, d_comms, (uint32_t)b, log_n, d_z);
  KZG_HIP(c, hipGetLastError());
  return KZG_OK;
}

template <class F>
int blob_to_fr_t(Ctx* c, uint32_t log_n, const uint8_t* blobs, size_t b, int bit_reversed, uint64_t* out_vals,
                 uint8_t* out_status) {
  const size_t bytes = (b << log_n) * 32;
  uint32_t *d_blobs, *d_vals;
  uint8_t* d_status;
  int rc = carve(c, c->io,
                 [&](Carve& ws) { d_blobs = ws.take(bytes);  d_vals = ws.take(bytes);  d_status = ws.take<uint8_t>(b); });
  if (rc) return rc;
  {
    ProfScope span(c, "blob_intake");
    KZG_HIP(c, hipMemcpyAsync(d_blobs, blobs, bytes, hipMemcpyHostToDevice, c->stream));
    if ((rc = intake_launch<F>(c, log_n, d_blobs, b, bit_reversed, d_vals, d_status))) return rc;
    KZG_HIP(c, hipMemcpyAsync(out_vals, d_vals, bytes, hipMemcpyDeviceToHost, c->stream));
    KZG_HIP(c, hipMemcpyAsync(out_status, d_status, b, hipMemcpyDeviceToHost, c->stream));
  }
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  return KZG_OK;
}

template <class F>
int fr_to_blob_t(Ctx* c, uint32_t log_n, const uint64_t* vals, size_t b, int bit_reversed, uint8_t* out_bytes,
                 uint8_t* out_status) {
  const size_t bytes = (b << log_n) * 32;
  uint32_t *d_vals, *d_out;
  uint8_t* d_status;
  int rc = carve(c, c->io,
                 [&](Carve& ws) { d_vals = ws.take(bytes);  d_out = ws.take(bytes);  d_status = ws.take<uint8_t>(b); });
  if (rc) return rc;
  {
    ProfScope span(c, "blob_output");
    KZG_HIP(c, hipMemcpyAsync(d_vals, vals, bytes, hipMemcpyHostToDevice, c->stream));
    if ((rc = output_launch<F>(c, log_n, d_vals, b, bit_reversed, d_out, d_status))) return rc;
    KZG_HIP(c, hipMemcpyAsync(out_bytes, d_out, bytes, hipMemcpyDeviceToHost, c->stream));
    KZG_HIP(c, hipMemcpyAsync(out_status, d_status, b, hipMemcpyDeviceToHost, c->stream));
  }
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  return KZG_OK;
}

template <class C>
int blob_challenges_t(Ctx* c, uint32_t log_n, const uint8_t* blobs, const uint8_t* commitments, size_t b,
                      uint64_t* out_z) {
  constexpr size_t G = G1Bytes<C>::SIZE;
  const size_t bytes = (b << log_n) * 32;
  uint32_t *d_blobs, *d_comms, *d_z;
  int rc = carve(c, c->io,
                 [&](Carve& ws) { d_blobs = ws.take(bytes);  d_comms = ws.take(b * G);  d_z = ws.take(b * 32); });
  if (rc) return rc;
  {
    ProfScope span(c, "blob_challenge");
    KZG_HIP(c, hipMemcpyAsync(d_blobs, blobs, bytes, hipMemcpyHostToDevice, c->stream));
    KZG_HIP(c, hipMemcpyAsync(d_comms, commitments, b * G, hipMemcpyHostToDevice, c->stream));
    if ((rc = challenge_launch<C>(c, log_n, d_blobs, d_comms, b, d_z))) return rc;
    KZG_HIP(c, hipMemcpyAsync(out_z, d_z, b * 32, hipMemcpyDeviceToHost, c->stream));
  }
  KZG_HIP(c, hipStreamSynchronize(c->stream));
  return KZG_OK;
}

int size_check(Ctx* c, uint32_t log_n, size_t b, const char* who) {
  if (log_n < 1 || log_n > BLOB_MAX_LOG_N || b > (BLOB_MAX_ELEMS >> log_n)) {
    const std::string msg = std::string(who) + ": need 1 <= log_n <= 24 and b * 2^log_n <= 2^26";
    return set_err(c, KZG_ERR_ARG, msg.c_str());
  }
  return KZG_OK;
}

}  // namespace

int blob_to_fr(Ctx* c, uint32_t log_n, const uint8_t* blobs, size_t b, int bit_reversed, uint64_t* out_vals,
               uint8_t* out_status) {
  if (int rc = size_check(c, log_n, b, "kzg_blob_to_fr")) return rc;
  if (b == 0) return KZG_OK;
  return KZG_BY_FR(c, blob_to_fr_t, c, log_n, blobs, b, bit_reversed, out_vals, out_status);
}
int blob_to_fr_device(Ctx* c, uint32_t log_n, const void* d_blobs, size_t b, int bit_reversed, void* d_vals,
                      void* d_status) {
  if (int rc = size_check(c, log_n, b, "kzg_blob_to_fr_device")) return rc;
  if (b == 0) return KZG_OK;
  if (!aligned(d_blobs, 16) || !aligned(d_vals, 32))
    return set_err(c, KZG_ERR_ARG, "kzg_blob_to_fr_device: misaligned device pointer");
  ProfScope span(c, "blob_intake");
  return KZG_BY_FR(c, intake_launch, c, log_n, static_cast<const uint32_t*>(d_blobs), b, bit_reversed,
                   static_cast<uint32_t*>(d_vals), static_cast<uint8_t*>(d_status));
}
int blob_intake_launch(Ctx* c, uint32_t log_n, const uint32_t* d_blobs, size_t b, int bit_reversed, uint32_t* d_vals,
                       uint8_t* d_status) {
  return KZG_BY_FR(c, intake_launch, c, log_n, d_blobs, b, bit_reversed, d_vals, d_status);
}
int fr_to_blob(Ctx* c, uint32_t log_n, const uint64_t* vals, size_t b, int bit_reversed, uint8_t* out_bytes,
               uint8_t* out_status) {
  if (int rc = size_check(c, log_n, b, "kzg_fr_to_blob")) return rc;
  if (b == 0) return KZG_OK;
  return KZG_BY_FR(c, fr_to_blob_t, c, log_n, vals, b, bit_reversed, out_bytes, out_status);
}
int fr_to_blob_device(Ctx* c, uint32_t log_n, const void* d_vals, size_t b, int bit_reversed, void* d_bytes,
                      void* d_status) {
  if (int rc = size_check(c, log_n, b, "kzg_fr_to_blob_device")) return rc;
  if (b == 0) return KZG_OK;
  if (!aligned(d_vals, 32) || !aligned(d_bytes, 16))
    return set_err(c, KZG_ERR_ARG, "kzg_fr_to_blob_device: misaligned device pointer");
  ProfScope span(c, "blob_output");
  return KZG_BY_FR(c, output_launch, c, log_n, static_cast<const uint32_t*>(d_vals), b, bit_reversed,
                   static_cast<uint32_t*>(d_bytes), static_cast<uint8_t*>(d_status));
}
int blob_challenges(Ctx* c, uint32_t log_n, const uint8_t* blobs, const uint8_t* commitments, size_t b,
                    uint64_t* out_z) {
  if (int rc = size_check(c, log_n, b, "kzg_blob_challenges")) return rc;
  if (b == 0) return KZG_OK;
  return KZG_BY_CURVE(c, blob_challenges_t, c, log_n, blobs, commitments, b, out_z);
}
int blob_challenges_device(Ctx* c, uint32_t log_n, const void* d_blobs, const void* d_commitments, size_t b,
                           void* d_z) {
  if (int rc = size_check(c, log_n, b, "kzg_blob_challenges_device")) return rc;
  if (b == 0) return KZG_OK;
  if (!aligned(d_blobs, 16) || !aligned(d_commitments, 16) || !aligned(d_z, 32))
    return set_err(c, KZG_ERR_ARG, "kzg_blob_challenges_device: misaligned device pointer");
  ProfScope span(c, "blob_challenge");
  return KZG_BY_CURVE(c, challenge_launch, c, log_n, static_cast<const uint32_t*>(d_blobs),
                      static_cast<const uint32_t*>(d_commitments), b, static_cast<uint32_t*>(d_z));
}

}  // namespace kzg
