// devmem.h -- who frees device memory, and how a scratch buffer is divided.  Host code that needs the HIP runtime's
// declarations and nothing else of the library: tests/shim/workspace_shim.cpp compiles it for the CPU.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>
#include <memory>
#include <vector>

namespace kzg {

struct Ctx;
struct DevBuf { void* p = nullptr; size_t cap = 0; };
int ensure_buf(Ctx* c, DevBuf& b, size_t bytes);

// a short-lived hipMalloc that its scope frees; release() hands it to a longer-lived object
struct HipFree { void operator()(void* p) const { (void)hipFree(p); } };
template <class T>
struct DevTmp : std::unique_ptr<T, HipFree> {
  hipError_t alloc(size_t bytes) {
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    this->reset(static_cast<T*>(p));
    return e;
  }
  operator T*() const { return this->get(); }
};
// a heap object that holds device memory, freed by Free unless release()d to the caller (Srs, DomainTable)
template <class T, void (*Free)(T*)> struct FreeWith { void operator()(T* p) const { Free(p); } };
template <class T, void (*Free)(T*)> using Owned = std::unique_ptr<T, FreeWith<T, Free>>;

// One pass over a layout: every segment starts on a multiple of 256 bytes, in the order taken.  Without a base the
// pass only measures (every pointer is null).
struct Carve {
  uint8_t* base = nullptr;
  size_t total = 0;
  static constexpr size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
  template <class T = uint32_t> T* take(size_t bytes) {
    uint8_t* p = base ? base + total : nullptr;
    total += up256(bytes);
    return reinterpret_cast<T*>(p);
  }
  // an optional array: absent (or empty) it is null and takes no room
  template <class T = uint8_t> T* take_if(bool present, size_t bytes) { return present && bytes ? take<T>(bytes) : nullptr; }
};
// layout(Carve&), a list of `ptr = ws.take(bytes)` lines, runs twice: to measure, then -- `buf` grown -- to assign
template <class Layout>
int carve(Ctx* c, DevBuf& buf, Layout&& layout, size_t* total = nullptr) {
  Carve measure, assign;
  layout(measure);
  if (int rc = ensure_buf(c, buf, measure.total)) return rc;
  assign.base = static_cast<uint8_t*>(buf.p);
  layout(assign);
  if (total) *total = assign.total;
  return 0;
}

// The counting sort of both bulk verifications: perm[off[j] .. off[j + 1]) are the k < K with idx[k] == j, rising.
// Returns K, or the first k with idx[k] >= n_groups (off and perm are then unfinished).
inline size_t group_by_index(const uint32_t* idx, size_t K, size_t n_groups, std::vector<uint32_t>& off,
                             std::vector<uint32_t>& perm) {
  off.assign(n_groups + 1, 0);
  perm.resize(K);
  for (size_t k = 0; k < K; ++k) {
    if (idx[k] >= n_groups) return k;
    ++off[idx[k] + 1];
  }
  for (size_t j = 0; j < n_groups; ++j) off[j + 1] += off[j];
  std::vector<uint32_t> cur(off.begin(), off.end() - 1);
  for (size_t k = 0; k < K; ++k) perm[cur[idx[k]]++] = (uint32_t)k;
  return K;
}

}  // namespace kzg
