// csrc/devmem.h and csrc/ver_layout.h on the CPU: a program of its own over a counting hipMalloc / hipFree defined
// here (no HIP library is linked).  Without arguments it checks the owners, the carve and the counting sort and
// prints "no violations"; `verify ...` / `points ...` print the offsets of one workspace layout for the sizes given
// (tests/test_workspace_host.py compares them with the arithmetic restated there); `plan ...` prints the launch plan
// of kzg_verify_cosets (VerPlan) for one call (tests/test_verify_scalars_host.py: each shape of the exact-point tests
// reaches the regime it is there for).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../kzg_snark_amd/csrc/ver_layout.h"

static int live = 0, calls = 0, fail_at = -1;            // allocations alive; hipMalloc calls; the call that fails
extern "C" hipError_t hipMalloc(void** p, size_t bytes) {
  if (calls++ == fail_at) { *p = nullptr; return hipErrorOutOfMemory; }
  *p = malloc(bytes ? bytes : 1);
  ++live;
  return hipSuccess;
}
extern "C" hipError_t hipFree(void* p) {
  if (p) { free(p); --live; }
  return hipSuccess;
}

namespace kzg {
struct Ctx {};
int ensure_buf(Ctx*, DevBuf& b, size_t bytes) {
  if (b.cap >= bytes) return 0;
  (void)hipFree(b.p);
  b.cap = 0;
  if (hipMalloc(&b.p, bytes) != hipSuccess) return -5;
  b.cap = bytes;
  return 0;
}
}  // namespace kzg
using namespace kzg;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { ++fails; printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

// a scope with three temporaries, as the key loaders have; `handed` takes the middle one over
static hipError_t three_temporaries(int fail, uint32_t** handed) {
  calls = 0;
  fail_at = fail;
  DevTmp<uint32_t> a, b;
  DevTmp<uint8_t> c;
  hipError_t e;
  if ((e = a.alloc(64)) != hipSuccess) return e;
  if ((e = b.alloc(128)) != hipSuccess) return e;
  if ((e = c.alloc(7)) != hipSuccess) return e;
  EXPECT(live == 3 && a.get() && static_cast<uint32_t*>(b) == b.get());
  if (handed) *handed = b.release();
  return hipSuccess;
}

struct Thing { uint32_t* d = nullptr; };
static void thing_free(Thing* t) { (void)hipFree(t->d); delete t; }

static void check_owners() {
  for (int fail = -1; fail < 3; ++fail) {
    EXPECT((three_temporaries(fail, nullptr) == hipSuccess) == (fail < 0));
    EXPECT(live == 0);
  }
  uint32_t* kept = nullptr;
  EXPECT(three_temporaries(-1, &kept) == hipSuccess && kept && live == 1);   // exactly one allocation changed hands
  (void)hipFree(kept);
  EXPECT(live == 0);
  fail_at = -1;
  {
    DevTmp<uint32_t> again;
    EXPECT(again.alloc(8) == hipSuccess && again.alloc(16) == hipSuccess && live == 1);   // the first one is not lost
    Owned<Thing, thing_free> t(new Thing());
    EXPECT(hipMalloc(reinterpret_cast<void**>(&t->d), 32) == hipSuccess && live == 2);
    Owned<Thing, thing_free> out(new Thing());
    Thing* raw = out.release();                           // handed to a caller: not freed here
    thing_free(raw);
  }
  EXPECT(live == 0);
}

static void check_carve() {
  Ctx ctx;
  DevBuf buf;
  uint32_t *a = nullptr, *b = nullptr;
  uint8_t *none = (uint8_t*)1, *empty = (uint8_t*)1, *flags = nullptr;
  size_t total = 0, passes = 0, before = 0, after = 0;
  auto layout = [&](Carve& w) {
    ++passes;
    a = w.take(1);
    before = w.total;
    none = w.take_if(false, 100);
    empty = w.take_if(true, 0);
    after = w.total;
    flags = w.take_if(true, 257);
    b = w.take(256);
  };
  fail_at = -1;
  EXPECT(carve(&ctx, buf, layout, &total) == 0 && passes == 2);
  Carve measure;
  layout(measure);
  EXPECT(measure.total == total && total == 256 + 512 + 256 && buf.cap == total);
  EXPECT(a == nullptr && b == nullptr && flags == nullptr);             // the measuring pass hands out nothing
  EXPECT(carve(&ctx, buf, layout) == 0);
  uint8_t* base = static_cast<uint8_t*>(buf.p);
  EXPECT((uint8_t*)a == base && none == nullptr && empty == nullptr && before == 256 && after == 256);
  EXPECT(flags == base + 256 && (uint8_t*)b == base + 768);
  EXPECT(Carve::up256(0) == 0 && Carve::up256(1) == 256 && Carve::up256(256) == 256 && Carve::up256(257) == 512);
  // a buffer that cannot grow: the error comes back and nothing is assigned
  passes = 0;
  calls = 0;
  fail_at = 0;
  DevBuf small;
  EXPECT(carve(&ctx, small, layout) == -5 && passes == 1 && small.p == nullptr);
  fail_at = -1;
  (void)hipFree(buf.p);
  EXPECT(live == 0);
}

static void check_sort() {
  std::vector<uint32_t> off, perm;
  const uint32_t idx[5] = {2, 0, 2, 1, 0};
  EXPECT(group_by_index(idx, 5, 3, off, perm) == 5);
  EXPECT(off == (std::vector<uint32_t>{0, 2, 3, 5}) && perm == (std::vector<uint32_t>{1, 4, 3, 0, 2}));
  const uint32_t one[1] = {0};
  EXPECT(group_by_index(one, 1, 1, off, perm) == 1);
  EXPECT(off == (std::vector<uint32_t>{0, 1}) && perm == (std::vector<uint32_t>{0}));
  const uint32_t bad[4] = {1, 0, 3, 7};
  EXPECT(group_by_index(bad, 4, 3, off, perm) == 2);                    // the first index that is n_groups or more
  EXPECT(group_by_index(one, 0, 2, off, perm) == 0 && off == (std::vector<uint32_t>{0, 0, 0}) && perm.empty());
}

// one layout through carve(): "name offset" per segment (-1: absent), then "total bytes"
template <class Ws, class Layout, class Print>
static int print_layout(Ws& d, Layout layout, Print print) {
  Ctx ctx;
  DevBuf buf;
  size_t total = 0;
  Carve measure;
  layout(measure);
  if (carve(&ctx, buf, layout, &total) || measure.total != total) return 1;
  const uint8_t* base = static_cast<const uint8_t*>(buf.p);
  print([&](const char* name, const void* p) {
    printf("%s %ld\n", name, p ? (long)(static_cast<const uint8_t*>(p) - base) : -1L);
  });
  printf("total %zu\n", total);
  (void)hipFree(buf.p);
  return live != 0;
}

int main(int argc, char** argv) {
  std::vector<size_t> v;
  for (int i = 2; i < argc; ++i) v.push_back(strtoull(argv[i], nullptr, 10));
#define P(f) row(#f, d.f)
  if (argc == 12 && !strcmp(argv[1], "verify")) {        // K n_comm l pflags cflags pt_bytes rb pow_tab sum_threads nsp
    VerifyWs d;
    return print_layout(d, [&](Carve& w) { d.layout(w, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9]); },
                        [&](auto row) {
      P(pxy); P(pinf); P(cxy); P(cinf); P(recs); P(vals); P(r); P(s); P(slice); P(cidx); P(perm); P(off); P(wtab);
      P(rtab); P(part); P(cpart); P(T); P(coef); P(bad);
    });
  }
  if (argc == 14 && !strcmp(argv[1], "points")) {        // K n_comm pflags cflags pt_bytes rb pow_tab weight_threads
    VerifyPointsWs d;                                    // nsp blocks xyzz tab_bytes
    return print_layout(d, [&](Carve& w) {
      d.layout(w, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11]);
    }, [&](auto row) {
      P(pxy); P(pinf); P(cxy); P(cinf); P(precs); P(crecs); P(z); P(y); P(r); P(s); P(perm); P(off); P(rtab);
      P(ypart); P(cpart); P(coef); P(partial); P(out); P(bad); P(tab);
    });
  }
#undef P
  if (argc == 7 && !strcmp(argv[1], "plan")) {           // K log_l n_comm win_bits fr_bits: "name value" per field
    const VerPlan p(v[0], (uint32_t)v[1], v[2], (uint32_t)v[3], (uint32_t)v[4]);
    printf("M %zu\nlog_e %u\nntiles %zu\nlds_bytes %zu\ncell_grid %u\nsum_threads %u\nsum_cnt %u\nshares %u\n"
           "slice_bits %u\nslices %u\n", p.M, p.log_e, p.ntiles, p.lds_bytes, p.cell_grid, p.sum_threads, p.sum_cnt,
           p.shares, p.slice_bits, p.slices);
    return 0;
  }
  if (argc != 1) { printf("usage: workspace_shim [verify ... | points ... | plan ...]\n"); return 2; }
  check_owners();
  check_carve();
  check_sort();
  if (fails) { printf("%d checks failed\n", fails); return 1; }
  printf("no violations\n");
  return 0;
}
