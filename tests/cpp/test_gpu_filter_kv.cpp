// test_gpu_filter_kv.cpp -- the counting BF across Save / Load of both drop-in
// facades (gpu_cceh.h, gpu_cceh_hybrid.h): a backend with a filter attached
// takes n per-op Inserts (each counted by the serving wave) and saves; a new
// backend object with a fresh filter loads the file, and Load rebuilds the
// filter from the table: its counters equal the first filter's (a
// duplicate-free stream with no drops), its packed bitmap is the counters'
// and no stored key is missing; more Inserts keep counting, and
// rebuild_counting_bf gives the same counters again.  A refused file leaves
// the filter as it was.  Usage: test_gpu_filter_kv <dir for the image files> [n_keys]
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../pmdfc_amd/host/gpu_cceh.h"
#include "../../pmdfc_amd/host/gpu_cceh_hybrid.h"

static uint64_t splitmix(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

static Value_t val(uint64_t v) { return reinterpret_cast<Value_t>(v); }

constexpr uint64_t kBits = 100003;  // not a multiple of 4, 64 or 4,096
constexpr uint32_t kHashes = 5;

struct Filter {
  pmdfc_cbf_t* f = nullptr;
  Filter() { pmdfc_cbf_create(kBits, kHashes, 0, &f); }
  ~Filter() { pmdfc_cbf_destroy(f); }
  std::vector<uint8_t> counters() const {
    std::vector<uint8_t> c(kBits, 0xEE);
    if (pmdfc_cbf_get_counters_host(f, c.data(), kBits) != PMDFC_OK) c.assign(kBits, 0xEE);
    return c;
  }
  // the packed bitmap is the counters' (MSB-first u64 words)
  int bitmap_bad(const std::vector<uint8_t>& c) const {
    std::vector<uint64_t> bm((kBits + 63) / 64), want((kBits + 63) / 64, 0);
    if (pmdfc_cbf_get_bitmap_host(f, bm.data(), bm.size()) != PMDFC_OK) return 1;
    for (uint64_t j = 0; j < kBits; ++j)
      if (c[j]) want[j / 64] |= 1ULL << (63 - j % 64);
    return bm != want;
  }
};

template <class Facade, class... A>
static int filter_trip(const char* what, const std::string& path, const std::vector<uint64_t>& keys, A... args) {
  const size_t n = keys.size() / 2;
  int bad = 0;
  std::vector<uint8_t> first;
  {
    Filter fa;
    Facade a(args...);
    a.attach_counting_bf(fa.f);
    for (size_t i = 0; i < n; ++i) {
      Key_t k = keys[i];
      a.Insert(k, val(keys[i] ^ 0x11ULL));
    }
    bad += !a.Save(path.c_str());
    bad += a.core().failed_ops() != 0;
    first = fa.counters();
    uint64_t st = 0, miss = 1;
    bad += a.core().AuditCountingBF(&st, &miss) != PMDFC_OK || st != n || miss != 0;
    a.attach_counting_bf(nullptr);
  }
  uint64_t sum = 0;
  for (uint8_t c : first) sum += c;
  bad += sum != (uint64_t)n * kHashes;  // (no counter saturates at this size: every Insert was counted)
  Filter fb;
  Facade b(args...);
  b.attach_counting_bf(fb.f);
  uint64_t stored = 0, missing = 0;
  bad += b.core().AuditCountingBF(&stored, &missing) != PMDFC_OK || stored != 0 || missing != 0;
  bad += !b.Load(path.c_str());
  std::vector<uint8_t> got = fb.counters();
  bad += got != first;
  bad += fb.bitmap_bad(got);
  bad += b.core().AuditCountingBF(&stored, &missing) != PMDFC_OK || stored != n || missing != 0;
  // a refused file: the filter as it was
  const std::string junk = path + ".junk";
  if (FILE* f = fopen(junk.c_str(), "wb")) {
    for (int i = 0; i < 5000; ++i) fputc(i & 0xFF, f);
    fclose(f);
  }
  bad += b.Load(junk.c_str());
  bad += fb.counters() != first;
  // the restarted waves count into the rebuilt filter
  for (size_t i = n; i < 2 * n; ++i) {
    Key_t k = keys[i];
    b.Insert(k, val(keys[i] ^ 0x22ULL));
  }
  bad += b.core().AuditCountingBF(&stored, &missing) != PMDFC_OK || stored != 2 * n || missing != 0;
  std::vector<uint8_t> grown = fb.counters();
  sum = 0;
  for (uint8_t c : grown) sum += c;
  bad += sum != (uint64_t)2 * n * kHashes;
  stored = 0;
  bad += b.rebuild_counting_bf(&stored) != PMDFC_OK || stored != 2 * n;
  bad += fb.counters() != grown;
  bad += fb.bitmap_bad(grown);
  bad += b.core().failed_ops() != 0;
  b.attach_counting_bf(nullptr);
  // without a filter there is nothing to rebuild, and Load is the plain one
  bad += b.rebuild_counting_bf() != PMDFC_ERR_STATE;
  bad += !b.Load(path.c_str());
  bad += fb.counters() != grown;
  printf("%s filter_trip_bad %d\n", what, bad);
  return bad;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  const size_t n = argc > 2 ? strtoull(argv[2], 0, 0) : 3000;
  std::vector<uint64_t> keys(2 * n);
  for (size_t i = 0; i < keys.size(); ++i) {
    keys[i] = splitmix(i + (91ULL << 40));  // (test_gpu_image_kv's stream: no split of it drops an entry)
    if (keys[i] >= (uint64_t)-2 || keys[i] == 0) keys[i] = 0x5555555555555555ULL + i;
  }
  pmdfc_host::BatchingConfig cfg;
  cfg.max_batch = 1 << 12;
  int bad = 0;
  bad += filter_trip<pmdfc_host::GpuCCEH>("GpuCCEH", dir + "/ihash_bf.img", keys, (size_t)8192, false, cfg, (uint64_t)1024);
  bad += filter_trip<pmdfc_host::GpuCCEHHybrid>("GpuCCEHHybrid", dir + "/iccch_bf.img", keys, (size_t)2, cfg,
                                                (uint64_t)1024);
  printf("filter_kv_bad %d\n", bad);
  return bad ? 1 : 0;
}
