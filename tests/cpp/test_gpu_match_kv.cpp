// test_gpu_match_kv.cpp -- EraseMatching of both drop-in facades (gpu_cceh.h,
// gpu_cceh_hybrid.h): a backend with a counting BF attached takes the pages of
// 40 files as per-op Inserts, keys inode << 32 | page index as the cleancache
// clients build them; five inodes are invalidated at once between served ops,
// then every page whose index is 3 mod 8, then a list of 1,024 patterns of
// which two exist; no pattern removes nothing and 1,025 patterns are refused;
// Delete stays the reference's stub.  Every Get afterwards is that of a
// std::map kept alongside, the filter holds exactly the stored keys' counts
// (it is rebuilt under the same stop), and the serving waves answer again
// after every call (Inserts and Gets follow each).
// Usage: test_gpu_match_kv [n_keys]
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../../pmdfc_amd/host/gpu_cceh.h"
#include "../../pmdfc_amd/host/gpu_cceh_hybrid.h"

static Value_t val(uint64_t v) { return reinterpret_cast<Value_t>(v); }

constexpr uint64_t kBits = 100003;
constexpr uint32_t kHashes = 5;
constexpr uint64_t kInodeMask = 0xFFFFFFFF00000000ULL;
constexpr uint64_t kInodes = 40, kFirstInode = 1000;

struct Filter {
  pmdfc_cbf_t* f = nullptr;
  Filter() { pmdfc_cbf_create(kBits, kHashes, 0, &f); }
  ~Filter() { pmdfc_cbf_destroy(f); }
  uint64_t sum() const {
    std::vector<uint8_t> c(kBits, 0);
    if (pmdfc_cbf_get_counters_host(f, c.data(), kBits) != PMDFC_OK) return ~0ULL;
    uint64_t s = 0;
    for (uint8_t x : c) s += x;
    return s;
  }
};

template <class Facade>
static int gets_bad(Facade& a, const std::vector<uint64_t>& keys, const std::map<uint64_t, uint64_t>& want) {
  int bad = 0;
  for (uint64_t key : keys) {
    Key_t k = key;
    const auto it = want.find(key);
    bad += a.Get(k) != (it == want.end() ? NONE : val(it->second));
  }
  return bad;
}

// the keys of `want` under the patterns leave it; returns how many
static uint64_t drop(std::map<uint64_t, uint64_t>& want, uint64_t mask, const std::vector<uint64_t>& pats) {
  uint64_t n = 0;
  for (auto it = want.begin(); it != want.end();) {
    bool hit = false;
    for (uint64_t p : pats) hit |= (it->first & mask) == (p & mask);
    if (hit) {
      it = want.erase(it);
      ++n;
    } else {
      ++it;
    }
  }
  return n;
}

template <class Facade>
static int filter_bad(Facade& a, const Filter& fa, const std::map<uint64_t, uint64_t>& want) {
  uint64_t stored = 0, missing = 1;
  int bad = a.core().AuditCountingBF(&stored, &missing) != PMDFC_OK || stored != want.size() || missing != 0;
  bad += fa.sum() != (uint64_t)want.size() * kHashes;
  return bad;
}

template <class Facade, class... A>
static int match_trip(const char* what, const std::vector<uint64_t>& keys, A... args) {
  int bad = 0;
  Filter fa;
  Facade a(args...);
  a.attach_counting_bf(fa.f);
  std::map<uint64_t, uint64_t> want;
  for (uint64_t key : keys) {
    Key_t k = key;
    a.Insert(k, val(key ^ 0x11ULL));
    want[key] = key ^ 0x11ULL;
  }
  Key_t k0 = keys[0];
  const bool deleted = a.Delete(k0);  // the reference's stub: false, and nothing removed
  bad += deleted || a.Get(k0) != val(keys[0] ^ 0x11ULL);
  printf("%s Delete %d\n", what, (int)deleted);
  pmdfc_erase_matching_result_t r{};
  // five inodes, one of them twice, and one that does not exist
  std::vector<uint64_t> five;
  for (uint64_t i : {3, 4, 17, 17, 30, 39, 5000}) five.push_back((kFirstInode + i) << 32);
  bad += a.EraseMatching(kInodeMask, five.data(), (uint32_t)five.size(), &r) != PMDFC_OK;
  bad += r.removed != drop(want, kInodeMask, five) || r.removed == 0 || r.segments_changed == 0;
  bad += gets_bad(a, keys, want) + filter_bad(a, fa, want);
  // served ops again: the pages of inode 3 come back
  for (uint64_t key : keys)
    if ((key >> 32) == kFirstInode + 3) {
      Key_t k = key;
      a.Insert(k, val(key ^ 0x22ULL));
      want[key] = key ^ 0x22ULL;
    }
  bad += gets_bad(a, keys, want) + filter_bad(a, fa, want);
  // any masked pattern: every page whose index is 3 mod 8
  const uint64_t three = 3;
  bad += a.EraseMatching(7, &three, 1, &r) != PMDFC_OK;
  bad += r.removed != drop(want, 7, {three}) || r.removed == 0;
  bad += a.EraseMatching(7, &three, 1, &r) != PMDFC_OK || r.removed != 0 || r.segments_changed != 0;
  // 1,024 patterns of which two exist; the result may be null
  std::vector<uint64_t> many;
  for (uint64_t i = 0; i < PMDFC_MATCH_MAX - 2; ++i) many.push_back((900000 + i) << 32);
  many.push_back((kFirstInode + 8) << 32);
  many.push_back((kFirstInode + 9) << 32);
  const size_t before = want.size();
  bad += a.EraseMatching(kInodeMask, many.data(), (uint32_t)many.size(), nullptr) != PMDFC_OK;
  bad += drop(want, kInodeMask, many) == 0 || want.size() == before;
  bad += gets_bad(a, keys, want) + filter_bad(a, fa, want);
  // no pattern removes nothing; one too many is refused with the table untouched
  bad += a.EraseMatching(0, nullptr, 0, &r) != PMDFC_OK || r.removed != 0 || r.segments_scanned != 0;
  many.push_back(0);
  bad += a.EraseMatching(0, many.data(), (uint32_t)many.size(), &r) != PMDFC_ERR_ARG;
  bad += a.EraseMatching(0, nullptr, 1, &r) != PMDFC_ERR_ARG;
  bad += gets_bad(a, keys, want) + filter_bad(a, fa, want);
  bad += a.core().failed_ops() != 0;
  // from a completion callback it fails at once and removes nothing
  struct Ctx {
    Facade* f;
    std::atomic<int> rc{0};
  } cx;
  cx.f = &a;
  a.core().GetAsync(keys[0], [](void* x, uint8_t, uint64_t) {
    Ctx* c = static_cast<Ctx*>(x);
    const uint64_t any = 0;
    c->rc = c->f->EraseMatching(0, &any, 1, nullptr);
  }, &cx);
  a.core().flush();
  bad += cx.rc.load() != PMDFC_ERR_STATE;
  bad += gets_bad(a, keys, want);
  // mask 0: the table is empty, and takes keys again
  const uint64_t any = 0x1234;
  bad += a.EraseMatching(0, &any, 1, &r) != PMDFC_OK || r.removed != want.size() || r.segments_cleared != r.segments_changed;
  want.clear();
  bad += gets_bad(a, keys, want) + filter_bad(a, fa, want);
  for (size_t i = 0; i < keys.size() / 4; ++i) {
    Key_t k = keys[i];
    a.Insert(k, val(keys[i] ^ 0x33ULL));
    want[keys[i]] = keys[i] ^ 0x33ULL;
  }
  bad += gets_bad(a, keys, want) + filter_bad(a, fa, want);
  pmdfc_cceh_stats_t s{};
  bad += a.core().Stats(&s) != PMDFC_OK || s.error_flags != 0;
  a.attach_counting_bf(nullptr);
  printf("%s match_bad %d\n", what, bad);
  return bad;
}

int main(int argc, char** argv) {
  const size_t n = argc > 1 ? strtoull(argv[1], 0, 0) : 3000;
  std::vector<uint64_t> keys;
  for (uint64_t ino = 0; ino < kInodes; ++ino)
    for (uint64_t idx = 0; idx < n / kInodes; ++idx) keys.push_back(((kFirstInode + ino) << 32) | idx);
  pmdfc_host::BatchingConfig cfg;
  cfg.max_batch = 1 << 10;
  int bad = 0;
  bad += match_trip<pmdfc_host::GpuCCEH>("GpuCCEH", keys, (size_t)8192, false, cfg, (uint64_t)1024);
  bad += match_trip<pmdfc_host::GpuCCEHHybrid>("GpuCCEHHybrid", keys, (size_t)2, cfg, (uint64_t)1024);
  printf("match_kv_bad %d\n", bad);
  return bad ? 1 : 0;
}
