// test_gpu_erase_kv.cpp -- Erase / EraseBatch of both drop-in facades
// (gpu_cceh.h, gpu_cceh_hybrid.h): a backend with a counting BF attached takes
// n per-op Inserts; Delete stays the reference's stub (false, nothing
// removed); Erase removes one key between served ops, EraseBatch half of the
// rest together with an absent key, a reserved key and a key erased earlier in
// the same batch; every Get afterwards is that of a std::map kept alongside,
// the filter holds exactly the stored keys' counts, and the serving waves
// answer again after every erase (Inserts and Gets follow each).
// Usage: test_gpu_erase_kv [n_keys]
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <map>
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

constexpr uint64_t kBits = 100003;
constexpr uint32_t kHashes = 5;

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

template <class Facade, class... A>
static int erase_trip(const char* what, const std::vector<uint64_t>& keys, A... args) {
  const size_t n = keys.size() / 2;  // keys [0, n) are inserted, [n, 2n) stay absent
  int bad = 0;
  Filter fa;
  Facade a(args...);
  a.attach_counting_bf(fa.f);
  std::map<uint64_t, uint64_t> want;
  for (size_t i = 0; i < n; ++i) {
    Key_t k = keys[i];
    a.Insert(k, val(keys[i] ^ 0x11ULL));
    want[keys[i]] = keys[i] ^ 0x11ULL;
  }
  // the reference's stub: false, and nothing removed
  Key_t k0 = keys[0];
  const bool deleted = a.Delete(k0);
  bad += deleted;
  bad += a.Get(k0) != val(keys[0] ^ 0x11ULL);
  printf("%s Delete %d\n", what, (int)deleted);
  // one key, then served ops again
  bad += !a.Erase(k0);
  want.erase(keys[0]);
  bad += a.Get(k0) != NONE;
  bad += a.Erase(k0);  // already gone
  Key_t absent = keys[n];
  bad += a.Erase(absent);
  a.Insert(k0, val(7));  // the freed slot is taken again
  want[keys[0]] = 7;
  bad += a.Get(k0) != val(7);
  // a batch: keys [1, n/2], an absent key, a reserved key, keys[1] a second time
  std::vector<uint64_t> eb(keys.begin() + 1, keys.begin() + 1 + n / 2);
  eb.push_back(keys[n + 1]);
  eb.push_back(~0ULL);
  eb.push_back(keys[1]);
  std::vector<uint8_t> st(eb.size(), 0xEE);
  bad += a.EraseBatch(eb.data(), st.data(), eb.size()) != PMDFC_OK;
  for (size_t i = 0; i < n / 2; ++i) {
    bad += st[i] != PMDFC_ST_ERASED;
    want.erase(eb[i]);
  }
  bad += st[n / 2] != PMDFC_ST_MISS;
  bad += st[n / 2 + 1] != PMDFC_ST_RESERVED_KEY;
  bad += st[n / 2 + 2] != PMDFC_ST_MISS;
  bad += gets_bad(a, keys, want);
  // the filter: one count per stored key and hash, no stored key missing
  uint64_t stored = 0, missing = 1;
  bad += a.core().AuditCountingBF(&stored, &missing) != PMDFC_OK || stored != want.size() || missing != 0;
  bad += fa.sum() != (uint64_t)want.size() * kHashes;
  // the waves count and serve again
  for (size_t i = n; i < n + n / 4; ++i) {
    Key_t k = keys[i];
    a.Insert(k, val(keys[i] ^ 0x22ULL));
    want[keys[i]] = keys[i] ^ 0x22ULL;
  }
  bad += gets_bad(a, keys, want);
  bad += a.core().AuditCountingBF(&stored, &missing) != PMDFC_OK || stored != want.size() || missing != 0;
  bad += fa.sum() != (uint64_t)want.size() * kHashes;
  bad += a.core().failed_ops() != 0;
  // from a completion callback Erase fails at once and removes nothing
  struct Ctx {
    pmdfc_host::BatchCore* core;
    uint64_t key;
    std::atomic<int> st{-1};
  } cx;
  cx.core = &a.core();
  cx.key = keys[0];
  a.core().GetAsync(keys[0], [](void* x, uint8_t, uint64_t) {
    Ctx* c = static_cast<Ctx*>(x);
    c->st = c->core->Erase(c->key);
  }, &cx);
  a.core().flush();
  const int cb_bad = (cx.st.load() != pmdfc_host::kBatchFailed) +
                     (a.core().last_error().find("completion callback") == std::string::npos) +
                     (a.Get(k0) != val(7)) + (a.core().failed_ops() != 1);
  printf("%s callback_bad %d\n", what, cb_bad);
  bad += cb_bad;
  pmdfc_cceh_stats_t s{};
  bad += a.core().Stats(&s) != PMDFC_OK || s.error_flags != 0;
  a.attach_counting_bf(nullptr);
  printf("%s erase_trip_bad %d\n", what, bad);
  return bad;
}

int main(int argc, char** argv) {
  const size_t n = argc > 1 ? strtoull(argv[1], 0, 0) : 3000;
  std::vector<uint64_t> keys(2 * n);
  for (size_t i = 0; i < keys.size(); ++i) {
    keys[i] = splitmix(i + (91ULL << 40));  // (test_gpu_image_kv's stream: no split of it drops an entry)
    if (keys[i] >= (uint64_t)-2 || keys[i] == 0) keys[i] = 0x5555555555555555ULL + i;
  }
  pmdfc_host::BatchingConfig cfg;
  cfg.max_batch = 1 << 10;  // (EraseBatch of n / 2 + 3 keys takes more than one engine batch)
  int bad = 0;
  bad += erase_trip<pmdfc_host::GpuCCEH>("GpuCCEH", keys, (size_t)8192, false, cfg, (uint64_t)1024);
  bad += erase_trip<pmdfc_host::GpuCCEHHybrid>("GpuCCEHHybrid", keys, (size_t)2, cfg, (uint64_t)1024);
  printf("erase_kv_bad %d\n", bad);
  return bad ? 1 : 0;
}
