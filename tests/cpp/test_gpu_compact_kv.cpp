// test_gpu_compact_kv.cpp -- Compact of both drop-in facades (gpu_cceh.h,
// gpu_cceh_hybrid.h): a backend with a counting BF attached takes n per-op
// Inserts (enough to split), EraseBatch removes four keys of five, Compact
// merges the thinned segments; every Get afterwards is that of a std::map kept
// alongside, the segment count fell to what the call reported, the filter
// holds exactly the stored keys' counts, a second Compact merges nothing, the
// serving waves answer again, and from a completion callback Compact fails at
// once.
// Usage: test_gpu_compact_kv [n_keys]
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

constexpr uint64_t kBits = 400009;
constexpr uint32_t kHashes = 5;

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
static int compact_trip(const char* what, const std::vector<uint64_t>& keys, A... args) {
  const size_t n = keys.size();
  int bad = 0;
  pmdfc_cbf_t* f = nullptr;
  if (pmdfc_cbf_create(kBits, kHashes, 0, &f) != PMDFC_OK) return 1;
  {
    Facade a(args...);
    a.attach_counting_bf(f);
    std::map<uint64_t, uint64_t> want;
    for (size_t i = 0; i < n; ++i) {
      Key_t k = keys[i];
      a.Insert(k, val(keys[i] ^ 0x11ULL));
      want[keys[i]] = keys[i] ^ 0x11ULL;
    }
    std::vector<uint64_t> gone;
    for (size_t i = 0; i < n; ++i)
      if (i % 5) gone.push_back(keys[i]);
    std::vector<uint8_t> st(gone.size(), 0xEE);
    bad += a.EraseBatch(gone.data(), st.data(), gone.size()) != PMDFC_OK;
    for (uint64_t k : gone) want.erase(k);
    pmdfc_cceh_stats_t s0{}, s1{};
    bad += a.core().Stats(&s0) != PMDFC_OK;
    pmdfc_compact_result_t r{}, r2{};
    bad += a.Compact(512, &r) != PMDFC_OK;
    bad += a.core().Stats(&s1) != PMDFC_OK;
    const int shape_bad = (r.merges == 0) + (r.segments_before != s0.segments) + (r.segments_after != s1.segments) +
                          (r.segments_after + r.merges != r.segments_before) + (s1.error_flags != 0);
    printf("%s segments %llu -> %llu merges %llu rounds %u shape_bad %d\n", what, (unsigned long long)r.segments_before,
           (unsigned long long)r.segments_after, (unsigned long long)r.merges, r.rounds, shape_bad);
    bad += shape_bad;
    bad += gets_bad(a, keys, want);
    uint64_t stored = 0, missing = 1;
    bad += a.core().AuditCountingBF(&stored, &missing) != PMDFC_OK || stored != want.size() || missing != 0;
    bad += a.Compact(512, &r2) != PMDFC_OK || r2.merges != 0 || r2.segments_after != r.segments_after;
    bad += a.Compact(1025, &r2) == PMDFC_OK;  // above 1024: refused
    // the waves serve again, and the table grows again
    for (size_t i = 0; i < n; ++i)
      if (i % 5 == 1) {
        Key_t k = keys[i];
        a.Insert(k, val(keys[i] ^ 0x22ULL));
        want[keys[i]] = keys[i] ^ 0x22ULL;
      }
    bad += gets_bad(a, keys, want);
    bad += a.core().AuditCountingBF(&stored, &missing) != PMDFC_OK || stored != want.size() || missing != 0;
    bad += a.core().failed_ops() != 0;
    // from a completion callback Compact fails at once and changes nothing
    struct Ctx {
      Facade* a;
      std::atomic<int> rc{1};
    } cx;
    cx.a = &a;
    a.core().GetAsync(keys[0], [](void* x, uint8_t, uint64_t) {
      Ctx* c = static_cast<Ctx*>(x);
      pmdfc_compact_result_t r{};
      c->rc = c->a->Compact(512, &r);
    }, &cx);
    a.core().flush();
    const int cb_bad = (cx.rc.load() != PMDFC_ERR_STATE) + gets_bad(a, keys, want);
    printf("%s callback_bad %d\n", what, cb_bad);
    bad += cb_bad;
    a.attach_counting_bf(nullptr);
  }
  pmdfc_cbf_destroy(f);
  printf("%s compact_trip_bad %d\n", what, bad);
  return bad;
}

int main(int argc, char** argv) {
  const size_t n = argc > 1 ? strtoull(argv[1], 0, 0) : 12000;
  std::vector<uint64_t> keys(n);
  for (size_t i = 0; i < keys.size(); ++i) {
    keys[i] = splitmix(i + (91ULL << 40));  // (test_gpu_image_kv's stream: no split of it drops an entry)
    if (keys[i] >= (uint64_t)-2 || keys[i] == 0) keys[i] = 0x5555555555555555ULL + i;
  }
  pmdfc_host::BatchingConfig cfg;
  cfg.max_batch = 1 << 12;
  int bad = 0;
  bad += compact_trip<pmdfc_host::GpuCCEH>("GpuCCEH", keys, (size_t)8192, false, cfg, (uint64_t)1024);
  bad += compact_trip<pmdfc_host::GpuCCEHHybrid>("GpuCCEHHybrid", keys, (size_t)2, cfg, (uint64_t)1024);
  printf("compact_kv_bad %d\n", bad);
  return bad ? 1 : 0;
}
