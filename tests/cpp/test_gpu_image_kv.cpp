// test_gpu_image_kv.cpp -- Save / Load of the table image through both drop-in
// facades and the per-op front-end (gpu_cceh.h, gpu_cceh_hybrid.h,
// batch_core.h): a table saved by one backend object is loaded by a new one
// (the restart) and answers every Get, then takes more inserts; a Load that is
// refused leaves the table alone; Save and Load from a completion callback
// fail at once.  Usage: test_gpu_image_kv <dir for the image files> [n_keys]
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
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

// n keys in, saved, loaded into a new object of the same kind, every Get a
// hit; then n more into the loaded table (its splits start from the restored
// occupancy and directory)
template <class Facade, class... A>
static int round_trip(const char* what, const std::string& path, const std::vector<uint64_t>& keys, A... args) {
  const size_t n = keys.size() / 2;
  int bad = 0;
  uint64_t cap = 0;
  {
    Facade a(args...);
    for (size_t i = 0; i < n; ++i) {
      Key_t k = keys[i];
      a.Insert(k, val(keys[i] ^ 0x11ULL));
    }
    bad += !a.Save(path.c_str());
    cap = a.Capacity();
    bad += a.core().failed_ops() != 0;
  }
  Facade b(args...);
  bad += !b.Load(path.c_str());
  bad += b.Capacity() != cap;
  for (size_t i = 0; i < n; ++i) {
    Key_t k = keys[i];
    bad += b.Get(k) != val(keys[i] ^ 0x11ULL);
  }
  for (size_t i = n; i < 2 * n; ++i) {
    Key_t k = keys[i];
    bad += b.Get(k) != NONE;
    b.Insert(k, val(keys[i] ^ 0x22ULL));
  }
  for (size_t i = 0; i < 2 * n; ++i) {
    Key_t k = keys[i];
    bad += b.Get(k) != val(keys[i] ^ (i < n ? 0x11ULL : 0x22ULL));
  }
  bad += b.Capacity() <= cap;  // it grew on
  // a file that is no image, and a missing one: refused, the table as it was
  const std::string junk = path + ".junk";
  if (FILE* f = fopen(junk.c_str(), "wb")) {
    for (int i = 0; i < 5000; ++i) fputc(i & 0xFF, f);
    fclose(f);
  }
  const uint64_t cap2 = b.Capacity();
  bad += b.Load(junk.c_str());
  bad += b.Load((path + ".missing").c_str());
  bad += b.Capacity() != cap2;
  Key_t k0 = keys[0];
  bad += b.Get(k0) != val(keys[0] ^ 0x11ULL);
  bad += b.core().failed_ops() != 0;
  printf("%s round_trip_bad %d\n", what, bad);
  return bad;
}

struct Ctx {
  pmdfc_host::BatchCore* core;
  std::string path;
  std::atomic<int> save_rc{1}, load_rc{1}, done{0};
};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  const size_t n = argc > 2 ? strtoull(argv[2], 0, 0) : 20000;
  std::vector<uint64_t> keys(2 * n);
  for (size_t i = 0; i < keys.size(); ++i) {
    keys[i] = splitmix(i + (91ULL << 40));
    if (keys[i] >= (uint64_t)-2 || keys[i] == 0) keys[i] = 0x5555555555555555ULL + i;
  }
  pmdfc_host::BatchingConfig cfg;
  cfg.max_batch = 1 << 12;
  int bad = 0;
  // src/cceh CCEH(8192) -> depth 3: the table splits many times on the way
  bad += round_trip<pmdfc_host::GpuCCEH>("GpuCCEH", dir + "/ihash.img", keys, (size_t)8192, false, cfg, (uint64_t)1024);
  // CCEH_hybrid(2), NUMA_KV's default
  bad += round_trip<pmdfc_host::GpuCCEHHybrid>("GpuCCEHHybrid", dir + "/iccch.img", keys, (size_t)2, cfg, (uint64_t)1024);
  // the two facades write the same format: CCEH_hybrid(8) also starts at depth 3
  {
    pmdfc_host::GpuCCEHHybrid h(8, cfg, 1024);
    int cross = !h.Load((dir + "/ihash.img").c_str());
    for (size_t i = 0; i < 2 * n; i += 13) {
      Key_t k = keys[i];
      cross += h.Get(k) != (i < n ? val(keys[i] ^ 0x11ULL) : NONE);  // (saved before the second half went in)
    }
    // another initial depth: refused
    pmdfc_host::GpuCCEHHybrid other(16, cfg, 1024);
    cross += other.Load((dir + "/ihash.img").c_str());
    printf("cross_load_bad %d\n", cross);
    bad += cross;
  }
  // from a completion callback both calls fail at once
  {
    pmdfc_host::GpuCCEH t(8192, false, cfg, 1024);
    Ctx cx;
    cx.core = &t.core();
    cx.path = dir + "/callback.img";
    t.core().InsertAsync(keys[1], keys[1], [](void* x, uint8_t, uint64_t) {
      Ctx* c = static_cast<Ctx*>(x);
      c->save_rc = c->core->Save(c->path.c_str());
      c->load_rc = c->core->Load(c->path.c_str());
      c->done = 1;
    }, &cx);
    for (int ms = 0; !cx.done.load() && ms < 30000; ++ms) std::this_thread::sleep_for(std::chrono::milliseconds(1));
    const int cb = !(cx.done.load() && cx.save_rc.load() == PMDFC_ERR_STATE && cx.load_rc.load() == PMDFC_ERR_STATE);
    FILE* f = fopen(cx.path.c_str(), "rb");
    if (f) fclose(f);
    printf("callback_bad %d\n", cb + (f ? 1 : 0));  // and no file was written
    bad += cb + (f ? 1 : 0);
  }
  printf("image_kv_bad %d\n", bad);
  return bad ? 1 : 0;
}
