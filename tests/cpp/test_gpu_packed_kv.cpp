// test_gpu_packed_kv.cpp -- SavePacked / Load through both drop-in facades
// (gpu_cceh.h, gpu_cceh_hybrid.h): a table saved as a packed image
// (packed_image.h: only the stored pairs) is loaded by a new backend object,
// answers every Get and takes more inserts; the packed file is smaller than
// the Save file of the same table, and a new object loaded from either holds
// the same table; a truncated packed file is refused and leaves the table
// alone.  Usage: test_gpu_packed_kv <dir for the image files> [n_keys]
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

static std::vector<uint8_t> slurp(const std::string& path) {
  std::vector<uint8_t> b;
  if (FILE* f = fopen(path.c_str(), "rb")) {
    fseek(f, 0, SEEK_END);
    b.resize((size_t)ftell(f));
    fseek(f, 0, SEEK_SET);
    if (fread(b.data(), 1, b.size(), f) != b.size()) b.clear();
    fclose(f);
  }
  return b;
}

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
    bad += !a.SavePacked(path.c_str());
    bad += !a.Save((path + ".v1").c_str());
    cap = a.Capacity();
    bad += a.core().failed_ops() != 0;
  }
  const std::vector<uint8_t> pk = slurp(path), v1 = slurp(path + ".v1");
  bad += pk.size() < 4096 || std::string(pk.begin(), pk.begin() + 8) != "PMDFCPAK";
  bad += v1.size() < 4096 || std::string(v1.begin(), v1.begin() + 8) != "PMDFCIMG";
  bad += pk.size() >= v1.size();
  Facade b(args...);
  bad += !b.Load(path.c_str());
  bad += b.Capacity() != cap;
  for (size_t i = 0; i < n; ++i) {
    Key_t k = keys[i];
    bad += b.Get(k) != val(keys[i] ^ 0x11ULL);
  }
  // the table loaded from the packed file saves the version-1 file's bytes
  bad += !b.Save((path + ".again").c_str());
  bad += slurp(path + ".again") != v1;
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
  // the packed file without its last byte: refused, the table as it was
  const std::string cut = path + ".cut";
  if (FILE* f = fopen(cut.c_str(), "wb")) {
    fwrite(pk.data(), 1, pk.size() - 1, f);
    fclose(f);
  }
  const uint64_t cap2 = b.Capacity();
  bad += b.Load(cut.c_str());
  bad += b.Capacity() != cap2;
  Key_t k0 = keys[2 * n - 1];
  bad += b.Get(k0) != val(keys[2 * n - 1] ^ 0x22ULL);
  bad += b.core().failed_ops() != 0;
  printf("%s packed_round_trip_bad %d\n", what, bad);
  return bad;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  const size_t n = argc > 2 ? strtoull(argv[2], 0, 0) : 20000;
  std::vector<uint64_t> keys(2 * n);
  for (size_t i = 0; i < keys.size(); ++i) {
    keys[i] = splitmix(i + (93ULL << 40));
    if (keys[i] >= (uint64_t)-2 || keys[i] == 0) keys[i] = 0x5555555555555555ULL + i;
  }
  pmdfc_host::BatchingConfig cfg;
  cfg.max_batch = 1 << 12;
  int bad = 0;
  bad += round_trip<pmdfc_host::GpuCCEH>("GpuCCEH", dir + "/ihash.pak", keys, (size_t)8192, false, cfg, (uint64_t)1024);
  bad += round_trip<pmdfc_host::GpuCCEHHybrid>("GpuCCEHHybrid", dir + "/iccch.pak", keys, (size_t)2, cfg, (uint64_t)1024);
  // the two facades write the same format: CCEH_hybrid(8) also starts at depth 3
  {
    pmdfc_host::GpuCCEHHybrid h(8, cfg, 1024);
    int cross = !h.Load((dir + "/ihash.pak").c_str());
    for (size_t i = 0; i < 2 * n; i += 13) {
      Key_t k = keys[i];
      cross += h.Get(k) != (i < n ? val(keys[i] ^ 0x11ULL) : NONE);
    }
    pmdfc_host::GpuCCEHHybrid other(16, cfg, 1024);  // another initial depth: refused
    cross += other.Load((dir + "/ihash.pak").c_str());
    printf("packed_cross_load_bad %d\n", cross);
    bad += cross;
  }
  printf("packed_kv_bad %d\n", bad);
  return bad ? 1 : 0;
}
