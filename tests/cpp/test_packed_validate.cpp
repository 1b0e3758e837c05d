// test_packed_validate.cpp -- the packed table image's host-side validation
// (pmdfc_amd/csrc/packed_image.h) on its own: plain C++, no HIP, no GPU.
//   no arguments : a built-in table through the accept and refuse cases
//   file ...     : one line "<error code> <name of the error>" per image file
//                  (0 = accepted), for tests/test_packed_image_format.py
// Built with -fsanitize=address,undefined by that test: every buffer here is
// exactly as long as the validator may read.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../pmdfc_amd/csrc/packed_image.h"

namespace img = pmdfc::image;
namespace pak = pmdfc::packed;

namespace {

// A whole packed image: segment i holds the slots of occ[i] (a list of slot
// numbers), every pair {1, 2} -- validate() never looks at the pairs' values.
std::vector<uint8_t> make(const std::vector<uint8_t>& ld, const std::vector<std::vector<uint32_t>>& occ,
                          uint32_t initial_depth, uint32_t shard_bits, uint32_t shard_id) {
  img::Header h;
  h.initial_depth = initial_depth;
  h.shard_bits = shard_bits;
  h.shard_id = shard_id;
  h.nseg = ld.size();
  for (const auto& s : occ) h.live += s.size();
  h.total_bytes = pak::total_bytes(h.nseg, h.live);
  h.min_ld = 255;
  for (uint8_t L : ld) {
    h.min_ld = L < h.min_ld ? L : h.min_ld;
    h.max_ld = L > h.max_ld ? L : h.max_ld;
  }
  h.depth = h.max_ld > initial_depth ? h.max_ld : initial_depth;
  std::vector<uint8_t> b(h.total_bytes, 0);
  pak::encode_header(h, b.data());
  for (size_t i = 0; i < ld.size(); ++i) b[img::kHeaderBytes + i] = ld[i];
  uint8_t* o = b.data() + pak::occ_offset(h.nseg);
  uint8_t* p = b.data() + pak::pairs_offset(h.nseg);
  for (size_t i = 0; i < occ.size(); ++i)
    for (uint32_t s : occ[i]) {
      o[i * 128 + (s >> 3)] |= (uint8_t)(1u << (s & 7));  // bit s & 31 of little-endian word s >> 5
      img::put64(p, 1);
      img::put64(p + 8, 2);
      p += 16;
    }
  return b;
}

int check(const std::vector<uint8_t>& b) {
  img::Header h;
  return pak::validate(b.data(), b.size(), &h);
}

int failures = 0;
void expect(const char* name, int got, int want) {
  if (got != want) {
    printf("FAIL %s: got %d (%s), want %d (%s)\n", name, got, pak::error_string(got), want, pak::error_string(want));
    ++failures;
  }
}

int self_test() {
  const std::vector<uint8_t> ld = {1, 2, 3, 3};  // 1/2 + 1/4 + 1/8 + 1/8
  std::vector<uint32_t> all(1024);
  for (uint32_t s = 0; s < 1024; ++s) all[s] = s;
  const std::vector<std::vector<uint32_t>> occ = {{0, 63, 64, 1023}, {}, all, {31, 32}};
  const auto good = make(ld, occ, 1, 0, 0);
  expect("untouched", check(good), pak::kOk);
  {
    img::Header h;
    expect("fields", pak::validate(good.data(), good.size(), &h) == 0 && h.nseg == 4 && h.live == 1030 &&
                             h.total_bytes == 4096 + 4096 + 4096 + 1030 * 16 / 4096 * 4096 + 4096
                         ? 0
                         : 1,
           0);
  }
  expect("empty table", check(make({1, 1}, {{}, {}}, 1, 0, 0)), pak::kOk);
  {
    auto b = good;
    b[3] ^= 0x20;
    expect("magic", check(b), pak::kMagic_);
  }
  {
    auto b = good;
    memcpy(b.data(), img::kMagic, 8);  // a version-1 magic is not a packed image
    expect("version-1 magic", check(b), pak::kMagic_);
  }
  {
    auto b = good;
    b[8] = 2;
    expect("version", check(b), pak::kVersion_);
  }
  {
    auto b = good;
    b.pop_back();
    expect("one byte short", check(b), pak::kSize);
  }
  expect("shorter than a header", check(std::vector<uint8_t>(100, 0)), pak::kShort);
  {
    auto b = good;
    b[pak::occ_offset(4) + 128 + 5] ^= 0x10;  // one more occupancy bit than pairs
    expect("occupancy bit set", check(b), pak::kLive);
  }
  {
    auto b = good;
    b[pak::occ_offset(4)] ^= 1;  // slot 0 of segment 0 cleared
    expect("occupancy bit cleared", check(b), pak::kLive);
  }
  {
    auto b = good;
    img::put64(b.data() + 48, 1031);  // same total_bytes: only the popcount tells
    expect("live off by one", check(b), pak::kLive);
  }
  {
    auto b = good;
    img::put64(b.data() + 48, 4 * 1024 + 1);
    expect("live beyond the slots", check(b), pak::kSize);
  }
  {
    auto b = make({1, 1}, {{}, {}}, 1, 0, 0);
    img::put64(b.data() + 48, 256);  // 256 pairs would need another 4,096 bytes
    expect("live beyond the buffer", check(b), pak::kSize);
  }
  {
    auto b = good;
    b[100] = 1;
    expect("header padding", check(b), pak::kPadding);
  }
  {
    auto b = good;
    b[img::kHeaderBytes + 10] = 7;
    expect("depth padding", check(b), pak::kPadding);
  }
  {
    auto b = good;
    b[pak::occ_offset(4) + 4 * 128] = 1;
    expect("occupancy padding", check(b), pak::kPadding);
  }
  {
    auto b = good;
    b.back() = 1;
    expect("pair padding", check(b), pak::kPadding);
  }
  expect("below initial_depth", check(make({2, 2, 1}, {{}, {}, {}}, 2, 0, 0)), pak::kDepthRange);
  expect("gap", check(make({1, 2, 3, 4}, occ, 1, 0, 0)), pak::kTiling);
  expect("overlap", check(make({1, 1, 3, 3}, occ, 1, 0, 0)), pak::kTiling);
  {
    auto b = good;
    img::put32(b.data() + 32, 4);  // max local depth
    expect("max disagrees", check(b), pak::kSummary);
  }
  expect("shard", check(make({3, 4, 4}, {{5}, {}, {6, 7}}, 2, 2, 3)), pak::kOk);
  expect("shard_id out of range", check(make({2}, {{}}, 2, 2, 4)), pak::kGeometry);
  if (failures) return 1;
  printf("OK\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 1) return self_test();
  for (int i = 1; i < argc; ++i) {
    FILE* f = fopen(argv[i], "rb");
    if (!f) {
      printf("-1 cannot open\n");
      continue;
    }
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> b((size_t)size);
    const size_t got = fread(b.data(), 1, b.size(), f);
    fclose(f);
    img::Header h;
    const int e = got == b.size() ? pak::validate(b.data(), b.size(), &h) : -1;
    printf("%d %s\n", e, e >= 0 ? pak::error_string(e) : "short read");
  }
  return 0;
}
