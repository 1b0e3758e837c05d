// test_image_validate.cpp -- the table image's host-side validation
// (pmdfc_amd/csrc/image.h) on its own: plain C++, no HIP, no GPU.
//   no arguments : a built-in table through the accept and refuse cases
//   file ...     : one line "<error code> <name of the error>" per image file
//                  (0 = accepted), for tests/test_image_format.py
// Built with -fsanitize=address,undefined by that test: every buffer here is
// exactly as long as the validator may read.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../pmdfc_amd/csrc/image.h"

namespace img = pmdfc::image;

namespace {

// header + local depths only: validate() never reads the pairs, and the
// sanitizer would catch it if it did
std::vector<uint8_t> make(const std::vector<uint8_t>& ld, uint32_t initial_depth, uint32_t shard_bits,
                          uint32_t shard_id) {
  img::Header h;
  h.initial_depth = initial_depth;
  h.shard_bits = shard_bits;
  h.shard_id = shard_id;
  h.nseg = ld.size();
  h.total_bytes = img::total_bytes(h.nseg);
  h.min_ld = 255;
  for (uint8_t L : ld) {
    h.min_ld = L < h.min_ld ? L : h.min_ld;
    h.max_ld = L > h.max_ld ? L : h.max_ld;
  }
  h.depth = h.max_ld > initial_depth ? h.max_ld : initial_depth;
  std::vector<uint8_t> b(img::kHeaderBytes + img::depth_bytes(h.nseg), 0);
  img::encode_header(h, b.data());
  for (size_t i = 0; i < ld.size(); ++i) b[img::kHeaderBytes + i] = ld[i];
  return b;
}

int check(const std::vector<uint8_t>& b, uint64_t bytes) {
  img::Header h;
  return img::validate(b.data(), bytes, &h);
}

int failures = 0;
void expect(const char* name, int got, int want) {
  if (got != want) {
    printf("FAIL %s: got %d (%s), want %d (%s)\n", name, got, img::error_string(got), want, img::error_string(want));
    ++failures;
  }
}

int self_test() {
  const std::vector<uint8_t> ld = {1, 2, 3, 3};  // 1/2 + 1/4 + 1/8 + 1/8
  const uint64_t total = img::total_bytes(ld.size());
  expect("untouched", check(make(ld, 1, 0, 0), total), img::kOk);
  {
    auto b = make(ld, 1, 0, 0);
    b[0] ^= 1;
    expect("magic", check(b, total), img::kMagic_);
  }
  {
    auto b = make(ld, 1, 0, 0);
    b[8] = 2;
    expect("version", check(b, total), img::kVersion_);
  }
  expect("one byte short", check(make(ld, 1, 0, 0), total - 1), img::kSize);
  expect("shorter than a header", check(std::vector<uint8_t>(100, 0), 100), img::kShort);
  expect("below initial_depth", check(make({2, 2, 1}, 2, 0, 0), img::total_bytes(3)), img::kDepthRange);
  {
    std::vector<uint8_t> deep(3, 1);
    deep[1] = 31;
    expect("local depth 31", check(make(deep, 1, 0, 0), img::total_bytes(3)), img::kDepthRange);
  }
  expect("gap at the end", check(make({1, 2, 3, 4}, 1, 0, 0), total), img::kTiling);
  expect("gap in the middle", check(make({1, 3, 3, 3}, 1, 0, 0), total), img::kTiling);
  expect("overlap", check(make({1, 1, 3, 3}, 1, 0, 0), total), img::kTiling);
  expect("misaligned", check(make({2, 1, 2}, 1, 0, 0), img::total_bytes(3)), img::kTiling);
  {
    auto b = make(ld, 1, 0, 0);
    img::put32(b.data() + 32, 4);  // max local depth
    expect("max disagrees", check(b, total), img::kSummary);
  }
  {
    auto b = make(ld, 1, 0, 0);
    img::put32(b.data() + 24, 5);  // depth
    expect("depth disagrees", check(b, total), img::kSummary);
  }
  {
    auto b = make(ld, 1, 0, 0);
    b[img::kHeaderBytes + 10] = 7;  // past the last local depth
    expect("padding", check(b, total), img::kPadding);
  }
  // a shard of four: its quarter of the space, depths from shard_bits up
  expect("shard", check(make({3, 4, 4}, 2, 2, 3), img::total_bytes(3)), img::kOk);
  expect("shard overfull", check(make({2, 3}, 2, 2, 3), img::total_bytes(2)), img::kTiling);
  expect("shard_id out of range", check(make({2}, 2, 2, 4), img::total_bytes(1)), img::kGeometry);
  // the deepest table the format allows
  expect("depth 30", check(make({1, 2, 30, 30, 29, 28, 27, 26, 25, 24, 23, 22, 21, 20, 19, 18, 17, 16, 15, 14, 13,
                                 12, 11, 10, 9, 8, 7, 6, 5, 4, 3}, 1, 0, 0), img::total_bytes(31)), img::kOk);
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
    const int e = got == b.size() ? img::validate(b.data(), b.size(), &h) : -1;
    printf("%d %s\n", e, e >= 0 ? img::error_string(e) : "short read");
  }
  return 0;
}
