// image.h -- the table image of pmdfc_cceh_snapshot / pmdfc_cceh_restore
// (DESIGN.md 4.7): its layout and the host-side validation.  Plain C++, no
// HIP: compilable alone (tests/cpp/test_image_validate.cpp).
//
// One contiguous buffer, little-endian:
//   [0, 4096)      header (below; every unused byte zero)
//   [4096, S)      nseg local-depth bytes (global hash bits) in canonical
//                  order, zero-padded to a multiple of 4096
//   [S, total)     nseg x 1024 x {u64 key, u64 value} in canonical order; the
//                  value of an empty slot (key == INVALID) is 0
// Canonical order is directory order, each segment once (the order of
// pmdfc_cceh_dump).  Header fields, by byte offset:
//    0  char[8]  magic "PMDFCIMG"
//    8  u32      format version (1)
//   12  u32      initial_depth
//   16  u32      shard_bits
//   20  u32      shard_id
//   24  u32      logical global depth = max(initial_depth, max local depth)
//   28  u32      min local depth
//   32  u32      max local depth
//   36  u32      0
//   40  u64      nseg
//   48  u64      live entries (slots with key != INVALID)
//   56  u64      total bytes of the image
// The image holds no segment ids, pool offsets, directory entries or
// occupancy words: segment i's hash prefix follows from the running sum of
// 2^-(L_i - shard_bits) over the local depths in order, occupancy is
// key != INVALID.  Every index a restore uses is derived from local depths
// that validate() accepted.
#pragma once
#include <stdint.h>
#include <string.h>

namespace pmdfc {
namespace image {

constexpr uint64_t kHeaderBytes = 4096;
constexpr uint64_t kAlign = 4096;
constexpr uint64_t kSegmentBytes = 1024 * 16;
constexpr uint32_t kVersion = 1;
constexpr uint32_t kMaxLocalDepth = 30;
constexpr uint64_t kMaxSegs = 1ULL << 30;
constexpr char kMagic[8] = {'P', 'M', 'D', 'F', 'C', 'I', 'M', 'G'};

struct Header {
  uint32_t version = kVersion;
  uint32_t initial_depth = 0, shard_bits = 0, shard_id = 0;
  uint32_t depth = 0, min_ld = 0, max_ld = 0;
  uint64_t nseg = 0, live = 0, total_bytes = 0;
};

enum Error {
  kOk = 0,
  kShort,      // fewer bytes than a header
  kMagic_,     // wrong magic
  kVersion_,   // unknown format version
  kGeometry,   // initial_depth / shard_bits / shard_id out of range
  kSize,       // byte counts inconsistent with nseg
  kPadding,    // a byte that must be zero is not
  kDepthRange, // a local depth outside [initial_depth, 30]
  kTiling,     // the local depths do not tile the shard's hash space exactly
  kSummary,    // min / max / depth of the header disagree with the depth bytes
};

inline const char* error_string(int e) {
  switch (e) {
    case kOk: return "ok";
    case kShort: return "image shorter than its header";
    case kMagic_: return "image magic mismatch";
    case kVersion_: return "unknown image format version";
    case kGeometry: return "image geometry out of range";
    case kSize: return "image byte count inconsistent with its segment count";
    case kPadding: return "image padding not zero";
    case kDepthRange: return "image local depth out of range";
    case kTiling: return "image local depths do not tile the hash space";
    case kSummary: return "image header disagrees with its local depths";
  }
  return "image error";
}

inline uint64_t depth_bytes(uint64_t nseg) { return (nseg + kAlign - 1) / kAlign * kAlign; }
inline uint64_t pairs_offset(uint64_t nseg) { return kHeaderBytes + depth_bytes(nseg); }
inline uint64_t total_bytes(uint64_t nseg) { return pairs_offset(nseg) + nseg * kSegmentBytes; }

inline void put32(uint8_t* p, uint32_t v) {
  for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(v >> (8 * i));
}
inline void put64(uint8_t* p, uint64_t v) {
  for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(v >> (8 * i));
}
inline uint32_t get32(const uint8_t* p) {
  uint32_t v = 0;
  for (int i = 0; i < 4; ++i) v |= (uint32_t)p[i] << (8 * i);
  return v;
}
inline uint64_t get64(const uint8_t* p) {
  uint64_t v = 0;
  for (int i = 0; i < 8; ++i) v |= (uint64_t)p[i] << (8 * i);
  return v;
}

// out: kHeaderBytes bytes
inline void encode_header(const Header& h, uint8_t* out) {
  memset(out, 0, kHeaderBytes);
  memcpy(out, kMagic, 8);
  put32(out + 8, h.version);
  put32(out + 12, h.initial_depth);
  put32(out + 16, h.shard_bits);
  put32(out + 20, h.shard_id);
  put32(out + 24, h.depth);
  put32(out + 28, h.min_ld);
  put32(out + 32, h.max_ld);
  put64(out + 40, h.nseg);
  put64(out + 48, h.live);
  put64(out + 56, h.total_bytes);
}

// The header alone: magic, version, geometry, and the byte counts against
// nseg and against `bytes`, the size of the buffer the caller holds.
inline int parse_header(const uint8_t* buf, uint64_t bytes, Header* h) {
  if (bytes < kHeaderBytes) return kShort;
  if (memcmp(buf, kMagic, 8) != 0) return kMagic_;
  h->version = get32(buf + 8);
  if (h->version != kVersion) return kVersion_;
  h->initial_depth = get32(buf + 12);
  h->shard_bits = get32(buf + 16);
  h->shard_id = get32(buf + 20);
  h->depth = get32(buf + 24);
  h->min_ld = get32(buf + 28);
  h->max_ld = get32(buf + 32);
  h->nseg = get64(buf + 40);
  h->live = get64(buf + 48);
  h->total_bytes = get64(buf + 56);
  if (h->initial_depth < 1 || h->initial_depth > kMaxLocalDepth || h->shard_bits > h->initial_depth ||
      h->shard_bits > 16 || (h->shard_bits ? h->shard_id >= (1u << h->shard_bits) : h->shard_id != 0))
    return kGeometry;
  if (h->nseg == 0 || h->nseg > kMaxSegs) return kSize;
  if (h->total_bytes != total_bytes(h->nseg) || bytes != h->total_bytes) return kSize;
  if (h->live > h->nseg * 1024) return kSize;
  if (get32(buf + 36) != 0) return kPadding;
  for (uint64_t i = 64; i < kHeaderBytes; ++i)
    if (buf[i]) return kPadding;
  return kOk;
}

// The local-depth region (depth_bytes(h.nseg) bytes at offset kHeaderBytes)
// against a header parse_header accepted.
inline int validate_depths(const Header& h, const uint8_t* ld) {
  const uint64_t space = 1ULL << (kMaxLocalDepth - h.shard_bits);  // the shard's hash space in units of 2^-30
  uint64_t pos = 0;
  uint32_t mn = ~0u, mx = 0;
  for (uint64_t i = 0; i < h.nseg; ++i) {
    const uint32_t L = ld[i];
    if (L < h.initial_depth || L > kMaxLocalDepth) return kDepthRange;
    const uint64_t span = 1ULL << (kMaxLocalDepth - L);
    if (pos & (span - 1)) return kTiling;  // not aligned to its own stride
    pos += span;
    if (pos > space) return kTiling;
    mn = L < mn ? L : mn;
    mx = L > mx ? L : mx;
  }
  if (pos != space) return kTiling;
  for (uint64_t i = h.nseg; i < depth_bytes(h.nseg); ++i)
    if (ld[i]) return kPadding;
  if (mn != h.min_ld || mx != h.max_ld) return kSummary;
  if (h.depth != (mx > h.initial_depth ? mx : h.initial_depth)) return kSummary;
  return kOk;
}

// A whole image in host memory (the pairs are not looked at).
inline int validate(const uint8_t* buf, uint64_t bytes, Header* h) {
  const int e = parse_header(buf, bytes, h);
  return e ? e : validate_depths(*h, buf + kHeaderBytes);
}

}  // namespace image
}  // namespace pmdfc
