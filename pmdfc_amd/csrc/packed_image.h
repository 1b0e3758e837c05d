// packed_image.h -- the packed table image of pmdfc_cceh_snapshot_packed /
// pmdfc_cceh_restore: only the live entries.  Plain C++, no
// HIP: compilable alone (tests/cpp/test_packed_validate.cpp).
//
// One contiguous buffer, little-endian:
//   [0, 4096)   header: magic "PMDFCPAK", u32 version (1), then the fields of
//               the version-1 header (image.h) at the same offsets; every
//               other byte zero
//   [4096, S)   nseg local-depth bytes in canonical order, zero-padded to a
//               multiple of 4096 (identical to image.h)
//   [S, O)      nseg x 32 u32 occupancy words in canonical order: bit s & 31
//               of word s >> 5 is set iff slot s holds an entry (the engine's
//               own occ layout); zero-padded to a multiple of 4096
//   [O, total)  live x {u64 key, u64 value}: the stored pairs in canonical
//               segment order, within a segment in slot order; zero-padded to
//               a multiple of 4096
// total_bytes(nseg, live) follows from the header alone.  The packed image
// holds exactly what the version-1 image holds: pack / unpack in either
// direction is byte-exact.  Segment i's offset into the pairs is the prefix sum
// of the popcounts of the segments before it; an image is accepted only when
// the popcounts sum to the header's live count, so no offset a restore derives
// can leave the pair region.
#pragma once
#include "image.h"

namespace pmdfc {
namespace packed {

using image::Header;
using image::kAlign;
using image::kHeaderBytes;

constexpr uint32_t kVersion = 1;
constexpr uint64_t kOccWords = 32;  // per segment
constexpr char kMagic[8] = {'P', 'M', 'D', 'F', 'C', 'P', 'A', 'K'};

enum Error {  // (the first ten are image::Error's, so validate_depths' answer passes through)
  kOk = 0,
  kShort,       // fewer bytes than a header
  kMagic_,      // wrong magic
  kVersion_,    // unknown format version
  kGeometry,    // initial_depth / shard_bits / shard_id out of range
  kSize,        // byte counts inconsistent with nseg and live
  kPadding,     // a byte that must be zero is not
  kDepthRange,  // a local depth outside [initial_depth, 30]
  kTiling,      // the local depths do not tile the shard's hash space exactly
  kSummary,     // min / max / depth of the header disagree with the depth bytes
  kLive,        // the occupancy words do not count the header's live entries
};

inline const char* error_string(int e) {
  switch (e) {
    case kOk: return "ok";
    case kShort: return "packed image shorter than its header";
    case kMagic_: return "packed image magic mismatch";
    case kVersion_: return "unknown packed image format version";
    case kGeometry: return "packed image geometry out of range";
    case kSize: return "packed image byte count inconsistent with its segment and entry counts";
    case kPadding: return "packed image padding not zero";
    case kDepthRange: return "packed image local depth out of range";
    case kTiling: return "packed image local depths do not tile the hash space";
    case kSummary: return "packed image header disagrees with its local depths";
    case kLive: return "packed image occupancy words do not count its live entries";
  }
  return "packed image error";
}

inline uint64_t align_up(uint64_t n) { return (n + kAlign - 1) / kAlign * kAlign; }
inline uint64_t occ_offset(uint64_t nseg) { return kHeaderBytes + image::depth_bytes(nseg); }
inline uint64_t occ_bytes(uint64_t nseg) { return align_up(nseg * kOccWords * 4); }
inline uint64_t pairs_offset(uint64_t nseg) { return occ_offset(nseg) + occ_bytes(nseg); }
inline uint64_t pair_bytes(uint64_t live) { return align_up(live * 16); }
inline uint64_t total_bytes(uint64_t nseg, uint64_t live) { return pairs_offset(nseg) + pair_bytes(live); }

// out: kHeaderBytes bytes
inline void encode_header(const Header& h, uint8_t* out) {
  image::encode_header(h, out);
  memcpy(out, kMagic, 8);
}

// The header alone: magic, version, geometry (the rules of image.h's
// parse_header), and the byte counts against nseg, live and `bytes`, the size
// of the buffer the caller holds.
inline int parse_header(const uint8_t* buf, uint64_t bytes, Header* h) {
  if (bytes < kHeaderBytes) return kShort;
  if (memcmp(buf, kMagic, 8) != 0) return kMagic_;
  h->version = image::get32(buf + 8);
  if (h->version != kVersion) return kVersion_;
  h->initial_depth = image::get32(buf + 12);
  h->shard_bits = image::get32(buf + 16);
  h->shard_id = image::get32(buf + 20);
  h->depth = image::get32(buf + 24);
  h->min_ld = image::get32(buf + 28);
  h->max_ld = image::get32(buf + 32);
  h->nseg = image::get64(buf + 40);
  h->live = image::get64(buf + 48);
  h->total_bytes = image::get64(buf + 56);
  if (h->initial_depth < 1 || h->initial_depth > image::kMaxLocalDepth || h->shard_bits > h->initial_depth ||
      h->shard_bits > 16 || (h->shard_bits ? h->shard_id >= (1u << h->shard_bits) : h->shard_id != 0))
    return kGeometry;
  if (h->nseg == 0 || h->nseg > image::kMaxSegs) return kSize;
  if (h->live > h->nseg * 1024) return kSize;
  if (h->total_bytes != total_bytes(h->nseg, h->live) || bytes != h->total_bytes) return kSize;
  if (image::get32(buf + 36) != 0) return kPadding;
  for (uint64_t i = 64; i < kHeaderBytes; ++i)
    if (buf[i]) return kPadding;
  return kOk;
}

// The occupancy region (occ_bytes(h.nseg) bytes) against an accepted header:
// its popcount is the header's live count, its padding is zero.
inline int validate_occupancy(const Header& h, const uint8_t* occ) {
  const uint64_t n = h.nseg * kOccWords * 4;
  uint64_t live = 0;
  for (uint64_t i = 0; i < n; ++i) live += (uint64_t)__builtin_popcount(occ[i]);
  if (live != h.live) return kLive;
  for (uint64_t i = n; i < occ_bytes(h.nseg); ++i)
    if (occ[i]) return kPadding;
  return kOk;
}

// The zero padding after the live pairs (`tail`: the pair region from byte
// live * 16 on, pair_bytes(live) - live * 16 bytes).
inline int validate_pair_padding(const Header& h, const uint8_t* tail) {
  for (uint64_t i = 0; i < pair_bytes(h.live) - h.live * 16; ++i)
    if (tail[i]) return kPadding;
  return kOk;
}

// A whole packed image in host memory (the pairs themselves are not looked
// at).  Never reads past `bytes`.
inline int validate(const uint8_t* buf, uint64_t bytes, Header* h) {
  if (int e = packed::parse_header(buf, bytes, h)) return e;
  if (int e = image::validate_depths(*h, buf + kHeaderBytes)) return e;
  if (int e = validate_occupancy(*h, buf + occ_offset(h->nseg))) return e;
  return validate_pair_padding(*h, buf + pairs_offset(h->nseg) + h->live * 16);
}

}  // namespace packed
}  // namespace pmdfc
