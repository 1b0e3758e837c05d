// knobs.h -- every PMDFC_* environment knob of libpmdfc_cceh.so (host only).
//
// Two structs, by when the environment is read (tests rely on which is which):
//   ProcessKnobs  parsed once per process, on the first use of any of them --
//                 a test that changes one starts a child process;
//   CreateKnobs   parsed at each pmdfc_cceh_create and kept in the table --
//                 engines created after a change of the environment see it.
// None is needed in production: each default is the measured best (DESIGN.md
// "Knobs" has the table and where each result is recorded).  getenv appears
// in this file and nowhere else under csrc/.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "cceh_device.h"
#include "cceh_kernels.h"

namespace pmdfc {

namespace knob {
// off only by a value that starts with '0'
inline bool on_unless_0(const char* name) {
  const char* e = getenv(name);
  return !(e && e[0] == '0');
}
// atoi(value) if that is positive, else the default
inline uint64_t positive_or(const char* name, uint64_t dflt) {
  const char* e = getenv(name);
  return e && atoi(e) > 0 ? (uint64_t)atoi(e) : dflt;
}
// strtoull(value, base 0) capped at `cap`; unset: the cap
inline uint64_t capped(const char* name, uint64_t cap) {
  const char* e = getenv(name);
  return e ? std::min<uint64_t>(strtoull(e, nullptr, 0), cap) : cap;
}
}  // namespace knob

struct ProcessKnobs {
  // PMDFC_FAST_LDS_PAD=bytes (A/B): dynamic LDS added to each k_apply_fast wave (lowers its occupancy)
  uint32_t fast_lds_pad;
  // PMDFC_FAST_APPLY=0 (A/B): the general first pass for every bucket instead of the lean one
  bool fast_apply;
  // PMDFC_SPLIT_TEAM_MAX=n (A/B, tests): split lists up to n long go by teams of four waves (default kSplitGroups)
  uint32_t split_team_max;
  // PMDFC_CP=0 (A/B): the fine partition for every batch (no k_apply_fast_cp)
  bool cp;
  // PMDFC_RAMP_OPS=n / PMDFC_RAMP_MIN=n (tuning): ops per directory bucket in a sub-batch while the
  // table is coarser than p1max (default 1024), and the smallest sub-batch (default 4096); > 0
  uint64_t ramp_ops, ramp_min;
  // PMDFC_GET_UNROLL=1|2|4 (A/B): Gets per thread issued together in k_get_u (else 2)
  int get_unroll;
  // PMDFC_GET_P2=0 (A/B): no speculative second-line load for even home lines
  uint32_t get_p2;
  // PMDFC_GET_GRID=blocks (A/B): grid cap of a launch over several batches' Gets (0: none)
  uint64_t get_grid;
  // PMDFC_MG_U=1|4 (A/B): Gets per quad issued together in k_mixed_get / k_mixed_get_iset (else 2)
  int mg_u;
  // PMDFC_SMALL_MAX=n (A/B, tests): batches up to n ops take k_mixed_small (<= kChunkWave, the default; 0: never)
  uint64_t small_max;
  // PMDFC_MEDIUM_MAX=n (A/B, tests): batches up to n ops take k_part + k_medium (<= kPartTile, the default; 0: never)
  uint64_t medium_max;
  // PMDFC_PIPE_GROUP=g (A/B, tests): insert batches partitioned ahead per event pair, in [1, kRecBufs / 2] (default 8)
  uint32_t pipe_group;
  // PMDFC_MIXED_SMALL=0 (A/B): the mixed passes of gated batches always on full grids
  bool mixed_small;
  // PMDFC_MIXED_JOIN=0|1 (A/B, tests): force the insert set / the join for mixed batches (-1, unset: by the last batch)
  int mixed_join;
  // PMDFC_ROUTE_DIRECT=0 (A/B, tests): the pack / exchange / unpack path even on one rank
  bool route_direct;
  // PMDFC_ROUTE_PIPE=1 (A/B): routed inserts through the engine's partition pipeline (measured slower on one rank)
  bool route_pipe;
};

inline const ProcessKnobs& process_knobs() {
  static const ProcessKnobs k = [] {
    ProcessKnobs k{};
    const char* e;
    k.fast_lds_pad = (e = getenv("PMDFC_FAST_LDS_PAD")) ? (uint32_t)atoi(e) : 0u;
    k.fast_apply = knob::on_unless_0("PMDFC_FAST_APPLY");
    k.split_team_max = (e = getenv("PMDFC_SPLIT_TEAM_MAX")) ? (uint32_t)strtoul(e, nullptr, 0) : kSplitGroups;
    k.cp = knob::on_unless_0("PMDFC_CP");
    k.ramp_ops = knob::positive_or("PMDFC_RAMP_OPS", 1024);
    k.ramp_min = knob::positive_or("PMDFC_RAMP_MIN", 4096);
    k.get_unroll = (e = getenv("PMDFC_GET_UNROLL")) ? atoi(e) : 2;
    if (k.get_unroll != 1 && k.get_unroll != 2 && k.get_unroll != 4) k.get_unroll = 2;
    k.get_p2 = knob::on_unless_0("PMDFC_GET_P2") ? 1u : 0u;
    k.get_grid = (e = getenv("PMDFC_GET_GRID")) ? strtoull(e, nullptr, 0) : 0ull;
    k.mg_u = (e = getenv("PMDFC_MG_U")) ? atoi(e) : 2;
    if (k.mg_u != 1 && k.mg_u != 4) k.mg_u = 2;
    k.small_max = knob::capped("PMDFC_SMALL_MAX", kChunkWave);
    k.medium_max = knob::capped("PMDFC_MEDIUM_MAX", kPartTile);
    k.pipe_group = (uint32_t)std::min<int>(std::max<int>((e = getenv("PMDFC_PIPE_GROUP")) ? atoi(e) : 8, 1),
                                           (int)kRecBufs / 2);
    k.mixed_small = knob::on_unless_0("PMDFC_MIXED_SMALL");
    k.mixed_join = (e = getenv("PMDFC_MIXED_JOIN")) ? atoi(e) : -1;
    k.route_direct = knob::on_unless_0("PMDFC_ROUTE_DIRECT");
    k.route_pipe = (e = getenv("PMDFC_ROUTE_PIPE")) && atoi(e) != 0;
    return k;
  }();
  return k;
}

struct CreateKnobs {
  // PMDFC_P1MAX=bits (A/B, tests): the directory bucket bits of the full-resolution table, capped at
  // kMaxP1 (-1, unset: from max_batch, about 128 ops per bucket)
  int p1max = -1;
  // PMDFC_CHUNK=n (A/B, tests): ops per wave chunk of the bucket passes (0 or past kChunkWave: kChunkWave)
  uint32_t chunk = 0;
  // PMDFC_FLAT_MAX=bits (A/B, tests): deeper directories skip the flat copy of pure-Get batches (<= kFlatMaxBits)
  uint32_t flat_max = kFlatMaxBits;
  // PMDFC_STAMPS=1 (debug): wall-clock phase stamps of the partition, bucket and split waves
  // (pmdfc_cceh_read_stamps); PMDFC_STAMP_ROT=R with it: R stamp sets, batch i writing set i % R
  bool stamps = false;
  uint32_t stamp_rot = 1;
  // PMDFC_PSTREAM_PRIO=0 (A/B): the partition stream at default instead of high priority
  bool pstream_prio = true;

  static CreateKnobs read() {
    CreateKnobs k;
    const char* e;
    if ((e = getenv("PMDFC_P1MAX"))) k.p1max = (int)std::min<uint32_t>((uint32_t)atoi(e), kMaxP1);
    if ((e = getenv("PMDFC_CHUNK"))) k.chunk = (uint32_t)atoi(e);
    if ((e = getenv("PMDFC_FLAT_MAX"))) k.flat_max = std::min<uint32_t>((uint32_t)atoi(e), kFlatMaxBits);
    k.stamps = (e = getenv("PMDFC_STAMPS")) && e[0] == '1';
    if (k.stamps && (e = getenv("PMDFC_STAMP_ROT")) && atoi(e) > 1) k.stamp_rot = (uint32_t)atoi(e);
    k.pstream_prio = knob::on_unless_0("PMDFC_PSTREAM_PRIO");
    return k;
  }
};

}  // namespace pmdfc
