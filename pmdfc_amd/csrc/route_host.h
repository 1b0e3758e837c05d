// route_host.h -- what the native routed loop (dist_host.hip) needs of the
// block router (route_host.hip): its state, and the pack that can put the
// local owner's block straight into a receive slot.  Host only.
#pragma once
#include <cstdint>

#include "../../include/pmdfc_cceh.h"

struct pmdfc_router {
  pmdfc_router_config cfg;
  uint32_t G = 1;
  uint64_t rows = 0;
  uint32_t parity = 0;      // carry buffer the next pack reads
  uint32_t last_width = 0;  // width of the carried records (fixed while the carry is non-empty)
  uint32_t* tile_cnt = nullptr;
  uint32_t* cnt = nullptr;  // [2][G] carry counts
  uint32_t* ovf = nullptr;  // sticky count of ops dropped on a full carry
  uint64_t* crec = nullptr; // [2][G][carry_cap][kCarryWords]
  uint32_t* cpos = nullptr; // [2][G][carry_cap]
};

namespace pmdfc {

// pmdfc_router_pack with two more arguments (route_host.hip)
int router_pack(pmdfc_router_t* r, const uint64_t* keys, const uint64_t* values, const uint8_t* ops,
                const uint8_t* keep, uint64_t n, uint32_t width, uint32_t base, uint64_t* send, uint32_t* rowpos,
                uint64_t* values_out, uint8_t* status_out, void* stream, uint32_t self_g, uint64_t* self_dst);

}  // namespace pmdfc
