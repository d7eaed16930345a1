// What the host-side planner of the cooperative solver (coop_plan.hpp) and its kernel (kernels_solve.hip, k_solve_coop) share: the
// item kinds, the sizes, the coefficient-word flags.  Plain constants: no HIP, no containers.
#pragma once
#include <stdint.h>

namespace spp {

// coefficient word of a matrix term on the device: bit31: coefficient is +1, bit30: coefficient is -1, low bits: table index
static constexpr uint32_t COEFF_ONE = 0x80000000u;
static constexpr uint32_t COEFF_MINUS_ONE = 0x40000000u;
static constexpr uint32_t COEFF_MASK = 0x3fffffffu;

// items = (kind, a, b) triples
enum : uint32_t {
  COOP_SEQ = 0, COOP_PAR = 1, COOP_LEVELS = 2, COOP_POSEIDON = 3, COOP_POSEIDON2 = 4, COOP_GRUMPKIN = 5, COOP_LEVEL_STREAM = 6,
  COOP_COUNTN = 7, COOP_KINDS = 8
};
static constexpr uint32_t COOP_CHUNK = 1024;
// independent item ranges of one stretch: track t (blockIdx.y) runs items [begin[t], end[t]); only track 0 may use `scratch`
static constexpr uint32_t COOP_TRACKS = 4;
struct CoopTracks { uint32_t n; uint32_t begin[COOP_TRACKS], end[COOP_TRACKS]; };

// A row of a level is a plain OP_SOLVE_C row or a generic one (OP_SOLVE_ROW: side, index of 1/cf, index of the constant inverse of
// the other factor).  Streamed form: word 2 of the row record carries COOP_ROW_GENERIC | side << 29 beside the B term count and two
// more header words follow (inv, odiv).  Table form: three words per row in DevCoop::lvl_gen, side = COOP_NONE for a plain row.
static constexpr uint32_t COOP_NONE = 0xffffffffu;
static constexpr uint32_t COOP_ROW_GENERIC = 0x80000000u;
static constexpr uint32_t COOP_ROW_SIDE_SHIFT = 29;
static constexpr uint32_t COOP_ROW_COUNT_MASK = 0x1fffffffu;

}  // namespace spp
