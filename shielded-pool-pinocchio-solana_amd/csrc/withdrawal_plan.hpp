// The withdrawal plan, host + gfx950: which notes of a batch still need an audit record.  The per-lane and per-tile pieces of the
// kernels in kernels_withdrawals.hip and of the host check tests/host/withdrawal_plan_check.cpp, on top of pool_table.hpp.
//
// A withdrawal is two transactions, submit_audit and then withdraw (demo-frontend/app/api/relay/withdraw/route.ts:129-287), but the
// audit record is keyed by wa_commitment = H(owner_x, owner_y): by the identity, not by the note, and process_submit_audit answers Ok
// before it looks at the proof when the record exists (shielded_pool_program/src/instructions/submit_audit.rs:65-73).  So a batch of
// notes needs one audit proof per identity the pool does not know yet.  For `count` 32-byte keys, compared bytewise as the pool
// compares them (v and v + r are two keys), and an optional pool:
//   resident(i)   a pool is given and pool_set_contains finds key i in its audit-record set
//   rep(i)        for a key that is not resident: the lowest j with key[j] == key[i]
//   audit_note    the ascending list of all i with rep(i) == i ("representatives"), n_audits long
//   audit_of[i]   the position of rep(i) in audit_note, or WPLAN_RESIDENT for a resident key
//
// Launches on one stream, their number fixed whatever the keys are (the resolve table is set to POOL_NONE in front of them):
//   claim     one lane per key: probe the resident set; a key that is not resident claims its slot with pool_resolve_claim
//   winners   one lane per key: rep(i) read back with pool_resolve_winner; the flags rep(i) == i counted per tile
//   scan      ONE workgroup: exclusive scan of the tile counts (at most WPLAN_MAX_TILES = one count per lane), n_audits
//   scatter   one lane per key: a representative's position = tile base + rank inside the tile; audit_note and pos[] written
//   assign    one lane per key: audit_of[i] = pos[rep(i)]
// Ordering.  The resident set is only read.  The resolve table is written by claim and read by winners, rep[] is written by winners
// and read by scatter and assign, the tile counts by winners and scan, the tile bases by scan and scatter, pos[] by scatter and
// assign: every dependence crosses a kernel boundary, which is the fence, as in the ledger.  No workgroup waits for another one: the
// compaction is counts, one scanning workgroup, scatter -- three launches -- and not a single-pass scan that spins on its neighbours'
// flags.  Inside claim, a slot only moves from POOL_NONE to an index and then to lower indices of the same key (pool_table.hpp), so
// after the launch it holds the minimum whatever order the lanes came in; a resident key claims nothing and a key that is not
// resident always finds at least its own claim.  The salt moves keys between slots and changes nothing a lane reads back: winners
// returns an index by comparing key bytes, never a slot number.  The compaction is stable -- rank = number of flags at lower
// indices, computed from ballots and sums, no atomics -- so audit_note ascends and nothing depends on scheduling.
//
// Wave64: a tile is WPLAN_TILE = 1024 keys = 16 waves of 64 lanes; __ballot gives the 64 flags of a wave, the rank of a lane inside
// its wave is the population count of the flags below it (wplan_rank_in_wave), the rank of a wave inside its tile the sum of the
// counts of the waves before it (wplan_wave_base), both plain functions shared with the host check, which builds the ballots with a
// loop.  count <= WPLAN_MAX = 2^20 gives at most 1024 tiles: two scan levels always suffice.
#pragma once
#include "pool_table.hpp"

namespace spp {

static constexpr uint32_t WPLAN_RESIDENT = 0xFFFFFFFFu;           // include/spp.h, SPP_AUDIT_RESIDENT; also POOL_NONE: a resident key has no winner
static constexpr uint32_t WPLAN_WAVE = 64, WPLAN_TILE = 1024, WPLAN_TILE_WAVES = WPLAN_TILE / WPLAN_WAVE;
static constexpr uint32_t WPLAN_MAX = 1u << 20, WPLAN_MAX_TILES = WPLAN_MAX / WPLAN_TILE;
static_assert(WPLAN_RESIDENT == POOL_NONE && WPLAN_MAX_TILES == WPLAN_TILE, "one lane per tile count in the scanning workgroup");

SPP_HD uint32_t wplan_tiles(uint32_t count) { return (count + WPLAN_TILE - 1) / WPLAN_TILE; }

// ---- per lane ----
// claim: resident[i] says whether the pool holds the key (audits == nullptr: no pool); every other key claims
SPP_HD void wplan_screen_claim(const PoolSet* audits, uint64_t salt, uint32_t* slots, uint32_t mask, const uint8_t* keys, size_t stride,
                               uint32_t i, uint8_t* resident) {
  const bool r = audits && pool_set_contains(*audits, salt, keys + (size_t)i * stride);
  resident[i] = r ? 1 : 0;
  if (!r) pool_resolve_claim(slots, mask, salt, keys, stride, i);
}
// winners, after every claim: rep(i), WPLAN_RESIDENT for a resident key
SPP_HD uint32_t wplan_rep(const uint32_t* slots, uint32_t mask, uint64_t salt, const uint8_t* keys, size_t stride, uint32_t i,
                          const uint8_t* resident) {
  return resident[i] ? WPLAN_RESIDENT : pool_resolve_winner(slots, mask, salt, keys, stride, i);
}
SPP_HD bool wplan_is_representative(uint32_t rep, uint32_t i) { return rep == i; }
// assign, after scatter
SPP_HD uint32_t wplan_audit_of(const uint32_t* rep, const uint32_t* pos, uint32_t i) {
  const uint32_t r = rep[i];
  return r == WPLAN_RESIDENT ? WPLAN_RESIDENT : pos[r];
}

// ---- per wave and per tile ----
SPP_HD uint32_t wplan_popcount(uint64_t ballot) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popcll(ballot);
#else
  return (uint32_t)__builtin_popcountll(ballot);
#endif
}
// flags of the lanes below `lane` in its wave
SPP_HD uint32_t wplan_rank_in_wave(uint64_t ballot, uint32_t lane) { return wplan_popcount(ballot & (((uint64_t)1 << lane) - 1)); }
// counts[w]: flags of wave w of a tile; the flags of the waves before `wave`, and of the whole tile
SPP_HD uint32_t wplan_wave_base(const uint32_t* counts, uint32_t wave) {
  uint32_t s = 0;
  for (uint32_t w = 0; w < wave; w++) s += counts[w];
  return s;
}
SPP_HD uint32_t wplan_tile_count(const uint32_t* counts) { return wplan_wave_base(counts, WPLAN_TILE_WAVES); }
// One step of the Hillis-Steele scan a wave runs over the tile counts (and wave 0 over the wave totals): lane l adds the value of
// lane l - d, d = 1, 2, .. 32.  `from_below` is what __shfl_up(v, d) delivered; lanes below d keep their value.
SPP_HD uint32_t wplan_scan_step(uint32_t v, uint32_t from_below, uint32_t lane, uint32_t d) { return lane >= d ? v + from_below : v; }

}  // namespace spp
