// Host build of csrc/withdrawal_plan.hpp (g++, no GPU): the per-lane and per-tile pieces of the kernels in kernels_withdrawals.hip
// driven as sequential loops with the launch structure of the device -- claim, winners + tile counts, scan, scatter, assign --, from
// stdin by tests/test_withdrawal_plan_host.py, which compares the plan with its own model (a set and a dict).
//   plan <salt> <order> <pool_capacity> <n_resident> <count>   then n_resident resident keys and count keys (hex, one per line)
//        -> "n_audits <n>", then the count values of audit_of, then the n values of audit_note (space separated)
//   pool_capacity 0: no pool.  order 0: lanes in index order; otherwise the claim loop and the winners loop each visit the lanes in
//   a shuffled order of their own derived from it: the plan must not depend on it, nor on the salt.
//   constants -> "<tile> <wave> <max> <resident>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "withdrawal_plan.hpp"

using namespace spp;

static bool unhex(const char* s, uint8_t* out, size_t n) {
  if (strlen(s) != 2 * n) return false;
  for (size_t i = 0; i < n; i++) {
    unsigned v;
    if (sscanf(s + 2 * i, "%2x", &v) != 1) return false;
    out[i] = (uint8_t)v;
  }
  return true;
}
static bool read_key(uint8_t* out) {
  char buf[128];
  return scanf("%100s", buf) == 1 && unhex(buf, out, 32);
}
static std::vector<uint32_t> lane_order(uint32_t count, uint64_t seed) {
  std::vector<uint32_t> o(count);
  std::iota(o.begin(), o.end(), 0u);
  if (seed)
    for (uint32_t i = count; i > 1; i--) {
      seed = pool_mix64(seed + 0x9E3779B97F4A7C15ull);
      std::swap(o[i - 1], o[seed % i]);
    }
  return o;
}
// what __ballot gives wave `wave` of tile `tile`: bit l = the flag of lane l; lanes past count take part with flag 0
static uint64_t ballot_of(const std::vector<uint32_t>& rep, uint32_t count, uint32_t tile, uint32_t wave) {
  uint64_t b = 0;
  for (uint32_t l = 0; l < WPLAN_WAVE; l++) {
    const uint32_t i = tile * WPLAN_TILE + wave * WPLAN_WAVE + l;
    if (i < count && wplan_is_representative(rep[i], i)) b |= (uint64_t)1 << l;
  }
  return b;
}
// the inclusive scan a wave runs with __shfl_up: every step reads the values of the step before
static void wave_scan(uint32_t v[WPLAN_WAVE]) {
  for (uint32_t d = 1; d < WPLAN_WAVE; d <<= 1) {
    uint32_t before[WPLAN_WAVE];
    memcpy(before, v, sizeof before);
    for (uint32_t l = 0; l < WPLAN_WAVE; l++) v[l] = wplan_scan_step(before[l], before[l >= d ? l - d : l], l, d);
  }
}

int main() {
  char cmd[32];
  while (scanf("%31s", cmd) == 1) {
    if (!strcmp(cmd, "constants")) {
      printf("%u %u %u %u\n", WPLAN_TILE, WPLAN_WAVE, WPLAN_MAX, WPLAN_RESIDENT);
    } else if (!strcmp(cmd, "plan")) {
      unsigned long long salt, order, cap;
      unsigned n_res, count;
      if (scanf("%llx %llu %llu %u %u", &salt, &order, &cap, &n_res, &count) != 5) return 2;
      if (count == 0 || count > WPLAN_MAX || (cap == 0 && n_res) || n_res > cap) return 2;
      // the pool's audit-record set
      const uint32_t set_slots = pool_slots_for(cap ? cap : 1);
      std::vector<uint32_t> claim(set_slots, 0);
      std::vector<uint8_t> set_keys((size_t)set_slots * 32, 0);
      PoolSet set{claim.data(), set_keys.data(), set_slots - 1};
      uint8_t key[32];
      for (unsigned i = 0; i < n_res; i++) {
        if (!read_key(key)) return 2;
        if (!pool_set_contains(set, salt, key)) pool_set_insert_unique(set, salt, key);
      }
      const size_t stride = 40;   // keys sit inside a wider record, as the wa_commitment does in a withdraw row
      std::vector<uint8_t> buf(stride * count + 8, 0xEE);
      for (unsigned i = 0; i < count; i++)
        if (!read_key(buf.data() + 8 + stride * i)) return 2;
      const uint8_t* keys = buf.data() + 8;

      const uint32_t rs = pool_slots_for(count), tiles = wplan_tiles(count);
      std::vector<uint32_t> slots(rs, POOL_NONE), rep(count, 0xDEADBEEF), pos(count, 0xDEADBEEF), audit_of(count, 0xDEADBEEF),
          audit_note(count, 0xDEADBEEF), tile_counts(WPLAN_MAX_TILES, 0xDEADBEEF), tile_base(WPLAN_MAX_TILES, 0xDEADBEEF);
      std::vector<uint8_t> resident(count, 0xEE);
      uint32_t n_audits = 0xDEADBEEF;
      // launch 1: claim
      for (uint32_t i : lane_order(count, order)) wplan_screen_claim(cap ? &set : nullptr, salt, slots.data(), rs - 1, keys, stride, i, resident.data());
      // launch 2: winners, and the counts of every tile
      for (uint32_t i : lane_order(count, order ? order + 1 : 0)) rep[i] = wplan_rep(slots.data(), rs - 1, salt, keys, stride, i, resident.data());
      for (uint32_t t = 0; t < tiles; t++) {
        uint32_t wave_counts[WPLAN_TILE_WAVES];
        for (uint32_t w = 0; w < WPLAN_TILE_WAVES; w++) wave_counts[w] = wplan_popcount(ballot_of(rep, count, t, w));
        tile_counts[t] = wplan_tile_count(wave_counts);
      }
      // launch 3: one workgroup of WPLAN_MAX_TILES lanes, two levels
      {
        uint32_t incl[WPLAN_MAX_TILES], wave_total[WPLAN_WAVE] = {0};
        for (uint32_t t = 0; t < WPLAN_MAX_TILES; t++) incl[t] = t < tiles ? tile_counts[t] : 0;
        for (uint32_t w = 0; w < WPLAN_TILE_WAVES; w++) {
          wave_scan(incl + w * WPLAN_WAVE);
          wave_total[w] = incl[w * WPLAN_WAVE + WPLAN_WAVE - 1];
        }
        uint32_t second[WPLAN_WAVE];
        memcpy(second, wave_total, sizeof second);
        wave_scan(second);
        for (uint32_t w = 0; w < WPLAN_TILE_WAVES; w++) wave_total[w] = second[w] - wave_total[w];
        for (uint32_t t = 0; t < WPLAN_MAX_TILES; t++) {
          const uint32_t total_incl = wave_total[t / WPLAN_WAVE] + incl[t];
          if (t < tiles) tile_base[t] = total_incl - tile_counts[t];
          if (t == WPLAN_MAX_TILES - 1) n_audits = total_incl;
        }
      }
      // launch 4: scatter
      for (uint32_t t = 0; t < tiles; t++) {
        uint32_t wave_counts[WPLAN_TILE_WAVES];
        uint64_t ballots[WPLAN_TILE_WAVES];
        for (uint32_t w = 0; w < WPLAN_TILE_WAVES; w++) wave_counts[w] = wplan_popcount(ballots[w] = ballot_of(rep, count, t, w));
        for (uint32_t l = 0; l < WPLAN_TILE; l++) {
          const uint32_t i = t * WPLAN_TILE + l, w = l / WPLAN_WAVE;
          if (!((ballots[w] >> (l % WPLAN_WAVE)) & 1)) continue;
          const uint32_t p = tile_base[t] + wplan_wave_base(wave_counts, w) + wplan_rank_in_wave(ballots[w], l % WPLAN_WAVE);
          if (p >= count) return 3;
          audit_note[p] = i;
          pos[i] = p;
        }
      }
      // launch 5: assign
      for (uint32_t i = 0; i < count; i++) audit_of[i] = wplan_audit_of(rep.data(), pos.data(), i);
      if (n_audits > count) return 3;
      printf("n_audits %u\n", n_audits);
      for (uint32_t i = 0; i < count; i++) printf("%u%c", audit_of[i], i + 1 == count ? '\n' : ' ');
      for (uint32_t s = 0; s < n_audits; s++) printf("%u%c", audit_note[s], s + 1 == n_audits ? '\n' : ' ');
      if (n_audits == 0) printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
