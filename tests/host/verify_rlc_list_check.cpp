// Test-only host build of the index arithmetic of the random-linear-combination verifier over a compacted list
// (csrc/verify_rlc_list.hpp): what k_verify_rlc_terms_list / k_verify_rlc_group_list and launch_verify_rlc_list do with positions,
// instruction indices, verdicts and the fallback list, run lane after lane and block after block.  No curve arithmetic: a proof is
// "dropped", "valid" or "invalid" by a fixed function of its INSTRUCTION index, and a group is accepted iff all its live members
// are valid -- what the combined equation decides except with negligible probability.
//   verify_rlc_list_check
//       the list lengths 0, 1, 63, 64, 65, 129 with group 64, the list a permutation with gaps of a batch of 200 instructions,
//       each as ONE slice and in slices of two groups.  Per case a line
//           CASE <length> <slice length> OK=<one digit per instruction> FALLBACK=<sorted indices, comma separated> STATS=<g>,<r>,<v>,<d>
//       then "OK <checks>", or "FAIL ..." at the first check that does not hold.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "verify_rlc_list.hpp"
using namespace spp;

static int checks = 0;
#define CHECK(c, msg) do { checks++; if (!(c)) { printf("FAIL %s (line %d)\n", msg, __LINE__); return false; } } while (0)

static const uint32_t BATCH = 200, GROUP = 64;
// by instruction index, never by position
static bool dropped(uint32_t i) { return i % 11 == 3; }
static bool valid(uint32_t i) { return i % 37 != 5; }

// a permutation with gaps: `len` distinct instruction indices below BATCH, in an order that is neither ascending nor descending
static std::vector<uint32_t> make_list(uint32_t len) {
  std::vector<uint32_t> all;
  for (uint32_t k = 0; k < BATCH; k++) all.push_back((k * 73 + 19) % BATCH);   // 73 is coprime to 200: a permutation
  std::vector<uint32_t> out;
  for (uint32_t k = 0; k < BATCH && out.size() < len; k++)
    if (k % 4 != 1 || BATCH - k <= len - out.size()) out.push_back(all[k]);    // gaps: every fourth index stays out while it can
  return out;
}

struct Result {
  std::vector<int32_t> ok;
  std::vector<uint32_t> fallback;          // all slices, sorted
  uint32_t stats[4] = {0, 0, 0, 0};
  uint32_t launches = 0;
};

// launch_verify_rlc_list with its three kernels emulated; max_count = BATCH, the length of the list "only on the device"
static bool run(const std::vector<uint32_t>& list, uint32_t slice_max, Result& R) {
  const uint32_t n_list = (uint32_t)list.size(), max_count = BATCH;
  const uint32_t slice_len = rlc_slice_len(GROUP, slice_max);
  CHECK(slice_len % GROUP == 0 && slice_len > 0 && slice_len <= slice_max, "slice length is a multiple of the group");
  const uint32_t stride = max_count < slice_len ? max_count : slice_len;
  R.ok.assign(BATCH, 0);
  std::vector<uint32_t> term_of(stride), live(stride), fb(stride);
  std::vector<uint32_t> visits(n_list, 0), grouped(n_list, 0);
  uint32_t blocks_with_work = 0;
  for (uint32_t s = 0; s < rlc_list_slices(slice_len, max_count); s++) {
    const RlcListSlice sl = rlc_list_slice(s, slice_len, max_count);
    CHECK(sl.n > 0 && sl.n <= stride && sl.pos0 == s * slice_len && sl.pos0 + sl.n <= max_count, "slice bounds");
    uint32_t n_fb = 0;
    // terms: a grid of whole waves over the slice
    std::fill(live.begin(), live.end(), 0xDEADu);                         // stale words of the slice before
    for (uint32_t p = 0; p < (sl.n + 63) / 64 * 64; p++) {
      if (!rlc_list_lane_active(sl, p, n_list)) continue;
      CHECK(p < stride && sl.pos0 + p < n_list, "an active lane is inside the workspace and the list");
      const uint32_t i = list[sl.pos0 + p];
      visits[sl.pos0 + p]++;
      term_of[p] = i;                                                     // the index the scalars are derived from
      live[p] = dropped(i) ? 0 : 1;
      if (dropped(i)) R.stats[3]++;
    }
    // groups: the grid for the worst case
    for (uint32_t b = 0; b < rlc_list_blocks(sl.n, GROUP); b++) {
      const RlcListSpan sp = rlc_list_span(sl, b, GROUP, n_list);
      if (sp.n == 0) {
        CHECK((uint64_t)sl.pos0 + (uint64_t)b * GROUP >= n_list, "a block without work lies past the end of the list");
        continue;
      }
      blocks_with_work++;
      R.stats[0]++;
      CHECK(sp.first == sl.pos0 + b * GROUP && sp.n <= GROUP && sp.first + sp.n <= n_list && sp.first + sp.n <= sl.pos0 + sl.n, "span bounds");
      CHECK(sp.n == GROUP || sp.first + sp.n == n_list, "only the last group of the list is short");
      const uint32_t w0 = sp.first - sl.pos0;
      const uint32_t* idx = list.data() + sp.first;
      uint32_t n_live = 0;
      bool accept = true;
      for (uint32_t k = 0; k < sp.n; k++) {
        grouped[sp.first + k]++;
        CHECK(term_of[w0 + k] == idx[k] && live[w0 + k] <= 1, "workspace position = list position - pos0, written by this slice");
        if (live[w0 + k]) { n_live++; accept = accept && valid(idx[k]); }
      }
      if (n_live == 0) continue;
      if (accept) {
        for (uint32_t lane = 0; lane < 64; lane++) rlc_list_accept(idx, live.data() + w0, sp.n, lane, 64, R.ok.data());
        continue;
      }
      R.stats[1]++;
      R.stats[2] += n_live;
      const uint32_t at = n_fb;
      n_fb += n_live;
      CHECK(n_fb <= sl.n, "the fallback list fits the slice");
      CHECK(rlc_list_refuse(idx, live.data() + w0, sp.n, fb.data(), at) == n_fb, "a refused group writes exactly its live members");
      std::vector<uint32_t> got(fb.begin() + at, fb.begin() + n_fb), want;
      for (uint32_t k = 0; k < sp.n; k++)
        if (!dropped(idx[k])) want.push_back(idx[k]);
      CHECK(got == want, "the fallback entries are the instruction indices of the live members, in list order");
    }
    // fallback: k_verify_list over the slice's fallback list, max_count = the slice
    for (uint32_t j = 0; j < n_fb; j++) {
      R.ok[fb[j]] = valid(fb[j]) ? 1 : 0;
      R.fallback.push_back(fb[j]);
    }
    R.launches += 3;
  }
  for (uint32_t j = 0; j < n_list; j++) CHECK(visits[j] == 1 && grouped[j] == 1, "every list position has one term and one group: exact and disjoint");
  CHECK(blocks_with_work == (n_list + GROUP - 1) / GROUP, "as many groups as the list needs");
  std::sort(R.fallback.begin(), R.fallback.end());
  return true;
}

static bool one_case(uint32_t len) {
  const std::vector<uint32_t> list = make_list(len);
  CHECK(list.size() == len, "list length");
  std::vector<bool> in_list(BATCH, false);
  for (uint32_t i : list) { CHECK(i < BATCH && !in_list[i], "distinct indices"); in_list[i] = true; }
  if (len > 2) CHECK(!std::is_sorted(list.begin(), list.end()) && len < BATCH, "a permutation with gaps");
  // what the kernels must produce, from the definition: the groups are consecutive runs of 64 list positions
  std::vector<int32_t> want_ok(BATCH, 0);
  std::vector<uint32_t> want_fb;
  uint32_t want_stats[4] = {(len + GROUP - 1) / GROUP, 0, 0, 0};
  for (uint32_t first = 0; first < len; first += GROUP) {
    const uint32_t n = std::min(GROUP, len - first);
    bool accept = true, any = false;
    for (uint32_t k = 0; k < n; k++)
      if (!dropped(list[first + k])) { any = true; accept = accept && valid(list[first + k]); }
    for (uint32_t k = 0; k < n; k++) {
      const uint32_t i = list[first + k];
      if (dropped(i)) { want_stats[3]++; continue; }
      want_ok[i] = valid(i) ? 1 : 0;
      if (!accept) { want_fb.push_back(i); want_stats[2]++; }
    }
    if (any && !accept) want_stats[1]++;
  }
  std::sort(want_fb.begin(), want_fb.end());
  Result one, two;
  if (!run(list, RLC_SLICE_MAX, one) || !run(list, 2 * GROUP, two)) return false;
  CHECK(one.launches == 3, "a batch of at most 2^18: terms, groups, fallback");
  CHECK(two.launches == 3 * ((BATCH + 2 * GROUP - 1) / (2 * GROUP)), "three launches per slice");
  for (const Result* r : {&one, &two}) {
    CHECK(r->ok == want_ok, "a verdict lands at list[j] and nowhere else");
    CHECK(r->fallback == want_fb, "exactly the live members of the refused groups reach the fallback list");
    CHECK(std::equal(r->stats, r->stats + 4, want_stats), "stats");
    std::string o, f;
    for (int32_t v : r->ok) o += v ? '1' : '0';
    for (uint32_t v : r->fallback) f += (f.empty() ? "" : ",") + std::to_string(v);
    printf("CASE %u %u OK=%s FALLBACK=%s STATS=%u,%u,%u,%u\n", len, r == &one ? rlc_slice_len(GROUP) : 2 * GROUP, o.c_str(), f.c_str(), r->stats[0],
           r->stats[1], r->stats[2], r->stats[3]);
  }
  return true;
}

int main() {
  // the slice arithmetic itself, at the sizes the library uses
  if (![] {
        CHECK(rlc_slice_len(64) == (1u << 18) && rlc_slice_len(4096) == (1u << 18) && rlc_slice_len(192) == 262080, "slice lengths");
        CHECK(rlc_list_slices(1u << 18, 1u << 24) == 64 && rlc_list_slices(1u << 18, (1u << 18) + 1) == 2 && rlc_list_slices(1u << 18, 1) == 1, "slice counts");
        const RlcListSlice last = rlc_list_slice(63, 1u << 18, 1u << 24), past = rlc_list_slice(64, 1u << 18, 1u << 24);
        CHECK(last.pos0 == 63u << 18 && last.n == 1u << 18 && past.n == 0, "the last slice of 2^24");
        const RlcListSpan late = rlc_list_span(last, 4095, 64, (1u << 24) - 1);   // the last block of the largest batch, one entry short
        CHECK(late.first == (1u << 24) - 64 && late.n == 63, "the last span of 2^24");
        CHECK(rlc_list_span(RlcListSlice{0, 128}, 2, 64, 1000).n == 0 && rlc_list_span(RlcListSlice{0, 128}, 1, 64, 65).n == 1, "span past the slice / the list");
        return true;
      }())
    return 1;
  for (uint32_t len : {0u, 1u, 63u, 64u, 65u, 129u})
    if (!one_case(len)) return 1;
  printf("OK %d\n", checks);
  return 0;
}
