// csrc/msm_ragged.hpp and csrc/msm_classes.hpp on the host: the ragged table layout on seeded random class vectors, the uniform
// layout as its all-wide special case, the range classes of the audit circuit as the product's builder emits it, and the split of
// the HBM budget with and without the classes.
//   g++ -O2 -std=c++17 -I csrc tests/host/msm_ragged_check.cpp csrc/circuit.cpp csrc/circuit_audit.cpp -o msm_ragged_check
//   ./msm_ragged_check layout
//   ./msm_ragged_check audit pk.txt bounds_out.txt      (pk.txt: 2048 integers, a then b)  -> "CLASSES ..." line, bounds file
//   ./msm_ragged_check withdraw bounds_out.txt
//   ./msm_ragged_check plan nA nB1 nK nZ nCB nCS nB2  bitsA limbsA lookA  bitsB limbsB lookB  bitsK  budget   -> "PLAN ..." lines
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "msm_classes.hpp"

using namespace spp;

static int bad = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      if (bad++ < 20) { printf(__VA_ARGS__); printf("\n"); } \
    }                                            \
  } while (0)

static int check_layout() {
  std::mt19937 rng(20240611);
  const uint32_t bounds[6] = {0, 1, 128, 255, 256, 40000};
  size_t cases = 0;
  for (uint32_t c : {6u, 9u, 12u, 15u, 16u})
    for (size_t N : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)1000, (size_t)4133})
      for (int mode = 0; mode < 4; mode++, cases++) {
        // mode 0: all wide; 1: random classes in wire order; 2: the same in class-major order; 3: all narrow
        std::vector<uint32_t> b(N);
        for (auto& x : b) x = mode == 0 ? 0 : mode == 3 ? bounds[1 + rng() % 3] : bounds[rng() % 6];
        if (mode == 2) {
          const std::vector<uint32_t> perm = msm_class_major_order(b.data(), N, c);
          std::vector<char> seen(N, 0);
          std::vector<uint32_t> o(N);
          for (size_t k = 0; k < N; k++) {
            CHECK(perm[k] < N && !seen[perm[k]], "c=%u N=%zu: the order is not a permutation", c, N);
            seen[perm[k]] = 1;
            o[k] = b[perm[k]];
            if (k) {
              const uint32_t e0 = msm_class_entries(b[perm[k - 1]], c), e1 = msm_class_entries(b[perm[k]], c);
              CHECK(e0 > e1 || (e0 == e1 && perm[k - 1] < perm[k]), "c=%u N=%zu: not class-major and stable at %zu", c, N, k);
            }
          }
          b = o;
        }
        const MsmRagged L = msm_ragged_layout(b.data(), N, c);
        const uint32_t full = 1u << (c - 1);
        CHECK(L.blocks.size() == (N + 63) / 64, "c=%u N=%zu: %zu blocks", c, N, L.blocks.size());
        uint64_t sum = 0;
        size_t mixed = 0;
        for (size_t k = 0; k < L.blocks.size(); k++) {
          const MsmBlock& blk = L.blocks[k];
          CHECK(blk.off == sum, "c=%u N=%zu block %zu: starts at %llu, the blocks before it end at %llu", c, N, k, (unsigned long long)blk.off, (unsigned long long)sum);
          if (k) CHECK(blk.off > L.blocks[k - 1].off, "c=%u N=%zu: offsets do not increase at block %zu", c, N, k);
          CHECK(blk.E >= 1 && blk.E <= full && (blk.E & (blk.E - 1)) == 0, "c=%u N=%zu block %zu: E = %u", c, N, k, blk.E);
          uint32_t need = 1;
          bool same = true;
          for (size_t r = k * 64; r < std::min(N, k * 64 + 64); r++) {
            const uint32_t e = msm_class_entries(b[r], c);
            need = std::max(need, e);
            same = same && e == msm_class_entries(b[k * 64], c);
            const uint32_t bound = b[r] == 0 || b[r] > full ? full : b[r];
            CHECK(e >= bound && e <= full, "c=%u bound %u: %u entries", c, b[r], e);
            for (uint32_t d : {0u, bound / 2, bound - 1}) {      // entry d holds the multiple d + 1 <= bound
              const size_t at = L.index(r, d);
              CHECK(at >= blk.off * 64 && at < (blk.off + blk.E) * 64, "c=%u N=%zu row %zu d=%u: index outside its block", c, N, r, d);
              CHECK(at % 64 == r % 64, "c=%u N=%zu row %zu: lane", c, N, r);
            }
          }
          CHECK(blk.E == need, "c=%u N=%zu block %zu: E = %u, its longest row needs %u", c, N, k, blk.E, need);
          mixed += !same;
          sum += blk.E;
        }
        CHECK(L.units == sum && L.elems() == (size_t)sum * 64, "c=%u N=%zu: total", c, N);
        if (mode == 2) CHECK(mixed <= 5, "c=%u N=%zu: %zu mixed blocks in class-major order", c, N, mixed);
        if (mode == 0) {
          CHECK(L.elems() == msm_table_elems((uint32_t)N, c, 1) && !L.narrow(c), "c=%u N=%zu: all wide is not the uniform size", c, N);
          for (size_t r = 0; r < N; r += 7)
            for (uint32_t d : {0u, 1u, full / 2, full - 1})
              CHECK(L.index(r, d) == ((size_t)(r >> 6) * full + d) * 64 + (r & 63), "c=%u N=%zu row %zu d=%u: not the uniform index", c, N, r, d);
          const std::vector<uint32_t> perm = msm_class_major_order(b.data(), N, c);
          for (size_t k = 0; k < N; k++) CHECK(perm[k] == k, "c=%u N=%zu: an all-wide set is reordered", c, N);
        }
      }
  CHECK(msm_class_entries(0, 16) == 32768 && msm_class_entries(1, 16) == 1 && msm_class_entries(2, 16) == 2 && msm_class_entries(128, 16) == 128 &&
            msm_class_entries(129, 16) == 256 && msm_class_entries(255, 16) == 256 && msm_class_entries(255, 8) == 128 && msm_class_entries(40000, 16) == 32768,
        "msm_class_entries");
  CHECK(byte_ranged_bound(0) == 255 && byte_ranged_bound(128) == 128 && byte_ranged_bound(-3) == 258 && byte_ranged_bound(255) == 255 && byte_ranged_bound(300) == 300,
        "byte_ranged_bound");
  if (bad) { printf("FAILED %d checks\n", bad); return 1; }
  printf("OK msm_ragged layout %zu cases\n", cases);
  return 0;
}

static void count_set(const Circuit& c, const WireClasses& wc, const Sparse& m, const char* name) {
  std::vector<char> in(c.n_wires, 0);
  for (auto& t : m.terms) in[t.wire] = 1;
  size_t n[4] = {};
  for (uint32_t w = 0; w < c.n_wires; w++)
    if (in[w]) n[wc.kind[w]]++;
  printf("CLASSES %s wide %zu bits %zu limbs %zu lookups %zu\n", name, n[0], n[1], n[2], n[3]);
}
static int dump_classes(const Circuit& c, const char* out) {
  const WireClasses wc = msm_wire_classes(c);
  count_set(c, wc, c.A, "A");
  count_set(c, wc, c.B, "B");
  {
    std::vector<char> com(c.n_wires, 0);
    for (uint32_t w : c.committed) com[w] = 1;
    size_t n[4] = {};
    for (uint32_t w = c.n_public; w < c.n_wires; w++)
      if (!com[w]) n[wc.kind[w]]++;
    printf("CLASSES K wide %zu bits %zu limbs %zu lookups %zu\n", n[0], n[1], n[2], n[3]);
  }
  FILE* f = fopen(out, "w");
  if (!f) return 2;
  for (uint32_t w = 0; w < c.n_wires; w++)
    if (wc.bound[w]) fprintf(f, "%u %u %u\n", w, wc.bound[w], (unsigned)wc.kind[w]);
  fclose(f);
  printf("OK msm_classes %u wires\n", c.n_wires);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "layout")) return check_layout();
  if (argc >= 4 && !strcmp(argv[1], "audit")) {
    std::vector<uint32_t> pk;
    FILE* f = fopen(argv[2], "r");
    unsigned v;
    while (f && fscanf(f, "%u", &v) == 1) pk.push_back(v);
    if (pk.size() != 2048) { printf("need 2048 pk coefficients\n"); return 2; }
    return dump_classes(build_audit_circuit(pk.data(), pk.data() + 1024, true), argv[3]);
  }
  if (argc >= 3 && !strcmp(argv[1], "withdraw")) return dump_classes(build_withdraw_circuit(true), argv[2]);
  if (argc >= 17 && !strcmp(argv[1], "plan")) {
    std::vector<PlanSet> sets;
    for (int s = 0; s < 7; s++) sets.push_back(plan_set(s, atof(argv[2 + s]), PLAN_WGT[s] != 0));
    const int at[7] = {9, 12, 15, -1, -1, -1, 12};   // A, B1, K (bits only), B2 = B1
    for (int s = 0; s < 7; s++) {
      if (at[s] < 0) continue;
      sets[s].narrow[0] = atof(argv[at[s]]);
      if (s != 2) sets[s].narrow[2] = atof(argv[at[s] + 1]) + atof(argv[at[s] + 2]);   // limbs and looked-up bytes: rows of 256
    }
    const double budget = atof(argv[16]);
    plan_greedy(sets, budget, 16);
    double bytes = 0;
    printf("PLAN bits");
    for (auto& s : sets) { printf(" %d", s.bits); bytes += plan_bytes(s, s.bits); }
    printf("\nPLAN bytes %.0f\n", bytes);
    return 0;
  }
  printf("usage: msm_ragged_check layout | audit pk.txt out | withdraw out | plan ...\n");
  return 2;
}
