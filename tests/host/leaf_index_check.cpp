// Host build of csrc/leaf_index.hpp (g++, no GPU, its own main): the leaf index of the resident tree -- one slot per leaf, no key
// bytes, queries over the run -- driven from stdin by tests/test_wallet_sync_host.py, which compares every line with a list of
// leaves scanned linearly.
//   <salt hex> <n> <q> <order> <k> <stage_1> .. <stage_k>     order: 0 ascending, 1 descending, 2 shuffled; stage_k == n
//   n leaves (hex, tree order), then q lines "<key hex> <from> <pmod> <prem>"      predicate(i) = i % pmod != prem
// Per stage the index is brought up to the first stage_j leaves the way the library does it (leaves [indexed, stage_j) inserted,
// in the given order; a table that would pass half full allocated again and every leaf reinserted), then:
//   "slots <count> rebuilt <0|1>"
//   "table <slot 0> <slot 1> ..."                              the leaf index in each slot, -1 = empty
//   per leaf  "<home>"                                          leaf_home, checked here against pool_slot() of the encoding
//   per query "<lowest | -1> <matches> <first | -1>"            leaf_index_lowest, its count, leaf_index_first under the predicate
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "leaf_index.hpp"

using namespace spp;

static bool read_key(uint8_t* out) {
  char buf[128];
  if (scanf("%100s", buf) != 1 || strlen(buf) != 64) return false;
  for (int i = 0; i < 32; i++) {
    unsigned v;
    if (sscanf(buf + 2 * i, "%2x", &v) != 1) return false;
    out[i] = (uint8_t)v;
  }
  return true;
}

struct Query {
  Fr key;
  unsigned long long from;
  unsigned pmod, prem;
};

int main() {
  unsigned long long salt;
  unsigned n, q, order, k;
  if (scanf("%llx %u %u %u %u", &salt, &n, &q, &order, &k) != 5 || order > 2 || k == 0) return 2;
  std::vector<unsigned> stages(k);
  for (unsigned& s : stages)
    if (scanf("%u", &s) != 1 || s > n) return 2;
  if (stages.back() != n) return 2;
  std::vector<Fr> leaves(n);
  std::vector<uint8_t> bytes((size_t)n * 32);
  for (unsigned i = 0; i < n; i++) {
    if (!read_key(&bytes[(size_t)i * 32]) || !be_is_canonical<FrParams>(&bytes[(size_t)i * 32])) return 2;
    leaves[i] = Fr::from_bytes_be(&bytes[(size_t)i * 32]);
  }
  std::vector<Query> queries(q);
  for (Query& qu : queries) {
    uint8_t key[32];
    if (!read_key(key) || scanf("%llu %u %u", &qu.from, &qu.pmod, &qu.prem) != 3 || qu.pmod == 0) return 2;
    qu.key = Fr::from_bytes_be(key);
  }

  std::vector<uint32_t> slots;
  unsigned indexed = 0;
  uint64_t lcg = 0x9E3779B97F4A7C15ull ^ salt;
  for (unsigned stage : stages) {
    if (stage < indexed) return 2;
    const uint32_t want = leaf_index_slots(stage);
    const bool rebuilt = want > slots.size();
    if (rebuilt) {
      slots.assign(want, LEAF_NONE);
      indexed = 0;
    }
    LeafIndex ix{slots.data(), (uint32_t)slots.size() - 1, salt};
    std::vector<uint32_t> todo;
    for (unsigned i = indexed; i < stage; i++) todo.push_back(i);
    if (order == 1)
      for (size_t a = 0, b = todo.size(); a + 1 < b; a++, b--) std::swap(todo[a], todo[b - 1]);
    if (order == 2)
      for (size_t a = todo.size(); a > 1; a--) {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        std::swap(todo[a - 1], todo[(size_t)((lcg >> 33) % a)]);
      }
    for (uint32_t i : todo) leaf_index_insert(ix, leaves.data(), i);
    indexed = stage;

    printf("slots %u rebuilt %d\ntable", (unsigned)slots.size(), rebuilt ? 1 : 0);
    for (uint32_t s : slots) printf(" %d", s == LEAF_NONE ? -1 : (int)s);
    printf("\n");
    for (unsigned i = 0; i < stage; i++) {
      const uint32_t home = leaf_home(leaves[i], salt, ix.mask);
      if (home != pool_slot(&bytes[(size_t)i * 32], salt, ix.mask)) return 3;   // the home slot IS pool_slot() of the encoding
      printf("%u\n", home);
    }
    for (const Query& qu : queries) {
      uint32_t m = 0;
      const uint32_t lo = leaf_index_lowest(ix, leaves.data(), qu.key, qu.from, &m);
      const uint32_t fi = leaf_index_first(ix, leaves.data(), qu.key, qu.from, [&](uint32_t i) { return i % qu.pmod != qu.prem; });
      printf("%d %u %d\n", lo == LEAF_NONE ? -1 : (int)lo, m, fi == LEAF_NONE ? -1 : (int)fi);
    }
  }
  return 0;
}
