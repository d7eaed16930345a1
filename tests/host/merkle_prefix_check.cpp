// Host build of csrc/merkle_prefix.hpp (g++, no GPU, its own main): the tree as of an earlier size -- the three cases of a node
// and the frontier recurrence -- instantiated with a toy 64-bit mixing hash instead of Poseidon and compared with trees REBUILT
// FROM SCRATCH.  Run by tests/test_tree_asof_host.py, plain and with -fsanitize=address,undefined.
//   merkle_prefix_check <seed hex>
// leaf i = mix(seed + i), or 0 when that value is a multiple of 4 (the default leaf is 0: zero-valued leaves make prefix roots
// repeat); H(a, b) = mix(mix(a ^ 0x9E3779B97F4A7C15) * 3 + b), so that H(0, 0) != 0; dflt[0] = 0, dflt[l+1] = H(dflt[l], dflt[l]).
// For depth 1..6, every stored size m in 0..2^depth (the tree "as it stands", level l holding exactly cnt_l(m) nodes, so that a read
// past what is stored is a heap overflow the sanitizer reports) and every n in 0..m:
//   - prefix_walk's F[l] against node (l, cnt_l(n) - 1) of the tree rebuilt from leaves[:n]; F[l] = dflt[l] for n = 0; its return
//     value, with and without F, against that tree's root;
//   - prefix_node(n, l, s) for EVERY l in 0..depth and s in 0..2^(depth-l)-1 against that tree's node, default where it has none;
//   - prefix_case against the definition.
// Prints per depth "depth <d> sizes <pairs (m, n) checked> nodes <nodes compared> zero_leaves <k>", then "roots <R[0]> .. <R[2^d]>"
// (hex) from prefix_walk over the full tree, which the test compares with its own Python model; exit status 1 and a line on stderr at
// the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "merkle_prefix.hpp"

using namespace spp;
typedef uint64_t Node;

static uint64_t mix(uint64_t z) {   // splitmix64's finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static Node toy_hash(const Node& a, const Node& b) { return mix(mix(a ^ 0x9E3779B97F4A7C15ull) * 3 + b); }

struct Tree {
  std::vector<std::vector<Node>> level;   // level[l].size() == cnt_l(leaves)
};
// client/merkle.ts:165-176 over the first n leaves, every level from the one below
static Tree rebuild(const std::vector<Node>& leaves, uint64_t n, uint32_t depth, const std::vector<Node>& dflt) {
  Tree t;
  t.level.resize(depth + 1);
  t.level[0].assign(leaves.begin(), leaves.begin() + n);
  for (uint32_t l = 0; l < depth; l++) {
    const std::vector<Node>& c = t.level[l];
    for (size_t j = 0; 2 * j < c.size(); j++) t.level[l + 1].push_back(toy_hash(c[2 * j], 2 * j + 1 < c.size() ? c[2 * j + 1] : dflt[l]));
  }
  return t;
}
static Node node_of(const Tree& t, uint32_t l, uint64_t s, const std::vector<Node>& dflt) { return s < t.level[l].size() ? t.level[l][s] : dflt[l]; }

#define FAIL(...)                      \
  do {                                 \
    fprintf(stderr, __VA_ARGS__);      \
    fprintf(stderr, "\n");             \
    return 1;                          \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const uint64_t seed = strtoull(argv[1], nullptr, 16);
  for (uint32_t depth = 1; depth <= 6; depth++) {
    const uint64_t full = (uint64_t)1 << depth;
    std::vector<Node> dflt(depth + 1), leaves(full);
    dflt[0] = 0;
    for (uint32_t l = 0; l < depth; l++) dflt[l + 1] = toy_hash(dflt[l], dflt[l]);
    unsigned zeros = 0;
    for (uint64_t i = 0; i < full; i++) {
      const uint64_t v = mix(seed + depth * 1000 + i);
      leaves[i] = v % 4 == 0 ? 0 : v;
      zeros += leaves[i] == 0;
    }
    std::vector<Tree> fresh;   // fresh[n]: the tree of the first n leaves
    for (uint64_t n = 0; n <= full; n++) fresh.push_back(rebuild(leaves, n, depth, dflt));
    unsigned long long pairs = 0, nodes = 0;
    for (uint64_t m = 0; m <= full; m++) {
      const Tree& stored = fresh[m];   // the tree as it stands; an append-only tree's stored nodes ARE those of the rebuilt one
      auto levels = [&](uint32_t l) { return stored.level[l].data(); };
      for (uint64_t n = 0; n <= m; n++, pairs++) {
        const Tree& want = fresh[n];
        std::vector<Node> F(depth + 1, 0x5555);
        const Node root = prefix_walk(n, depth, levels, dflt.data(), toy_hash, F.data());
        const Node root2 = prefix_walk(n, depth, levels, dflt.data(), toy_hash, (Node*)nullptr);
        if (root != node_of(want, depth, 0, dflt) || root2 != root || F[depth] != root) FAIL("depth %u m %llu n %llu: root", depth, (unsigned long long)m, (unsigned long long)n);
        for (uint32_t l = 0; l <= depth; l++) {
          const uint64_t cnt = prefix_count(n, l);
          if (cnt != want.level[l].size()) FAIL("depth %u n %llu level %u: prefix_count", depth, (unsigned long long)n, l);
          if (F[l] != (n ? want.level[l][cnt - 1] : dflt[l])) FAIL("depth %u m %llu n %llu level %u: frontier", depth, (unsigned long long)m, (unsigned long long)n, l);
          for (uint64_t s = 0; s < (full >> l); s++, nodes++) {
            const uint32_t c = prefix_case(n, l, s), expect = s >= cnt ? PREFIX_DEFAULT : s == cnt - 1 ? PREFIX_FRONTIER : PREFIX_STORED;
            if (c != expect) FAIL("depth %u n %llu node (%u, %llu): case %u", depth, (unsigned long long)n, l, (unsigned long long)s, c);
            if (prefix_node(n, l, s, levels(l), dflt.data(), F.data()) != node_of(want, l, s, dflt))
              FAIL("depth %u m %llu n %llu node (%u, %llu): value", depth, (unsigned long long)m, (unsigned long long)n, l, (unsigned long long)s);
          }
        }
      }
    }
    printf("depth %u sizes %llu nodes %llu zero_leaves %u\nroots", depth, pairs, nodes, zeros);
    const Tree& stored = fresh[full];
    for (uint64_t n = 0; n <= full; n++)
      printf(" %016llx", (unsigned long long)prefix_walk(n, depth, [&](uint32_t l) { return stored.level[l].data(); }, dflt.data(), toy_hash, (Node*)nullptr));
    printf("\n");
  }
  return 0;
}
