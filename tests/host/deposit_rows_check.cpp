// Host build of csrc/deposit_rows.hpp (g++, no GPU, its own main): the walk k_deposit_rows does per lane, instantiated over the
// host's Fr with a plain Poseidon t=3 permutation from the builder's constants (csrc/circuit.cpp), against big-integer vectors the
// Python model wrote (tests/deposit_model.py).  Run by tests/test_deposit_rows_host.py, plain and with -fsanitize=address,undefined.
//   deposit_rows_check <vectors file>
// vectors: "depth n", n leaves, then per leaf i a line "old_root new_root sibling_0 .. sibling_{depth-1}", all 64-digit hex.
// The tree is rebuilt here level by level, level l holding exactly cnt_l(m) nodes for the size m it is rebuilt at, so that a read past
// what is stored is a heap overflow the sanitizer reports.  For every leaf i the walk runs against the tree of size i + 1 (the
// smallest that holds leaf i) and against the full tree: both must give the model's row, i.e. later leaves change nothing.  It also
// runs with a commitment that is NOT the stored leaf: old_root and the siblings stay, new_root moves.
// Prints "rows <n> walks <k>"; exit status 1 and a line on stderr at the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "circuit.hpp"
#include "deposit_rows.hpp"

namespace spp {
Fr fr_from_hex(const char* h);   // csrc/circuit.cpp
}
using namespace spp;

static Fr hash2(const Fr& a, const Fr& b) {
  const PoseidonParams& pp = poseidon_params(3);
  Fr s[3] = {Fr::zero(), a, b};
  for (int r = 0; r < pp.rf + pp.rp; r++) {
    for (int i = 0; i < 3; i++) s[i] = s[i] + pp.rc[r * 3 + i];
    const bool full = r < pp.rf / 2 || r >= pp.rf / 2 + pp.rp;
    for (int i = 0; i < (full ? 3 : 1); i++) {
      const Fr x2 = s[i] * s[i];
      s[i] = x2 * x2 * s[i];
    }
    Fr n[3];
    for (int i = 0; i < 3; i++) n[i] = pp.mds[i][0] * s[0] + pp.mds[i][1] * s[1] + pp.mds[i][2] * s[2];
    for (int i = 0; i < 3; i++) s[i] = n[i];
  }
  return s[0];
}

static bool read_fr(FILE* f, Fr* out) {
  char buf[80];
  if (fscanf(f, "%79s", buf) != 1 || std::string(buf).size() != 64) return false;
  *out = fr_from_hex(buf);
  return true;
}

struct Tree {
  std::vector<std::vector<Fr>> level;
};
static Tree rebuild(const std::vector<Fr>& leaves, size_t m, uint32_t depth, const std::vector<Fr>& dflt) {
  Tree t;
  t.level.resize(depth + 1);
  t.level[0].assign(leaves.begin(), leaves.begin() + m);
  for (uint32_t l = 0; l < depth; l++) {
    const std::vector<Fr>& c = t.level[l];
    for (size_t j = 0; 2 * j < c.size(); j++) t.level[l + 1].push_back(hash2(c[2 * j], 2 * j + 1 < c.size() ? c[2 * j + 1] : dflt[l]));
  }
  return t;
}

#define FAIL(...)                 \
  do {                            \
    fprintf(stderr, __VA_ARGS__); \
    fprintf(stderr, "\n");        \
    return 1;                     \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) FAIL("cannot read %s", argv[1]);
  unsigned depth = 0, n = 0;
  if (fscanf(f, "%u %u", &depth, &n) != 2 || depth < 1 || depth > 32 || n < 1 || n > 4096) FAIL("bad header");
  std::vector<Fr> leaves(n), dflt(depth + 1);
  for (auto& v : leaves)
    if (!read_fr(f, &v)) FAIL("bad leaf");
  std::vector<std::vector<Fr>> want(n, std::vector<Fr>(2 + depth));
  for (auto& row : want)
    for (auto& v : row)
      if (!read_fr(f, &v)) FAIL("bad row");
  fclose(f);
  dflt[0] = Fr::zero();
  for (uint32_t l = 0; l < depth; l++) dflt[l + 1] = hash2(dflt[l], dflt[l]);
  const Tree full = rebuild(leaves, n, depth, dflt);
  unsigned long walks = 0;
  for (unsigned i = 0; i < n; i++) {
    const Tree just = rebuild(leaves, i + 1, depth, dflt);
    for (int which = 0; which < 3; which++, walks++) {
      const Tree& t = which == 0 ? just : full;
      const Fr c = which == 2 ? leaves[i] + Fr::one() : leaves[i];
      std::vector<Fr> sibs(depth);
      Fr roots[2];
      deposit_walk(i, depth, [&](uint32_t l) { return t.level[l].data(); }, dflt.data(), Fr::zero(), c, hash2,
                   [&](uint32_t l, const Fr& s) { sibs[l] = s; }, roots);
      if (!(roots[0] == want[i][0])) FAIL("leaf %u tree %d: old_root", i, which);
      if ((roots[1] == want[i][1]) != (which != 2)) FAIL("leaf %u tree %d: new_root", i, which);
      for (uint32_t l = 0; l < depth; l++)
        if (!(sibs[l] == want[i][2 + l])) FAIL("leaf %u tree %d: sibling %u", i, which, l);
    }
    // the roots are the rebuilt trees' own: size i before, size i + 1 after
    if (!(want[i][1] == just.level[depth][0])) FAIL("leaf %u: new_root is not the root of %u leaves", i, i + 1);
    if (i + 1 < n && !(want[i + 1][0] == just.level[depth][0])) FAIL("leaf %u: the next old_root is not this new_root", i);
  }
  if (!(want[0][0] == dflt[depth])) FAIL("leaf 0: old_root is not the empty root");
  printf("rows %u walks %lu\n", n, walks);
  return 0;
}
