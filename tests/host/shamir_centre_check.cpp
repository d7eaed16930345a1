// Host run of ao_centred_mod_q (csrc/audit_open.hpp), the lines of k_shamir_combine that turn a reconstructed value of Fr into a
// key coefficient mod q.  Reads from stdin the number of cases, then per case one value below r as 64 hex digits, and prints one
// line per case: the coefficient in decimal.  tests/test_auditor_vectors_host.py compares them with Python big ints.
#include <cstdio>
#include <string>
#include "audit_open.hpp"

using namespace spp;

int main() {
  int cases;
  if (scanf("%d", &cases) != 1) return 2;
  for (int k = 0; k < cases; k++) {
    char hex[80];
    if (scanf("%79s", hex) != 1 || std::string(hex).size() != 64) return 2;
    uint32_t c[8];
    for (int i = 0; i < 8; i++) c[i] = (uint32_t)std::stoul(std::string(hex).substr(56 - 8 * i, 8), nullptr, 16);   // little-endian limbs
    if (Fr::geq_mod(c)) return 3;
    // the kernel's way in: through the field element and back to canonical limbs
    uint32_t back[8];
    Fr::from_canonical(c).to_canonical(back);
    for (int i = 0; i < 8; i++)
      if (back[i] != c[i]) return 4;
    printf("%u\n", ao_centred_mod_q(back));
  }
  printf("OK shamir_centre %d cases\n", cases);
  return 0;
}
