// Host run of csrc/rlwe_partial.hpp, the per-lane pieces of k_rlwe_partial and k_rlwe_combine.  Reads commands from stdin, one
// answer line each, and ends with "OK partial_decrypt <n> commands":
//   S <lambda> <n> <s_0> .. <s_n-1>              -> n scaled share values (rp_scaled_share); field elements are 64 hex digits
//   D <u_0> .. <u_1023> <c1_0> .. <c1_1023>      -> the 64 slots of rp_dot_slot over the limb-major table of u; c1 decimal
//   B <e> <rho> <t> <x_0> .. <x_t-1> <self> <seeds: 0 | 1 then t seeds of 64 hex digits> <ct> <k>   -> rp_blind_slot
//   C <w>                                        -> "<residue> <bad>" of rp_combine_residue
//   R <c0> <prod>                                -> the byte of ao_round_slot
// tests/test_partial_decrypt_host.py compares every answer with tests/partial_vectors.py (Python integers).
#include <cstdio>
#include <string>
#include <vector>
#include "rlwe_partial.hpp"

using namespace spp;

static bool read_hex32(uint8_t out[32]) {
  char buf[80];
  if (scanf("%79s", buf) != 1) return false;
  const std::string s(buf);
  if (s.size() != 64) return false;
  for (int i = 0; i < 32; i++) out[i] = (uint8_t)std::stoul(s.substr(2 * i, 2), nullptr, 16);
  return true;
}
static void print_fr(const Fr& v) {
  uint8_t be[32];
  v.to_bytes_be(be);
  for (int i = 0; i < 32; i++) printf("%02x", be[i]);
}
static void limbs_of(const uint8_t be[32], uint32_t c[8]) {
  for (int i = 0; i < 8; i++)
    c[7 - i] = ((uint32_t)be[4 * i] << 24) | ((uint32_t)be[4 * i + 1] << 16) | ((uint32_t)be[4 * i + 2] << 8) | be[4 * i + 3];
}

int main() {
  char cmd[8];
  int done = 0;
  while (scanf("%7s", cmd) == 1) {
    uint8_t be[32];
    if (cmd[0] == 'S') {
      int n;
      if (!read_hex32(be) || !be_is_canonical<FrParams>(be) || scanf("%d", &n) != 1) return 2;
      const Fr lambda = Fr::from_bytes_be(be);
      for (int i = 0; i < n; i++) {
        uint32_t u[8];
        if (!read_hex32(be) || !be_is_canonical<FrParams>(be)) return 2;
        rp_scaled_share(lambda, be, u);
        print_fr(Fr::from_canonical(u));
        printf(i + 1 < n ? " " : "\n");
      }
    } else if (cmd[0] == 'D') {
      std::vector<uint32_t> U(RP_TABLE_WORDS), c1(AO_N);
      for (uint32_t j = 0; j < AO_N; j++) {
        uint32_t c[8];
        if (!read_hex32(be) || !be_is_canonical<FrParams>(be)) return 2;
        limbs_of(be, c);
        for (uint32_t i = 0; i < RP_LIMBS; i++) U[AO_N * i + j] = c[i];
      }
      for (uint32_t j = 0; j < AO_N; j++) {
        unsigned long long v;
        if (scanf("%llu", &v) != 1 || v >= (1ull << 28)) return 2;
        c1[j] = (uint32_t)v;
      }
      for (uint32_t k = 0; k < AO_SLOTS; k++) {          // one lane after the other
        print_fr(rp_dot_slot(U.data(), c1.data(), k));
        printf(k + 1 < AO_SLOTS ? " " : "\n");
      }
    } else if (cmd[0] == 'B') {
      long long e;
      unsigned long long rho;
      unsigned t, self, k;
      int with;
      if (scanf("%lld %llu %u", &e, &rho, &t) != 3 || t == 0 || t > RP_MAX_T) return 2;
      std::vector<uint32_t> xs(t);
      for (unsigned i = 0; i < t; i++) {
        unsigned long long x;
        if (scanf("%llu", &x) != 1) return 2;
        xs[i] = (uint32_t)x;
      }
      if (scanf("%u %d", &self, &with) != 2 || self >= t) return 2;
      std::vector<uint8_t> seeds(32 * (size_t)t);
      if (with)
        for (unsigned i = 0; i < t; i++)
          if (!read_hex32(seeds.data() + 32 * i)) return 2;
      if (!read_hex32(be) || scanf("%u", &k) != 1) return 2;
      print_fr(rp_blind_slot((int32_t)e, rho, t, xs.data(), self, with ? seeds.data() : nullptr, be, k));
      printf("\n");
    } else if (cmd[0] == 'C') {
      uint32_t w[8];
      if (!read_hex32(be) || !be_is_canonical<FrParams>(be)) return 2;
      limbs_of(be, w);
      bool bad = false;
      const uint32_t res = rp_combine_residue(w, bad);
      printf("%u %d\n", res, bad ? 1 : 0);
    } else if (cmd[0] == 'R') {
      unsigned c0, prod;
      if (scanf("%u %u", &c0, &prod) != 2 || c0 >= AO_Q || prod >= AO_Q) return 2;
      printf("%u\n", (unsigned)ao_round_slot(c0, prod));
    } else {
      return 2;
    }
    done++;
  }
  printf("OK partial_decrypt %d commands\n", done);
  return 0;
}
