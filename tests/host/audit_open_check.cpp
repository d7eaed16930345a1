// Host run of csrc/audit_open.hpp, the per-lane pieces of k_audit_open: range check, packing, decryption, owner decoding, the
// curve check and the decision against the public witness.  Reads from stdin
//   1024 secret-key coefficients, then the number of cases, then per case:
//   64 + 1024 ciphertext coefficients, ct_commitment as computed (64 hex digits), wa_commitment as computed, the 76-byte pw (152)
// and prints one line per case:  <coeff_bad> <point_ok> <flags> <64 message bytes, hex> <64 owner bytes, hex> <157 packed fields, hex>
// tests/test_audit_records_host.py compares them with tests/golden/rlwe_vectors.json / rlwe_decrypt.json and Python big ints.
#include <cstdio>
#include <string>
#include <vector>
#include "audit_open.hpp"

using namespace spp;

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out(s.size() / 2);
  for (size_t i = 0; i < out.size(); i++) out[i] = (uint8_t)std::stoul(s.substr(2 * i, 2), nullptr, 16);
  return out;
}

int main() {
  std::vector<uint32_t> sk2(2 * AO_N);
  for (uint32_t i = 0; i < AO_N; i++) {
    unsigned long long v;
    if (scanf("%llu", &v) != 1) return 2;
    ao_sk2_entry((uint32_t)v, sk2[i], sk2[AO_N + i]);
  }
  int cases;
  if (scanf("%d", &cases) != 1) return 2;
  for (int k = 0; k < cases; k++) {
    std::vector<uint32_t> ct(AO_CT_WORDS);
    bool bad = false;
    for (uint32_t i = 0; i < AO_CT_WORDS; i++) {
      unsigned long long v;
      if (scanf("%llu", &v) != 1) return 2;
      ct[i] = ao_coeff((uint32_t)v, bad);
    }
    char b0[160], b1[160], b2[160];
    if (scanf("%159s %159s %159s", b0, b1, b2) != 3) return 2;
    const std::vector<uint8_t> ct_be = unhex(b0), wa_be = unhex(b1), pw = unhex(b2);
    if (ct_be.size() != 32 || wa_be.size() != 32 || pw.size() != 76) return 2;
    uint8_t msg[AO_SLOTS], owners[64];
    for (uint32_t t = 0; t < AO_SLOTS; t++) {          // one lane after the other
      msg[t] = ao_decrypt_slot(sk2.data(), ct.data() + AO_SLOTS, ct[t], t);
      owners[ao_owner_byte(t)] = msg[t];
    }
    uint32_t x[8], y[8];
    ao_owner_limbs(msg, x, y);
    Fr fx, fy;
    const bool point_ok = ao_owner_on_curve(x, y, &fx, &fy);
    const uint32_t flags = ao_decide(bad, ct_be.data(), point_ok, wa_be.data(), pw.data());
    printf("%d %d %u ", bad ? 1 : 0, point_ok ? 1 : 0, flags);
    for (uint32_t t = 0; t < AO_SLOTS; t++) printf("%02x", msg[t]);
    printf(" ");
    for (int i = 0; i < 64; i++) printf("%02x", owners[i]);
    printf(" ");
    for (uint32_t f = 0; f < AO_FIELDS; f++) {
      uint8_t be[32];
      ao_packed_field(ct.data(), ct.data() + AO_SLOTS, f).to_bytes_be(be);   // through Fr and back: what the sponge absorbs
      for (int i = 0; i < 32; i++) printf("%02x", be[i]);
      // and the words themselves
      for (uint32_t j = 0; j < 8; j++) {
        const uint32_t w = ao_packed_word(ct.data(), ct.data() + AO_SLOTS, f, j);
        const uint32_t from_be = ((uint32_t)be[28 - 4 * j] << 24) | ((uint32_t)be[29 - 4 * j] << 16) | ((uint32_t)be[30 - 4 * j] << 8) | be[31 - 4 * j];
        if (w != from_be) return 3;
      }
      printf(f + 1 < AO_FIELDS ? "," : "\n");
    }
  }
  printf("OK audit_open %d cases\n", cases);
  return 0;
}
