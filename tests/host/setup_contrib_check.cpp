// csrc/setup_contrib.hpp on the host: the recoding of the ceremony's scalar, the scaling of points by its digits, the point check and
// the structural comparison of two proving keys, driven by the caller's values (tests/test_setup_contrib_host.py).
//   g++ -O1 -std=c++17 -fsanitize=address,undefined -I csrc -I include tests/host/setup_contrib_check.cpp -o setup_contrib_check
//   ./setup_contrib_check recode k...      (hex, 64 digits)   -> per scalar "NAF len d_0 d_1 ... d_255" (all SC_MAX_DIGITS entries)
//   ./setup_contrib_check scale in.txt     line 1: the scalar; then "x y" per point (hex, 64 digits; x = y = 0: infinity)
//                                          -> per point "PT flag x y": the flag of sc_decode_point, k * point by sc_scale_point
//   ./setup_contrib_check diff before after       two proving-key files -> "DIFF verdict n_k n_z delta1 delta2 k_points z_points"
//   ./setup_contrib_check vkdiff before after     two verifying-key files -> "VKDIFF 0|1"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "setup_contrib.hpp"

using namespace spp;

static bool hex32(const char* s, uint8_t out[32]) {
  if (strlen(s) != 64) return false;
  for (int i = 0; i < 32; i++) {
    unsigned v;
    if (sscanf(s + 2 * i, "%2x", &v) != 1) return false;
    out[i] = (uint8_t)v;
  }
  return true;
}
static void limbs_of(const uint8_t be[32], uint32_t k[8]) {
  for (int i = 0; i < 8; i++) k[7 - i] = sc_load_be32(be + 4 * i);
}
static void print_hex(const Fq& v) {
  uint8_t b[32];
  v.to_bytes_be(b);
  for (int i = 0; i < 32; i++) printf("%02x", b[i]);
}
static bool slurp(const char* path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  uint8_t buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
  fclose(f);
  return true;
}

int main(int argc, char** argv) {
  if (argc >= 3 && !strcmp(argv[1], "recode")) {
    for (int a = 2; a < argc; a++) {
      uint8_t be[32];
      uint32_t k[8];
      if (!hex32(argv[a], be)) return 2;
      limbs_of(be, k);
      int8_t dig[SC_MAX_DIGITS];
      memset(dig, 0x55, sizeof dig);   // every entry must be written
      const uint32_t len = sc_naf_recode(k, dig);
      printf("NAF %u", len);
      for (uint32_t i = 0; i < SC_MAX_DIGITS; i++) printf(" %d", dig[i]);
      printf("\n");
    }
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "scale")) {
    FILE* f = fopen(argv[2], "r");
    if (!f) return 2;
    char sx[80], sy[80];
    uint8_t be[32];
    uint32_t k[8];
    if (fscanf(f, "%79s", sx) != 1 || !hex32(sx, be)) return 2;
    limbs_of(be, k);
    int8_t dig[SC_MAX_DIGITS];
    const uint32_t len = sc_naf_recode(k, dig);
    while (fscanf(f, "%79s %79s", sx, sy) == 2) {
      uint8_t raw[64];
      if (!hex32(sx, raw) || !hex32(sy, raw + 32)) return 2;
      Affine<Fq> p;
      const uint32_t flag = sc_decode_point(raw, &p);
      const Affine<Fq> r = sc_scale_point(p, dig, len).to_affine();
      printf("PT %u ", flag);
      if (r.is_inf()) printf("%064x %064x\n", 0, 0);
      else { print_hex(r.x); printf(" "); print_hex(r.y); printf("\n"); }
    }
    fclose(f);
    return 0;
  }
  if (argc == 4 && (!strcmp(argv[1], "diff") || !strcmp(argv[1], "vkdiff"))) {
    std::vector<uint8_t> b, a;
    if (!slurp(argv[2], b) || !slurp(argv[3], a)) return 2;
    if (!strcmp(argv[1], "vkdiff")) {
      printf("VKDIFF %d\n", vk_delta_diff_ok(b.data(), b.size(), a.data(), a.size()) ? 1 : 0);
      return 0;
    }
    SppkLayout L;
    const int v = sppk_delta_diff(b.data(), b.size(), a.data(), a.size(), &L);
    printf("DIFF %d %u %u %zu %zu %zu %zu\n", v, L.n_k, L.n_z, L.delta1, L.delta2, L.k_points, L.z_points);
    return 0;
  }
  fprintf(stderr, "usage: setup_contrib_check recode|scale|diff|vkdiff ...\n");
  return 2;
}
