// csrc/vss.hpp on the host: the generators, the common a of a joint key, the window table, commitments read off it and the
// receiver's check of one value, driven by the caller's values (tests/test_vss_host.py).
//   g++ -O1 -std=c++17 -fsanitize=address,undefined -I csrc -I include tests/host/vss_check.cpp -o vss_check
//   ./vss_check gens                -> "G x y" and "H ctr x y"
//   ./vss_check a seed...           (hex, 64 digits) -> per seed "A v_0 ... v_1023"
//   ./vss_check entry i...          table indices -> per index "E i x y", by vss_table_entry from the window bases
//   ./vss_check commit in.txt       "c c'" per line (hex, 64 digits) -> per line "C" and the 64 bytes of vss_store_point(vss_commit)
//   ./vss_check check in.txt        per record: "t x zero" then t commitments (hex, 128 digits), y, y' and, if zero = 1, the published
//                                   blind -> per record "F flags" of vss_check_value
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vss.hpp"

using namespace spp;

static bool hexn(const char* s, uint8_t* out, size_t n) {
  if (strlen(s) != 2 * n) return false;
  for (size_t i = 0; i < n; i++) {
    unsigned v;
    if (sscanf(s + 2 * i, "%2x", &v) != 1) return false;
    out[i] = (uint8_t)v;
  }
  return true;
}
static void print_bytes(const uint8_t* b, size_t n) {
  for (size_t i = 0; i < n; i++) printf("%02x", b[i]);
}
static void print_point(const G1Affine& p) {
  uint8_t b[64];
  vss_store_point(G1XYZZ::from_affine(p), b);
  print_bytes(b, 32);
  printf(" ");
  print_bytes(b + 32, 32);
}
static std::vector<G1Affine> full_table() {
  G1Affine wb[2 * VSS_WINDOWS];
  vss_window_bases(wb);
  std::vector<G1Affine> t(VSS_TABLE_POINTS);
  for (uint32_t i = 0; i < VSS_TABLE_POINTS; i++) t[i] = vss_table_entry(wb, i);
  return t;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "gens")) {
    uint32_t ctr = 99;
    const G1Affine h = vss_generator_h(&ctr);
    printf("G ");
    print_point(vss_generator_g());
    printf("\nH %u ", ctr);
    print_point(h);
    printf("\n");
    return 0;
  }
  if (argc >= 3 && !strcmp(argv[1], "a")) {
    for (int k = 2; k < argc; k++) {
      uint8_t seed[32];
      if (!hexn(argv[k], seed, 32)) return 2;
      std::vector<uint32_t> a(VSS_RLWE_N, 0xffffffffu);   // every entry must be written
      vss_a_from_seed(seed, a.data());
      printf("A");
      for (uint32_t v : a) printf(" %u", v);
      printf("\n");
    }
    return 0;
  }
  if (argc >= 3 && !strcmp(argv[1], "entry")) {
    G1Affine wb[2 * VSS_WINDOWS];
    vss_window_bases(wb);
    for (int k = 2; k < argc; k++) {
      const uint32_t i = (uint32_t)strtoul(argv[k], nullptr, 10);
      if (i >= VSS_TABLE_POINTS) return 2;
      printf("E %u ", i);
      print_point(vss_table_entry(wb, i));
      printf("\n");
    }
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "commit")) {
    FILE* f = fopen(argv[2], "r");
    if (!f) return 2;
    const std::vector<G1Affine> table = full_table();
    char sc[80], sb[80];
    while (fscanf(f, "%79s %79s", sc, sb) == 2) {
      // the scalars in exact-size heap blocks: a read past either end is the sanitizer's to find
      std::vector<uint8_t> c(32), cb(32);
      uint8_t out[64];
      if (!hexn(sc, c.data(), 32) || !hexn(sb, cb.data(), 32)) return 2;
      memset(out, 0x55, sizeof out);
      vss_store_point(vss_commit(table.data(), c.data(), cb.data()), out);
      printf("C ");
      print_bytes(out, 64);
      printf("\n");
    }
    fclose(f);
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "check")) {
    FILE* f = fopen(argv[2], "r");
    if (!f) return 2;
    const std::vector<G1Affine> table = full_table();
    unsigned t, x, zero;
    while (fscanf(f, "%u %u %u", &t, &x, &zero) == 3) {
      if (t == 0 || t > 64 || x == 0) return 2;
      std::vector<uint8_t> cm((size_t)t * 64), y(32), yb(32), z(32);
      char s[200];
      for (unsigned k = 0; k < t; k++)
        if (fscanf(f, "%199s", s) != 1 || !hexn(s, cm.data() + 64 * k, 64)) return 2;
      if (fscanf(f, "%199s", s) != 1 || !hexn(s, y.data(), 32)) return 2;
      if (fscanf(f, "%199s", s) != 1 || !hexn(s, yb.data(), 32)) return 2;
      if (zero && (fscanf(f, "%199s", s) != 1 || !hexn(s, z.data(), 32))) return 2;
      printf("F %u\n", vss_check_value(table.data(), t, x, cm.data(), 64, y.data(), yb.data(), zero ? z.data() : nullptr));
    }
    fclose(f);
    return 0;
  }
  fprintf(stderr, "usage: vss_check gens | a seed... | entry i... | commit file | check file\n");
  return 2;
}
