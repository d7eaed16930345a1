// The reshare section of csrc/vss.hpp on the host: the weighted sum of dealers' points by one shared scan, the public commitment
// of a share, the NOT_SHARE decision, the Lagrange weights and the weighted sum of sub-shares, driven by the caller's values
// (tests/test_reshare_host.py).
//   g++ -O1 -std=c++17 -fsanitize=address,undefined -I csrc -I include tests/host/reshare_check.cpp -o reshare_check
//   ./reshare_check lincomb in.txt    per record: "dealers weighted based" then the dealers' points (hex, 128 digits), the weights if
//                                     weighted = 1 (hex, 64 digits), the base if based = 1 -> "L flags" and the 64 bytes of
//                                     vss_store_point(vss_lincomb); flags: the OR of vss_decode over the inputs
//   ./reshare_check ex in.txt         per record: "t x" then t commitments -> "E ok" and the 64 bytes of sum_k x^k C_k
//   ./reshare_check isshare in.txt    per record: "t x" then t committee commitments and one constant term -> "S flags" of vss_is_share
//   ./reshare_check lagrange x...     -> per x "A" and its Lagrange coefficient at 0 (hex, 64 digits)
//   ./reshare_check wsum in.txt       per record: "dealers" then the weights and the values (hex, 64 digits) -> "W" and the sum
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
static bool read_hex(FILE* f, uint8_t* out, size_t n) {
  char s[200];
  return fscanf(f, "%199s", s) == 1 && hexn(s, out, n);
}

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "lincomb")) {
    FILE* f = fopen(argv[2], "r");
    if (!f) return 2;
    unsigned dealers, weighted, based;
    while (fscanf(f, "%u %u %u", &dealers, &weighted, &based) == 3) {
      if (dealers == 0 || dealers > 255 || (weighted && dealers > VSS_LINCOMB_MAX)) return 2;
      // exact-size heap blocks: a read past either end is the sanitizer's to find
      std::vector<G1Affine> pts(dealers), base(1);
      std::vector<uint32_t> words((size_t)8 * dealers);
      std::vector<uint8_t> raw(64), w(32);
      uint32_t flags = 0;
      for (unsigned d = 0; d < dealers; d++) {
        if (!read_hex(f, raw.data(), 64)) return 2;
        flags |= vss_decode(raw.data(), &pts[d]);
      }
      for (unsigned d = 0; weighted && d < dealers; d++) {
        if (!read_hex(f, w.data(), 32)) return 2;
        Fr::from_bytes_be(w.data()).to_canonical(words.data() + 8 * d);
      }
      if (based) {
        if (!read_hex(f, raw.data(), 64)) return 2;
        flags |= vss_decode(raw.data(), &base[0]);
      }
      uint8_t out[64];
      memset(out, 0x55, sizeof out);
      vss_store_point(vss_lincomb(dealers, weighted ? words.data() : nullptr, pts.data(), 1, based ? base.data() : nullptr), out);
      printf("L %u ", flags);
      print_bytes(out, 64);
      printf("\n");
    }
    fclose(f);
    return 0;
  }
  if (argc == 3 && (!strcmp(argv[1], "ex") || !strcmp(argv[1], "isshare"))) {
    const bool share = argv[1][0] == 'i';
    FILE* f = fopen(argv[2], "r");
    if (!f) return 2;
    unsigned t, x;
    while (fscanf(f, "%u %u", &t, &x) == 2) {
      if (t == 0 || t > 64 || x == 0) return 2;
      std::vector<uint8_t> cm((size_t)t * 64), c0(64);
      for (unsigned k = 0; k < t; k++)
        if (!read_hex(f, cm.data() + 64 * k, 64)) return 2;
      if (share) {
        if (!read_hex(f, c0.data(), 64)) return 2;
        printf("S %u\n", vss_is_share(t, x, cm.data(), 64, c0.data()));
        continue;
      }
      G1XYZZ e = G1XYZZ::infinity();
      G1Affine d0;
      uint8_t out[64];
      memset(out, 0x55, sizeof out);
      const bool ok = vss_eval_commitments(t, x, cm.data(), 64, &e, &d0);
      vss_store_point(e, out);
      printf("E %d ", ok ? 1 : 0);
      print_bytes(out, 64);
      printf("\n");
    }
    fclose(f);
    return 0;
  }
  if (argc >= 3 && !strcmp(argv[1], "lagrange")) {
    std::vector<uint32_t> xs;
    for (int k = 2; k < argc; k++) xs.push_back((uint32_t)strtoul(argv[k], nullptr, 10));
    std::vector<Fr> lam(xs.size());
    vss_lagrange_at_zero(xs.data(), (uint32_t)xs.size(), lam.data());
    for (const Fr& l : lam) {
      uint8_t b[32];
      l.to_bytes_be(b);
      printf("A ");
      print_bytes(b, 32);
      printf("\n");
    }
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "wsum")) {
    FILE* f = fopen(argv[2], "r");
    if (!f) return 2;
    unsigned dealers;
    while (fscanf(f, "%u", &dealers) == 1) {
      if (dealers == 0 || dealers > 255) return 2;
      std::vector<Fr> w(dealers);
      std::vector<uint8_t> ys((size_t)32 * dealers), one(32);
      for (unsigned d = 0; d < dealers; d++) {
        if (!read_hex(f, one.data(), 32)) return 2;
        w[d] = Fr::from_bytes_be(one.data());
      }
      for (unsigned d = 0; d < dealers; d++)
        if (!read_hex(f, ys.data() + 32 * d, 32)) return 2;
      uint8_t out[32];
      vss_weighted_sum(dealers, w.data(), ys.data(), 32, out);
      printf("W ");
      print_bytes(out, 32);
      printf("\n");
    }
    fclose(f);
    return 0;
  }
  fprintf(stderr, "usage: reshare_check lincomb file | ex file | isshare file | lagrange x... | wsum file\n");
  return 2;
}
