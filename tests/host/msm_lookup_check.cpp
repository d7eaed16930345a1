// csrc/msm_lookup.hpp on the host: the scan for lookup-inverse wires over the product's circuits (and over a circuit file), and the
// second level -- recoding, bucket accumulation, running sum, Horner -- over points and scalars given by the caller.
//   g++ -O2 -std=c++17 -I csrc -I include tests/host/msm_lookup_check.cpp csrc/circuit.cpp csrc/circuit_audit.cpp -o msm_lookup_check
//   ./msm_lookup_check audit pk.txt out.txt     (pk.txt: 2048 integers, a then b)  -> "LOOKUPS n", out.txt: "wire hint" lines
//   ./msm_lookup_check withdraw out.txt
//   ./msm_lookup_check file circuit.sppc out.txt
//   ./msm_lookup_check unknown                  the withdraw circuit with an instruction the scan does not know -> "LOOKUPS 0"
//   ./msm_lookup_check sum in.txt               in.txt: 256 lines "x y scalar" (hex, 64 digits, big-endian; x = y = 0: infinity)
//                                               -> "SUM x y": sum_t scalar_t * (x_t, y_t) by the second level
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "msm_lookup.hpp"

using namespace spp;

static int dump(const Circuit& c, const char* out) {
  const std::vector<LookupInverse> lk = msm_lookup_inverses(c);
  FILE* f = out ? fopen(out, "w") : nullptr;
  if (out && !f) return 2;
  for (const LookupInverse& l : lk)
    if (f) fprintf(f, "%u %u\n", l.wire, l.hint);
  if (f) fclose(f);
  printf("LOOKUPS %zu\n", lk.size());
  return 0;
}
static bool hex32(const char* s, uint8_t out[32]) {
  if (strlen(s) != 64) return false;
  for (int i = 0; i < 32; i++) {
    unsigned v;
    if (sscanf(s + 2 * i, "%2x", &v) != 1) return false;
    out[i] = (uint8_t)v;
  }
  return true;
}
static void print_hex(const Fq& v) {
  uint8_t b[32];
  v.to_bytes_be(b);
  for (int i = 0; i < 32; i++) printf("%02x", b[i]);
}
// the second level as the device runs it: digit planes by lkb_recode, one lkb_window_sum per window, then the Horner of
// k_msm_horner (LKB_C doublings between two windows, from the top window down)
static int second_level(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) return 2;
  std::vector<XYZZ<Fq>> pts(LKB_VALUES);
  std::vector<std::vector<int8_t>> dig(LKB_VALUES, std::vector<int8_t>(LKB_WINDOWS));
  char sx[80], sy[80], ss[80];
  for (uint32_t t = 0; t < LKB_VALUES; t++) {
    uint8_t bx[32], by[32], bs[32];
    if (fscanf(f, "%79s %79s %79s", sx, sy, ss) != 3 || !hex32(sx, bx) || !hex32(sy, by) || !hex32(ss, bs)) { printf("line %u: malformed\n", t); return 2; }
    pts[t] = XYZZ<Fq>::from_affine(Affine<Fq>{Fq::from_bytes_be(bx), Fq::from_bytes_be(by)});
    lkb_recode(Fr::from_bytes_be(bs), dig[t].data());
    for (uint32_t j = 0; j < LKB_WINDOWS; j++)
      if (dig[t][j] < -(int)LKB_BUCKETS || dig[t][j] > (int)LKB_BUCKETS) { printf("line %u: digit %d of window %u out of range\n", t, dig[t][j], j); return 1; }
  }
  fclose(f);
  const size_t stride = 3;   // any stride: the device's is the batch size
  std::vector<XYZZ<Fq>> scratch(LKB_BUCKETS * stride);
  XYZZ<Fq> acc = XYZZ<Fq>::infinity();
  for (uint32_t w = LKB_WINDOWS; w-- > 0;) {
    for (uint32_t k = 0; k < LKB_C; k++) acc.dbl_inplace();
    acc.add(lkb_window_sum(scratch.data(), stride, [&](uint32_t t) { return (int)dig[t][w]; }, [&](uint32_t t) { return pts[t]; }));
  }
  const Affine<Fq> a = acc.to_affine();
  printf("SUM ");
  print_hex(a.x);
  printf(" ");
  print_hex(a.y);
  printf("\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 4 && !strcmp(argv[1], "audit")) {
    std::vector<uint32_t> pk;
    FILE* f = fopen(argv[2], "r");
    unsigned v;
    while (f && fscanf(f, "%u", &v) == 1) pk.push_back(v);
    if (pk.size() != 2048) { printf("need 2048 pk coefficients\n"); return 2; }
    return dump(build_audit_circuit(pk.data(), pk.data() + 1024, true), argv[3]);
  }
  if (argc >= 3 && !strcmp(argv[1], "withdraw")) return dump(build_withdraw_circuit(true), argv[2]);
  if (argc >= 4 && !strcmp(argv[1], "file")) {
    Circuit c;
    if (!c.load(argv[2])) { printf("cannot read %s\n", argv[2]); return 2; }
    return dump(c, argv[3]);
  }
  if (argc >= 2 && !strcmp(argv[1], "unknown")) {
    Circuit c = build_withdraw_circuit(true);
    if (msm_lookup_inverses(c).empty()) { printf("the withdraw circuit has no lookup inverse to lose\n"); return 1; }
    c.program.insert(c.program.begin(), {OP_LIMBS, 0u, 1u, 8u, 1u});   // a generic-solver instruction in front of the program
    return dump(c, nullptr);
  }
  if (argc >= 3 && !strcmp(argv[1], "sum")) return second_level(argv[2]);
  printf("usage: msm_lookup_check audit pk.txt out | withdraw out | file circuit.sppc out | unknown | sum in.txt\n");
  return 2;
}
