// Test-only host build of the random-linear-combination batch verifier (csrc/verify_rlc.hpp, csrc/f12_coop.hpp).
//   verify_rlc_check
//       every wave-cooperative routine, its 64 lanes run one after another (CoopEmu), against its one-lane counterpart of
//       csrc/pairing_fast.hpp on random and extremal inputs.  Prints "OK <n>" or "FAIL ...".
//   verify_rlc_check <vk> <batch file> <seed: 64 hex digits> <group> [flags]
//       the whole pipeline on a file of records proof[388] || pw: terms, fold, the tail twice (rlc_final_serial and the emulated
//       cooperative tail), the fallback through verify_one.  Prints
//           VERDICTS <one digit per proof>
//           STATS <groups> <groups refused> <proofs re-verified> <proofs dropped>
//           TAILS <agree | DISAGREE>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "pairing_fast_host.hpp"
#include "verify_rlc.hpp"
#include "f12_coop.hpp"
using namespace spp;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd32() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}
static int checks = 0;
#define CHECK(c, msg) do { checks++; if (!(c)) { printf("FAIL %s (line %d)\n", msg, __LINE__); return 1; } } while (0)

static Fq fq_rand() { uint32_t w[8]; for (auto& x : w) x = rnd32(); return Fq::from_u256(w); }
static bool f12_eq(const F12& a, const F12& b) {
  for (int i = 0; i < 12; i++) if (a.c[i] != b.c[i]) return false;
  return true;
}
static Fq fq_hex(const char* h) {
  uint32_t c[8];
  for (int i = 0; i < 8; i++) { char b[9]; memcpy(b, h + 8 * i, 8); b[8] = 0; c[7 - i] = (uint32_t)strtoul(b, nullptr, 16); }
  return Fq::from_canonical(c);
}

// the cooperative tail of one folded group, emulated: what k_verify_rlc_group does after the fold
struct Tail {
  CoopShared sh;
  CoopMiller mil;
  CoopFinal fin;
  F12 extra, f;
};
static bool coop_tail(const VerifyKeyDev& vk, const RlcKeyDev& rk, const W256* folded, Tail& T) {
  CoopEmu x;
  T.sh.cc = make_coop_consts(vk.pc);
  std::vector<G1XYZZ> parts(vk.nk + 1);
  for (uint32_t k = 0; k <= vk.nk; k++) rlc_key_scalar_mul(vk, rk, folded, k, parts[k]);
  G1XYZZ kagg = rlc_get_point(folded, 1, RLC_P_RCM);
  for (uint32_t k = 0; k < vk.nk; k++) g1_add_call(kagg, parts[k]);
  for (uint32_t k = 0; k < 5; k++) {
    rlc_tail_point(folded, kagg, parts[vk.nk], k, T.mil.P[k]);
    T.mil.tab[k] = k < 4 ? vk.tab[k] : rk.tab_beta;
  }
  for (int e = 0; e < 12; e++) T.extra.c[e] = w256_as<Fq>(folded[RLC_E_MILLER + e]);
  coop_miller5(x, T.sh, T.mil, T.extra, T.f);
  return coop_final_exp_is_one(x, T.sh, T.fin, T.f);
}

struct HostKey {
  std::vector<G1Affine> K;
  std::vector<LineStep> t[5];
  VerifyKeyDev h;
  RlcKeyDev rk;
  bool load(const std::vector<uint8_t>& vk) {
    if (vk.size() < 580) return false;
    const uint32_t nk = be32_at(vk.data() + 576);
    size_t off = 580;
    if (nk < 2 || nk > RLC_MAX_NK || vk.size() != off + (size_t)nk * 64 + 12 + 256) return false;
    K.resize(nk);
    for (uint32_t i = 0; i < nk; i++) K[i] = g1_from_raw_hd(vk.data() + off + 64 * (size_t)i);
    off += (size_t)nk * 64 + 12;
    const G1Affine alpha1 = g1_from_raw_hd(vk.data());
    const G2Affine beta2 = g2_from_raw_hd(vk.data() + 128);
    const G2Affine q[5] = {g2_from_raw_hd(vk.data() + 256), g2_from_raw_hd(vk.data() + 448), g2_from_raw_hd(vk.data() + off),
                           g2_from_raw_hd(vk.data() + off + 128), beta2};
    for (int k = 0; k < 5; k++) t[k] = build_line_table(q[k]);
    h.pc = make_pairing_fast_consts();
    for (int k = 0; k < 4; k++) h.tab[k] = t[k].data();
    h.e_alpha_beta = f12_from(miller_loop(alpha1.neg(), beta2));
    h.twist_b = twist_b();
    h.K = K.data();
    h.nk = nk;
    rk.tab_beta = t[4].data();
    rk.neg_alpha = alpha1.neg();
    return true;
  }
};

static std::vector<uint8_t> slurp(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) return v;
  int c;
  while ((c = fgetc(f)) != EOF) v.push_back((uint8_t)c);
  fclose(f);
  return v;
}

static int pipeline(const char* vkp, const char* batchp, const char* seedhex, uint32_t group, uint32_t flags) {
  HostKey key;
  const std::vector<uint8_t> batch = slurp(batchp);
  if (!key.load(slurp(vkp)) || strlen(seedhex) != 64 || group < 64 || group % 64) { printf("RLC bad-arguments\n"); return 2; }
  const size_t pw_len = 12 + 32 * (size_t)(key.h.nk - 2), rec = 388 + pw_len;
  if (batch.size() % rec) { printf("RLC bad-batch\n"); return 2; }
  const size_t count = batch.size() / rec;
  uint8_t seed[32];
  for (int i = 0; i < 32; i++) { char b[3] = {seedhex[2 * i], seedhex[2 * i + 1], 0}; seed[i] = (uint8_t)strtoul(b, nullptr, 16); }
  const uint32_t ne = rlc_elems(key.h.nk);
  std::vector<W256> ws((size_t)ne * count), folded(ne);
  std::vector<uint32_t> live(count);
  std::vector<int> ok(count, 0);
  uint32_t stats[4] = {0, 0, 0, 0};
  for (size_t i = 0; i < count; i++) {
    live[i] = rlc_term(key.h, batch.data() + i * rec, batch.data() + i * rec + 388, seed, (uint32_t)i, ws.data() + i, count) ? 1 : 0;
    stats[3] += !live[i];
  }
  bool agree = true;
  Tail* T = new Tail;
  for (size_t first = 0; first < count; first += group) {
    const size_t n = count - first < group ? count - first : group;
    stats[0]++;
    size_t n_live = 0;
    for (size_t i = first; i < first + n; i++) n_live += live[i];
    if (!n_live) continue;
    rlc_fold(key.h, ws.data(), count, live.data(), first, n, folded.data());
    const bool serial = rlc_final_serial(key.h, key.rk, folded.data());
    const bool coop = coop_tail(key.h, key.rk, folded.data(), *T);
    agree = agree && serial == coop;
    const bool accept = (flags & 1) ? serial : coop;
    if (!accept) stats[1]++;
    for (size_t i = first; i < first + n; i++) {
      if (!live[i]) continue;
      if (accept) ok[i] = 1;
      else if (!(flags & 2)) { ok[i] = verify_one(key.h, batch.data() + i * rec, batch.data() + i * rec + 388) ? 1 : 0; stats[2]++; }
    }
  }
  delete T;
  std::string v;
  for (size_t i = 0; i < count; i++) v += ok[i] ? '1' : '0';
  printf("VERDICTS %s\nSTATS %u %u %u %u\nTAILS %s\n", v.c_str(), stats[0], stats[1], stats[2], stats[3], agree ? "agree" : "DISAGREE");
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 5) return pipeline(argv[1], argv[2], argv[3], (uint32_t)strtoul(argv[4], nullptr, 10), argc > 5 ? (uint32_t)strtoul(argv[5], nullptr, 10) : 0);
  CHECK(pairing_fast_consts_consistent(), "Frobenius sparsity");
  const PairingFastConsts pc = make_pairing_fast_consts();
  CoopEmu x;
  Tail* T = new Tail;
  CoopShared& sh = T->sh;
  sh.cc = make_coop_consts(pc);
  CHECK(sh.cc.k242 == Fq::from_u64(242) && sh.cc.k1476 == Fq::from_u64(1476), "fold constants");

  // inputs: random elements, and 0, 1, p-1 in every coefficient (and against a random element)
  std::vector<F12> ins;
  const Fq ext[3] = {Fq::zero(), Fq::one(), Fq::one().neg()};
  for (int e = 0; e < 3; e++) { F12 a; for (int i = 0; i < 12; i++) a.c[i] = ext[e]; ins.push_back(a); }
  { F12 a; for (int i = 0; i < 12; i++) a.c[i] = ext[i % 3]; ins.push_back(a); }
  ins.push_back(f12_one(pc));
  for (int k = 0; k < 4; k++) { F12 a; for (int i = 0; i < 12; i++) a.c[i] = fq_rand(); ins.push_back(a); }
  F12 out, out2;
  for (const F12& a : ins) {
    for (const F12& b : ins) {
      coop_f12_mul(x, sh, a, b, out);
      CHECK(f12_eq(out, f12_mul(a, b, pc)), "coop f12_mul");
    }
    out = a;
    coop_f12_mul(x, sh, out, out, out);                       // in place, as the squarings of the loops run it
    CHECK(f12_eq(out, f12_mul(a, a, pc)), "coop f12_mul in place");
    coop_f12_frob(x, sh, a, out);
    CHECK(f12_eq(out, f12_frob(a, pc)), "coop f12_frob");
    out = a;
    coop_f12_conj6(x, out);
    CHECK(f12_eq(out, f12_conj6(a)), "coop f12_conj6");
    for (int t = 0; t < 5; t++) {                              // lines: extremal coefficients, then random ones
      Fq l[6];
      for (int i = 0; i < 6; i++) l[i] = t < 3 ? ext[t] : t == 3 ? ext[(i + 1) % 3] : fq_rand();
      coop_f12_mul_line(x, sh, a, l, out);
      CHECK(f12_eq(out, f12_mul_line(a, l[0], l[1], l[2], l[3], l[4], l[5], pc)), "coop f12_mul_line");
      out2 = a;
      coop_f12_mul_line(x, sh, out2, l, out2);
      CHECK(f12_eq(out2, out), "coop f12_mul_line in place");
    }
  }
  for (size_t k = 0; k < ins.size(); k++) {                    // pow_x: 0, 1, p-1 everywhere, mixed, one, two random
    if (k >= 7) break;
    coop_f12_pow_x(x, sh, ins[k], out);
    CHECK(f12_eq(out, f12_pow_x(ins[k], pc)), "coop f12_pow_x");
  }

  // the five-table Miller loop and the final exponentiation, on products that are one by bilinearity and on ones that are not
  G1Affine G1{Fq::one(), Fq::one().dbl()};
  G2Affine G2{{fq_hex("1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed"),
               fq_hex("198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2")},
              {fq_hex("12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa"),
               fq_hex("090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b")}};
  for (int trial = 0; trial < 3; trial++) {
    // e(aP, q0 Q) e(bP, q1 Q) e(cP, q2 Q) e(dP, q3 Q) e(-(a q0 + b q1 + c q2 + d q3) P, Q) * extra, extra = miller(eP, Q) * miller(-eP, Q)
    uint32_t s[9][8];
    for (auto& k : s) for (int j = 0; j < 8; j++) k[j] = j < 2 ? rnd32() : 0;
    Fr sum = Fr::zero();
    for (int k = 0; k < 4; k++) sum = sum + Fr::from_canonical(s[k]) * Fr::from_canonical(s[4 + k]);
    uint32_t sl[8];
    sum.to_canonical(sl);
    std::vector<LineStep> tab[5];
    G1Affine Ps[5];
    for (int k = 0; k < 4; k++) {
      Ps[k] = scalar_mul(G1, s[k]).to_affine();
      tab[k] = build_line_table(scalar_mul(G2, s[4 + k]).to_affine());
    }
    Ps[4] = scalar_mul(G1, sl).to_affine().neg();
    tab[4] = build_line_table(G2);
    if (trial == 1) Ps[2] = G1Affine::infinity();              // a pair at infinity contributes 1: the product is no longer one
    const LineStep* tabs[5] = {tab[0].data(), tab[1].data(), tab[2].data(), tab[3].data(), tab[4].data()};
    const G1Affine eP = scalar_mul(G1, s[8]).to_affine();
    const F12 extra = trial == 2 ? f12_from(miller_loop(eP, G2)) : f12_mul(f12_from(miller_loop(eP, G2)), f12_from(miller_loop(eP.neg(), G2)), pc);
    const F12 want = miller_multi(5, tabs, Ps, false, G1Affine::infinity(), G2Affine::infinity(), extra, pc);
    for (int k = 0; k < 5; k++) { T->mil.tab[k] = tabs[k]; T->mil.P[k] = Ps[k]; }
    T->extra = extra;
    coop_miller5(x, sh, T->mil, T->extra, T->f);
    CHECK(f12_eq(T->f, want), "coop five-table Miller loop");
    const bool one = final_exp_is_one(want, pc);
    CHECK(one == (trial == 0), "one-lane final exponentiation");
    CHECK(coop_final_exp_is_one(x, sh, T->fin, T->f) == one, "coop final_exp_is_one");
  }
  for (int k = 0; k < 3; k++) {                                // extremal inputs: 0 (0^-1 = 0 must not pass), 1, p-1 everywhere
    CHECK(coop_final_exp_is_one(x, sh, T->fin, ins[k]) == final_exp_is_one(ins[k], pc), "coop final_exp_is_one, extremal");
  }
  CHECK(coop_final_exp_is_one(x, sh, T->fin, ins[4]), "coop final_exp_is_one(1)");
  delete T;
  printf("OK %d\n", checks);
  return 0;
}
