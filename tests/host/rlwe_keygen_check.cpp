// Host check of csrc/rlwe_keygen.hpp: the per-lane phases of k_rlwe_keygen and k_rlwe_key_noise (exactly the functions the kernels
// run on the GPU, with the passes of rlwe_ntt.hpp between them) executed lane by lane on the host, against the schoolbook
// negacyclic product of the reference (scripts/rlwe_keygen.py:32-42,104-116).
//   g++ -O2 -std=c++17 -I <csrc> rlwe_keygen_check.cpp && ./a.out [key.txt]
// key.txt (optional): 4 x 1024 integers, sk (signed), a, e (signed), and the b the reference wrote for them.
// Every value a phase leaves in a lane is tracked; the largest magnitude is printed and must stay below 2^31.  Sums INSIDE a phase
// are covered by the bound rlwe_ntt_check.cpp derives for rn_dft16 (inputs in (-p, p), which every phase here delivers) and by the
// build of this file with -fsanitize=undefined, which traps a signed overflow anywhere.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rlwe_keygen.hpp"
using namespace spp;

static RnHostTables T;
static long long max_abs;            // largest |value| any lane held after a phase
static long long max_abs_unit;       // ... among the values that must be in (-p, p): inputs of rn_dft16 and of the final steps
struct Wave {
  int32_t x[64][16];
  int32_t lds[RN_LDS_WORDS];
};
static void track(const Wave& w, bool unit) {
  for (int l = 0; l < 64; l++)
    for (int j = 0; j < 16; j++) {
      const long long a = w.x[l][j] < 0 ? -(long long)w.x[l][j] : w.x[l][j];
      if (a > max_abs) max_abs = a;
      if (unit && a > max_abs_unit) max_abs_unit = a;
    }
}
// rn_ntt1<true> of kernels_witness.hip: the loops over l stand for the 64 lanes between two barriers
static void ntt(Wave& w, int dir) {
  const RnField& f = T.f[0];
  for (uint32_t l = 0; l < 64; l++) rn_pass1<true>(l, w.x[l], w.lds, f, T.w[0][dir], dir);
  track(w, false);
  for (uint32_t l = 0; l < 64; l++) rn_pass2_read(l, w.x[l], w.lds);
  track(w, true);                    // what pass 1 wrote to LDS: fresh products
  for (uint32_t l = 0; l < 64; l++) rn_pass2<true>(l, w.x[l], w.lds, f, T.w[0][dir], dir);
  track(w, false);
  for (uint32_t l = 0; l < 64; l++) rn_pass3(l, w.x[l], w.lds, f, dir);
  track(w, false);
}
// rk_negacyclic of kernels_witness.hip: A <- a * s, s any int32 per coefficient
static void negacyclic(Wave& A, Wave& S) {
  const RnField& f = T.f[0];
  for (uint32_t l = 0; l < 64; l++) { rk_twist(l, A.x[l], T.psi[0], f); rk_twist(l, S.x[l], T.psi[0], f); }
  track(A, true); track(S, true);
  ntt(A, 0);
  ntt(S, 0);
  for (uint32_t l = 0; l < 64; l++) rk_pointwise(A.x[l], S.x[l], T.pk_scale[0], f);
  track(A, true);
  ntt(A, 1);
  for (uint32_t l = 0; l < 64; l++) rk_twist(l, A.x[l], T.ipsi[0], f);
  track(A, true);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 11); }

static int bad = 0;
static const long long Q = RN_P[0];

// one key through both kernels' phases; expect_b (optional): what b must be
static void run_case(const char* name, const std::vector<int>& sk, const std::vector<uint32_t>& a, const std::vector<int>& e,
                     const std::vector<uint32_t>* expect_b) {
  const RnField& f = T.f[0];
  // schoolbook: prod = a * sk mod (X^1024 + 1), signed sk: |terms| < 2^28 * 2^7, |sums| < 2^45
  std::vector<long long> prod(1024, 0);
  for (int i = 0; i < 1024; i++)
    for (int j = 0; j < 1024; j++) {
      const long long t = (long long)a[i] * sk[j];
      if (i + j < 1024) prod[i + j] += t; else prod[i + j - 1024] -= t;
    }
  static Wave A, S;
  // ---- k_rlwe_keygen ----
  std::vector<uint32_t> b(1024), skq(1024);
  for (uint32_t l = 0; l < 64; l++)
    for (int j = 0; j < 16; j++) {
      const uint32_t i = l + 64 * j;
      A.x[l][j] = (int32_t)a[i];
      S.x[l][j] = sk[i];
      skq[i] = (uint32_t)rn_canon(sk[i], f);
    }
  negacyclic(A, S);
  int mism = 0;
  for (uint32_t l = 0; l < 64; l++)
    for (int j = 0; j < 16; j++) {
      const uint32_t i = l + 64 * j;
      b[i] = rk_public_b(A.x[l][j], e[i], f);
      long long want = (e[i] - prod[i]) % Q;
      if (want < 0) want += Q;
      if ((long long)b[i] != want || (expect_b && b[i] != (*expect_b)[i])) {
        if (mism < 3) printf("MISMATCH %s: b[%u] = %u, schoolbook %lld%s\n", name, i, b[i], want, expect_b ? " (or the reference's b differs)" : "");
        mism++;
      }
      long long sq = sk[i] % Q;
      if (sq < 0) sq += Q;
      if ((long long)skq[i] != sq) mism++;
    }
  // ---- k_rlwe_key_noise on (a, b, sk mod q): the maxima must be max |e| and max |sk| ----
  for (uint32_t l = 0; l < 64; l++)
    for (int j = 0; j < 16; j++) {
      A.x[l][j] = (int32_t)a[l + 64 * j];
      S.x[l][j] = (int32_t)skq[l + 64 * j];
    }
  uint32_t msk = 0, mnoise = 0;
  for (int i = 0; i < 1024; i++) msk = rk_max(msk, rk_abs_centred(skq[i], f));
  negacyclic(A, S);
  for (uint32_t l = 0; l < 64; l++)
    for (int j = 0; j < 16; j++) {
      const uint32_t i = l + 64 * j;
      const uint32_t v = rk_noise(b[i], A.x[l][j], f);
      if ((long long)v != (e[i] < 0 ? -e[i] : e[i])) { if (mism < 3) printf("MISMATCH %s: noise[%u] = %u, e = %d\n", name, i, v, e[i]); mism++; }
      mnoise = rk_max(mnoise, v);
    }
  uint32_t want_sk = 0, want_e = 0;
  for (int i = 0; i < 1024; i++) {
    want_sk = std::max<uint32_t>(want_sk, (uint32_t)abs(sk[i]));
    want_e = std::max<uint32_t>(want_e, (uint32_t)abs(e[i]));
  }
  if (msk != want_sk || mnoise != want_e) { printf("MISMATCH %s: maxima %u %u, expected %u %u\n", name, mnoise, msk, want_e, want_sk); mism++; }
  // a key that is not the secret of (a, b): one coefficient of b moved by 1000 shows as 1000 +- |e|
  {
    const uint32_t moved = (uint32_t)((b[5] + 1000) % Q);
    const uint32_t v = rk_noise(moved, A.x[5][0], f);
    if (v != (uint32_t)abs(e[5] + 1000)) { printf("MISMATCH %s: moved b[5] shows %u\n", name, v); mism++; }
  }
  printf("%-28s %s\n", name, mism ? "FAIL" : "ok");
  bad += mism;
}

int main(int argc, char** argv) {
  rn_build_tables(T);
  std::vector<int> sk(1024), e(1024);
  std::vector<uint32_t> a(1024);
  auto fill = [&](auto fs, auto fa, auto fe) { for (int i = 0; i < 1024; i++) { sk[i] = fs(i); a[i] = fa(i); e[i] = fe(i); } };
  auto small = [](int) { return (int)(rnd() % 7) - 3; };
  auto unif = [](int) { return rnd() % (uint32_t)Q; };
  for (int k = 0; k < 3; k++) { fill(small, unif, small); run_case("random key", sk, a, e, nullptr); }
  fill([](int) { return 0; }, unif, small);                                         run_case("sk = 0", sk, a, e, nullptr);
  fill([](int) { return 3; }, [](int) { return (uint32_t)(Q - 1); }, small);       run_case("sk = +3, a = q - 1", sk, a, e, nullptr);
  fill([](int) { return -3; }, unif, small);                                        run_case("sk = -3", sk, a, e, nullptr);
  fill(small, [](int) { return 0u; }, small);                                       run_case("a = 0", sk, a, e, nullptr);
  fill([](int i) { return i == 1023 ? 1 : 0; }, unif, [](int) { return -3; });      run_case("sk = X^1023, e = -3", sk, a, e, nullptr);
  // the extremes of the int8 the kernel takes, beyond what a key uses
  fill([](int i) { return (i & 1) ? 127 : -128; }, [](int) { return (uint32_t)(Q - 1); }, [](int i) { return (i & 2) ? 127 : -128; });
  run_case("int8 extremes, a = q - 1", sk, a, e, nullptr);
  int ncases = 9;
  if (argc > 1) {
    FILE* fp = fopen(argv[1], "r");
    std::vector<uint32_t> want(1024);
    long long v;
    bool ok = fp != nullptr;
    for (int part = 0; ok && part < 4; part++)
      for (int i = 0; ok && i < 1024; i++) {
        ok = fscanf(fp, "%lld", &v) == 1;
        if (part == 0) sk[i] = (int)v; else if (part == 1) a[i] = (uint32_t)v; else if (part == 2) e[i] = (int)v; else want[i] = (uint32_t)v;
      }
    if (fp) fclose(fp);
    if (!ok) { printf("FAIL cannot read 4096 integers from %s\n", argv[1]); return 1; }
    run_case("the reference's key", sk, a, e, &want);
    ncases++;
  }
  if (T.pk_scale[0] < 0 || T.pk_scale[0] >= RN_P[0]) bad++;   // the multiplier bound of rn_mul
  printf("largest |intermediate| met: %lld = %.2f p (2^31 = %.2f p); where (-p, p) is required: %.4f p\n", max_abs, (double)max_abs / Q,
         2147483648.0 / Q, (double)max_abs_unit / Q);
  if (max_abs >= 2147483648ll) { printf("an intermediate reached 2^31\n"); bad++; }
  if (max_abs_unit >= Q) { printf("a value that must lie in (-p, p) does not\n"); bad++; }
  if (bad) { printf("FAIL %d\n", bad); return 1; }
  printf("OK rlwe_keygen: %d keys x 1024 coefficients, b, sk mod q and both maxima equal the schoolbook values\n", ncases);
  return 0;
}
