// csrc/ptau.hpp on the host: the transcript's layout, the scalar-per-point loop that k_g1_mul_each and k_g2_mul_each run, the G2 point
// check, the scalar range test, the butterfly and the stages of the group inverse NTT, the signed-coefficient rule and the column
// gather with its planner, driven by the caller's values (tests/test_ptau_host.py).
//   g++ -O1 -std=c++17 -fsanitize=address,undefined -I csrc -I include tests/host/ec_ntt_check.cpp -o ec_ntt_check
//   ./ec_ntt_check layout file        -> "LAYOUT ok log n n_t1 t1 t2 a1 b1 beta2 size" (ok = 0: not a transcript, the rest zero)
//   ./ec_ntt_check mul in.txt         per line "group scalar point" (group 1: 64 B point, 2: 128 B point, hex)
//                                     -> per line "PT flag hex": the flag of the point check, scalar * point by pt_mul_each
//   ./ec_ntt_check scalar k...        (hex, 64 digits) -> per scalar "SCALAR 0|1" (pt_scalar_ok)
//   ./ec_ntt_check bfly in.txt        per line "group a b tw" (a, b raw affine points, tw a scalar; tw = 1 takes the no-product path)
//                                     -> per line "BF sum diff": pt_bfly_sum and pt_bfly_diff, what a lane of k_ec_ntt_pass computes
//   ./ec_ntt_check intt in.txt        line 1 "logn", then 2^logn raw points -> per output "PT hex": the stages and the finish
//                                     in the kernels' index order (pt_bfly_index, pt_bitrev, pt_ntt_finish); then n / 2 twiddles w^-j and 1 / n
//   ./ec_ntt_check coeff c...         (hex) -> per coefficient "COEFF bits neg magnitude" (pt_signed_coeff)
//   ./ec_ntt_check gather in.txt      line 1 "nbases ncoef ncols nentries", then the G1 bases, the coefficients, "col row coeff" entries
//                                     -> "PLAN 0" when col_plan refuses, else "PLAN 1 | terms | chunk_ptr | col_ptr" and per column
//                                     "COL hex" by pt_gather_chunk and pt_gather_combine
//   ./ec_ntt_check gather2 in.txt     the same over Fq2, the instance the G2 gather compiles: the bases are 128 B G2 points
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ptau.hpp"

using namespace spp;

static bool unhex(const char* s, std::vector<uint8_t>& out) {
  const size_t n = strlen(s);
  if (n % 2) return false;
  out.resize(n / 2);
  for (size_t i = 0; i < n / 2; i++) {
    unsigned v;
    if (sscanf(s + 2 * i, "%2x", &v) != 1) return false;
    out[i] = (uint8_t)v;
  }
  return true;
}
static void limbs_of(const uint8_t be[32], uint32_t k[8]) {
  for (int i = 0; i < 8; i++) k[7 - i] = sc_load_be32(be + 4 * i);
}
static void print_fq(const Fq& v) {
  uint8_t b[32];
  v.to_bytes_be(b);
  for (int i = 0; i < 32; i++) printf("%02x", b[i]);
}
static void print_g1(const Affine<Fq>& r) {
  if (r.is_inf()) { printf("%0128x", 0); return; }
  print_fq(r.x); print_fq(r.y);
}
static void print_g2(const Affine<Fq2>& r) {
  if (r.is_inf()) { printf("%0256x", 0); return; }
  print_fq(r.x.c1); print_fq(r.x.c0); print_fq(r.y.c1); print_fq(r.y.c0);
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

// one raw base of a gather file: 64 B in G1, 128 B in G2 (on the curve; the subgroup is the caller's business)
static bool decode_base(const std::vector<uint8_t>& raw, Affine<Fq>* p) { return raw.size() == 64 && sc_decode_point(raw.data(), p) != SC_POINT_BAD; }
static bool decode_base(const std::vector<uint8_t>& raw, Affine<Fq2>* p) {
  const Fq2 twist_b = Fq2{Fq::from_u64(3), Fq::zero()} * Fq2{Fq::from_u64(9), Fq::one()}.inv();
  return raw.size() == 128 && pt_decode_g2(raw.data(), twist_b, p) != SC_POINT_BAD;
}
static void print_point(const Affine<Fq>& r) { print_g1(r); }
static void print_point(const Affine<Fq2>& r) { print_g2(r); }
// the modes gather (F = Fq) and gather2 (F = Fq2): the planner, then the text of k_col_gather<F> and k_col_combine<F>
template <class F>
static int run_gather(FILE* f) {
  unsigned nbases, ncoef, ncols, nentries;
  if (fscanf(f, "%u %u %u %u", &nbases, &ncoef, &ncols, &nentries) != 4) return 2;
  static char sp[300];
  std::vector<Affine<F>> bases(nbases);
  std::vector<uint32_t> mags((size_t)8 * ncoef), meta(ncoef);
  for (unsigned i = 0; i < nbases; i++) {
    std::vector<uint8_t> raw;
    if (fscanf(f, "%299s", sp) != 1 || !unhex(sp, raw) || !decode_base(raw, &bases[i])) return 2;
  }
  for (unsigned i = 0; i < ncoef; i++) {
    std::vector<uint8_t> kb;
    uint32_t c[8];
    if (fscanf(f, "%299s", sp) != 1 || !unhex(sp, kb) || kb.size() != 32) return 2;
    limbs_of(kb.data(), c);
    meta[i] = pt_signed_coeff(c, &mags[(size_t)8 * i]);
  }
  std::vector<ColEntry> entries(nentries);
  for (auto& e : entries)
    if (fscanf(f, "%u %u %u", &e.col, &e.row, &e.coeff) != 3) return 2;
  ColPlan plan;
  if (!col_plan(ncols, nbases, ncoef, entries, &plan)) { printf("PLAN 0\n"); return 0; }
  printf("PLAN 1 |");
  for (uint32_t v : plan.terms) printf(" %u", v);
  printf(" |");
  for (uint32_t v : plan.chunk_ptr) printf(" %u", v);
  printf(" |");
  for (uint32_t v : plan.col_ptr) printf(" %u", v);
  printf("\n");
  std::vector<XYZZ<F>> partial(plan.chunk_ptr.size() - 1);
  for (size_t c = 0; c + 1 < plan.chunk_ptr.size(); c++)
    partial[c] = pt_gather_chunk(bases.data(), plan.terms.data(), plan.chunk_ptr[c], plan.chunk_ptr[c + 1], mags.data(), meta.data());
  for (uint32_t j = 0; j < ncols; j++) {
    printf("COL ");
    print_point(pt_gather_combine(partial.data(), plan.col_ptr[j], plan.col_ptr[j + 1]));
    printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "layout")) {
    std::vector<uint8_t> b;
    if (!slurp(argv[2], b)) return 2;
    PtauLayout L;
    if (!ptau_layout(b.data(), b.size(), &L)) L = PtauLayout{};
    printf("LAYOUT %d %u %u %u %zu %zu %zu %zu %zu %zu\n", L.size ? 1 : 0, L.log, L.n, L.n_t1, L.t1, L.t2, L.a1, L.b1, L.beta2, L.size);
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "mul")) {
    FILE* f = fopen(argv[2], "r");
    if (!f) return 2;
    const Fq2 twist_b = Fq2{Fq::from_u64(3), Fq::zero()} * Fq2{Fq::from_u64(9), Fq::one()}.inv();
    static char sg[8], sk[80], sp[300];
    while (fscanf(f, "%7s %79s %299s", sg, sk, sp) == 3) {
      std::vector<uint8_t> kb, raw;
      uint32_t k[8];
      if (!unhex(sk, kb) || kb.size() != 32 || !unhex(sp, raw)) return 2;
      limbs_of(kb.data(), k);
      if (!strcmp(sg, "1") && raw.size() == 64) {
        Affine<Fq> p;
        const uint32_t flag = sc_decode_point(raw.data(), &p);
        const Affine<Fq> r = pt_mul_each(p, k).to_affine();
        printf("PT %u ", flag);
        if (r.is_inf()) printf("%0128x", 0);
        else { print_fq(r.x); print_fq(r.y); }
      } else if (!strcmp(sg, "2") && raw.size() == 128) {
        Affine<Fq2> p;
        const uint32_t flag = pt_decode_g2(raw.data(), twist_b, &p);
        const Affine<Fq2> r = pt_mul_each(p, k).to_affine();
        printf("PT %u ", flag);
        if (r.is_inf()) printf("%0256x", 0);
        else { print_fq(r.x.c1); print_fq(r.x.c0); print_fq(r.y.c1); print_fq(r.y.c0); }
      } else {
        return 2;
      }
      printf("\n");
    }
    fclose(f);
    return 0;
  }
  if (argc >= 3 && !strcmp(argv[1], "scalar")) {
    for (int a = 2; a < argc; a++) {
      std::vector<uint8_t> kb;
      uint32_t k[8];
      if (!unhex(argv[a], kb) || kb.size() != 32) return 2;
      limbs_of(kb.data(), k);
      printf("SCALAR %d\n", pt_scalar_ok(k) ? 1 : 0);
    }
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "bfly")) {
    FILE* f = fopen(argv[2], "r");
    if (!f) return 2;
    const Fq2 twist_b = Fq2{Fq::from_u64(3), Fq::zero()} * Fq2{Fq::from_u64(9), Fq::one()}.inv();
    static char sg[8], sa[300], sb[300], st[80];
    while (fscanf(f, "%7s %299s %299s %79s", sg, sa, sb, st) == 4) {
      std::vector<uint8_t> ra, rb, tb;
      uint32_t tw[8];
      if (!unhex(sa, ra) || !unhex(sb, rb) || !unhex(st, tb) || tb.size() != 32) return 2;
      limbs_of(tb.data(), tw);
      bool one = tw[0] == 1;
      for (int i = 1; i < 8; i++) one = one && tw[i] == 0;
      printf("BF ");
      if (!strcmp(sg, "1") && ra.size() == 64 && rb.size() == 64) {
        Affine<Fq> a, b;
        if (sc_decode_point(ra.data(), &a) == SC_POINT_BAD || sc_decode_point(rb.data(), &b) == SC_POINT_BAD) return 2;
        const XYZZ<Fq> xa = XYZZ<Fq>::from_affine(a), xb = XYZZ<Fq>::from_affine(b);
        print_g1(pt_bfly_sum(xa, xb).to_affine());
        printf(" ");
        print_g1(pt_bfly_diff(xa, xb, tw, one).to_affine());
      } else if (!strcmp(sg, "2") && ra.size() == 128 && rb.size() == 128) {
        Affine<Fq2> a, b;
        if (pt_decode_g2(ra.data(), twist_b, &a) == SC_POINT_BAD || pt_decode_g2(rb.data(), twist_b, &b) == SC_POINT_BAD) return 2;
        const XYZZ<Fq2> xa = XYZZ<Fq2>::from_affine(a), xb = XYZZ<Fq2>::from_affine(b);
        print_g2(pt_bfly_sum(xa, xb).to_affine());
        printf(" ");
        print_g2(pt_bfly_diff(xa, xb, tw, one).to_affine());
      } else {
        return 2;
      }
      printf("\n");
    }
    fclose(f);
    return 0;
  }
  if (argc >= 3 && !strcmp(argv[1], "coeff")) {
    for (int a = 2; a < argc; a++) {
      std::vector<uint8_t> kb;
      uint32_t c[8], mag[8];
      if (!unhex(argv[a], kb) || kb.size() != 32) return 2;
      limbs_of(kb.data(), c);
      const uint32_t meta = pt_signed_coeff(c, mag);
      printf("COEFF %u %u ", meta & 0x1ffu, meta >> 31);
      for (int i = 7; i >= 0; i--) printf("%08x", mag[i]);
      printf("\n");
    }
    return 0;
  }
  if (argc == 3 && (!strcmp(argv[1], "gather") || !strcmp(argv[1], "gather2"))) {
    FILE* f = fopen(argv[2], "r");
    if (!f) return 2;
    const int rc = strcmp(argv[1], "gather") ? run_gather<Fq2>(f) : run_gather<Fq>(f);
    fclose(f);
    return rc;
  }
  if (argc == 3 && !strcmp(argv[1], "intt")) {
    FILE* f = fopen(argv[2], "r");
    if (!f) return 2;
    unsigned logn;
    static char sp[300];
    if (fscanf(f, "%u", &logn) != 1 || logn == 0 || logn > 10) return 2;
    const uint32_t n = 1u << logn;
    std::vector<XYZZ<Fq>> buf[2] = {std::vector<XYZZ<Fq>>(n), std::vector<XYZZ<Fq>>(n)};
    for (uint32_t i = 0; i < n; i++) {
      std::vector<uint8_t> raw;
      Affine<Fq> p;
      if (fscanf(f, "%299s", sp) != 1 || !unhex(sp, raw) || raw.size() != 64 || sc_decode_point(raw.data(), &p) == SC_POINT_BAD) return 2;
      buf[1][i] = XYZZ<Fq>::from_affine(p);
    }
    std::vector<uint32_t> tw((size_t)8 * (n / 2));
    for (uint32_t j = 0; j < n / 2; j++) {
      std::vector<uint8_t> kb;
      if (fscanf(f, "%299s", sp) != 1 || !unhex(sp, kb) || kb.size() != 32) return 2;
      limbs_of(kb.data(), &tw[(size_t)8 * j]);
    }
    std::vector<uint8_t> nb;
    uint32_t ninv[8];
    if (fscanf(f, "%299s", sp) != 1 || !unhex(sp, nb) || nb.size() != 32) return 2;
    fclose(f);
    limbs_of(nb.data(), ninv);
    int8_t dig[SC_MAX_DIGITS];
    const uint32_t len = sc_naf_recode(ninv, dig);
    for (uint32_t s = 0; s < logn; s++) {           // stage s reads buf[(s + 1) & 1] and writes buf[s & 1], as launch_ec_intt
      const std::vector<XYZZ<Fq>>& src = buf[(s + 1) & 1];
      std::vector<XYZZ<Fq>>& dst = buf[s & 1];
      for (uint32_t u = 0; u < n / 2; u++) {
        uint32_t i0, i1, e;
        pt_bfly_index(u, logn, s, &i0, &i1, &e);
        dst[i0] = pt_bfly_sum(src[i0], src[i1]);
        dst[i1] = pt_bfly_diff(src[i0], src[i1], &tw[(size_t)8 * e], e == 0);
      }
    }
    std::vector<Affine<Fq>> out(n);
    for (uint32_t t = 0; t < n; t++) out[pt_bitrev(t, logn)] = pt_ntt_finish(buf[(logn - 1) & 1][t], dig, len);
    for (uint32_t k = 0; k < n; k++) { printf("PT "); print_g1(out[k]); printf("\n"); }
    return 0;
  }
  fprintf(stderr, "usage: ec_ntt_check layout|mul|scalar|bfly|intt|coeff|gather|gather2 ...\n");
  return 2;
}
