// Test-only host twin of spp_debug_arith: the dispatch of csrc/arith_probe.hpp -- the very function the gfx950 probe kernels
// call -- built with g++ and run on the operand words tests/arith_vectors.py generates.  It only loads, calls and stores; the
// results go back to Python, which judges them against big integers (tests/test_arith_raw_host.py).
//   usage: arith_raw_check <in.bin> <out.bin>
//   in.bin : u32 magic, u32 batches; per batch u32 selector, arg, n, in_words, out_words, then n * in_words operand words
//   out.bin: per batch n * out_words result words
// Prints one line per batch "<field> <operation> arg <arg> cases <n>", for the inverse also how many cases PROVABLY enter the
// zero-low-word branch of strip() (x[0] == 0: the shift by 31) -- counted here from the operand words, with nothing compiled into
// the header: the canonical word is a non-zero multiple of 2^32 (the strip of v before the loop meets it), or it is p - 2^k with
// k >= 32 (v is odd, the first difference u - v = 2^k is stripped) -- and "OK <cases>" at the end.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "arith_probe.hpp"
using namespace spp;

static const char* op_name(uint32_t code) {
  switch (code) {
#define X(name, c, iw, ow, fq) \
  case c:                      \
    return #name;
    SPP_ARITH_OPS(X)
#undef X
  }
  return "?";
}

template <uint32_t OP, class Pm>
static void run(uint32_t arg, uint32_t n, uint32_t iw, uint32_t ow, const uint32_t* in, uint32_t* out) {
  for (uint32_t i = 0; i < n; i++) arith_probe_case<OP, Pm>(arg, in + (size_t)i * iw, out + (size_t)i * ow);
}
template <uint32_t OP, int FIELDS>
static void run_field(bool is_fq, uint32_t arg, uint32_t n, uint32_t iw, uint32_t ow, const uint32_t* in, uint32_t* out) {
  if (is_fq) {
    if constexpr (FIELDS != ARITH_FIELDS_FR) run<OP, FqParams>(arg, n, iw, ow, in, out);
  } else {
    if constexpr (FIELDS != ARITH_FIELDS_FQ) run<OP, FrParams>(arg, n, iw, ow, in, out);
  }
}

template <class Pm>
static bool enters_zero_low_word_branch(const uint32_t* w) {
  uint32_t c[8], d[8];
  for (int i = 0; i < 8; i++) c[i] = w[i];
  Fp<Pm>::cond_sub(c);
  uint32_t any = 0;
  for (int i = 0; i < 8; i++) any |= c[i];
  if (any && c[0] == 0) return true;
  uint32_t br = 0;
  for (int i = 0; i < 8; i++) d[i] = subb32(Pm::MOD(i), c[i], br);   // p - c > 0
  int bits = 0;
  for (int i = 0; i < 8; i++) bits += __builtin_popcount(d[i]);
  return (c[0] & 1u) && bits == 1 && d[0] == 0;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  FILE* g = fopen(argv[2], "wb");
  if (!f || !g) return 2;
  uint32_t head[2];
  if (fread(head, 4, 2, f) != 2 || head[0] != 0x31565241u) { printf("FAIL header\n"); return 1; }
  size_t total = 0;
  for (uint32_t b = 0; b < head[1]; b++) {
    uint32_t h[5];
    if (fread(h, 4, 5, f) != 5) { printf("FAIL batch header\n"); return 1; }
    const uint32_t selector = h[0], arg = h[1], n = h[2];
    uint32_t iw = 0, ow = 0;
    if (!arith_probe_shape(selector, &iw, &ow) || !arith_probe_arg_ok(selector, arg) || iw != h[3] || ow != h[4] || n == 0) {
      printf("FAIL batch %u: selector 0x%x arg %u words %u -> %u\n", b, selector, arg, h[3], h[4]);
      return 1;
    }
    std::vector<uint32_t> in((size_t)n * iw), out((size_t)n * ow, 0xdeadbeefu);
    if (fread(in.data(), 4, in.size(), f) != in.size()) { printf("FAIL batch %u: short read\n", b); return 1; }
    const bool is_fq = (selector & ARITH_FIELD_FQ) != 0;
    switch (selector & 0xffu) {
#define X(name, code, IW, OW, fq)                                             \
  case code:                                                                  \
    run_field<code, fq>(is_fq, arg, n, iw, ow, in.data(), out.data());        \
    break;
      SPP_ARITH_OPS(X)
#undef X
    }
    fwrite(out.data(), 4, out.size(), g);
    printf("%s %s arg %u cases %u\n", is_fq ? "fq" : "fr", op_name(selector & 0xffu), arg, n);
    if ((selector & 0xffu) == ARITH_FP_INV) {
      uint32_t z = 0;
      for (uint32_t i = 0; i < n; i++)
        z += is_fq ? enters_zero_low_word_branch<FqParams>(&in[(size_t)i * iw]) : enters_zero_low_word_branch<FrParams>(&in[(size_t)i * iw]);
      printf("%s FP_INV zero_low_word_branch %u\n", is_fq ? "fq" : "fr", z);
    }
    total += n;
  }
  fclose(f);
  fclose(g);
  printf("OK %zu\n", total);
  return 0;
}
