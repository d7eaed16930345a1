// The raw-word probe of the arithmetic headers on gfx950 (spp_debug_arith): one lane per case, block 64; the lane loads its
// operand words, calls one header function (arith_probe.hpp) and stores the result.  Test-only: nothing of the proving path is here.
#include "kernels.hpp"
#include "arith_probe.hpp"

namespace spp {

template <uint32_t OP, class Pm, uint32_t IW, uint32_t OW>
__global__ __launch_bounds__(64) void k_arith_probe(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n, uint32_t arg) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  arith_probe_case<OP, Pm>(arg, in + (size_t)i * IW, out + (size_t)i * OW);
}

// FIELDS: the fields an operation exists for (ARITH_FIELDS_*); arith_probe_shape has refused the others
template <uint32_t OP, uint32_t IW, uint32_t OW, int FIELDS>
static void launch_one(hipStream_t st, bool is_fq, uint32_t arg, const uint32_t* in, uint32_t* out, uint32_t n) {
  const dim3 grid((n + 63u) / 64u), block(64);
  if (is_fq) {
    if constexpr (FIELDS != ARITH_FIELDS_FR) k_arith_probe<OP, FqParams, IW, OW><<<grid, block, 0, st>>>(in, out, n, arg);
  } else {
    if constexpr (FIELDS != ARITH_FIELDS_FQ) k_arith_probe<OP, FrParams, IW, OW><<<grid, block, 0, st>>>(in, out, n, arg);
  }
}

// in: n * in_words, out: n * out_words device words (arith_probe_shape); false = unknown selector / arg, nothing launched
bool launch_arith_probe(hipStream_t st, uint32_t selector, uint32_t arg, const uint32_t* in, uint32_t* out, uint32_t n) {
  uint32_t iw = 0, ow = 0;
  if (n == 0 || !arith_probe_shape(selector, &iw, &ow) || !arith_probe_arg_ok(selector, arg)) return false;
  const bool is_fq = (selector & ARITH_FIELD_FQ) != 0;
  switch (selector & 0xffu) {
#define X(name, code, IW, OW, fq)                              \
  case code:                                                   \
    launch_one<code, IW, OW, fq>(st, is_fq, arg, in, out, n);      \
    return true;
    SPP_ARITH_OPS(X)
#undef X
  }
  return false;
}

}  // namespace spp
