// Range class of every wire of a circuit, read off its solver program (msm_ragged.hpp: what the classes are for).  Host only:
// circuit.hpp and the standard library, so a host compiler can test it against the circuit builders.
//   * outputs of OP_BITS: bound 1; outputs of OP_LIMBS8: bound 255.  The solver writes these wires itself, whatever the input.
//   * a wire that a looked-up value of an OP_COUNT8 range check names alone, plus a constant cst (byte_ranged_lookup): values in
//     [-cst, 255 - cst].  These may be prover inputs: the bound holds for every row that passes the satisfaction check, and a row
//     that does not is refused through its status word -- the table walk only has to stay inside the table for it (k_msm_flat).
// Everything else is wide, and so is any wire of a program with instructions this scan does not know.
#pragma once
#include "circuit.hpp"
#include "msm_ragged.hpp"

namespace spp {

// signed small value (|v| < 2^30) of a field element, if it has one
inline bool fr_small_signed(const Fr& x, int64_t* out) {
  uint32_t v[8];
  x.to_canonical(v);
  bool hi0 = true;
  for (int k = 1; k < 8; k++) hi0 = hi0 && v[k] == 0;
  if (hi0 && v[0] < (1u << 30)) { *out = (int64_t)v[0]; return true; }
  x.neg().to_canonical(v);
  hi0 = true;
  for (int k = 1; k < 8; k++) hi0 = hi0 && v[k] == 0;
  if (hi0 && v[0] < (1u << 30)) { *out = -(int64_t)v[0]; return true; }
  return false;
}
// the looked-up value H_h of a circuit as (wire, cst), if it is byte-ranged
inline bool circuit_byte_ranged_lookup(const Circuit& circ, uint32_t h, uint32_t* wire, int64_t* cst) {
  if (h >= circ.H.rows()) return false;
  const Term* t = circ.H.terms.data();
  return byte_ranged_lookup(t + circ.H.rowptr[h], t + circ.H.rowptr[h + 1], [&](uint32_t ci, int64_t* v) { return fr_small_signed(circ.coeffs[ci], v); },
                            wire, cst);
}

enum : uint8_t { WIRE_WIDE = 0, WIRE_BIT = 1, WIRE_LIMB8 = 2, WIRE_LOOKUP = 3 };
struct WireClasses {
  std::vector<uint32_t> bound;   // per wire: bound on |signed value|, 0 = wide
  std::vector<uint8_t> kind;     // per wire: the rule that classified it first
};
inline WireClasses msm_wire_classes(const Circuit& circ) {
  WireClasses wc;
  wc.bound.assign(circ.n_wires, 0);
  wc.kind.assign(circ.n_wires, WIRE_WIDE);
  auto mark = [&](uint32_t w, uint32_t b, uint8_t kind) {
    if (w == 0 || w >= circ.n_wires) return;
    if (wc.kind[w] == WIRE_WIDE) wc.kind[w] = kind;
    narrow_wire(wc.bound, w, b);
  };
  const std::vector<uint32_t>& pr = circ.program;
  auto all_wide = [&]() {
    wc.bound.assign(circ.n_wires, 0);
    wc.kind.assign(circ.n_wires, WIRE_WIDE);
    return wc;
  };
  for (size_t pc = 0; pc < pr.size() && pr[pc] != OP_END;) {
    size_t len = 0;
    switch (pr[pc]) {
      case OP_SOLVE_C: case OP_SOLVE_A: case OP_MASK: len = 2; break;
      case OP_BATCH_DIV: case OP_POSEIDON2: case OP_INV_H: len = 3; break;
      case OP_COUNT8: case OP_BITS: case OP_LIMBS8: case OP_POSEIDON: len = 4; break;
      case OP_COMMIT: len = 1; break;
      case OP_GRUMPKIN: len = pc + 4 < pr.size() ? 5 + (size_t)pr[pc + 4] : 0; break;
      default: return all_wide();   // the solver of a decoded gnark system, or a malformed program: no classes
    }
    if (len == 0 || pc + len > pr.size()) return all_wide();
    if (pr[pc] == OP_BITS)
      for (uint32_t i = 0; i < pr[pc + 2]; i++) mark(pr[pc + 3] + i, 1, WIRE_BIT);
    if (pr[pc] == OP_LIMBS8)
      for (uint32_t i = 0; i < pr[pc + 2]; i++) mark(pr[pc + 3] + i, 255, WIRE_LIMB8);
    if (pr[pc] == OP_COUNT8)
      for (uint32_t i = 0; i < pr[pc + 2]; i++) {
        uint32_t w;
        int64_t cst;
        if (circuit_byte_ranged_lookup(circ, pr[pc + 1] + i, &w, &cst)) mark(w, byte_ranged_bound(cst), WIRE_LOOKUP);
      }
    pc += len;
  }
  return wc;
}
// class of the bases of a set whose base i carries the scalar of row rows[i] (rows >= n_wires: blinding rows, wide)
inline std::vector<uint32_t> msm_base_bounds(const WireClasses& wc, const std::vector<uint32_t>& rows) {
  std::vector<uint32_t> b(rows.size(), 0);
  for (size_t i = 0; i < rows.size(); i++)
    if (rows[i] < wc.bound.size()) b[i] = wc.bound[rows[i]];
  return b;
}

}  // namespace spp
