// libspp, load-time planners: how the solver program and the constraint matrices of one circuit are laid out for the kernels
// (items of the cooperative solver, small and long rows of the matrix evaluation).  Host code that builds vectors from the
// Circuit and uploads them in its last lines; called once per circuit by load_circuit_impl (spp_load.cpp).
#include "spp_circuit.hpp"

// Item list of the cooperative solver (kernels_solve.hip, k_solve_coop) for every sequential stretch of the schedule: built by
// coop_build_plan (coop_plan.hpp), uploaded here.
int coop_plan(spp_circuit* c) {
  CoopPlan pl;
  if (!coop_build_plan(c->circ, c->schedule, c->sw.no_level_stream, &pl)) return fail(SPP_ERR_FORMAT, "bad opcode %u in solver program", pl.bad_opcode);
  for (uint32_t k = 0; k < COOP_KINDS; k++) c->coop_item_count[k] = pl.item_count[k];
  c->coop_stream_chunks = pl.stream_chunks;
  c->coop_generic_rows = pl.generic_rows;
  c->coop_generic_divs = pl.generic_divs;
  if (pl.items.empty()) pl.items.assign(3, 0);
  if (pl.par.empty()) pl.par.assign(2, 0);
  if (pl.lvl_rows.empty()) { pl.lvl_rows.push_back(0); pl.lvl_gen.assign(3, COOP_NONE); }
  if (pl.stream.empty()) pl.stream.assign(COOP_CHUNK, 0xffffffffu);
  uint32_t *d_items, *d_par, *d_lp, *d_lr, *d_lg, *d_ls;
  int e;
  if ((e = own_upload(c, &d_items, pl.items)) || (e = own_upload(c, &d_par, pl.par)) || (e = own_upload(c, &d_lp, pl.lvl_ptr)) ||
      (e = own_upload(c, &d_lr, pl.lvl_rows)) || (e = own_upload(c, &d_lg, pl.lvl_gen)) || (e = own_upload(c, &d_ls, pl.stream)))
    return e;
  c->coop.items = d_items; c->coop.par = d_par; c->coop.lvl_ptr = d_lp; c->coop.lvl_rows = d_lr; c->coop.lvl_gen = d_lg; c->coop.lvl_stream = d_ls;
  c->coop.generic = c->generic_solver ? 1u : 0u;
  return 0;
}

// Small rows of the matrix evaluation (DevCircuit::sm_*).  A wire is "byte-ranged" when one of the looked-up values of an OP_COUNT8
// range check is exactly that wire, or that wire plus a small constant: the log-derivative argument then holds only if the wire's
// value lies in [-c, 255 - c].  A row of A, B or C with at least SMALL_ROW_MIN terms, all of them (small integer coefficient) x
// (byte-ranged wire or the constant one), is evaluated in 64-bit integer arithmetic from an int16 copy of those wires: the audit
// circuit's 1 088 quotient equations (1 024 public-key coefficients each) are 1.13 M of the 1.8 M matrix terms of a proof, and
// re-read the same 1 024 witness rows 1 088 times -- 73 GB of L2 misses per 2 048-proof batch in the general kernel (20 ms,
// profiles/round2_audit_b2048_pmc_hbm.json); as integers over a 13 MB array they take well under a millisecond.
// SPP_NO_SMALL_ROWS=1 (diagnostic): off.
static constexpr uint32_t SMALL_ROW_MIN = 64, SMALL_ROW_REST = 32;
static int small_rows_plan(spp_circuit* c, std::vector<uint8_t>& flags_out) {
  const Circuit& circ = c->circ;
  c->dc.sm_nrows = 0;
  c->dc.sm_nslots = 0;
  c->dc.row_small = nullptr;
  if (getenv("SPP_NO_SMALL_ROWS")) return 0;
  auto small_of = [&](uint32_t ci, int64_t* out) { return fr_small_signed(circ.coeffs[ci], out); };
  std::vector<int32_t> slot_of(circ.n_wires, -1);
  std::vector<uint32_t> wires{0};
  std::vector<int32_t> lo{0};
  slot_of[0] = 0;   // the constant one
  for (const SolveStep& st : c->schedule) {
    if (st.kind != SolveStep::COUNT8) continue;
    for (uint32_t h = st.a; h < st.a + st.b && h < circ.H.rows(); h++) {
      uint32_t w = 0;
      int64_t cst = 0;
      if (!circuit_byte_ranged_lookup(circ, h, &w, &cst) || slot_of[w] >= 0) continue;   // msm_classes.hpp: the rule the range classes use
      slot_of[w] = (int32_t)wires.size();
      wires.push_back(w);
      lo.push_back((int32_t)-cst);
    }
  }
  if (wires.size() < 2) return 0;
  std::vector<uint32_t> rowptr{0}, slots, row_out, rest_ptr{0}, rest_wire, rest_coeff;
  std::vector<int32_t> coefs;
  std::vector<uint8_t> flags(std::max<uint32_t>(circ.n_constraints, 1), 0);
  const Sparse* mats[3] = {&circ.A, &circ.B, &circ.C};
  for (uint32_t mi = 0; mi < 3; mi++) {
    const Sparse& m = *mats[mi];
    for (uint32_t k = 0; k < circ.n_constraints; k++) {
      const uint32_t b = m.rowptr[k], e = m.rowptr[k + 1];
      if (e - b < SMALL_ROW_MIN || e - b > (1u << 20)) continue;
      // terms that qualify (small coefficient x byte-ranged wire) go to the integer sum, at most SMALL_ROW_REST others stay
      // field arithmetic (a quotient equation has nine: k * q and the eight message bits times Delta * 2^i)
      // ... and only while the integer sum cannot leave a signed 64-bit accumulator whatever the values: the sum of |coefficient| x
      // (largest magnitude the slot's range allows) stays below 2^63 (2^30 x 32 255 x 2^18 terms still does, twice that does not)
      uint32_t n_small = 0;
      uint64_t bound = 0;
      for (uint32_t t = b; t < e; t++) {
        int64_t v;
        if (slot_of[m.terms[t].wire] >= 0 && small_of(m.terms[t].coeff, &v)) {
          n_small++;
          const int64_t l = lo[slot_of[m.terms[t].wire]];
          const uint64_t mag = m.terms[t].wire == 0 ? 1 : (uint64_t)std::max(l < 0 ? -l : l, l + 255 < 0 ? -(l + 255) : l + 255);
          if (bound < (1ull << 63)) bound += (uint64_t)(v < 0 ? -v : v) * mag;   // each step adds less than 2^45
        }
      }
      if (n_small < SMALL_ROW_MIN || (e - b) - n_small > SMALL_ROW_REST || bound >= (1ull << 63)) continue;
      for (uint32_t t = b; t < e; t++) {
        int64_t v = 0;
        if (slot_of[m.terms[t].wire] >= 0 && small_of(m.terms[t].coeff, &v)) {
          slots.push_back((uint32_t)slot_of[m.terms[t].wire]);
          coefs.push_back((int32_t)v);
        } else {
          rest_wire.push_back(m.terms[t].wire);
          rest_coeff.push_back(m.terms[t].coeff);
        }
      }
      rowptr.push_back((uint32_t)slots.size());
      rest_ptr.push_back((uint32_t)rest_wire.size());
      row_out.push_back((mi << 30) | k);
      flags[k] |= (uint8_t)(1u << mi);
    }
  }
  if (row_out.empty()) return 0;
  // a run of constraints shares ONE B evaluation (its first row's): the flag of the first row decides for the run, and the rows of
  // a run have identical B rows, so they qualify together
  uint32_t *d_w, *d_rp, *d_sl, *d_ro, *d_xp, *d_xw, *d_xc;
  int32_t *d_lo, *d_co;
  int e;
  if (rest_wire.empty()) { rest_wire.push_back(0); rest_coeff.push_back(0); }   // never read: keeps the uploads non-empty
  if ((e = own_upload(c, &d_w, wires)) || (e = own_upload(c, &d_lo, lo)) || (e = own_upload(c, &d_rp, rowptr)) || (e = own_upload(c, &d_sl, slots)) ||
      (e = own_upload(c, &d_co, coefs)) || (e = own_upload(c, &d_ro, row_out)) ||
      (e = own_upload(c, &d_xp, rest_ptr)) || (e = own_upload(c, &d_xw, rest_wire)) || (e = own_upload(c, &d_xc, rest_coeff)))
    return e;
  c->dc.sm_rest_ptr = d_xp; c->dc.sm_rest_wire = d_xw; c->dc.sm_rest_coeff = d_xc;
  c->dc.sm_wires = d_w; c->dc.sm_lo = d_lo; c->dc.sm_nslots = (uint32_t)wires.size();
  c->dc.sm_rowptr = d_rp; c->dc.sm_slot = d_sl; c->dc.sm_coef = d_co; c->dc.sm_row_out = d_ro; c->dc.sm_nrows = (uint32_t)row_out.size();
  flags_out = flags;
  return 0;
}

// the "already in abc" bits of k_spmv_check: small rows (above) and long rows (DevCircuit::lg_rows)
static constexpr uint32_t LONG_ROW_MIN = 512;
int row_paths_plan(spp_circuit* c) {
  const Circuit& circ = c->circ;
  std::vector<uint8_t> small_flags;
  if (int e = small_rows_plan(c, small_flags)) return e;
  const uint32_t nc = std::max<uint32_t>(circ.n_constraints, 1);
  if (small_flags.empty()) small_flags.assign(nc, 0);
  std::vector<uint8_t> long_flags(nc, 0);
  std::vector<uint32_t> lg;
  c->dc.lg_n = 0;
  c->dc.lg_rows = nullptr;
  c->dc.row_long = nullptr;
  if (!getenv("SPP_NO_LONG_ROWS")) {
    const Sparse* mats[3] = {&circ.A, &circ.B, &circ.C};
    for (uint32_t mi = 0; mi < 3; mi++)
      for (uint32_t k = 0; k < circ.n_constraints; k++)
        if (mats[mi]->rowptr[k + 1] - mats[mi]->rowptr[k] > LONG_ROW_MIN && !(small_flags[k] & (1u << mi))) {
          lg.push_back((mi << 30) | k);
          long_flags[k] |= (uint8_t)(1u << mi);
        }
  }
  int e;
  if (!lg.empty()) {
    uint32_t* d_lg;
    uint8_t* d_lf;
    if ((e = own_upload(c, &d_lg, lg)) || (e = own_upload(c, &d_lf, long_flags))) return e;
    c->dc.lg_rows = d_lg;
    c->dc.lg_n = (uint32_t)lg.size();
    c->dc.row_long = d_lf;
  }
  if (c->dc.sm_nrows) {
    for (uint32_t k = 0; k < nc; k++) small_flags[k] |= long_flags[k];
    uint8_t* d_fl;
    if ((e = own_upload(c, &d_fl, small_flags))) return e;
    c->dc.row_small = d_fl;
  } else {
    c->dc.row_small = c->dc.row_long;
  }
  return 0;
}
