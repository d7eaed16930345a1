// Host-side planning of the solver phase: the schedule of a solver program (sequential stretches and wide steps) and, for every
// stretch, the item list of the cooperative solver (kernels_solve.hip, k_solve_coop) with its level tables and level stream.
// No HIP call and nothing of the device in here: spp_plan.cpp uploads what this builds, tests/host/coop_generic_check.cpp
// executes it on the CPU.
#pragma once
#include <algorithm>
#include <string>
#include <utility>
#include <vector>
#include "circuit.hpp"
#include "coop_items.hpp"

namespace spp {

struct SolveStep {
  enum Kind { SEQ, BATCH_DIV, COUNT8, COMMIT } kind;
  uint32_t a = 0, b = 0, c = 0;   // SEQ: [pc_begin, pc_end) ; BATCH_DIV: k0, n ; COUNT8: h0, n, out0
  // SEQ: the same stretch as items of the cooperative solver (small batches), dealt over independent tracks (coop_build_plan)
  uint32_t ntracks = 0, tr_begin[COOP_TRACKS] = {}, tr_end[COOP_TRACKS] = {};
};

// words of the instruction at pc (0: unknown opcode)
inline uint32_t solver_op_len(const std::vector<uint32_t>& pr, size_t pc) {
  switch (pr[pc]) {
    case OP_SOLVE_C: case OP_SOLVE_A: case OP_MASK: return 2;
    case OP_BATCH_DIV: case OP_POSEIDON2: case OP_INV_H: return 3;
    case OP_COUNT8: case OP_BITS: case OP_LIMBS8: case OP_POSEIDON: return 4;
    case OP_COMMIT: return 1;
    case OP_GRUMPKIN: return 5 + pr[pc + 4];
    case OP_SOLVE_ROW: case OP_LIMBS: case OP_COUNTN: return 5;
    case OP_GK_MUL: return 7;
    case OP_GLV: return 3 + 28;
    case OP_EMUL: return 3 + 16;
    default: return 0;
  }
}

// Program scan: sequential segments (one lane per proof, or the cooperative items below) and wide steps (data-parallel
// instructions that get their own kernels: batch divisions and lookup histograms), with the commitment boundary in between.
// split_by_op (SPP_SOLVE_TRACE=1, diagnostic): one segment per run of one instruction class.  Returns the bad opcode, or 0.
inline uint32_t solver_schedule(const std::vector<uint32_t>& pr, bool split_by_op, std::vector<SolveStep>* schedule, uint32_t* max_batch_div,
                                bool* generic_ops) {
  size_t pc = 0, seg = 0;
  auto flush = [&](size_t end) {
    if (end > seg) schedule->push_back({SolveStep::SEQ, (uint32_t)seg, (uint32_t)end, 0});
  };
  uint32_t prev_op = OP_END;
  while (pc < pr.size() && pr[pc] != OP_END) {
    if (split_by_op && pr[pc] != prev_op) {
      flush(pc);
      seg = std::max(seg, pc);
    }
    prev_op = pr[pc];
    switch (pr[pc]) {
      case OP_BATCH_DIV:
        *max_batch_div = std::max(*max_batch_div, pr[pc + 2]);
        if (pr[pc + 2] >= 64) {
          flush(pc);
          schedule->push_back({SolveStep::BATCH_DIV, pr[pc + 1], pr[pc + 2], 0});
          seg = pc + 3;
        }
        pc += 3;
        break;
      case OP_COUNT8:
        flush(pc);
        schedule->push_back({SolveStep::COUNT8, pr[pc + 1], pr[pc + 2], pr[pc + 3]});
        seg = pc + 4;
        pc += 4;
        break;
      case OP_COMMIT:
        flush(pc);
        schedule->push_back({SolveStep::COMMIT, 0, 0, 0});
        pc += 1;
        seg = pc;
        break;
      // the solver of a decoded gnark system (spp/ccs.py to_sppc_solved)
      case OP_SOLVE_ROW: case OP_LIMBS: case OP_COUNTN: case OP_GK_MUL: case OP_GLV: case OP_EMUL:
        *generic_ops = true;
        pc += solver_op_len(pr, pc);
        break;
      default: {
        const uint32_t n = solver_op_len(pr, pc);
        if (n == 0) return pr[pc];
        pc += n;
      }
    }
  }
  flush(pc);
  return 0;
}

struct CoopPlan {
  std::vector<uint32_t> items, par, lvl_ptr{0}, lvl_rows, lvl_gen, stream;
  uint32_t item_count[COOP_KINDS] = {};
  uint32_t stream_chunks = 0;
  uint32_t generic_rows = 0, generic_divs = 0;   // OP_SOLVE_ROW rows in level items; those whose other factor is inverted at run time
  uint32_t bad_opcode = 0;
};

// Item list of the cooperative solver for every sequential stretch of the schedule.
// Nothing here changes what is computed: permutations become their lane-parallel form, runs of SOLVE_C / SOLVE_ROW rows are ordered
// by dependency level (level of a row = 1 + the highest level among the rows of the run that write one of its inputs; the wire a
// row writes is the last term of its side), runs of independent BITS / LIMBS8 / LIMBS / INV_H instructions go one per lane, a
// COUNTN histogram deals its queries over the lanes, the rest stays on lane 0.  Items that share no wire (directly or through
// other items of the stretch) form independent components; the components are dealt over up to COOP_TRACKS waves per proof, longest
// first (the Merkle chain beside the key derivation; the ciphertext sponge beside the rest of the audit circuit).  Components that
// use the per-proof scratch rows stay together on track 0.  Fills the track fields of the schedule's SEQ steps; false: bad_opcode.
inline bool coop_build_plan(const Circuit& circ, std::vector<SolveStep>& schedule, bool no_level_stream, CoopPlan* plan) {
  const auto& pr = circ.program;
  struct Item { uint32_t kind, a, b; double extra; };
  // one row of a run: a plain OP_SOLVE_C row (side 2, !gen) or an OP_SOLVE_ROW row
  struct Row { uint32_t level, k, side, inv, odiv; bool gen; };
  std::vector<uint32_t>&items = plan->items, &par = plan->par, &lvl_ptr = plan->lvl_ptr, &lvl_rows = plan->lvl_rows, &lvl_gen = plan->lvl_gen,
                       &stream = plan->stream;
  const Fr f_one = Fr::one(), f_mone = Fr::one().neg();
  auto coeff_word = [&](uint32_t ci) -> uint32_t {
    return ci | (circ.coeffs[ci] == f_one ? COEFF_ONE : circ.coeffs[ci] == f_mone ? COEFF_MINUS_ONE : 0u);
  };
  const Sparse* mats[3] = {&circ.A, &circ.B, &circ.C};
  auto out_wire = [&](uint32_t k, uint32_t side) { return mats[side]->terms[mats[side]->rowptr[k + 1] - 1].wire; };
  auto row_at = [&](size_t q) -> Row {
    if (pr[q] == OP_SOLVE_C) return {0, pr[q + 1], 2, COOP_NONE, COOP_NONE, false};
    return {0, pr[q + 1], pr[q + 2], pr[q + 3], pr[q + 4], true};
  };
  auto runtime_div = [](const Row& r) { return r.gen && r.side != 2 && r.odiv == COOP_NONE; };
  // f(wire) for every wire the row reads: all terms but the last of its side
  auto for_reads = [&](uint32_t k, uint32_t side, auto&& f) {
    for (uint32_t mi = 0; mi < 3; mi++) {
      const Sparse& m = *mats[mi];
      for (uint32_t t = m.rowptr[k]; t + (mi == side ? 1u : 0u) < m.rowptr[k + 1]; t++) f(m.terms[t].wire);
    }
  };
  // one row of the level stream (see DevCoop::lvl_stream)
  auto row_record = [&](const Row& r, std::vector<uint32_t>& out) {
    const uint32_t k = r.k;
    const bool square = !r.gen && [&] {
      const uint32_t a0 = circ.A.rowptr[k], a1 = circ.A.rowptr[k + 1], b0 = circ.B.rowptr[k], b1 = circ.B.rowptr[k + 1];
      if (a1 - a0 != b1 - b0) return false;
      for (uint32_t i = 0; i < a1 - a0; i++)
        if (circ.A.terms[a0 + i].wire != circ.B.terms[b0 + i].wire || circ.A.terms[a0 + i].coeff != circ.B.terms[b0 + i].coeff) return false;
      return true;
    }();
    uint32_t n[3];
    for (uint32_t mi = 0; mi < 3; mi++) n[mi] = mats[mi]->rowptr[k + 1] - mats[mi]->rowptr[k] - (mi == r.side ? 1u : 0u);
    if (square) n[0] = 0;
    out.push_back(out_wire(k, r.side));
    out.push_back(n[0] | (square ? 0x80000000u : 0u));
    out.push_back(n[1] | (r.gen ? COOP_ROW_GENERIC | (r.side << COOP_ROW_SIDE_SHIFT) : 0u));
    out.push_back(n[2]);
    if (r.gen) { out.push_back(r.inv); out.push_back(r.odiv); }
    for (uint32_t mi = 0; mi < 3; mi++)
      for (uint32_t t = mats[mi]->rowptr[k]; t < mats[mi]->rowptr[k] + n[mi]; t++) {
        out.push_back(mats[mi]->terms[t].wire);
        out.push_back(coeff_word(mats[mi]->terms[t].coeff));
      }
  };
  std::vector<uint32_t> level_of(circ.n_wires + 3, 0), stamp(circ.n_wires + 3, 0), writer(circ.n_wires + 3, 0);
  uint32_t epoch = 0;
  auto op_len = [&](size_t pc) -> uint32_t { return solver_op_len(pr, pc); };
  auto is_par_op = [&](uint32_t op) { return op == OP_BITS || op == OP_LIMBS8 || op == OP_INV_H || op == OP_LIMBS; };
  auto is_row_op = [&](uint32_t op) { return op == OP_SOLVE_C || op == OP_SOLVE_ROW; };
  // first output wire and output count of a lane-independent instruction
  auto par_out = [&](size_t pc, uint32_t* out0, uint32_t* n) {
    if (pr[pc] == OP_INV_H) { *out0 = pr[pc + 2]; *n = 1; }
    else if (pr[pc] == OP_LIMBS) { *out0 = pr[pc + 4]; *n = pr[pc + 2]; }
    else { *out0 = pr[pc + 3]; *n = pr[pc + 2]; }
  };
  // wires an instruction reads / writes, a rough cost in microseconds of a lone wave, whether it uses the scratch rows
  struct RW { std::vector<uint32_t> rd, wr; double cost = 0; bool scratch = false; };
  auto row_rd = [&](RW& x, const Sparse& m, uint32_t k, uint32_t skip_last) {
    for (uint32_t t = m.rowptr[k]; t + skip_last < m.rowptr[k + 1]; t++) x.rd.push_back(m.terms[t].wire);
  };
  auto solve_row_rw = [&](RW& x, uint32_t k, uint32_t side) {
    for_reads(k, side, [&](uint32_t w) { x.rd.push_back(w); });
    x.wr.push_back(out_wire(k, side));
  };
  auto div_rw = [&](RW& x, uint32_t k) {
    row_rd(x, circ.B, k, 0); row_rd(x, circ.C, k, 0);
    x.wr.push_back(circ.A.terms[circ.A.rowptr[k]].wire);
  };
  auto op_rw = [&](RW& x, size_t pc, bool coop_form) {
    switch (pr[pc]) {
      case OP_SOLVE_C: solve_row_rw(x, pr[pc + 1], 2); x.cost += 5; break;
      case OP_SOLVE_ROW:
        solve_row_rw(x, pr[pc + 1], pr[pc + 2]);
        x.cost += runtime_div(row_at(pc)) ? 45 : 5;
        break;
      case OP_SOLVE_A: div_rw(x, pr[pc + 1]); x.cost += 60; x.scratch = true; break;
      case OP_BATCH_DIV:
        for (uint32_t k = 0; k < pr[pc + 2]; k++) div_rw(x, pr[pc + 1] + k);
        x.cost += 60 + 10.0 * pr[pc + 2]; x.scratch = true;
        break;
      case OP_BITS: case OP_LIMBS8: case OP_LIMBS: {
        uint32_t out0, n;
        par_out(pc, &out0, &n);
        row_rd(x, circ.H, pr[pc + 1], 0);
        for (uint32_t i = 0; i < n; i++) x.wr.push_back(out0 + i);
        x.cost += 5 + 0.2 * n;
        break;
      }
      case OP_INV_H: row_rd(x, circ.H, pr[pc + 1], 0); x.wr.push_back(pr[pc + 2]); x.cost += 40; break;
      case OP_MASK: x.wr.push_back(pr[pc + 1]); x.cost += 5; break;
      case OP_COUNTN:
        for (uint32_t i = 0; i < pr[pc + 2]; i++) row_rd(x, circ.H, pr[pc + 1] + i, 0);
        for (uint32_t i = 0; i < pr[pc + 4]; i++) x.wr.push_back(pr[pc + 3] + i);
        x.cost += coop_form ? 10 + 0.1 * pr[pc + 2] : 3.0 * pr[pc + 2];
        break;
      case OP_GK_MUL:
        row_rd(x, circ.H, pr[pc + 1], 0); row_rd(x, circ.H, pr[pc + 2], 0);
        for (uint32_t i = 4; i < 7; i++) x.wr.push_back(pr[pc + i]);
        x.cost += 2000;
        break;
      case OP_GLV:
        row_rd(x, circ.H, pr[pc + 1], 0);
        for (uint32_t i = 0; i < 8; i++) x.wr.push_back(pr[pc + 2] + i);
        x.cost += 50;
        break;
      case OP_EMUL:
        for (uint32_t i = 0; i < 6; i++) row_rd(x, circ.H, pr[pc + 1] + i, 0);
        for (uint32_t i = 0; i < 14; i++) x.wr.push_back(pr[pc + 2] + i);
        x.cost += 100;
        break;
      case OP_POSEIDON: {
        const uint32_t t = pr[pc + 1], nsbox = 8 * t + (t == 3 ? 57 : 60);
        for (uint32_t i = 0; i < t; i++) row_rd(x, circ.H, pr[pc + 2] + i, 0);
        for (uint32_t i = 0; i < 4 * nsbox; i++) x.wr.push_back(pr[pc + 3] + i);
        x.cost += coop_form ? 175 : 450;
        break;
      }
      case OP_POSEIDON2:
        for (uint32_t i = 0; i < 4; i++) row_rd(x, circ.H, pr[pc + 1] + i, 0);
        for (uint32_t i = 0; i < 4 * 88; i++) x.wr.push_back(pr[pc + 2] + i);
        x.cost += coop_form ? 185 : 480;
        break;
      case OP_GRUMPKIN:
        for (uint32_t i = 0; i < pr[pc + 2]; i++) x.rd.push_back(pr[pc + 1] + i);
        for (uint32_t i = 0; i < pr[pc + 4]; i++) x.wr.push_back(pr[pc + 5 + i]);
        x.cost += coop_form ? 300 : 1800;
        x.scratch = x.scratch || !coop_form;
        break;
      default: break;
    }
  };
  for (SolveStep& st : schedule) {
    if (st.kind != SolveStep::SEQ) continue;
    std::vector<Item> its;
    size_t pc = st.a, seq0 = st.a;
    auto push = [&](uint32_t kind, uint32_t a, uint32_t b, double extra = 0) { its.push_back({kind, a, b, extra}); };
    auto flush = [&](size_t end) {
      if (end > seq0) push(COOP_SEQ, (uint32_t)seq0, (uint32_t)end);
    };
    while (pc < st.b) {
      const uint32_t op = pr[pc];
      if (op == OP_POSEIDON || op == OP_POSEIDON2 || (op == OP_GRUMPKIN && pr[pc + 4] >= 64 && pr[pc + 4] <= 65) || op == OP_COUNTN) {
        flush(pc);
        push(op == OP_POSEIDON ? COOP_POSEIDON : op == OP_POSEIDON2 ? COOP_POSEIDON2 : op == OP_COUNTN ? COOP_COUNTN : COOP_GRUMPKIN,
             (uint32_t)pc, 0);
        pc += op_len(pc);
        seq0 = pc;
      } else if (is_row_op(op)) {
        size_t e = pc;
        std::vector<Row> rows;
        while (e < st.b && is_row_op(pr[e])) { rows.push_back(row_at(e)); e += op_len(e); }
        if (rows.size() < 8) { pc = e; continue; }
        flush(pc);
        epoch++;
        uint32_t max_level = 0;
        for (Row& r : rows) {
          uint32_t lv = 0;
          for_reads(r.k, r.side, [&](uint32_t w) { if (stamp[w] == epoch) lv = std::max(lv, level_of[w]); });
          const uint32_t out = out_wire(r.k, r.side);
          stamp[out] = epoch;
          level_of[out] = lv + 1;
          r.level = lv;
          max_level = std::max(max_level, lv);
        }
        // rows of the run that share no wire written inside it are independent of each other: one LEVELS item per connected
        // component (small ones lumped together), so that the tracks below can take them apart (a compiled program keeps the
        // key derivation and the hash chain in the same run of rows)
        std::vector<uint32_t> rp(rows.size());
        for (size_t i = 0; i < rows.size(); i++) rp[i] = (uint32_t)i;
        auto rfind = [&](uint32_t x) { while (rp[x] != x) x = rp[x] = rp[rp[x]]; return x; };
        epoch++;
        for (size_t i = 0; i < rows.size(); i++) {
          for_reads(rows[i].k, rows[i].side, [&](uint32_t w) {
            if (stamp[w] == epoch) { const uint32_t ra = rfind((uint32_t)i), rb = rfind(writer[w]); if (ra != rb) rp[ra] = rb; }
          });
          const uint32_t out = out_wire(rows[i].k, rows[i].side);
          stamp[out] = epoch;
          writer[out] = (uint32_t)i;
        }
        std::vector<uint32_t> comp_size(rows.size(), 0), comp_id(rows.size(), 0);
        for (size_t i = 0; i < rows.size(); i++) comp_size[rfind((uint32_t)i)]++;
        const uint32_t MISC = 0xffffffffu;
        std::vector<uint32_t> comp_order;     // big components in order of first appearance, then the lump of small ones
        std::vector<char> comp_seen(rows.size(), 0);
        bool any_misc = false;
        for (size_t i = 0; i < rows.size(); i++) {
          const uint32_t r = rfind((uint32_t)i);
          if (comp_size[r] < 32) { comp_id[i] = MISC; any_misc = true; continue; }
          comp_id[i] = r;
          if (!comp_seen[r]) { comp_seen[r] = 1; comp_order.push_back(r); }
        }
        if (any_misc) comp_order.push_back(MISC);
        std::vector<size_t> order(rows.size());
        for (size_t i = 0; i < rows.size(); i++) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return rows[x].level < rows[y].level; });
        for (uint32_t cid : comp_order) {
          const uint32_t l0 = (uint32_t)lvl_ptr.size() - 1;
          uint32_t cur = 0xffffffffu;
          std::vector<std::vector<Row>> by_level;      // rows of this component, level by level
          uint32_t n_gen = 0, n_div = 0, div_levels = 0;
          for (size_t oi : order) {
            if (comp_id[oi] != cid) continue;
            const Row& r = rows[oi];
            if (r.level != cur) {
              if (cur != 0xffffffffu) lvl_ptr.push_back((uint32_t)lvl_rows.size());
              cur = r.level;
              by_level.emplace_back();
            }
            lvl_rows.push_back(r.k);
            lvl_gen.push_back(r.gen ? r.side : COOP_NONE); lvl_gen.push_back(r.inv); lvl_gen.push_back(r.odiv);
            by_level.back().push_back(r);
            n_gen += r.gen;
            n_div += runtime_div(r);
          }
          lvl_ptr.push_back((uint32_t)lvl_rows.size());
          for (const auto& lv : by_level) div_levels += std::any_of(lv.begin(), lv.end(), runtime_div);
          plan->generic_rows += n_gen;
          plan->generic_divs += n_div;
          // the streamed form: levels as self-contained records in chunks of COOP_CHUNK words; a level too big for a chunk is cut
          // into consecutive sub-levels (its rows are independent), a single row too big for one sends the component down the
          // table-driven path
          std::vector<uint32_t> local;          // this component's chunks
          uint32_t used = 0;                    // words used in the current chunk
          bool fits = !no_level_stream;
          auto close_chunk = [&] {
            if (used < COOP_CHUNK) local.push_back(0xffffffffu), used++;
            local.resize(local.size() + (COOP_CHUNK - used), 0xffffffffu);
            used = 0;
          };
          for (const auto& lv : by_level) {
            if (!fits) break;
            size_t i = 0;
            while (i < lv.size() && fits) {
              // greedily take rows while the sub-level record fits one chunk
              std::vector<std::vector<uint32_t>> recs;
              uint32_t words = 2;
              while (i < lv.size()) {
                std::vector<uint32_t> rec;
                row_record(lv[i], rec);
                if (words + 1 + rec.size() > COOP_CHUNK - 1) break;
                words += 1 + (uint32_t)rec.size();
                recs.push_back(std::move(rec));
                i++;
              }
              if (recs.empty()) { fits = false; break; }
              if (used + words > COOP_CHUNK - 1 && used) close_chunk();
              // lanes per row: enough for the longest linear form of the sub-level (every extra doubling costs three shuffle-add
              // rounds), at most 16, and rows x lanes within the wave when possible
              uint32_t longest = 1;
              for (const auto& rec : recs) longest = std::max({longest, rec[1] & 0x7fffffffu, rec[2] & COOP_ROW_COUNT_MASK, rec[3]});
              uint32_t G = 1;
              while (G < 16 && G < longest && recs.size() * (G * 2) <= 64) G *= 2;
              uint32_t need = 0;
              for (const auto& rec : recs) need |= ((rec[1] & 0x7fffffffu) ? 1u << 29 : 0u) | (rec[3] ? 1u << 30 : 0u);
              local.push_back((uint32_t)recs.size() | (G << 24) | need);
              local.push_back(words);
              uint32_t off = 2 + (uint32_t)recs.size();
              for (const auto& rec : recs) { local.push_back(off); off += (uint32_t)rec.size(); }
              for (const auto& rec : recs) local.insert(local.end(), rec.begin(), rec.end());
              used += words;
            }
          }
          if (fits && !local.empty()) {
            if (used) close_chunk();
            const uint32_t chunk0 = (uint32_t)(stream.size() / COOP_CHUNK);
            stream.insert(stream.end(), local.begin(), local.end());
            push(COOP_LEVEL_STREAM, chunk0, (uint32_t)(local.size() / COOP_CHUNK), 40.0 * div_levels);
          } else {
            push(COOP_LEVELS, l0, (uint32_t)lvl_ptr.size() - 1, 40.0 * div_levels);
          }
        }
        pc = e;
        seq0 = pc;
      } else if (is_par_op(op)) {
        // maximal run of lane-independent instructions: none may read a wire an earlier one of the run writes
        size_t e = pc;
        epoch++;
        std::vector<uint32_t> group;
        while (e < st.b && is_par_op(pr[e])) {
          const uint32_t h = pr[e + 1];
          bool dep = false;
          for (uint32_t t = circ.H.rowptr[h]; t < circ.H.rowptr[h + 1]; t++) dep = dep || stamp[circ.H.terms[t].wire] == epoch;
          uint32_t out0, n;
          par_out(e, &out0, &n);
          for (uint32_t i = 0; i < n; i++) dep = dep || stamp[out0 + i] == epoch;   // nor write one (a shared scratch wire)
          if (dep) break;
          for (uint32_t i = 0; i < n; i++) stamp[out0 + i] = epoch;
          group.push_back((uint32_t)e);
          e += op_len(e);
        }
        if (group.size() < 4) { pc = group.empty() ? pc + op_len(pc) : e; continue; }
        flush(pc);
        const uint32_t g0 = (uint32_t)(par.size() / 2);
        for (uint32_t q : group) { par.push_back(q); par.push_back(q + op_len(q)); }
        push(COOP_PAR, g0, g0 + (uint32_t)group.size());
        pc = e;
        seq0 = pc;
      } else {
        const uint32_t n = op_len(pc);
        if (n == 0) { plan->bad_opcode = op; return false; }
        pc += n;
      }
    }
    flush(st.b);

    // ---- independent components of this stretch -> tracks ----
    const size_t n = its.size();
    std::vector<RW> rw(n);
    for (size_t i = 0; i < n; i++) {
      const Item& it = its[i];
      switch (it.kind) {
        case COOP_SEQ:
          for (size_t q = it.a; q < it.b; q += op_len(q)) op_rw(rw[i], q, false);
          break;
        case COOP_PAR:
          for (uint32_t g = it.a; g < it.b; g++) op_rw(rw[i], par[2 * g], false);
          rw[i].cost = 10 + rw[i].cost / 32;
          break;
        case COOP_LEVELS:
          for (uint32_t r = lvl_ptr[it.a]; r < lvl_ptr[it.b]; r++) solve_row_rw(rw[i], lvl_rows[r], lvl_gen[3 * r] == COOP_NONE ? 2 : lvl_gen[3 * r]);
          rw[i].cost = 4.5 * (it.b - it.a) + it.extra;
          break;
        case COOP_LEVEL_STREAM: {
          uint32_t nlev = 0;
          for (uint32_t ch = it.a; ch < it.a + it.b; ch++) {
            const uint32_t* sb = stream.data() + (size_t)ch * COOP_CHUNK;
            for (uint32_t pos = 0; pos < COOP_CHUNK && sb[pos] != 0xffffffffu; pos += sb[pos + 1]) {
              nlev++;
              for (uint32_t r = 0; r < (sb[pos] & 0xffffffu); r++) {
                const uint32_t base = pos + sb[pos + 2 + r];
                const uint32_t nt = (sb[base + 1] & 0x7fffffffu) + (sb[base + 2] & COOP_ROW_COUNT_MASK) + sb[base + 3];
                const uint32_t hdr = (sb[base + 2] & COOP_ROW_GENERIC) ? 6 : 4;
                rw[i].wr.push_back(sb[base]);
                for (uint32_t t = 0; t < nt; t++) rw[i].rd.push_back(sb[base + hdr + 2 * t]);
              }
            }
          }
          rw[i].cost = 3.0 * nlev + it.extra;
          break;
        }
        default: op_rw(rw[i], it.a, true); break;
      }
    }
    std::vector<uint32_t> parent(n);
    for (size_t i = 0; i < n; i++) parent[i] = (uint32_t)i;
    auto find = [&](uint32_t x) { while (parent[x] != x) x = parent[x] = parent[parent[x]]; return x; };
    epoch++;
    for (size_t i = 0; i < n; i++) {
      for (uint32_t w : rw[i].rd)
        if (stamp[w] == epoch) { const uint32_t ra = find((uint32_t)i), rb = find(writer[w]); if (ra != rb) parent[ra] = rb; }
      // (two writers of one wire -- hint outputs nothing reads share a scratch wire -- stay in program order on one track)
      for (uint32_t w : rw[i].wr) {
        if (stamp[w] == epoch) { const uint32_t ra = find((uint32_t)i), rb = find(writer[w]); if (ra != rb) parent[ra] = rb; }
        stamp[w] = epoch;
        writer[w] = (uint32_t)i;
      }
    }
    std::vector<double> comp_cost(n, 0.0);
    std::vector<char> comp_scratch(n, 0);
    for (size_t i = 0; i < n; i++) { const uint32_t r = find((uint32_t)i); comp_cost[r] += rw[i].cost; comp_scratch[r] |= rw[i].scratch; }
    std::vector<uint32_t> roots;
    for (size_t i = 0; i < n; i++) if (find((uint32_t)i) == i) roots.push_back((uint32_t)i);
    std::sort(roots.begin(), roots.end(), [&](uint32_t x, uint32_t y) { return comp_cost[x] > comp_cost[y]; });
    double load[COOP_TRACKS] = {};
    std::vector<uint32_t> track_of(n, 0);
    for (uint32_t r : roots) if (comp_scratch[r]) { track_of[r] = 0; load[0] += comp_cost[r]; }
    for (uint32_t r : roots) {
      if (comp_scratch[r]) continue;
      uint32_t best = 0;
      for (uint32_t t = 1; t < COOP_TRACKS; t++) if (load[t] < load[best]) best = t;
      track_of[r] = best;
      load[best] += comp_cost[r];
    }
    st.ntracks = 0;
    for (uint32_t t = 0; t < COOP_TRACKS; t++) {
      st.tr_begin[t] = (uint32_t)(items.size() / 3);
      for (size_t i = 0; i < n; i++)
        if (track_of[find((uint32_t)i)] == t) { items.push_back(its[i].kind); items.push_back(its[i].a); items.push_back(its[i].b); }
      st.tr_end[t] = (uint32_t)(items.size() / 3);
      if (st.tr_end[t] > st.tr_begin[t]) st.ntracks = t + 1;
    }
  }
  for (size_t i = 0; i < items.size(); i += 3) plan->item_count[items[i]]++;
  plan->stream_chunks = (uint32_t)(stream.size() / COOP_CHUNK);
  return true;
}

}  // namespace spp
