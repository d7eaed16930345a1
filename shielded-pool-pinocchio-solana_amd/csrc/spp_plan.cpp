// libspp, load-time planners: how the solver program and the constraint matrices of one circuit are laid out for the kernels
// (items of the cooperative solver, small and long rows of the matrix evaluation).  Host code that builds vectors from the
// Circuit and uploads them in its last lines; called once per circuit by load_circuit_impl (spp_load.cpp).
#include "spp_circuit.hpp"

// Item list of the cooperative solver (kernels_solve.hip, k_solve_coop) for every sequential stretch of the schedule.
// Nothing here changes what is computed: permutations become their lane-parallel form, runs of SOLVE_C rows are ordered
// by dependency level (level of a row = 1 + the highest level among the rows of the run that write one of its inputs),
// runs of independent BITS / LIMBS8 / INV_H instructions go one per lane, the rest stays on lane 0.  Items that share no
// wire (directly or through other items of the stretch) form independent components; the components are dealt over up to
// COOP_TRACKS waves per proof, longest first (the Merkle chain beside the key derivation; the ciphertext sponge beside the
// rest of the audit circuit).  Components that use the per-proof scratch rows stay together on track 0.
int coop_plan(spp_circuit* c) {
  const Circuit& circ = c->circ;
  const auto& pr = circ.program;
  struct Item { uint32_t kind, a, b; };
  std::vector<uint32_t> items, par, lvl_ptr{0}, lvl_rows, stream;
  const Fr f_one = Fr::one(), f_mone = Fr::one().neg();
  auto coeff_word = [&](uint32_t ci) -> uint32_t {
    return ci | (circ.coeffs[ci] == f_one ? COEFF_ONE : circ.coeffs[ci] == f_mone ? COEFF_MINUS_ONE : 0u);
  };
  // one row of the level stream (see DevCoop::lvl_stream)
  auto row_record = [&](uint32_t k, std::vector<uint32_t>& out) {
    const bool square = [&] {
      const uint32_t a0 = circ.A.rowptr[k], a1 = circ.A.rowptr[k + 1], b0 = circ.B.rowptr[k], b1 = circ.B.rowptr[k + 1];
      if (a1 - a0 != b1 - b0) return false;
      for (uint32_t i = 0; i < a1 - a0; i++)
        if (circ.A.terms[a0 + i].wire != circ.B.terms[b0 + i].wire || circ.A.terms[a0 + i].coeff != circ.B.terms[b0 + i].coeff) return false;
      return true;
    }();
    const uint32_t nA = square ? 0 : circ.A.rowptr[k + 1] - circ.A.rowptr[k], nB = circ.B.rowptr[k + 1] - circ.B.rowptr[k],
                   nC = circ.C.rowptr[k + 1] - circ.C.rowptr[k] - 1;
    out.push_back(circ.C.terms[circ.C.rowptr[k + 1] - 1].wire);
    out.push_back(nA | (square ? 0x80000000u : 0u));
    out.push_back(nB);
    out.push_back(nC);
    auto put = [&](const Sparse& m, uint32_t n) {
      for (uint32_t t = m.rowptr[k]; t < m.rowptr[k] + n; t++) { out.push_back(m.terms[t].wire); out.push_back(coeff_word(m.terms[t].coeff)); }
    };
    put(circ.A, nA); put(circ.B, nB); put(circ.C, nC);
  };
  std::vector<uint32_t> level_of(circ.n_wires + 3, 0), stamp(circ.n_wires + 3, 0), writer(circ.n_wires + 3, 0);
  uint32_t epoch = 0;
  auto op_len = [&](size_t pc) -> uint32_t {
    switch (pr[pc]) {
      case OP_SOLVE_C: case OP_SOLVE_A: case OP_MASK: return 2;
      case OP_BATCH_DIV: case OP_POSEIDON2: case OP_INV_H: return 3;
      case OP_COUNT8: case OP_BITS: case OP_LIMBS8: case OP_POSEIDON: return 4;
      case OP_COMMIT: return 1;
      case OP_GRUMPKIN: return 5 + pr[pc + 4];
      default: return 0;
    }
  };
  auto is_par_op = [&](uint32_t op) { return op == OP_BITS || op == OP_LIMBS8 || op == OP_INV_H; };
  // wires an instruction reads / writes, a rough cost in microseconds of a lone wave, whether it uses the scratch rows
  struct RW { std::vector<uint32_t> rd, wr; double cost = 0; bool scratch = false; };
  auto row_rd = [&](RW& x, const Sparse& m, uint32_t k, uint32_t skip_last) {
    for (uint32_t t = m.rowptr[k]; t + skip_last < m.rowptr[k + 1]; t++) x.rd.push_back(m.terms[t].wire);
  };
  auto solve_c_rw = [&](RW& x, uint32_t k) {
    row_rd(x, circ.A, k, 0); row_rd(x, circ.B, k, 0); row_rd(x, circ.C, k, 1);
    x.wr.push_back(circ.C.terms[circ.C.rowptr[k + 1] - 1].wire);
  };
  auto div_rw = [&](RW& x, uint32_t k) {
    row_rd(x, circ.B, k, 0); row_rd(x, circ.C, k, 0);
    x.wr.push_back(circ.A.terms[circ.A.rowptr[k]].wire);
  };
  auto op_rw = [&](RW& x, size_t pc, bool coop_form) {
    switch (pr[pc]) {
      case OP_SOLVE_C: solve_c_rw(x, pr[pc + 1]); x.cost += 5; break;
      case OP_SOLVE_A: div_rw(x, pr[pc + 1]); x.cost += 60; x.scratch = true; break;
      case OP_BATCH_DIV:
        for (uint32_t k = 0; k < pr[pc + 2]; k++) div_rw(x, pr[pc + 1] + k);
        x.cost += 60 + 10.0 * pr[pc + 2]; x.scratch = true;
        break;
      case OP_BITS: case OP_LIMBS8:
        row_rd(x, circ.H, pr[pc + 1], 0);
        for (uint32_t i = 0; i < pr[pc + 2]; i++) x.wr.push_back(pr[pc + 3] + i);
        x.cost += 5 + 0.2 * pr[pc + 2];
        break;
      case OP_INV_H: row_rd(x, circ.H, pr[pc + 1], 0); x.wr.push_back(pr[pc + 2]); x.cost += 40; break;
      case OP_MASK: x.wr.push_back(pr[pc + 1]); x.cost += 5; break;
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
  for (SolveStep& st : c->schedule) {
    if (st.kind != SolveStep::SEQ) continue;
    std::vector<Item> its;
    size_t pc = st.a, seq0 = st.a;
    auto push = [&](uint32_t kind, uint32_t a, uint32_t b) { its.push_back({kind, a, b}); };
    auto flush = [&](size_t end) {
      if (end > seq0) push(COOP_SEQ, (uint32_t)seq0, (uint32_t)end);
    };
    while (pc < st.b) {
      const uint32_t op = pr[pc];
      if (op == OP_POSEIDON || op == OP_POSEIDON2 || (op == OP_GRUMPKIN && pr[pc + 4] >= 64 && pr[pc + 4] <= 65)) {
        flush(pc);
        push(op == OP_POSEIDON ? COOP_POSEIDON : op == OP_POSEIDON2 ? COOP_POSEIDON2 : COOP_GRUMPKIN, (uint32_t)pc, 0);
        pc += op_len(pc);
        seq0 = pc;
      } else if (op == OP_SOLVE_C) {
        size_t e = pc;
        while (e < st.b && pr[e] == OP_SOLVE_C) e += 2;
        const size_t nrows = (e - pc) / 2;
        if (nrows < 8) { pc = e; continue; }
        flush(pc);
        epoch++;
        std::vector<std::pair<uint32_t, uint32_t>> rows;   // (level, constraint)
        uint32_t max_level = 0;
        for (size_t q = pc; q < e; q += 2) {
          const uint32_t k = pr[q + 1];
          uint32_t lv = 0;
          auto scan = [&](const Sparse& m, uint32_t skip_last) {
            for (uint32_t t = m.rowptr[k]; t + skip_last < m.rowptr[k + 1]; t++) {
              const uint32_t w = m.terms[t].wire;
              if (stamp[w] == epoch) lv = std::max(lv, level_of[w]);
            }
          };
          scan(circ.A, 0); scan(circ.B, 0); scan(circ.C, 1);
          const uint32_t out = circ.C.terms[circ.C.rowptr[k + 1] - 1].wire;
          stamp[out] = epoch;
          level_of[out] = lv + 1;
          rows.push_back({lv, k});
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
          const uint32_t k = rows[i].second;
          auto link = [&](const Sparse& m, uint32_t skip_last) {
            for (uint32_t t = m.rowptr[k]; t + skip_last < m.rowptr[k + 1]; t++) {
              const uint32_t w = m.terms[t].wire;
              if (stamp[w] == epoch) { const uint32_t ra = rfind((uint32_t)i), rb = rfind(writer[w]); if (ra != rb) rp[ra] = rb; }
            }
          };
          link(circ.A, 0); link(circ.B, 0); link(circ.C, 1);
          const uint32_t out = circ.C.terms[circ.C.rowptr[k + 1] - 1].wire;
          stamp[out] = epoch;
          writer[out] = (uint32_t)i;
        }
        std::vector<uint32_t> comp_size(rows.size(), 0), comp_id(rows.size(), 0);
        for (size_t i = 0; i < rows.size(); i++) comp_size[rfind((uint32_t)i)]++;
        const uint32_t MISC = 0xffffffffu;
        std::vector<uint32_t> comp_order;     // big components in order of first appearance, then the lump of small ones
        bool any_misc = false;
        for (size_t i = 0; i < rows.size(); i++) {
          const uint32_t r = rfind((uint32_t)i);
          if (comp_size[r] < 32) { comp_id[i] = MISC; any_misc = true; continue; }
          comp_id[i] = r;
          if (std::find(comp_order.begin(), comp_order.end(), r) == comp_order.end()) comp_order.push_back(r);
        }
        if (any_misc) comp_order.push_back(MISC);
        std::vector<size_t> order(rows.size());
        for (size_t i = 0; i < rows.size(); i++) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return rows[x].first < rows[y].first; });
        for (uint32_t cid : comp_order) {
          const uint32_t l0 = (uint32_t)lvl_ptr.size() - 1;
          uint32_t cur = 0xffffffffu;
          std::vector<std::vector<uint32_t>> by_level;      // constraints of this component, level by level
          for (size_t oi : order) {
            if (comp_id[oi] != cid) continue;
            if (rows[oi].first != cur) {
              if (cur != 0xffffffffu) lvl_ptr.push_back((uint32_t)lvl_rows.size());
              cur = rows[oi].first;
              by_level.emplace_back();
            }
            lvl_rows.push_back(rows[oi].second);
            by_level.back().push_back(rows[oi].second);
          }
          lvl_ptr.push_back((uint32_t)lvl_rows.size());
          // the streamed form: levels as self-contained records in chunks of COOP_CHUNK words; a level too big for a chunk is cut
          // into consecutive sub-levels (its rows are independent), a single row too big for one sends the component down the
          // table-driven path
          std::vector<uint32_t> local;          // this component's chunks
          uint32_t used = 0;                    // words used in the current chunk
          bool fits = !c->sw.no_level_stream;
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
              for (const auto& rec : recs) longest = std::max({longest, rec[1] & 0x7fffffffu, rec[2], rec[3]});
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
            push(COOP_LEVEL_STREAM, chunk0, (uint32_t)(local.size() / COOP_CHUNK));
          } else {
            push(COOP_LEVELS, l0, (uint32_t)lvl_ptr.size() - 1);
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
          if (dep) break;
          if (pr[e] == OP_INV_H) stamp[pr[e + 2]] = epoch;
          else for (uint32_t i = 0; i < pr[e + 2]; i++) stamp[pr[e + 3] + i] = epoch;
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
        if (n == 0) return fail(SPP_ERR_FORMAT, "bad opcode %u in solver program", op);
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
          for (uint32_t r = lvl_ptr[it.a]; r < lvl_ptr[it.b]; r++) solve_c_rw(rw[i], lvl_rows[r]);
          rw[i].cost = 4.5 * (it.b - it.a);
          break;
        case COOP_LEVEL_STREAM: {
          uint32_t nlev = 0;
          for (uint32_t ch = it.a; ch < it.a + it.b; ch++) {
            const uint32_t* sb = stream.data() + (size_t)ch * COOP_CHUNK;
            for (uint32_t pos = 0; pos < COOP_CHUNK && sb[pos] != 0xffffffffu; pos += sb[pos + 1]) {
              nlev++;
              for (uint32_t r = 0; r < (sb[pos] & 0xffffffu); r++) {
                const uint32_t base = pos + sb[pos + 2 + r];
                const uint32_t nt = (sb[base + 1] & 0x7fffffffu) + sb[base + 2] + sb[base + 3];
                rw[i].wr.push_back(sb[base]);
                for (uint32_t t = 0; t < nt; t++) rw[i].rd.push_back(sb[base + 4 + 2 * t]);
              }
            }
          }
          rw[i].cost = 3.0 * nlev;
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
      for (uint32_t w : rw[i].wr) { stamp[w] = epoch; writer[w] = (uint32_t)i; }
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
  for (size_t i = 0; i < items.size(); i += 3) c->coop_item_count[items[i]]++;
  c->coop_stream_chunks = (uint32_t)(stream.size() / COOP_CHUNK);
  if (items.empty()) items.assign(3, 0);
  if (par.empty()) par.assign(2, 0);
  if (lvl_rows.empty()) lvl_rows.push_back(0);
  if (stream.empty()) stream.assign(COOP_CHUNK, 0xffffffffu);
  uint32_t *d_items, *d_par, *d_lp, *d_lr, *d_ls;
  int e;
  if ((e = own_upload(c, &d_items, items)) || (e = own_upload(c, &d_par, par)) || (e = own_upload(c, &d_lp, lvl_ptr)) ||
      (e = own_upload(c, &d_lr, lvl_rows)) || (e = own_upload(c, &d_ls, stream)))
    return e;
  c->coop.items = d_items; c->coop.par = d_par; c->coop.lvl_ptr = d_lp; c->coop.lvl_rows = d_lr; c->coop.lvl_stream = d_ls;
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
