// Test-only host driver: the cooperative solver's plan (csrc/coop_plan.hpp) executed on the CPU against the program in program order.
//   coop_generic_check circuit.sppc [no_level_stream]
// The plan's items run in an order chosen to expose a missed dependency: the tracks of a stretch in REVERSE order, the items of a
// track in order, the rows of a level in REVERSE order, the instructions of a lane-parallel group in REVERSE order.  Streamed levels
// are executed from the words of the stream itself (wires, coefficient words, side, inv, odiv), table levels from lvl_rows / lvl_gen.
// Every wire must then equal the program executed instruction by instruction.  No level of a level item may read a wire that the
// same or a later level of that item writes.
// The three hints whose arithmetic lives in gnark_hints.hpp (OP_GK_MUL, OP_GLV, OP_EMUL) and OP_MASK are replaced, in both
// executions alike, by a fixed function of the values they read: what is under test is the order, not the hints.
// Prints one line of facts; exit status 0 iff every check holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>
#include "coop_plan.hpp"
using namespace spp;

static const Circuit* g_c;
static std::vector<Fr>* g_w;

static Fr dot(const Sparse& m, uint32_t k, uint32_t skip_last) {
  Fr acc = Fr::zero();
  for (uint32_t t = m.rowptr[k]; t + skip_last < m.rowptr[k + 1]; t++) acc = acc + g_c->coeffs[m.terms[t].coeff] * (*g_w)[m.terms[t].wire];
  return acc;
}
static Fr inv0(const Fr& v) { return v.is_zero() ? Fr::zero() : v.inv(); }
static Fr row_value(uint32_t side, const Fr& a, const Fr& b, const Fr& c, uint32_t inv_ci, uint32_t odiv_ci) {
  Fr v;
  if (side == 2) v = a * b - c;
  else {
    const Fr oi = odiv_ci != COOP_NONE ? g_c->coeffs[odiv_ci] : inv0(side == 0 ? b : a);
    v = c * oi - (side == 0 ? a : b);
  }
  if (inv_ci != COOP_NONE) v = v * g_c->coeffs[inv_ci];
  return v;
}
static void solve_row(uint32_t k, uint32_t side, uint32_t inv_ci, uint32_t odiv_ci) {
  const Circuit& c = *g_c;
  const Sparse* mats[3] = {&c.A, &c.B, &c.C};
  const Fr a = dot(c.A, k, side == 0), b = dot(c.B, k, side == 1), cc = dot(c.C, k, side == 2);
  (*g_w)[mats[side]->terms[mats[side]->rowptr[k + 1] - 1].wire] = row_value(side, a, b, cc, inv_ci, odiv_ci);
}
static void canonical(const Fr& v, uint32_t c[8]) { v.to_canonical(c); }
// a stand-in for a hint: output i = (sum of the forms it reads + 1) * (i + 2) + tag
static void stand_in(uint32_t h0, uint32_t nh, uint32_t out0, uint32_t nout, uint32_t tag) {
  Fr s = Fr::one();
  for (uint32_t i = 0; i < nh; i++) s = s + dot(g_c->H, h0 + i, 0) * Fr::from_u64(i + 3);
  for (uint32_t i = 0; i < nout; i++) (*g_w)[out0 + i] = s * Fr::from_u64(i + 2) + Fr::from_u64(tag);
}

// one instruction at pc; returns its length (0: not supported here)
static uint32_t exec_op(size_t pc) {
  const Circuit& c = *g_c;
  const auto& pr = c.program;
  std::vector<Fr>& W = *g_w;
  switch (pr[pc]) {
    case OP_SOLVE_C: solve_row(pr[pc + 1], 2, COOP_NONE, COOP_NONE); break;
    case OP_SOLVE_ROW: solve_row(pr[pc + 1], pr[pc + 2], pr[pc + 3], pr[pc + 4]); break;
    case OP_SOLVE_A: case OP_BATCH_DIV: {
      const uint32_t k0 = pr[pc + 1], n = pr[pc] == OP_SOLVE_A ? 1 : pr[pc + 2];
      for (uint32_t k = k0; k < k0 + n; k++) W[c.A.terms[c.A.rowptr[k]].wire] = dot(c.C, k, 0) * inv0(dot(c.B, k, 0));
      break;
    }
    case OP_BITS: case OP_LIMBS8: {
      uint32_t cw[8];
      canonical(dot(c.H, pr[pc + 1], 0), cw);
      const uint32_t per = pr[pc] == OP_BITS ? 1 : 8;
      for (uint32_t i = 0; i < pr[pc + 2]; i++) {
        const uint32_t bit = i * per;
        W[pr[pc + 3] + i] = Fr::from_u64(bit < 256 ? (cw[bit >> 5] >> (bit & 31)) & ((1u << per) - 1u) : 0);
      }
      break;
    }
    case OP_INV_H: W[pr[pc + 2]] = inv0(dot(c.H, pr[pc + 1], 0)); break;
    case OP_LIMBS: {
      const uint32_t nl = pr[pc + 2], width = pr[pc + 3] & 0x7fffffffu, out0 = pr[pc + 4];
      const bool reversed = (pr[pc + 3] >> 31) != 0;
      uint32_t cw[8];
      canonical(dot(c.H, pr[pc + 1], 0), cw);
      for (uint32_t i = 0; i < nl; i++) {
        uint32_t o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t b = 0; b < width; b++) {
          const uint32_t bit = i * width + b;
          if (bit < 256 && ((cw[bit >> 5] >> (bit & 31)) & 1u)) o[b >> 5] |= 1u << (b & 31);
        }
        W[out0 + (reversed ? nl - 1 - i : i)] = Fr::from_canonical(o);
      }
      break;
    }
    case OP_COUNT8: case OP_COUNTN: {
      const uint32_t h0 = pr[pc + 1], n = pr[pc + 2], out0 = pr[pc + 3], size = pr[pc] == OP_COUNT8 ? 256 : pr[pc + 4];
      std::vector<uint64_t> cnt(size, 0);
      for (uint32_t i = 0; i < n; i++) {
        uint32_t cw[8];
        canonical(dot(c.H, h0 + i, 0), cw);
        if (cw[0] < size && (cw[1] | cw[2] | cw[3] | cw[4] | cw[5] | cw[6] | cw[7]) == 0) cnt[cw[0]]++;
      }
      for (uint32_t j = 0; j < size; j++) W[out0 + j] = Fr::from_u64(cnt[j]);
      break;
    }
    case OP_MASK: W[pr[pc + 1]] = Fr::from_u64(0x5eed0000u + pr[pc + 1]); break;
    case OP_GK_MUL:
      stand_in(pr[pc + 1], 1, pr[pc + 4], 1, 16); stand_in(pr[pc + 2], 1, pr[pc + 5], 1, 17);
      W[pr[pc + 6]] = Fr::zero();
      break;
    case OP_GLV: stand_in(pr[pc + 1], 1, pr[pc + 2], 8, 18); break;
    case OP_EMUL: stand_in(pr[pc + 1], 6, pr[pc + 2], 14, 19); break;
    default: return 0;
  }
  return solver_op_len(pr, pc);
}
static bool exec_range(size_t a, size_t b) {
  for (size_t pc = a; pc < b;) {
    const uint32_t n = exec_op(pc);
    if (!n) { fprintf(stderr, "opcode %u not supported by the check\n", g_c->program[pc]); return false; }
    pc += n;
  }
  return true;
}

// a row of a level, whatever form it came in: its terms, and what the leader does with the sums
struct LevelRow {
  uint32_t out, side, inv, odiv;
  bool gen, square;
  std::vector<std::pair<uint32_t, uint32_t>> t[3];   // (wire, coefficient word)
};
static Fr word_dot(const std::vector<std::pair<uint32_t, uint32_t>>& t) {
  Fr acc = Fr::zero();
  for (auto& e : t) {
    const Fr w = (*g_w)[e.first];
    if (e.second & COEFF_ONE) acc = acc + w;
    else if (e.second & COEFF_MINUS_ONE) acc = acc - w;
    else acc = acc + g_c->coeffs[e.second & COEFF_MASK] * w;
  }
  return acc;
}
static void exec_level_row(const LevelRow& r) {
  Fr b = word_dot(r.t[1]), a = r.square ? b : word_dot(r.t[0]), c = word_dot(r.t[2]);
  (*g_w)[r.out] = r.gen ? row_value(r.side, a, b, c, r.inv, r.odiv) : a * b - c;
}
// the levels of one item; false: a level reads what the same or a later level writes
static bool exec_levels(const std::vector<std::vector<LevelRow>>& levels) {
  std::map<uint32_t, size_t> written;     // wire -> level that writes it
  for (size_t l = 0; l < levels.size(); l++)
    for (auto& r : levels[l]) written[r.out] = l;
  for (size_t l = 0; l < levels.size(); l++)
    for (auto& r : levels[l])
      for (int s = 0; s < 3; s++)
        for (auto& e : r.t[s]) {
          auto it = written.find(e.first);
          if (it != written.end() && it->second >= l) { fprintf(stderr, "level %zu reads wire %u written in level %zu\n", l, e.first, it->second); return false; }
        }
  for (auto& lv : levels)
    for (size_t i = lv.size(); i-- > 0;) exec_level_row(lv[i]);
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: coop_generic_check circuit.sppc [no_level_stream]\n"); return 2; }
  Circuit c;
  if (!c.load(argv[1])) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  const bool no_stream = argc > 2 && !strcmp(argv[2], "no_level_stream");
  std::vector<SolveStep> schedule;
  uint32_t max_div = 0;
  bool generic_ops = false;
  if (solver_schedule(c.program, false, &schedule, &max_div, &generic_ops)) return 2;
  CoopPlan pl;
  if (!coop_build_plan(c, schedule, no_stream, &pl)) return 2;
  g_c = &c;
  const Sparse* mats[3] = {&c.A, &c.B, &c.C};

  auto fresh = [&] {
    std::vector<Fr> W(c.n_wires + 3, Fr::zero());
    W[0] = Fr::one();
    uint64_t x = 0x9e3779b97f4a7c15ull;
    for (uint32_t i = 1; i <= c.n_inputs(); i++) {
      x = x * 6364136223846793005ull + 1442695040888963407ull;
      W[i] = Fr::from_u64(x) * Fr::from_u64(x >> 7) + Fr::from_u64(i);
    }
    return W;
  };
  auto run = [&](bool by_plan, std::vector<Fr>& W) -> bool {
    g_w = &W;
    for (const SolveStep& st : schedule) {
      switch (st.kind) {
        case SolveStep::COMMIT: W[c.challenge_wire] = Fr::from_u64(0xc0ffee); break;
        case SolveStep::BATCH_DIV:
          for (uint32_t k = st.a; k < st.a + st.b; k++) W[c.A.terms[c.A.rowptr[k]].wire] = dot(c.C, k, 0) * inv0(dot(c.B, k, 0));
          break;
        case SolveStep::COUNT8: {
          std::vector<uint64_t> cnt(256, 0);
          for (uint32_t i = 0; i < st.b; i++) {
            uint32_t cw[8];
            canonical(dot(c.H, st.a + i, 0), cw);
            if (cw[0] < 256 && (cw[1] | cw[2] | cw[3] | cw[4] | cw[5] | cw[6] | cw[7]) == 0) cnt[cw[0]]++;
          }
          for (uint32_t j = 0; j < 256; j++) W[st.c + j] = Fr::from_u64(cnt[j]);
          break;
        }
        case SolveStep::SEQ:
          if (!by_plan) { if (!exec_range(st.a, st.b)) return false; break; }
          for (uint32_t t = st.ntracks; t-- > 0;)
            for (uint32_t it = st.tr_begin[t]; it < st.tr_end[t]; it++) {
              const uint32_t kind = pl.items[3 * it], a = pl.items[3 * it + 1], b = pl.items[3 * it + 2];
              if (kind == COOP_SEQ) { if (!exec_range(a, b)) return false; }
              else if (kind == COOP_PAR) {
                for (uint32_t g = b; g-- > a;) if (!exec_range(pl.par[2 * g], pl.par[2 * g + 1])) return false;
              } else if (kind == COOP_COUNTN) { if (!exec_op(a)) return false; }
              else if (kind == COOP_LEVELS) {
                std::vector<std::vector<LevelRow>> levels;
                for (uint32_t lv = a; lv < b; lv++) {
                  levels.emplace_back();
                  for (uint32_t r = pl.lvl_ptr[lv]; r < pl.lvl_ptr[lv + 1]; r++) {
                    const uint32_t k = pl.lvl_rows[r], gs = pl.lvl_gen[3 * r];
                    LevelRow lr{0, gs == COOP_NONE ? 2u : gs, pl.lvl_gen[3 * r + 1], pl.lvl_gen[3 * r + 2], gs != COOP_NONE, false, {}};
                    lr.out = mats[lr.side]->terms[mats[lr.side]->rowptr[k + 1] - 1].wire;
                    for (uint32_t mi = 0; mi < 3; mi++)
                      for (uint32_t t2 = mats[mi]->rowptr[k]; t2 + (mi == lr.side ? 1u : 0u) < mats[mi]->rowptr[k + 1]; t2++)
                        lr.t[mi].push_back({mats[mi]->terms[t2].wire, mats[mi]->terms[t2].coeff});
                    levels.back().push_back(lr);
                  }
                }
                if (!exec_levels(levels)) return false;
              } else if (kind == COOP_LEVEL_STREAM) {
                std::vector<std::vector<LevelRow>> levels;
                for (uint32_t ch = a; ch < a + b; ch++) {
                  const uint32_t* sb = pl.stream.data() + (size_t)ch * COOP_CHUNK;
                  for (uint32_t pos = 0; pos < COOP_CHUNK && sb[pos] != 0xffffffffu; pos += sb[pos + 1]) {
                    levels.emplace_back();
                    const uint32_t nr = sb[pos] & 0xffffffu, G = (sb[pos] >> 24) & 31u;
                    if (G == 0 || (G & (G - 1)) || G > 16 || pos + sb[pos + 1] > COOP_CHUNK) { fprintf(stderr, "bad level header\n"); return false; }
                    for (uint32_t r = 0; r < nr; r++) {
                      const uint32_t base = pos + sb[pos + 2 + r];
                      const bool gen = (sb[base + 2] & COOP_ROW_GENERIC) != 0;
                      LevelRow lr{sb[base], gen ? (sb[base + 2] >> COOP_ROW_SIDE_SHIFT) & 3u : 2u, gen ? sb[base + 4] : COOP_NONE,
                                  gen ? sb[base + 5] : COOP_NONE, gen, (sb[base + 1] >> 31) != 0, {}};
                      const uint32_t n3[3] = {sb[base + 1] & 0x7fffffffu, sb[base + 2] & COOP_ROW_COUNT_MASK, sb[base + 3]};
                      uint32_t at = base + (gen ? 6 : 4);
                      for (uint32_t mi = 0; mi < 3; mi++)
                        for (uint32_t t2 = 0; t2 < n3[mi]; t2++, at += 2) lr.t[mi].push_back({sb[at], sb[at + 1]});
                      if (at > pos + sb[pos + 1]) { fprintf(stderr, "row record leaves its level\n"); return false; }
                      levels.back().push_back(lr);
                    }
                  }
                }
                // consecutive sub-levels of one level are independent, so the rule "no read of the same or a later level" is asked
                // of the sub-levels as they stand: stricter than the levels need
                if (!exec_levels(levels)) return false;
              } else { fprintf(stderr, "item kind %u not supported by the check\n", kind); return false; }
            }
          break;
      }
    }
    return true;
  };
  std::vector<Fr> W0 = fresh(), W1 = fresh();
  // (the level rows built from the tables carry coefficient indices, those from the stream coefficient words: an index is a word
  // with no flag set, so word_dot reads both)
  if (!run(false, W0) || !run(true, W1)) return 1;
  uint32_t mismatches = 0, first = 0;
  for (uint32_t w = 0; w < c.n_wires; w++)
    if (!(W0[w] - W1[w]).is_zero()) { if (!mismatches) first = w; mismatches++; }
  uint32_t tracks = 0;
  for (const SolveStep& st : schedule) if (st.kind == SolveStep::SEQ) tracks = std::max(tracks, st.ntracks);
  printf("generic_ops %d generic_rows %u generic_divs %u items_seq %u items_par %u items_levels %u items_level_stream %u items_countn %u "
         "stream_chunks %u tracks %u mismatches %u first %u\n",
         generic_ops ? 1 : 0, pl.generic_rows, pl.generic_divs, pl.item_count[COOP_SEQ], pl.item_count[COOP_PAR], pl.item_count[COOP_LEVELS],
         pl.item_count[COOP_LEVEL_STREAM], pl.item_count[COOP_COUNTN], pl.stream_chunks, tracks, mismatches, first);
  return mismatches ? 1 : 0;
}
