// libspp C ABI, circuit loading: the proving-key container, the window plan and the window tables in HBM, load_circuit_impl as
// a list of steps, the circuit queries, and the fixed-base MSM unit calls (they share the table builder).
#include "spp_circuit.hpp"

static std::vector<PendingTable<Fq>>& pending(spp_circuit* c, Fq*) { return c->pending1; }
static std::vector<PendingTable<Fq2>>& pending(spp_circuit* c, Fq2*) { return c->pending2; }

static int upload_sparse(spp_circuit* c, const Circuit& circ, const Sparse& m, DevSparse* out) {
  std::vector<uint32_t> wire(m.terms.size()), coeff(m.terms.size()), lit(m.terms.size(), 0);
  Fr one = Fr::one(), mone = Fr::one().neg();
  // small literals, per coefficient-table entry: canonical value v < 2^28, or p - v < 2^28
  std::vector<uint32_t> small(circ.coeffs.size(), 0);
  for (size_t ci = 0; ci < circ.coeffs.size(); ci++) {
    uint32_t v[8], nv[8];
    circ.coeffs[ci].to_canonical(v);
    bool hi0 = true;
    for (int k = 1; k < 8; k++) hi0 = hi0 && v[k] == 0;
    if (hi0 && v[0] != 0 && v[0] < (1u << 28)) { small[ci] = v[0]; continue; }
    circ.coeffs[ci].neg().to_canonical(nv);
    hi0 = true;
    for (int k = 1; k < 8; k++) hi0 = hi0 && nv[k] == 0;
    if (hi0 && nv[0] != 0 && nv[0] < (1u << 28)) small[ci] = nv[0] | 0x80000000u;
  }
  for (size_t i = 0; i < m.terms.size(); i++) {
    wire[i] = m.terms[i].wire;
    uint32_t ci = m.terms[i].coeff;
    uint32_t flag = 0;
    if (circ.coeffs[ci] == one) flag = COEFF_ONE;
    else if (circ.coeffs[ci] == mone) flag = COEFF_MINUS_ONE;
    else lit[i] = small[ci];
    coeff[i] = ci | flag;
  }
  uint32_t *rp, *w, *co, *li;
  if (int e = own_upload(c, &li, lit)) return e;
  out->lit = li;
  if (int e = own_upload(c, &rp, m.rowptr)) return e;
  if (int e = own_upload(c, &w, wire)) return e;
  if (int e = own_upload(c, &co, coeff)) return e;
  out->rowptr = rp;
  out->wire = w;
  out->coeff = co;
  return 0;
}

// window tables: allocate first (all sets), then build with temporaries sized from the HBM that is left, so that
// each launch has enough rows (>= tens of thousands of lanes) to fill the chip
template <class F>
static int alloc_table_elems(spp_circuit* c, size_t table_elems, Affine<F>** table_out) {
  table_elems = std::max<size_t>(table_elems, 1);
  Affine<F>* table;
  HIP_TRY(hipMalloc((void**)&table, table_elems * sizeof(Affine<F>)));
  c->owned.push_back(table);
  c->table_bytes += table_elems * sizeof(Affine<F>);   // the bytes really allocated
  *table_out = table;
  return 0;
}
template <class F>
static int alloc_table(spp_circuit* c, size_t N, uint32_t cbits, uint32_t Wt, Affine<F>** table_out) {
  return alloc_table_elems<F>(c, msm_table_elems((uint32_t)N, cbits, Wt), table_out);
}
// layout / blocks: the ragged layout of a flat set and its device copy (null: the uniform layout).  Blocks of equal length are
// built together, in launches of at most `chunk` rows; the rows of narrow blocks cost at most 256 additions each.
template <class F>
static int build_table(spp_circuit* c, const std::vector<Affine<F>>& pts, uint32_t cbits, uint32_t Wt, Affine<F>* table, size_t temp_budget,
                       const MsmRagged* layout = nullptr, const MsmBlock* blocks = nullptr) {
  hipStream_t st = c->ctx->stream;
  const uint32_t Wn = Wt, Efull = 1u << (cbits - 1);
  const size_t N = pts.size();
  if (N == 0) return 0;
  if (!layout || layout->blocks.empty()) { layout = nullptr; blocks = nullptr; }
  const size_t rows_total = msm_table_rows(N, Wn);
  uint32_t Emax = layout ? 1 : Efull;
  if (layout) for (const MsmBlock& b : layout->blocks) Emax = std::max(Emax, b.E);
  const size_t per_row = (size_t)Emax * (sizeof(XYZZ<F>) + sizeof(F));
  size_t chunk = std::max<size_t>(64, ((temp_budget / per_row) / 64) * 64);
  chunk = std::min(chunk, (size_t)65536);   // larger launches only add TLB misses (the d-stride is chunk * 128 B)
  chunk = std::min(chunk, rows_total);
  DevBuf d_bases, tmp, tmp_pre;   // released on every return path
  HIP_TRY(d_bases.alloc(N * sizeof(Affine<F>)));
  HIP_TRY(hipMemcpy(d_bases.p, pts.data(), N * sizeof(Affine<F>), hipMemcpyHostToDevice));
  HIP_TRY(tmp.alloc(chunk * Emax * sizeof(XYZZ<F>)));
  HIP_TRY(tmp_pre.alloc(chunk * Emax * sizeof(F)));
  for (size_t r0 = 0; r0 < rows_total;) {
    size_t r1 = rows_total;   // end of the run of blocks as long as the one at r0
    uint32_t E = Efull;
    if (layout) {
      E = layout->blocks[r0 >> 6].E;
      r1 = r0 + 64;
      while (r1 < rows_total && layout->blocks[r1 >> 6].E == E) r1 += 64;
    }
    uint32_t cnt = (uint32_t)std::min(chunk, r1 - r0);
    launch_build_table<F>(st, d_bases.as<Affine<F>>(), (uint32_t)N, cbits, Wt, (uint32_t)r0, cnt, table, tmp.as<XYZZ<F>>(), tmp_pre.as<F>(), blocks, E);
    r0 += cnt;
  }
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return 0;
}
static size_t table_temp_budget() {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return (size_t)2 << 30;
  size_t b = free_b / 2;                       // leave room for the batch workspaces
  b = std::min(b, (size_t)48 << 30);
  return std::max(b, (size_t)1 << 28);
}
template <class F>
static int build_table_chunked(spp_circuit* c, const std::vector<Affine<F>>& pts, uint32_t cbits, uint32_t Wt, Affine<F>** table_out) {
  if (int e = alloc_table<F>(c, pts.size(), cbits, Wt, table_out)) return e;
  return build_table<F>(c, pts, cbits, Wt, *table_out, std::min(table_temp_budget(), (size_t)2 << 30));
}


// bound: range class of every base (msm_classes.hpp; empty: all wide).  A flat set is put in class-major order and gets the ragged
// table layout (msm_ragged.hpp); with every base wide both leave the set as it is, the uniform layout bit for bit.
template <class F>
static int make_set(spp_circuit* c, MsmSet<F>* set, std::vector<uint32_t> rows, std::vector<Affine<F>> pts, bool from_h, uint32_t cbits,
                    bool flat, std::vector<uint32_t> bound = {}, std::vector<uint32_t>* rows_kept = nullptr) {
  set->N = (uint32_t)pts.size();
  set->from_h = from_h;
  set->c = cbits;
  set->Wt = flat ? 1 : msm_windows(cbits);
  if (!flat) {
    if (int e = own_upload(c, &set->rows, rows)) return e;
    if (int e = alloc_table<F>(c, pts.size(), cbits, set->Wt, &set->table)) return e;
    pending(c, (F*)nullptr).push_back({std::move(pts), set->table, cbits, set->Wt, MsmRagged{}, nullptr});
    return 0;
  }
  bound.resize(pts.size(), 0);
  if (!c->sw.ragged) std::fill(bound.begin(), bound.end(), 0u);
  const std::vector<uint32_t> perm = msm_class_major_order(bound.data(), bound.size(), cbits);
  std::vector<uint32_t> rows_o(perm.size()), bound_o(perm.size());
  std::vector<Affine<F>> pts_o(perm.size());
  for (size_t k = 0; k < perm.size(); k++) {
    rows_o[k] = rows[perm[k]];
    pts_o[k] = pts[perm[k]];
    bound_o[k] = bound[perm[k]];
  }
  MsmRagged layout = msm_ragged_layout(bound_o.data(), bound_o.size(), cbits);
  set->narrow = layout.narrow(cbits);
  if (int e = own_upload(c, &set->rows, rows_o)) return e;
  if (rows_kept) *rows_kept = rows_o;   // the set's rows in table order (load_lookup_buckets)
  if (layout.blocks.empty()) layout.blocks.push_back({0, 1u << (cbits - 1), 0});   // an empty set: nothing is read, the upload is not empty
  if (int e = own_upload(c, &set->blocks, layout.blocks)) return e;
  if (int e = alloc_table_elems<F>(c, layout.elems(), &set->table)) return e;
  if (pts_o.empty()) layout.blocks.clear();
  pending(c, (F*)nullptr).push_back({std::move(pts_o), set->table, cbits, set->Wt, std::move(layout), set->blocks});
  return 0;
}
static int build_pending(spp_circuit* c) {
  const size_t budget = table_temp_budget();
  int e = 0;
  for (auto& p : pending(c, (Fq*)nullptr)) if (!e) e = build_table<Fq>(c, p.pts, p.c, p.Wt, p.table, budget, &p.layout, p.blocks);
  for (auto& p : pending(c, (Fq2*)nullptr)) if (!e) e = build_table<Fq2>(c, p.pts, p.c, p.Wt, p.table, budget, &p.layout, p.blocks);
  pending(c, (Fq*)nullptr).clear();
  pending(c, (Fq2*)nullptr).clear();
  return e;
}

// -----------------------------------------------------------------------------------------------------
// pk container
// -----------------------------------------------------------------------------------------------------
namespace {
struct PkFile {
  uint32_t circuit_id, n_wires, domain_log, n_public, challenge_wire;
  G1Affine alpha1, beta1, delta1;
  G2Affine beta2, delta2;
  std::vector<uint32_t> A_w, B1_w, B2_w, K_w, CB_w, CS_w;
  std::vector<G1Affine> A, B1, K, Z, CB, CS;
  std::vector<G2Affine> B2;
};
struct Rd {
  const uint8_t* p;
  const uint8_t* end;
  bool ok = true;
  uint32_t u32() {
    if (p + 4 > end) { ok = false; return 0; }
    uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    p += 4;
    return v;
  }
  const uint8_t* take(size_t n) {
    if (p + n > end) { ok = false; return nullptr; }
    const uint8_t* q = p;
    p += n;
    return q;
  }
};
bool rd_g1_section(Rd& r, std::vector<uint32_t>* wires, std::vector<G1Affine>& pts) {
  uint32_t n = r.u32();
  if (!r.ok || (size_t)n * 64 > (size_t)(r.end - r.p)) return false;
  if (wires) {
    wires->resize(n);
    for (auto& w : *wires) w = r.u32();
  }
  pts.resize(n);
  for (auto& pt : pts) {
    const uint8_t* b = r.take(64);
    if (!b) return false;
    pt = g1_from_raw(b);
  }
  return r.ok;
}
bool parse_pk(const std::vector<uint8_t>& buf, PkFile& k) {
  Rd r{buf.data(), buf.data() + buf.size()};
  if (r.u32() != 0x4b505053u || r.u32() != 1) return false;
  k.circuit_id = r.u32(); k.n_wires = r.u32(); k.domain_log = r.u32(); k.n_public = r.u32(); k.challenge_wire = r.u32();
  const uint8_t* b;
  if (!(b = r.take(64))) return false; k.alpha1 = g1_from_raw(b);
  if (!(b = r.take(64))) return false; k.beta1 = g1_from_raw(b);
  if (!(b = r.take(64))) return false; k.delta1 = g1_from_raw(b);
  if (!(b = r.take(128))) return false; k.beta2 = g2_from_raw(b);
  if (!(b = r.take(128))) return false; k.delta2 = g2_from_raw(b);
  if (!rd_g1_section(r, &k.A_w, k.A)) return false;
  if (!rd_g1_section(r, &k.B1_w, k.B1)) return false;
  uint32_t n2 = r.u32();
  if (!r.ok || (size_t)n2 * 128 > (size_t)(r.end - r.p)) return false;
  k.B2_w.resize(n2);
  for (auto& w : k.B2_w) w = r.u32();
  k.B2.resize(n2);
  for (auto& pt : k.B2) {
    if (!(b = r.take(128))) return false;
    pt = g2_from_raw(b);
  }
  if (!rd_g1_section(r, &k.K_w, k.K)) return false;
  if (!rd_g1_section(r, nullptr, k.Z)) return false;
  if (!rd_g1_section(r, &k.CB_w, k.CB)) return false;
  if (!rd_g1_section(r, &k.CS_w, k.CS)) return false;
  return r.ok && r.p == r.end;
}
}  // namespace


// merge `extra` into the entry of `wire` (or append one)
template <class F>
static void merge_point(std::vector<uint32_t>& wires, std::vector<Affine<F>>& pts, uint32_t wire, const Affine<F>& extra) {
  for (size_t i = 0; i < wires.size(); i++)
    if (wires[i] == wire) {
      pts[i] = host_add(pts[i], extra);
      return;
    }
  wires.push_back(wire);
  pts.push_back(extra);
}

// What the steps of load_circuit_impl share beyond the circuit itself.
struct LoadState {
  PkFile pk;
  uint32_t cw[7];   // window bits per MSM set: A, B1, K, Z, CB, CS, B2
  WireClasses wc;   // range class of every wire (msm_classes.hpp; all wide under SPP_RAGGED=0)
  bool flat[7] = {false, false, false, false, false, false, false};   // one table row per base (else one per window)
  // the H bases as rows / points of the Z set and, in the product form, the per-wire column sums that join the K set
  std::vector<uint32_t> rows_a, rows_k;   // rows of the flat A and K sets in table order (empty: not flat)
  std::vector<uint32_t> z_w, xk_w;
  std::vector<G1Affine> z_p, xk_p;
};

// the experiment switches of the proving path, from the environment (see Switches, spp_circuit.hpp)
static Switches read_switches() {
  Switches sw;
  const char* hm = getenv("SPP_H_MODE");
  sw.h_mode = hm ? atoi(hm) : (getenv("SPP_Z_COEFF") ? 0 : 2);
  if (sw.h_mode < 0 || sw.h_mode > 2) sw.h_mode = 2;
  sw.no_coop = getenv("SPP_NO_COOP") != nullptr;
  sw.trace_items = getenv("SPP_COOP_TRACE") != nullptr;
  sw.one_track = getenv("SPP_COOP_ONE_TRACK") != nullptr;
  sw.no_level_stream = getenv("SPP_NO_LEVEL_STREAM") != nullptr;
  if (const char* e = getenv("SPP_COOP_MAX")) sw.coop_max_batch = (uint32_t)atoi(e);
  sw.no_side = getenv("SPP_NO_SIDE") != nullptr;
  const char* de = getenv("SPP_DEPTH");
  const int depth = de ? atoi(de) : 0;
  sw.forced_depth = depth >= 1 && depth <= SPP_NWS ? depth : 0;
  sw.no_split = getenv("SPP_NO_SPLIT") != nullptr;
  const char* rg = getenv("SPP_RAGGED");
  sw.ragged = !(rg && rg[0] == '0');
  if (const char* lb = getenv("SPP_LOOKUP_BUCKETS")) {
    const int v = atoi(lb);
    sw.lookup_min_batch = v <= 0 ? 0u : (uint32_t)std::max(v, 64);
    sw.lookup_forced = v > 0;
  }
  sw.msm = msm_tuning_from_env(getenv("SPP_MSM_WAVES"), getenv("SPP_MSM_WAVES_SMALL"));
  return sw;
}

// Window bits and table layout per MSM set.
//  * window_bits given: every set gets one table row per window (msm_windows(c) rows of 2^(c-1) multiples per base) -- small
//    tables, a single pass, no Horner step: the layout of the one-proof latency path (the drop-in helpers load 8 bits).
//  * window_bits = 0 (throughput): the five big sets keep ONE row per base and walk it once per window ("flat", see
//    msm_table.hpp); the window of every set is a greedy split of the HBM budget (env SPP_TABLE_BUDGET_GB, default 240 of the
//    288 GB, capped at 85 % of the free HBM): repeatedly widen the set whose next window bit removes the most mixed-addition
//    work per extra byte (a G2 addition is weighted 3 G1 additions, as measured).  A flat G1 row at 16 bits is 2 MB per base
//    and costs 16 additions per full-size scalar; the row-per-window layout of rounds 1-2 afforded 11-12 bits (22-24
//    additions) in the same bytes (SPP_FLAT=0 brings it back for comparison).  The two commitment sets only ever see bytes /
//    small counters and sit on the critical path of the challenge: row-per-window tables at 9 bits, no passes.
//    A bit is priced at what it costs (plan_greedy, msm_ragged.hpp): the bases of A, B1, B2 and K whose wire is a bit or a byte
//    (wc) keep rows of 1 / 256 entries whatever the window, so only the wide bases pay for a bit and only they gain by it.
static int plan_load_windows(const PkFile& pk, const WireClasses& wc, int window_bits, const uint32_t* forced_bits, uint32_t cw[7], bool flat[7]) {
  const double nset[7] = {(double)pk.A.size() + 2, (double)pk.B1.size() + 2, (double)pk.K.size() + 1, (double)pk.Z.size(),
                          (double)pk.CB.size(), (double)pk.CS.size(), (double)pk.B2.size() + 2};
  if (forced_bits) {           // spp_load_circuit_with_windows: the caller planned the windows (spp_plan_windows), throughput layout
    for (int s = 0; s < 7; s++) {
      cw[s] = forced_bits[s];
      flat[s] = PLAN_WGT[s] != 0;
    }
  } else if (window_bits != 0) {
    for (int s = 0; s < 7; s++) cw[s] = (uint32_t)window_bits;
  } else {
    const char* fe = getenv("SPP_FLAT");
    const bool use_flat = !(fe && fe[0] == '0');
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    double budget = 240e9;
    if (const char* env = getenv("SPP_TABLE_BUDGET_GB")) budget = atof(env) * 1e9;
    budget = std::min(budget, 0.85 * (double)free_b);
    std::vector<PlanSet> sets;
    for (int s = 0; s < 7; s++) {
      flat[s] = use_flat && PLAN_WGT[s] != 0;
      sets.push_back(plan_set(s, nset[s], flat[s]));
    }
    const std::vector<uint32_t>* keyed[7] = {&pk.A_w, &pk.B1_w, &pk.K_w, nullptr, nullptr, nullptr, &pk.B2_w};
    for (int s = 0; s < 7; s++)
      if (keyed[s] && flat[s])
        for (uint32_t b : msm_base_bounds(wc, *keyed[s])) plan_count(sets[s], b);
    plan_greedy(sets, budget, use_flat ? 16 : 15);
    for (int s = 0; s < 7; s++) cw[s] = (uint32_t)sets[s].bits;
  }
  return 0;
}

static int load_r1cs(spp_circuit* c) {
  const Circuit& circ = c->circ;
  int e;
  if ((e = upload_sparse(c, circ, circ.A, &c->dc.A)) || (e = upload_sparse(c, circ, circ.B, &c->dc.B)) ||
      (e = upload_sparse(c, circ, circ.C, &c->dc.C)) || (e = upload_sparse(c, circ, circ.H, &c->dc.H)))
    return e;
  Fr* d_coeffs;
  Fr* d_aux;
  uint32_t* d_prog;
  if ((e = own_upload(c, &d_coeffs, circ.coeffs)) || (e = own_upload(c, &d_prog, circ.program)) || (e = own_upload(c, &d_aux, circ.aux))) return e;
  c->dc.coeffs = d_coeffs;
  c->dc.aux = d_aux;
  c->dc.program = d_prog;
  c->dc.n_wires = circ.n_wires;
  c->dc.n_constraints = circ.n_constraints;
  {
    // runs of consecutive constraints with identical B rows (at most 8 long, so lanes stay comparable in cost)
    std::vector<uint32_t> runs;
    auto same_b = [&](uint32_t k) {
      const uint32_t a0 = circ.B.rowptr[k - 1], a1 = circ.B.rowptr[k], b1 = circ.B.rowptr[k + 1];
      if (a1 - a0 != b1 - a1 || a1 == a0) return false;
      for (uint32_t t = 0; t < a1 - a0; t++)
        if (circ.B.terms[a0 + t].wire != circ.B.terms[a1 + t].wire || circ.B.terms[a0 + t].coeff != circ.B.terms[a1 + t].coeff) return false;
      return true;
    };
    uint32_t len = 0;
    for (uint32_t k = 0; k < circ.n_constraints; k++) {
      if (k == 0 || len >= 8 || !same_b(k)) { runs.push_back(k); len = 0; }
      len++;
    }
    const uint32_t n_runs = (uint32_t)runs.size();
    runs.push_back(circ.n_constraints);
    uint32_t* d_runs;
    if ((e = own_upload(c, &d_runs, runs))) return e;
    c->dc.run_start = d_runs;
    c->dc.n_runs = n_runs;
    uint32_t longest = 0;
    for (const Sparse* m : {&circ.A, &circ.B, &circ.C})
      for (uint32_t k = 0; k < circ.n_constraints; k++) longest = std::max(longest, m->rowptr[k + 1] - m->rowptr[k]);
    c->dc.max_row_terms = longest;
    std::vector<uint8_t> flags(std::max<uint32_t>(circ.n_constraints, 1), 0);
    for (uint32_t k = 0; k < circ.n_constraints; k++) {
      if (k > 0 && same_b(k)) flags[k] |= 1;
      const uint32_t a0 = circ.A.rowptr[k], a1 = circ.A.rowptr[k + 1], b0 = circ.B.rowptr[k], b1 = circ.B.rowptr[k + 1];
      bool eq = a1 - a0 == b1 - b0 && a1 != a0;
      for (uint32_t t = 0; eq && t < a1 - a0; t++)
        eq = circ.A.terms[a0 + t].wire == circ.B.terms[b0 + t].wire && circ.A.terms[a0 + t].coeff == circ.B.terms[b0 + t].coeff;
      if (eq) flags[k] |= 2;
    }
    uint8_t* d_flags;
    if ((e = own_upload(c, &d_flags, flags))) return e;
    c->dc.row_flags = d_flags;
  }
  c->dc.n_public = circ.n_public;
  c->dc.n_inputs = circ.n_inputs();
  c->dc.challenge_wire = circ.challenge_wire;
  // the hash constants are the context's (one copy in HBM for every circuit and the stand-alone hash kernels)
  if ((e = spp_ensure_ctx_consts(c->ctx))) return e;
  c->dc.hc = c->ctx->hc;
  std::vector<Fr> bytes(256);
  for (int i = 0; i < 256; i++) bytes[i] = Fr::from_u64((uint64_t)i);
  Fr* bm;
  if ((e = own_upload(c, &bm, bytes))) return e;
  c->dc.byte_mont = bm;
  return 0;
}

static int load_program(spp_circuit* c) {
  const Circuit& circ = c->circ;
  // the schedule (coop_plan.hpp, solver_schedule): sequential segments and wide steps, the commitment boundary in between.
  // SPP_SOLVE_TRACE=1 (diagnostic): one launch per instruction class run, so a kernel trace of a proof shows where the
  // sequential solver spends its time
  bool generic_ops = false;
  const bool trace_ops = getenv("SPP_SOLVE_TRACE") != nullptr;
  if (trace_ops) c->sw.no_coop = true;
  if (const uint32_t bad = solver_schedule(circ.program, trace_ops, &c->schedule, &c->max_batch_div, &generic_ops))
    return fail(SPP_ERR_FORMAT, "bad opcode %u in solver program", bad);

  // the solver of a decoded gnark system (spp/ccs.py to_sppc_solved) is planned like any other program: coop_build_plan puts its
  // rows into levels and its hints into items; only the batch size up to which one wave per proof pays is the program's own
  c->generic_solver = generic_ops;
  if (generic_ops && !getenv("SPP_COOP_MAX")) c->sw.coop_max_batch = c->sw.coop_max_batch_generic;
  if (int e = coop_plan(c)) return e;
  if (int e = row_paths_plan(c)) return e;
  return 0;
}

static int load_ntt_tables(spp_circuit* c) {
  int e;
  const uint32_t n = c->n, logn = c->logn;
  Fr w = fr_root_of_unity(logn), wi = w.inv();
  std::vector<Fr> tf(n / 2), ti(n / 2), cb(n), cib(n);
  Fr a = Fr::one(), b = Fr::one();
  for (uint32_t k = 0; k < n / 2; k++) {
    tf[k] = a;
    ti[k] = b;
    a = a * w;
    b = b * wi;
  }
  // the coset: gnark's multiplicative generator 5, or -- product form -- zeta, the primitive 2n-th root of unity with
  // zeta^2 = w, so that H u zeta*H are the 2n-th roots of unity
  Fr g = c->sw.h_mode == 2 ? fr_root_of_unity(logn + 1) : Fr::from_u64(5), gi = g.inv(), ninv = Fr::from_u64(n).inv();
  std::vector<Fr> gp(n), gip(n);
  Fr x = ninv, y = ninv;
  for (uint32_t i = 0; i < n; i++) {
    gp[i] = x;
    gip[i] = y;
    x = x * g;
    y = y * gi;
  }
  for (uint32_t pos = 0; pos < n; pos++) {
    uint32_t i = bitrev(pos, logn);
    cb[pos] = gp[i];
    cib[pos] = gip[i];
  }
  if ((e = own_upload(c, &c->tw_fwd, tf)) || (e = own_upload(c, &c->tw_inv, ti)) || (e = own_upload(c, &c->coset_br, cb)) ||
      (e = own_upload(c, &c->coset_inv_br, cib)))
    return e;
  Fr gn = g.pow_u64(n);
  c->zinv = (gn - Fr::one()).inv();
  return 0;
}

// the sets whose bases come straight from the key: A, B1, B2
static int load_key_sets(spp_circuit* c, LoadState& s) {
  const PkFile& pk = s.pk;
  const uint32_t* cw = s.cw;
  const bool* flat = s.flat;
  int e;
  {
    std::vector<uint32_t> w = pk.A_w;
    std::vector<G1Affine> p = pk.A;
    merge_point(w, p, 0u, pk.alpha1);
    w.push_back(c->row_r); p.push_back(pk.delta1);
    if ((e = make_set(c, &c->A, w, p, false, cw[0], flat[0], msm_base_bounds(s.wc, w), &s.rows_a))) return e;
  }
  {
    std::vector<uint32_t> w = pk.B1_w;
    std::vector<G1Affine> p = pk.B1;
    merge_point(w, p, 0u, pk.beta1);
    w.push_back(c->row_s); p.push_back(pk.delta1);
    if ((e = make_set(c, &c->B1, w, p, false, cw[1], flat[1], msm_base_bounds(s.wc, w)))) return e;
  }
  {
    std::vector<uint32_t> w = pk.B2_w;
    std::vector<G2Affine> p = pk.B2;
    merge_point(w, p, 0u, pk.beta2);
    w.push_back(c->row_s); p.push_back(pk.delta2);
    if ((e = make_set(c, &c->B2, w, p, false, cw[6], flat[6], msm_base_bounds(s.wc, w)))) return e;
  }
  return 0;
}

// the H bases (and, in the product form, the per-wire column sums that join the K set)
static int load_h_bases(spp_circuit* c, LoadState& s) {
  const PkFile& pk = s.pk;
  const Circuit& circ = c->circ;
  spp_ctx* ctx = c->ctx;
  std::vector<uint32_t>&z_w = s.z_w, &xk_w = s.xk_w;
  std::vector<G1Affine>&z_p = s.z_p, &xk_p = s.xk_p;
  int e;
  if (pk.Z.size() != (size_t)c->n - 1) return fail(SPP_ERR_FORMAT, "Z section has %zu points, expected %u", pk.Z.size(), c->n - 1);
  const uint32_t n = c->n;
  hipStream_t st = ctx->stream;
  // out[i] = sum_j scale[j] w^(-ij) Z_j, natural order (group DFT on the device, kernels_msm.hip)
  auto eval_basis = [&](const std::vector<Fr>& scale, std::vector<G1Affine>& out) -> int {
    DevBuf d_pts, d_scale, d_work, d_out;
    HIP_TRY(d_pts.alloc(pk.Z.size() * sizeof(G1Affine)));
    HIP_TRY(d_scale.alloc((size_t)n * sizeof(Fr)));
    HIP_TRY(d_work.alloc((size_t)n * sizeof(G1XYZZ)));
    HIP_TRY(d_out.alloc((size_t)n * sizeof(G1Affine)));
    HIP_TRY(hipMemcpyAsync(d_pts.p, pk.Z.data(), pk.Z.size() * sizeof(G1Affine), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_scale.p, scale.data(), (size_t)n * sizeof(Fr), hipMemcpyHostToDevice, st));
    launch_g1_eval_basis(st, d_pts.as<G1Affine>(), (uint32_t)pk.Z.size(), c->logn, d_scale.as<Fr>(), c->tw_inv, d_work.as<G1XYZZ>(),
                         d_out.as<G1Affine>());
    std::vector<G1Affine> br(n);
    HIP_TRY(hipMemcpyAsync(br.data(), d_out.p, (size_t)n * sizeof(G1Affine), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipGetLastError());
    out.resize(n);
    for (uint32_t pos = 0; pos < n; pos++) out[bitrev(pos, c->logn)] = br[pos];     // the DIF stages leave element i at bitrev(i)
    return 0;
  };
  if (c->sw.h_mode == 0) {
    // h comes out of the last DIF pass in bit-reversed order: row `pos` holds h_{bitrev(pos)}
    for (uint32_t pos = 0; pos < n; pos++) {
      uint32_t i = bitrev(pos, c->logn);
      if (i == n - 1) continue;
      z_w.push_back(pos);
      z_p.push_back(pk.Z[i]);
    }
  } else if (c->sw.h_mode == 1) {
    // sum_j h_j Z_j = sum_i h(g w^i) Z'_i with Z'_i = sum_j (g^-j / n) w^(-ij) Z_j; row i of the a-slot holds h(g w^i)
    Fr gi = Fr::from_u64(5).inv(), x = Fr::from_u64(n).inv();
    std::vector<Fr> scale(n);
    for (uint32_t j = 0; j < n; j++) { scale[j] = x; x = x * gi; }
    if ((e = eval_basis(scale, z_p))) return e;
    for (uint32_t i = 0; i < n; i++) z_w.push_back(i);
  } else {
    // Product form.  P = A B has degree <= 2n - 2 and h_j = P_{n+j}; over D = the 2n-th roots of unity P_k = (1/2n) sum_{x in D}
    // P(x) x^-k, hence  sum_j h_j Z_j = sum_{x in D} P(x) W_x  with  W_x = (1/2n) sum_j x^-(n+j) Z_j:
    //   x = w^i        (x^-n = 1):   W_i  =  (1/2n) sum_j w^(-ij) Z_j,              P(x) = a_i b_i = c_i = <C_i, witness>
    //   x = zeta w^i   (x^-n = -1):  W'_i = -(1/2n) sum_j zeta^-j w^(-ij) Z_j,      P(x) = A(x) B(x) from two coset transforms
    // The first sum is linear in the witness: sum_i c_i W_i = sum_wire w_wire X_wire, X_wire = sum_i C[i][wire] W_i -- a point per
    // wire, computed here once and added to the wire's base in the K set (wires without one -- public, committed, the
    // challenge -- join the set with X_wire alone: the sum is part of Krs whatever the wire's class).
    const Fr inv2n = Fr::from_u64(2 * (uint64_t)n).inv();
    std::vector<Fr> scale(n, inv2n);
    std::vector<G1Affine> WH;
    if ((e = eval_basis(scale, WH))) return e;
    Fr zi = fr_root_of_unity(c->logn + 1).inv(), x = inv2n.neg();
    for (uint32_t j = 0; j < n; j++) { scale[j] = x; x = x * zi; }
    if ((e = eval_basis(scale, z_p))) return e;
    for (uint32_t i = 0; i < n; i++) z_w.push_back(i);
    // column sums of C against W
    struct Tm { uint32_t wire, row; Fr cf; };
    std::vector<Tm> tms;
    for (uint32_t k = 0; k < circ.n_constraints; k++)
      for (uint32_t t = circ.C.rowptr[k]; t < circ.C.rowptr[k + 1]; t++) tms.push_back({circ.C.terms[t].wire, k, circ.coeffs[circ.C.terms[t].coeff]});
    std::stable_sort(tms.begin(), tms.end(), [](const Tm& a, const Tm& b) { return a.wire < b.wire; });
    std::vector<uint32_t> rows(tms.size()), seg{0};
    std::vector<Fr> cfs(tms.size());
    for (size_t t = 0; t < tms.size(); t++) {
      rows[t] = tms[t].row;
      cfs[t] = tms[t].cf;
      if (t + 1 == tms.size() || tms[t + 1].wire != tms[t].wire) {
        xk_w.push_back(tms[t].wire);
        seg.push_back((uint32_t)t + 1);
      }
    }
    if (!tms.empty()) {
      DevBuf d_base, d_rows, d_cfs, d_seg, d_work, d_out;
      HIP_TRY(d_base.alloc((size_t)n * sizeof(G1Affine)));
      HIP_TRY(d_rows.alloc(rows.size() * 4));
      HIP_TRY(d_cfs.alloc(cfs.size() * sizeof(Fr)));
      HIP_TRY(d_seg.alloc(seg.size() * 4));
      HIP_TRY(d_work.alloc(tms.size() * sizeof(G1XYZZ)));
      HIP_TRY(d_out.alloc(xk_w.size() * sizeof(G1Affine)));
      HIP_TRY(hipMemcpyAsync(d_base.p, WH.data(), (size_t)n * sizeof(G1Affine), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(d_rows.p, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(d_cfs.p, cfs.data(), cfs.size() * sizeof(Fr), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(d_seg.p, seg.data(), seg.size() * 4, hipMemcpyHostToDevice, st));
      launch_g1_column_sums(st, d_base.as<G1Affine>(), d_rows.as<uint32_t>(), d_cfs.as<Fr>(), (uint32_t)tms.size(), d_seg.as<uint32_t>(),
                            (uint32_t)xk_w.size(), d_work.as<G1XYZZ>(), d_out.as<G1Affine>());
      xk_p.resize(xk_w.size());
      HIP_TRY(hipMemcpyAsync(xk_p.data(), d_out.p, xk_p.size() * sizeof(G1Affine), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      HIP_TRY(hipGetLastError());
    }
  }
  return 0;
}

// the sets that depend on the H bases (K, Z) and the two commitment sets; then every table is built
static int load_h_sets(spp_circuit* c, LoadState& s) {
  const PkFile& pk = s.pk;
  const uint32_t* cw = s.cw;
  const bool* flat = s.flat;
  int e;
  const Circuit& circ = c->circ;
  const std::vector<uint32_t>&z_w = s.z_w, &xk_w = s.xk_w;
  const std::vector<G1Affine>&z_p = s.z_p, &xk_p = s.xk_p;
  {
    std::vector<uint32_t> w = pk.K_w;
    std::vector<G1Affine> p = pk.K;
    if (!xk_w.empty()) {   // product form: K_wire + X_wire (one pass over a wire -> position map; merge_point is linear per call)
      std::vector<int32_t> at(circ.n_wires + 3, -1);
      for (size_t i = 0; i < w.size(); i++) at[w[i]] = (int32_t)i;
      for (size_t i = 0; i < xk_w.size(); i++) {
        if (xk_p[i].is_inf()) continue;
        if (at[xk_w[i]] >= 0) p[at[xk_w[i]]] = host_add(p[at[xk_w[i]]], xk_p[i]);
        else {
          at[xk_w[i]] = (int32_t)w.size();
          w.push_back(xk_w[i]);
          p.push_back(xk_p[i]);
        }
      }
    }
    w.push_back(c->row_rs); p.push_back(pk.delta1.neg());
    // the key's own K bases inherit the class of their wire (a column sum added to the point does not change the scalar); the
    // wires that join the set through their column sum alone stay wide, like the blinding row
    std::vector<uint32_t> kb = msm_base_bounds(s.wc, pk.K_w);
    if ((e = make_set(c, &c->K, w, p, false, cw[2], flat[2], kb, &s.rows_k))) return e;
  }
  if ((e = make_set(c, &c->Z, z_w, z_p, true, cw[3], flat[3]))) return e;
  if ((e = make_set(c, &c->CB, pk.CB_w, pk.CB, false, cw[4], false))) return e;
  if ((e = make_set(c, &c->CS, pk.CS_w, pk.CS, false, cw[5], false))) return e;
  return build_pending(c);
}

// The lookup-inverse wires of the circuit on the flat A and K sets (msm_lookup.hpp): where their bases sit, and a copy of each
// set's rows in which they read MSM_ROW_ZERO.  Nothing is made -- and the proving path is the table walks alone -- when the switch
// is off, when either set has a table row per window, or when the scan finds too few such wires to pay for the second level
// (LKB_MIN_LOOKUPS; none at all under SPP_LOOKUP_BUCKETS=N).
static int load_lookup_buckets(spp_circuit* c, const LoadState& s) {
  if (c->sw.lookup_min_batch == 0 || c->A.Wt != 1 || c->K.Wt != 1 || c->A.N == 0 || c->K.N == 0) return 0;
  const std::vector<LookupInverse> lk = msm_lookup_inverses(c->circ);
  if (lk.empty() || (!c->sw.lookup_forced && lk.size() < LKB_MIN_LOOKUPS)) return 0;
  std::vector<int32_t> at(c->circ.n_wires, -1);
  std::vector<uint32_t> hints(lk.size());
  for (size_t j = 0; j < lk.size(); j++) {
    at[lk[j].wire] = (int32_t)j;
    hints[j] = lk[j].hint;
  }
  const std::vector<uint32_t>* rows[2] = {&s.rows_a, &s.rows_k};
  size_t found = 0;
  for (int k = 0; k < 2; k++) {
    std::vector<uint32_t> pos(lk.size(), MSM_ROW_ZERO), zeroed = *rows[k];
    for (size_t i = 0; i < zeroed.size(); i++)
      if (zeroed[i] < at.size() && at[zeroed[i]] >= 0) {
        pos[at[zeroed[i]]] = (uint32_t)i;
        zeroed[i] = MSM_ROW_ZERO;
        found++;
      }
    if (int e = own_upload(c, &c->lk_pos[k], pos)) return e;
    if (int e = own_upload(c, &c->lk_rows[k], zeroed)) return e;
  }
  if (found == 0) return 0;
  if (int e = own_upload(c, &c->lk_hints, hints)) return e;
  c->lk_n = (uint32_t)lk.size();
  return 0;
}

// streams and events of the batch workspaces
static int load_streams(spp_circuit* c) {
  spp_ctx* ctx = c->ctx;
  for (int k = 0; k < SPP_NWS; k++) {
    Workspace& w = c->ws[k];
    // SPP_SERIAL=1 (profiling aid): one stream for everything, so per-stage / per-kernel times are not stretched by
    // the other batch or by the G2 side stream
    const bool serial = getenv("SPP_SERIAL") != nullptr;
    w.own_st = ctx->pstream[k];
    if (int e = pick_concurrent_stream(w.own_st, &w.own_st2)) return e;
    {
      // Batches run the G2 sum on a side stream with a priority of its own.  Streams of one priority share a few hardware queues
      // round-robin; when st and st2 land on the same one the G2 sum runs in front of the matrix evaluation instead of beside it.
      // Measured on 2048-proof audit batches (same box, alternating): 4 747-4 760 proofs/s with the priority stream, 4 662-4 707
      // without.  Small batches keep the default-priority side stream: with a second queue class in use every dispatch of a single
      // proof's ~120 short kernels started later (audit 12.3 -> 13.6 ms).  SPP_ST2_PRIORITY=0 (diagnostic): never use it.
      int lo = 0, hi = 0;
      HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
      const char* pe = getenv("SPP_ST2_PRIORITY");
      if (!(pe && pe[0] == '0') && hi < lo) HIP_TRY(hipStreamCreateWithPriority(&w.own_st2p, hipStreamDefault, hi));
    }
    w.st = serial ? ctx->pstream[0] : w.own_st;
    w.st2 = serial ? w.st : w.own_st2;
    HIP_TRY(hipEventCreate(&w.g2_ev.first));
    HIP_TRY(hipEventCreate(&w.g2_ev.second));
    HIP_TRY(hipEventCreateWithFlags(&w.ev_w, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&w.ev_b2, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&w.ev_in, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&w.ev_rows, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(w.ev_in, w.st));
    for (auto& evt : w.ev) HIP_TRY(hipEventCreate(&evt));
    w.msm_ev.resize(8);
    for (auto& pr : w.msm_ev) {
      HIP_TRY(hipEventCreate(&pr.first));
      HIP_TRY(hipEventCreate(&pr.second));
    }
  }
  return 0;
}

static int load_circuit_impl(spp_ctx* ctx, const char* circuit_path, const char* pk_path, int window_bits, const uint32_t* forced_bits,
                             spp_circuit** out) {
  if (!ctx || !circuit_path || !pk_path || !out) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (window_bits != 0 && (window_bits < 4 || window_bits > 16)) return fail(SPP_ERR_BAD_INPUT, "window_bits %d outside [4,16]", window_bits);
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  spp_circuit* c = new spp_circuit();
  c->ctx = ctx;
  c->c_bits = (uint32_t)window_bits;
  // every early return below releases what has been allocated so far
  struct Guard {
    spp_circuit* c;
    ~Guard() { if (c) destroy_circuit(c); }
  } guard{c};
  if (!c->circ.load(circuit_path)) return fail(SPP_ERR_IO, "cannot read circuit %s", circuit_path);
  std::vector<uint8_t> pkbuf;
  LoadState s;
  PkFile& pk = s.pk;
  if (!read_file(pk_path, pkbuf)) return fail(SPP_ERR_IO, "cannot read proving key %s", pk_path);
  if (!parse_pk(pkbuf, pk)) return fail(SPP_ERR_FORMAT, "malformed proving key %s", pk_path);
  const Circuit& circ = c->circ;
  if (pk.circuit_id != circ.id || pk.n_wires != circ.n_wires || pk.domain_log != circ.domain_log)
    return fail(SPP_ERR_FORMAT, "proving key does not match the circuit");
  c->sw = read_switches();
  s.wc = msm_wire_classes(circ);
  if (!c->sw.ragged) s.wc = WireClasses{std::vector<uint32_t>(circ.n_wires, 0), std::vector<uint8_t>(circ.n_wires, WIRE_WIDE)};
  if (int e = plan_load_windows(pk, s.wc, window_bits, forced_bits, s.cw, s.flat)) return e;
  c->c_bits = s.cw[3];   // reported window = that of the largest set (Z)
  c->logn = circ.domain_log;
  c->n = 1u << c->logn;
  c->row_r = circ.n_wires;
  c->row_s = circ.n_wires + 1;
  c->row_rs = circ.n_wires + 2;
  c->n_rows = circ.n_wires + 3;
  c->in_stride = (size_t)circ.n_inputs() * 32;
  c->pw_stride = 12 + 32 * (size_t)(circ.n_public - 1);
  int e;
  if ((e = load_r1cs(c)) || (e = load_program(c)) || (e = load_ntt_tables(c)) || (e = load_key_sets(c, s)) || (e = load_h_bases(c, s)) ||
      (e = load_h_sets(c, s)) || (e = load_lookup_buckets(c, s)) || (e = load_streams(c)))
    return e;
  guard.c = nullptr;
  *out = c;
  return SPP_OK;
}
extern "C" int spp_load_circuit(spp_ctx* ctx, const char* circuit_path, const char* pk_path, int window_bits, spp_circuit** out) {
  return load_circuit_impl(ctx, circuit_path, pk_path, window_bits, nullptr, out);
}
extern "C" int spp_load_circuit_with_windows(spp_ctx* ctx, const char* circuit_path, const char* pk_path, const uint32_t bits[7],
                                             spp_circuit** out) {
  if (!bits) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  for (int s = 0; s < 7; s++)
    if (bits[s] < 4 || bits[s] > 16) return fail(SPP_ERR_BAD_INPUT, "window bits %u of set %d outside [4,16]", bits[s], s);
  return load_circuit_impl(ctx, circuit_path, pk_path, 0, bits, out);
}

void free_workspace(Workspace& w) {
  if (w.audit_scratch) hipFree(w.audit_scratch);
  w.audit_scratch = nullptr;
  w.audit_scratch_cap = 0;
  for (void* p : w.owned) hipFree(p);
  w.owned.clear();
  w.cap = 0;
}
void destroy_circuit(spp_circuit* c) {
  if (!c) return;
  hipSetDevice(c->ctx->device);
  hipStreamSynchronize(c->ctx->stream);
  for (auto& w : c->ws) {
    if (w.st) hipStreamSynchronize(w.st);
    if (w.own_st2) { hipStreamSynchronize(w.own_st2); hipStreamDestroy(w.own_st2); }
    if (w.own_st2p) { hipStreamSynchronize(w.own_st2p); hipStreamDestroy(w.own_st2p); }
    if (w.g2_ev.first) hipEventDestroy(w.g2_ev.first);
    if (w.g2_ev.second) hipEventDestroy(w.g2_ev.second);
    if (w.ev_w) hipEventDestroy(w.ev_w);
    if (w.ev_b2) hipEventDestroy(w.ev_b2);
    if (w.ev_in) hipEventDestroy(w.ev_in);
    if (w.ev_rows) hipEventDestroy(w.ev_rows);
    free_workspace(w);
    for (auto& evt : w.ev) if (evt) hipEventDestroy(evt);
    for (auto& pr : w.msm_ev) {
      if (pr.first) hipEventDestroy(pr.first);
      if (pr.second) hipEventDestroy(pr.second);
    }
  }
  for (void* p : c->owned) hipFree(p);
  delete c;
}
extern "C" void spp_free_circuit(spp_circuit* c) { destroy_circuit(c); }
extern "C" int spp_circuit_info(const spp_circuit* c, uint32_t info[8]) {
  if (!c || !info) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  info[0] = c->circ.id; info[1] = c->circ.n_public - 1; info[2] = c->circ.n_secret; info[3] = c->circ.n_wires;
  info[4] = c->circ.n_constraints; info[5] = c->circ.domain_log; info[6] = c->circ.n_inputs(); info[7] = c->c_bits;
  return SPP_OK;
}
extern "C" uint64_t spp_circuit_table_bytes(const spp_circuit* c) { return c ? c->table_bytes : 0; }
extern "C" int spp_circuit_small_rows(const spp_circuit* c, uint32_t out[2]) {
  if (!c || !out) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  out[0] = c->dc.sm_nrows;
  out[1] = c->dc.sm_nslots;
  return SPP_OK;
}
extern "C" int spp_circuit_plan_stats(const spp_circuit* c, uint32_t out[16]) {
  if (!c || !out) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  for (int i = 0; i < 16; i++) out[i] = 0;
  out[0] = c->dc.n_runs; out[1] = c->dc.max_row_terms; out[2] = c->dc.sm_nrows; out[3] = c->dc.sm_nslots; out[4] = c->dc.lg_n;
  out[5] = c->coop_item_count[COOP_SEQ]; out[6] = c->coop_item_count[COOP_PAR]; out[7] = c->coop_item_count[COOP_LEVELS];
  out[8] = c->coop_item_count[COOP_LEVEL_STREAM];
  out[9] = c->coop_stream_chunks;
  if (!c->sw.no_coop) { out[14] = c->coop_generic_rows; out[15] = c->coop_generic_divs; }
  for (const SolveStep& s : c->schedule) {
    if (s.kind == SolveStep::SEQ) out[10] = std::max(out[10], s.ntracks);
    if (s.kind == SolveStep::BATCH_DIV) { out[11] = std::max(out[11], s.b); out[13]++; }
    if (s.kind == SolveStep::BATCH_DIV || s.kind == SolveStep::COUNT8) out[12]++;
  }
  return SPP_OK;
}
extern "C" int spp_circuit_msm_windows(const spp_circuit* c, uint32_t bits[7]) {
  if (!c || !bits) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  bits[0] = c->A.c; bits[1] = c->B1.c; bits[2] = c->K.c; bits[3] = c->Z.c; bits[4] = c->CB.c; bits[5] = c->CS.c; bits[6] = c->B2.c;
  return SPP_OK;
}
extern "C" int spp_circuit_msm_table_rows(const spp_circuit* c, uint32_t rows[7]) {
  if (!c || !rows) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  rows[0] = c->A.Wt; rows[1] = c->B1.Wt; rows[2] = c->K.Wt; rows[3] = c->Z.Wt; rows[4] = c->CB.Wt; rows[5] = c->CS.Wt; rows[6] = c->B2.Wt;
  return SPP_OK;
}
extern "C" int spp_circuit_lookup_buckets(const spp_circuit* c, uint32_t out[2]) {
  if (!c || !out) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  out[0] = c->lk_n;
  out[1] = c->lk_n ? c->sw.lookup_min_batch : 0;
  return SPP_OK;
}
extern "C" int spp_circuit_msm_sizes(const spp_circuit* c, uint32_t sizes[7]) {
  if (!c || !sizes) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  sizes[0] = c->A.N; sizes[1] = c->B1.N; sizes[2] = c->K.N; sizes[3] = c->Z.N; sizes[4] = c->CB.N; sizes[5] = c->CS.N; sizes[6] = c->B2.N;
  return SPP_OK;
}

// bases per MSM set of a proving key file, as spp_circuit_msm_sizes reports them after loading (A, B1, K, Z, CB, CS, B2): what
// spp_plan_windows needs before anything is loaded
extern "C" int spp_pk_msm_sizes(const char* pk_path, uint32_t sizes[7]) {
  if (!pk_path || !sizes) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  std::vector<uint8_t> pkbuf;
  PkFile pk;
  if (!read_file(pk_path, pkbuf)) return fail(SPP_ERR_IO, "cannot read proving key %s", pk_path);
  if (!parse_pk(pkbuf, pk)) return fail(SPP_ERR_FORMAT, "malformed proving key %s", pk_path);
  sizes[0] = (uint32_t)pk.A.size() + 2; sizes[1] = (uint32_t)pk.B1.size() + 2; sizes[2] = (uint32_t)pk.K.size() + 1;
  sizes[3] = (uint32_t)pk.Z.size(); sizes[4] = (uint32_t)pk.CB.size(); sizes[5] = (uint32_t)pk.CS.size(); sizes[6] = (uint32_t)pk.B2.size() + 2;
  return SPP_OK;
}
// window bits for the sets of n_circuits circuits that are to live on one GPU TOGETHER: sizes / bits = n_circuits x 7 (the order
// above); one greedy split of budget_bytes over the union of their sets (see plan_greedy).  Host only.
extern "C" int spp_plan_windows(uint32_t n_circuits, const uint32_t* sizes, double budget_bytes, uint32_t* bits) {
  if (!sizes || !bits || n_circuits == 0 || n_circuits > 16) return fail(SPP_ERR_BAD_INPUT, "bad argument");
  std::vector<PlanSet> sets;
  for (uint32_t k = 0; k < n_circuits; k++)
    for (int s = 0; s < 7; s++) sets.push_back(plan_set(s, (double)sizes[7 * k + s], PLAN_WGT[s] != 0));
  double floor_bytes = 0;
  for (auto& ps : sets) floor_bytes += plan_bytes(ps, ps.bits);
  if (floor_bytes > budget_bytes) return fail(SPP_ERR_BAD_INPUT, "the budget does not hold even 6-bit tables (%.1f GB needed)", floor_bytes / 1e9);
  plan_greedy(sets, budget_bytes, 16);
  for (size_t i = 0; i < sets.size(); i++) bits[i] = (uint32_t)sets[i].bits;
  return SPP_OK;
}
// -----------------------------------------------------------------------------------------------------
// table-based MSM over caller-supplied bases (unit entry point; uses the table builder above)
// -----------------------------------------------------------------------------------------------------
template <class F> static Affine<F> point_from_raw(const uint8_t* b);
template <> Affine<Fq> point_from_raw<Fq>(const uint8_t* b) { return g1_from_raw(b); }
template <> Affine<Fq2> point_from_raw<Fq2>(const uint8_t* b) { return g2_from_raw(b); }
static void point_to_raw(const G1Affine& p, uint8_t* b) { g1_to_raw(p, b); }
static void point_to_raw(const G2Affine& p, uint8_t* b) { g2_to_raw(p, b); }
template <class F, size_t PT_BYTES>
static int msm_fixed_unit(spp_ctx* ctx, const uint8_t* bases, const uint8_t* scalars, size_t n, int window_bits, uint8_t* out) {
  if (!ctx || !out || (n && (!bases || !scalars))) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (window_bits == 0) window_bits = 8;
  if (window_bits < 4 || window_bits > 16) return fail(SPP_ERR_BAD_INPUT, "window_bits outside [4,16]");
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint32_t cb = (uint32_t)window_bits, Wn = msm_windows(cb);
  if ((uint64_t)msm_table_elems((uint32_t)n, cb, Wn) * PT_BYTES > ((uint64_t)64 << 30)) return fail(SPP_ERR_BAD_INPUT, "table would exceed 64 GiB; use a smaller window");
  std::vector<Affine<F>> pts(n);
  std::vector<Fr> sc(n);
  std::vector<uint32_t> rows(n);
  for (size_t i = 0; i < n; i++) {
    pts[i] = point_from_raw<F>(bases + PT_BYTES * i);
    sc[i] = Fr::from_bytes_be(scalars + 32 * i);
    rows[i] = (uint32_t)i;
  }
  spp_circuit tmpc;   // only used as an owner of device allocations
  tmpc.ctx = ctx;
  tmpc.c_bits = cb;
  Affine<F>* table = nullptr;
  int e = build_table_chunked<F>(&tmpc, pts, cb, Wn, &table);
  Fr* d_sc = nullptr;
  uint32_t* d_rows = nullptr;
  XYZZ<F> *partial = nullptr, *d_out = nullptr;
  DevBuf dig;
  const MsmPlan pl = msm_plan((uint32_t)n, 1, cb, Wn, MsmWalk<F>::occ(Wn), read_switches().msm);
  if (!e) e = own_upload(&tmpc, &d_sc, sc);
  if (!e) e = own_upload(&tmpc, &d_rows, rows);
  if (!e && hipMalloc((void**)&partial, sizeof(XYZZ<F>) * std::max<size_t>(pl.partial_elems(1), 1)) != hipSuccess) e = fail(SPP_ERR_HIP, "hipMalloc");
  if (!e && hipMalloc((void**)&d_out, sizeof(XYZZ<F>)) != hipSuccess) e = fail(SPP_ERR_HIP, "hipMalloc");
  if (!e && dig.alloc(sizeof(int16_t) * std::max<size_t>(msm_digit_elems((uint32_t)n, 1, cb), 1)) != hipSuccess) e = fail(SPP_ERR_HIP, "hipMalloc");
  XYZZ<F> res = XYZZ<F>::infinity();
  if (!e) {
    launch_msm_digits(st, d_rows, d_sc, dig.as<int16_t>(), (uint32_t)n, 1, cb);
    launch_msm_accumulate<F>(st, table, nullptr, dig.as<int16_t>(), partial, (uint32_t)n, 1, cb, pl);
    launch_msm_reduce<F>(st, partial, d_out, 1, pl, cb, n == 0);
    if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) e = fail(SPP_ERR_HIP, "msm kernels failed");
    else if (hipMemcpy(&res, d_out, sizeof res, hipMemcpyDeviceToHost) != hipSuccess) e = fail(SPP_ERR_HIP, "copy back failed");
  }
  for (void* p : tmpc.owned) hipFree(p);
  if (partial) hipFree(partial);
  if (d_out) hipFree(d_out);
  if (e) return e;
  point_to_raw(res.to_affine(), out);
  return SPP_OK;
}
extern "C" int spp_msm_g1(spp_ctx* ctx, const uint8_t* bases, const uint8_t* scalars, size_t n, int window_bits, uint8_t out[64]) {
  return msm_fixed_unit<Fq, 64>(ctx, bases, scalars, n, window_bits, out);
}
// the same walk over G2 bases (128 B, gnark raw X.A1|X.A0|Y.A1|Y.A0): what Bs of a proof comes from (k_msm_fixed<Fq2>)
extern "C" int spp_msm_g2(spp_ctx* ctx, const uint8_t* bases, const uint8_t* scalars, size_t n, int window_bits, uint8_t out[128]) {
  return msm_fixed_unit<Fq2, 128>(ctx, bases, scalars, n, window_bits, out);
}

// The flat walk (one table row per base, the throughput layout of the proving sets) over caller-supplied bases: P scalar rows against
// one table, launched as run_msm launches a flat set -- digits, the fast walk, the redo kernel, the folds, Horner.  The block list is
// uniform (every block holds 2^(c-1) entries per row).  redo_lanes (optional): how many lanes the redo kernel walked again.
template <class F, size_t PT_BYTES>
static int msm_flat_unit(spp_ctx* ctx, const uint8_t* bases, size_t n, const uint8_t* scalars, size_t P, int window_bits, uint8_t* out,
                         uint32_t* redo_lanes) {
  if (!ctx || !out || !bases || !scalars || n == 0 || P == 0) return fail(SPP_ERR_BAD_INPUT, "NULL or empty argument");
  if (window_bits == 0) window_bits = 8;
  if (window_bits < 4 || window_bits > 16) return fail(SPP_ERR_BAD_INPUT, "window_bits outside [4,16]");
  if (n > (1u << 20) || P > (1u << 16)) return fail(SPP_ERR_BAD_INPUT, "too many bases or rows");
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint32_t cb = (uint32_t)window_bits, N = (uint32_t)n, Pn = (uint32_t)P, E = 1u << (cb - 1);
  if ((uint64_t)msm_table_elems(N, cb, 1) * PT_BYTES > ((uint64_t)64 << 30)) return fail(SPP_ERR_BAD_INPUT, "table would exceed 64 GiB; use a smaller window");
  std::vector<Affine<F>> pts(n);
  std::vector<Fr> sc(n * P);                 // [base][row]: what the digit kernel reads
  std::vector<uint32_t> rows(n);
  for (size_t i = 0; i < n; i++) {
    pts[i] = point_from_raw<F>(bases + PT_BYTES * i);
    rows[i] = (uint32_t)i;
    for (size_t p = 0; p < P; p++) sc[i * P + p] = Fr::from_bytes_be(scalars + 32 * (p * n + i));
  }
  std::vector<MsmBlock> blocks(msm_table_rows(n, 1) / 64);
  for (size_t b = 0; b < blocks.size(); b++) blocks[b] = {(uint64_t)b * E, E, 0};
  spp_circuit tmpc;   // only used as an owner of device allocations
  tmpc.ctx = ctx;
  tmpc.c_bits = cb;
  Affine<F>* table = nullptr;
  int e = build_table_chunked<F>(&tmpc, pts, cb, 1, &table);
  Fr* d_sc = nullptr;
  uint32_t* d_rows = nullptr;
  MsmBlock* d_blocks = nullptr;
  const MsmPlan pl = msm_plan(N, Pn, cb, 1, MsmWalk<F>::occ(1), read_switches().msm);
  DevBuf partial, d_out, dig, count;
  if (!e) e = own_upload(&tmpc, &d_sc, sc);
  if (!e) e = own_upload(&tmpc, &d_rows, rows);
  if (!e) e = own_upload(&tmpc, &d_blocks, blocks);
  if (!e && (partial.alloc(sizeof(XYZZ<F>) * pl.partial_elems(Pn)) != hipSuccess || d_out.alloc(sizeof(XYZZ<F>) * P) != hipSuccess ||
             dig.alloc(sizeof(int16_t) * msm_digit_elems(N, Pn, cb)) != hipSuccess || count.alloc(sizeof(uint32_t)) != hipSuccess))
    e = fail(SPP_ERR_HIP, "hipMalloc");
  std::vector<XYZZ<F>> res(P);
  uint32_t redone = 0;
  if (!e) {
    hipMemsetAsync(count.p, 0, sizeof(uint32_t), st);
    launch_msm_digits(st, d_rows, d_sc, dig.as<int16_t>(), N, Pn, cb);
    launch_msm_accumulate<F>(st, table, d_blocks, dig.as<int16_t>(), partial.as<XYZZ<F>>(), N, Pn, cb, pl, nullptr, nullptr, count.as<uint32_t>());
    launch_msm_reduce<F>(st, partial.as<XYZZ<F>>(), d_out.as<XYZZ<F>>(), Pn, pl, cb, false);
    if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) e = fail(SPP_ERR_HIP, "msm kernels failed");
    else if (hipMemcpy(res.data(), d_out.p, sizeof(XYZZ<F>) * P, hipMemcpyDeviceToHost) != hipSuccess ||
             hipMemcpy(&redone, count.p, sizeof redone, hipMemcpyDeviceToHost) != hipSuccess)
      e = fail(SPP_ERR_HIP, "copy back failed");
  }
  for (void* p : tmpc.owned) hipFree(p);
  if (e) return e;
  for (size_t p = 0; p < P; p++) point_to_raw(res[p].to_affine(), out + PT_BYTES * p);
  if (redo_lanes) *redo_lanes = redone;
  return SPP_OK;
}
extern "C" int spp_msm_flat_unit(spp_ctx* ctx, int group, const uint8_t* bases, size_t n, const uint8_t* scalars, size_t P, int window_bits,
                                 uint8_t* out, uint32_t* redo_lanes) {
  if (group == 1) return msm_flat_unit<Fq, 64>(ctx, bases, n, scalars, P, window_bits, out, redo_lanes);
  if (group == 2) return msm_flat_unit<Fq2, 128>(ctx, bases, n, scalars, P, window_bits, out, redo_lanes);
  return fail(SPP_ERR_BAD_INPUT, "group is 1 or 2");
}
// The digit planes on their own (test only): launch_msm_digits as run_msm and the two unit entries above launch it, and the planes
// as the walks read them -- dig[j][i][p], Pp per row.  The device buffer is zeroed first: entries with p >= P, which the kernel
// does not write, come back as 0 rather than as whatever the allocation held.
extern "C" int spp_debug_msm_digits(spp_ctx* ctx, const uint8_t* scalars, size_t M, size_t P, const uint32_t* rows, size_t N, int window_bits,
                                    int16_t* planes, size_t planes_elems, uint32_t* padded_batch) {
  if (!ctx || !scalars || !rows || !planes || !padded_batch) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (window_bits < 4 || window_bits > 16) return fail(SPP_ERR_BAD_INPUT, "window_bits outside [4,16]");
  if (M == 0 || N == 0 || P == 0 || M > (1u << 20) || N > (1u << 20) || P > (1u << 16)) return fail(SPP_ERR_BAD_INPUT, "M, N in [1, 2^20], P in [1, 2^16]");
  for (size_t i = 0; i < N; i++)
    if (rows[i] >= M) return fail(SPP_ERR_BAD_INPUT, "rows[%zu] = %u is no scalar row (M = %zu)", i, rows[i], M);
  const uint32_t cb = (uint32_t)window_bits;
  const size_t elems = msm_digit_elems((uint32_t)N, (uint32_t)P, cb);
  if (planes_elems < elems) return fail(SPP_ERR_BAD_INPUT, "the planes of this call hold %zu digits, the buffer %zu", elems, planes_elems);
  if (elems > ((size_t)1 << 28)) return fail(SPP_ERR_BAD_INPUT, "more than 2^28 digits");
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  std::vector<Fr> sc(M * P);
  for (size_t k = 0; k < M * P; k++) sc[k] = Fr::from_bytes_be(scalars + 32 * k);
  DevBuf d_sc, d_rows, dig;
  UP(d_sc, sc.data(), sizeof(Fr) * sc.size());
  UP(d_rows, rows, sizeof(uint32_t) * N);
  HIP_TRY(dig.alloc(sizeof(int16_t) * elems));
  HIP_TRY(hipMemsetAsync(dig.p, 0, sizeof(int16_t) * elems, st));
  launch_msm_digits(st, d_rows.as<uint32_t>(), d_sc.as<Fr>(), dig.as<int16_t>(), (uint32_t)N, (uint32_t)P, cb);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipMemcpy(planes, dig.p, sizeof(int16_t) * elems, hipMemcpyDeviceToHost));
  *padded_batch = msm_padded_batch((uint32_t)P);
  return SPP_OK;
}
