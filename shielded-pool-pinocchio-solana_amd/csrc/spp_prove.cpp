// libspp C ABI, proving: the batch workspaces, the proving pipeline of one batch (prove_on_device) and the entry points that
// schedule batches over the workspaces and proving streams of a circuit; timing queries.  Nothing here reads the environment:
// the experiment switches are fields of the circuit (Switches, spp_circuit.hpp).
#include "spp_circuit.hpp"

#include <thread>

template <class T>
static int ws_alloc(Workspace& w, T** p, size_t count) {
  HIP_TRY(hipMalloc((void**)p, sizeof(T) * std::max<size_t>(count, 1)));
  w.owned.push_back((void*)*p);
  return 0;
}
template <class F>
static int ws_set(const spp_circuit* c, Workspace& w, const MsmSet<F>* s, MsmBuf<F>* b, size_t P) {
  b->partial_cap = msm_partial_cap(s->N, P, s->c, s->Wt, MsmWalk<F>::occ(s->Wt), c->sw.msm);
  int e;
  if ((e = ws_alloc(w, &b->partial, b->partial_cap))) return e;
  return ws_alloc(w, &b->out, P);
}
// whether a batch (or batch body) of P proofs sums its lookup-inverse wires by byte bucket: the circuit has such wires on flat A
// and K sets (spp_load.cpp) and the batch reaches the threshold (Switches::lookup_min_batch)
static bool lookup_buckets_on(const spp_circuit* c, size_t P) { return c->lk_n != 0 && c->sw.lookup_min_batch != 0 && P >= c->sw.lookup_min_batch; }
static int ensure_workspace(spp_circuit* c, Workspace& w, size_t P) {
  if (P <= w.cap) return 0;
  HIP_TRY(hipStreamSynchronize(w.st));
  free_workspace(w);
  int e;
  if ((e = ws_alloc(w, &w.W, (size_t)c->n_rows * P)) || (e = ws_alloc(w, &w.abc, (size_t)3 * c->n * P)) ||
      (e = ws_alloc(w, &w.scratch, (size_t)c->max_batch_div * P)) || (e = ws_alloc(w, &w.commit_affine, P)) ||
      (e = ws_alloc(w, &w.d_inputs, c->in_stride * P)) || (e = ws_alloc(w, &w.d_rs, 64 * P)) ||
      (e = ws_alloc(w, &w.d_proofs, (size_t)SPP_PROOF_LEN * P)) || (e = ws_alloc(w, &w.d_pws, c->pw_stride * P)) ||
      (e = ws_alloc(w, &w.d_status, P)) || (e = ws_alloc(w, &w.counters, 256 * P)))
    return e;
  if ((e = ws_set(c, w, &c->A, &w.A, P)) || (e = ws_set(c, w, &c->B1, &w.B1, P)) || (e = ws_set(c, w, &c->B2, &w.B2, P)) ||
      (e = ws_set(c, w, &c->K, &w.K, P)) || (e = ws_set(c, w, &c->Z, &w.Z, P)) || (e = ws_set(c, w, &c->CB, &w.CB, P)) ||
      (e = ws_set(c, w, &c->CS, &w.CS, P)))
    return e;
  {
    const size_t Ps = std::min<size_t>(P, scaled_blind_max_batch(c->A.N, c->B1.N));
    if ((e = ws_set(c, w, &c->A, &w.sA, Ps)) || (e = ws_set(c, w, &c->B1, &w.rB, Ps)) || (e = ws_alloc(w, &w.Ws, (size_t)c->n_rows * Ps)) ||
        (e = ws_alloc(w, &w.Wr, (size_t)c->n_rows * Ps)))
      return e;
  }
  {
    // digit planes: the G1 sets share one buffer (they run one after the other on `st`), the G2 set has its own
    size_t d1 = 0;
    for (const MsmSet<Fq>* s : {&c->A, &c->B1, &c->K, &c->Z, &c->CB, &c->CS}) d1 = std::max(d1, msm_digit_elems(s->N, (uint32_t)P, s->c));
    w.dig1_cap = d1;
    w.dig2_cap = msm_digit_elems(c->B2.N, (uint32_t)P, c->B2.c);
    if ((e = ws_alloc(w, &w.dig1, w.dig1_cap)) || (e = ws_alloc(w, &w.dig2, w.dig2_cap))) return e;
    if (c->dc.sm_nrows && (e = ws_alloc(w, &w.small, (size_t)c->dc.sm_nslots * P))) return e;
  }
  w.lk_bkt = nullptr;
  if (lookup_buckets_on(c, P)) {
    // the byte-bucket sums of the lookup-inverse wires (msm_lookup.hpp): 2 sets x LKB_SLICES x 256 buckets of 128 B = 512 KiB per
    // proof, plus 34 KiB of inverses, digits and window sums and one byte per lookup -- 1.1 GB for a workspace of 2 048 audit proofs
    if ((e = ws_alloc(w, &w.lk_bkt, lkb_bucket_elems(P))) || (e = ws_alloc(w, &w.lk_win, (size_t)2 * LKB_WINDOWS * P)) ||
        (e = ws_alloc(w, &w.lk_sum, (size_t)2 * P)) || (e = ws_alloc(w, &w.lk_inv, (size_t)LKB_VALUES * P)) ||
        (e = ws_alloc(w, &w.lk_dig, (size_t)LKB_WINDOWS * LKB_VALUES * P)) || (e = ws_alloc(w, &w.lk_bytes, (size_t)c->lk_n * P)))
      return e;
  }
  w.cap = P;
  return 0;
}

static int16_t* ws_dig(Workspace& w, Fq*) { return w.dig1; }
static int16_t* ws_dig(Workspace& w, Fq2*) { return w.dig2; }
// digits + accumulate of one set; the caller folds (several sets share the fold launches): b.plan holds the lane layout
template <class F>
static void run_msm(spp_circuit* c, Workspace& w, const MsmSet<F>& s, MsmBuf<F>& b, uint32_t P, bool timed, hipStream_t st_override = nullptr,
                    std::pair<hipEvent_t, hipEvent_t>* ev_override = nullptr, bool fold = true, const Fr* scal_override = nullptr,
                    const uint32_t* rows_override = nullptr) {
  hipStream_t st = st_override ? st_override : w.st;
  const Fr* scal = scal_override ? scal_override : s.from_h ? w.abc : w.W;
  MsmPlan pl = msm_plan(s.N, P, s.c, s.Wt, MsmWalk<F>::occ(s.Wt), c->sw.msm);
  pl.fit(P, b.partial_cap);   // never exceed the allocated partial buffer
  b.plan = pl;
  std::pair<hipEvent_t, hipEvent_t>* ev = nullptr;
  if (timed && w.msm_ev_used < w.msm_ev.size()) ev = &w.msm_ev[w.msm_ev_used++];
  if (ev_override) ev = ev_override;
  int16_t* dig = ws_dig(w, (F*)nullptr);
  launch_msm_digits(st, rows_override ? rows_override : s.rows, scal, dig, s.N, P, s.c);
  // the event pair receives the dispatch's own start/stop timestamps (what rocprofv3 reports as the kernel's duration)
  launch_msm_accumulate<F>(st, s.table, s.blocks, dig, b.partial, s.N, P, s.c, pl, ev ? ev->first : nullptr, ev ? ev->second : nullptr);
  if (fold) launch_msm_reduce<F>(st, b.partial, b.out, P, pl, s.c, s.N == 0);
}

static int prove_on_device(spp_circuit* c, Workspace& w, uint32_t P, const uint8_t* d_inputs, const uint8_t* d_rs, uint8_t* d_proofs,
                           uint8_t* d_pws, uint32_t* d_status) {
  hipStream_t st = w.st;
  const Circuit& circ = c->circ;
  const uint32_t n = c->n;
  w.msm_ev_used = 0;
  w.last_P = P;
  // (the two scaled sums walk the A and B1 tables with full-size scalars for every base: not over tables whose narrow rows only
  // serve their wires' range classes -- such a circuit keeps the per-lane multiplication at every batch size)
  const bool scaled_blind = P <= scaled_blind_max_batch(c->A.N, c->B1.N) && !c->sw.no_coop && !c->A.narrow && !c->B1.narrow;
  HIP_TRY(hipMemsetAsync(d_status, 0, sizeof(uint32_t) * P, st));
  hipEventRecord(w.ev[0], st);
  // 1. inputs, solver phase 1, commitment, challenge, solver phase 2
  launch_load_inputs(st, d_inputs, d_rs, w.W, circ.n_inputs(), circ.n_wires, P);
  hipEventRecord(w.ev_in, st);
  for (const SolveStep& s : c->schedule) {
    switch (s.kind) {
      case SolveStep::SEQ:
        if (P <= c->sw.coop_max_batch && !c->sw.no_coop && c->sw.trace_items) {
          for (uint32_t t = 0; t < s.ntracks; t++)
            for (uint32_t it = s.tr_begin[t]; it < s.tr_end[t]; it++) {
              CoopTracks one{};
              one.n = 1; one.begin[0] = it; one.end[0] = it + 1;
              launch_solve_coop(st, c->dc, c->coop, w.W, w.scratch, one, P);
            }
        } else if (P <= c->sw.coop_max_batch && !c->sw.no_coop) {
          CoopTracks tr{};
          tr.n = c->sw.one_track ? 1 : s.ntracks;
          for (uint32_t t = 0; t < s.ntracks; t++) { tr.begin[t] = s.tr_begin[t]; tr.end[t] = s.tr_end[t]; }
          if (c->sw.one_track) {   // SPP_COOP_ONE_TRACK=1 (diagnostic): the tracks one after the other
            for (uint32_t t = 0; t < s.ntracks; t++) {
              CoopTracks one{};
              one.n = 1; one.begin[0] = s.tr_begin[t]; one.end[0] = s.tr_end[t];
              launch_solve_coop(st, c->dc, c->coop, w.W, w.scratch, one, P);
            }
          } else launch_solve_coop(st, c->dc, c->coop, w.W, w.scratch, tr, P);
        }
        else launch_solve(st, c->dc, w.W, w.scratch, s.a, s.b, P);
        break;
      case SolveStep::BATCH_DIV: launch_batch_div(st, c->dc, w.W, w.scratch, s.a, s.b, P); break;
      case SolveStep::COUNT8: launch_count8(st, c->dc, w.W, w.counters, s.a, s.b, s.c, P); break;
      case SolveStep::COMMIT:
        run_msm(c, w, c->CB, w.CB, P, true);
        launch_challenge(st, w.CB.out, w.W, circ.challenge_wire, P, w.commit_affine, d_status);
        break;
    }
  }
  hipEventRecord(w.ev[1], st);
  // the G2 MSM depends on the witness only: start it now on the side stream
  hipEventRecord(w.ev_w, st);
  hipStream_t side = (w.st2 != w.st && w.own_st2p && P > c->sw.coop_max_batch) ? w.own_st2p : w.st2;
  if (c->sw.no_side && P <= c->sw.coop_max_batch) side = st;   // experiment: the G2 sum on the batch's own stream
  hipStreamWaitEvent(side, w.ev_w, 0);
  run_msm(c, w, c->B2, w.B2, P, false, side, &w.g2_ev);
  hipEventRecord(w.ev_b2, side);
  // 2. constraint evaluations + satisfaction check
  launch_spmv_check(st, c->dc, w.W, w.abc, n, P, d_status, w.small);
  hipEventRecord(w.ev[2], st);
  // 3. h = (a*b - c)/Z  (coefficients land bit-reversed in the a-slot of abc)
  const size_t bs = (size_t)n * P;
  // the coset shifts ride on the stores of the inverse transforms' last pass (no separate pass over the arrays)
  const uint32_t nt = c->sw.h_mode == 2 ? 2 : 3;      // product form: A and B only
  launch_ntt(st, w.abc, c->logn, P, c->tw_inv, true, nt, bs, c->coset_br);
  launch_ntt(st, w.abc, c->logn, P, c->tw_fwd, false, nt, bs);
  if (c->sw.h_mode == 2) launch_qap_product(st, w.abc, n, P);
  else launch_qap_pointwise(st, w.abc, n, P, c->zinv);
  if (c->sw.h_mode == 0) launch_ntt(st, w.abc, c->logn, P, c->tw_inv, true, 1, bs, c->coset_inv_br);   // else: the Z bases are in the evaluation basis
  hipEventRecord(w.ev[3], st);
  // 4. MSMs
  {
    MsmFoldSets<Fq> fs{};
    const MsmSet<Fq>* sets[7] = {&c->A, &c->B1, &c->K, &c->Z, &c->CS, &c->A, &c->B1};
    MsmBuf<Fq>* bufs[7] = {&w.A, &w.B1, &w.K, &w.Z, &w.CS, &w.sA, &w.rB};
    const Fr* scal[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, w.Ws, w.Wr};
    const int nsets = scaled_blind ? 7 : 5;
    if (scaled_blind) launch_scale_witness(st, w.W, w.Ws, w.Wr, c->n_rows, c->row_r, c->row_s, P);
    // The lookup-inverse wires of A and K (msm_lookup.hpp): their digit planes are zero in the two walks below, their share is
    // summed by byte bucket here and joins A.out / K.out behind the folds.  Inside this stage, so the stage times stay comparable
    // (spp_timings: msm_g1); the per-launch times of spp_msm_kernel_ms are those of the walks alone, as before.
    const bool lkb = lookup_buckets_on(c, P) && w.lk_bkt;
    const LkbSets lks{{c->A.table, c->K.table}, {c->A.blocks, c->K.blocks}, {c->lk_pos[0], c->lk_pos[1]}, {w.A.out, w.K.out}};
    const uint32_t* rows[7] = {lkb ? c->lk_rows[0] : nullptr, nullptr, lkb ? c->lk_rows[1] : nullptr, nullptr, nullptr, nullptr, nullptr};
    if (lkb) {
      launch_lookup_bytes(st, c->dc, w.W, c->lk_hints, c->lk_n, P, w.lk_bytes);
      launch_lkb_inverses(st, w.W, circ.challenge_wire, P, w.lk_inv, w.lk_dig, d_status);
      launch_lkb_sums(st, lks, w.lk_bytes, w.lk_dig, w.lk_bkt, w.lk_win, c->lk_n, P);
      MsmFoldSets<Fq> lf{};
      for (uint32_t k = 0; k < 2; k++) {
        lf.partial[k] = w.lk_win + (size_t)k * LKB_WINDOWS * P;
        lf.out[k] = w.lk_sum + (size_t)k * P;
        lf.Sg[k] = 1;
        lf.R[k] = LKB_WINDOWS;
        lf.c[k] = LKB_C;
      }
      launch_msm_reduce_multi<Fq>(st, lf, 2, P);   // no slices to fold: the Horner over the window sums
    }
    for (int i = 0; i < nsets; i++) {
      run_msm(c, w, *sets[i], *bufs[i], P, i < 5, nullptr, nullptr, false, scal[i], rows[i]);
      fs.partial[i] = bufs[i]->partial;
      fs.out[i] = bufs[i]->out;
      fs.Sg[i] = sets[i]->N ? bufs[i]->plan.Sg : 0;
      fs.R[i] = bufs[i]->plan.R;
      fs.c[i] = sets[i]->c;
    }
    launch_msm_reduce_multi<Fq>(st, fs, nsets, P);   // the slice sums are folded level by level in shared launches, then Horner
    if (lkb) launch_lkb_join(st, lks, w.lk_sum, P);
  }
  hipEventRecord(w.ev[4], st);
  hipStreamWaitEvent(st, w.ev_b2, 0);   // join the G2 MSM
  hipEventRecord(w.ev[5], st);
  // 5. assembly
  AssembleArgs a;
  a.mA = w.A.out; a.mB1 = w.B1.out; a.mB2 = w.B2.out; a.mK = w.K.out; a.mZ = w.Z.out; a.mPok = w.CS.out;
  a.commit_affine = w.commit_affine;
  a.W = w.W; a.row_r = c->row_r; a.row_s = c->row_s; a.n_public = circ.n_public;
  a.sAr = scaled_blind ? w.sA.out : nullptr;
  a.rBs1 = scaled_blind ? w.rB.out : nullptr;
  a.proofs = d_proofs; a.pws = d_pws; a.P = P;
  launch_assemble(st, a);
  hipEventRecord(w.ev[6], st);
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}

// -----------------------------------------------------------------------------------------------------
// scheduling: which workspace a batch takes, where a batch is cut, where its outputs go
// -----------------------------------------------------------------------------------------------------
// Batches in flight: two for big batches (more adds nothing once the latency-bound phases are covered: DESIGN 8.3); small
// batches -- 128 proofs are one of 8 ranks' share of BASELINE.json configs[2] -- spend a larger part of their time in
// latency-bound kernels (11 ms of sponge chain in the solver, the Horner combines), so up to six take turns
// (128-proof audit batches, ms per step on one box: 25.3 with four in flight, 23.3 with five, 23.1 with six).
static int ws_depth(const spp_circuit* c, size_t count, bool generic_solver) {
  if (c->sw.forced_depth) return c->sw.forced_depth;
  return count <= 256 ? 6 : count <= 768 ? 4 : generic_solver ? 3 : 2;
}
// the next workspace of the rotation over the first `depth`; c->ws[c->next_ws] is then the one after it
static Workspace& take_workspace(spp_circuit* c, int depth) {
  if (c->next_ws >= depth) c->next_ws = 0;
  const int wi = c->next_ws;
  c->prev_ws = c->last_ws;
  c->last_ws = wi;
  c->next_ws = (wi + 1) % depth;
  return c->ws[wi];
}
// The start of a device call: the batch's workspace, with every workspace of the depth sized to `count` on the first call, so
// that no allocation ever lands inside a caller's timed / pipelined region.
static int take_sized_workspace(spp_circuit* c, size_t count, bool generic_solver, Workspace** w) {
  const int depth = ws_depth(c, count, generic_solver);
  *w = &take_workspace(c, depth);
  for (int k = 0; k < depth; k++)
    if (int e = ensure_workspace(c, c->ws[k], count)) return e;
  return 0;
}
// A batch that is not a multiple of the wave width is cut into a 64-aligned body and a tail of < 64 proofs: the size of the tail.
// Every kernel of the path maps 64 proofs to a wave, so 1025 proofs used to cost a 17th wave per (slice, window) everywhere -- and
// before the lanes were padded to waves, every wave of the MSM straddled two slices (1024 -> 1025 proofs: +23 % time, profiles/
// round2_batch_size_sweep.txt).  The tail takes the small-batch paths (cooperative solver, lanes per (base, proof)) on the
// NEXT workspace of the rotation and its proving stream, beside the body; the next call starts on that stream, behind the short
// tail.  SPP_NO_SPLIT=1: off.
static size_t batch_tail(const spp_circuit* c, size_t count) { return count > 64 && !c->sw.no_split ? count % 64 : 0; }
// where a batch reads its blinding and writes its outputs, in device memory
struct BatchIO {
  const uint8_t* rs;
  uint8_t *proofs, *pws;
  uint32_t* status;
  BatchIO at(const spp_circuit* c, size_t off) const {   // the same for the batch that starts at proof `off`
    return {rs + off * 64, proofs + off * SPP_PROOF_LEN, pws + off * c->pw_stride, status + off};
  }
};
static int prove_on_device(spp_circuit* c, Workspace& w, size_t P, const uint8_t* d_inputs, const BatchIO& io) {
  return prove_on_device(c, w, (uint32_t)P, d_inputs, io.rs, io.proofs, io.pws, io.status);
}

// -----------------------------------------------------------------------------------------------------
// entry points: argument checks, the input stage that is their own, the shared tail
// -----------------------------------------------------------------------------------------------------
extern "C" int spp_prove_batch_device(spp_circuit* c, size_t count, const void* d_inputs, const void* d_rs, void* d_proofs, void* d_pws,
                                      void* d_status) {
  if (!c || !d_inputs || !d_rs || !d_proofs || !d_pws || !d_status) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count == 0) return SPP_OK;
  if (count > (1u << 20)) return fail(SPP_ERR_BAD_INPUT, "batch too large");
  std::lock_guard<std::mutex> lk(c->ctx->mu);
  HIP_TRY(hipSetDevice(c->ctx->device));
  Workspace* w;
  if (int e = take_sized_workspace(c, count, c->generic_solver, &w)) return e;
  const BatchIO io{(const uint8_t*)d_rs, (uint8_t*)d_proofs, (uint8_t*)d_pws, (uint32_t*)d_status};
  const size_t tail = batch_tail(c, count), body = count - tail;
  if (int e = prove_on_device(c, *w, body, (const uint8_t*)d_inputs, io)) return e;
  if (!tail) return SPP_OK;
  return prove_on_device(c, c->ws[c->next_ws], tail, (const uint8_t*)d_inputs + body * c->in_stride, io.at(c, body));
}
// rs = NULL of the host entry points: 64 bytes of OS randomness per proof
static int os_blinding(std::vector<uint8_t>& rnd, size_t count) {
  rnd.resize(64 * count);
  FILE* f = fopen("/dev/urandom", "rb");
  if (!f || fread(rnd.data(), 1, rnd.size(), f) != rnd.size()) {
    if (f) fclose(f);
    return fail(SPP_ERR_IO, "cannot read /dev/urandom");
  }
  fclose(f);
  return SPP_OK;
}
// End to end: the audit proof from the prover's raw secrets.  The input pipeline of scripts/generate_audit.py:468-641 (keygen,
// wa_commitment, RLWE encryption, quotients, packing, ct_commitment) is enqueued on the batch's own proving stream in front of the
// solver, into the workspace's input rows: nothing returns to the host between the secrets and the proof bytes, and the
// pipelining of consecutive calls is that of spp_prove_batch_device.
// d_c0 / d_c1 (both or neither): the ciphertext every proof commits to, written by the RLWE kernel of the input pipeline -- on
// the batch's own proving stream, in front of the solver, so a refused row has its ciphertext like any other.  *stream
// (optional): the proving stream the batch went to.
static int prove_audit_from_secrets(spp_circuit* c, size_t count, const void* d_pk_a, const void* d_pk_b, const void* d_sk, const void* d_r,
                                    const void* d_e1, const void* d_e2, const void* d_rs, void* d_proofs, void* d_pws, void* d_status,
                                    void* d_c0, void* d_c1, hipStream_t* stream = nullptr) {
  if (!c || !d_pk_a || !d_pk_b || !d_sk || !d_r || !d_e1 || !d_e2 || !d_rs || !d_proofs || !d_pws || !d_status)
    return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (c->circ.id != SPP_CIRCUIT_AUDIT || c->circ.n_inputs() != 3360) return fail(SPP_ERR_BAD_INPUT, "not the audit circuit");
  if (count == 0) return SPP_OK;
  if (count > (1u << 20)) return fail(SPP_ERR_BAD_INPUT, "batch too large");
  std::lock_guard<std::mutex> lk(c->ctx->mu);
  HIP_TRY(hipSetDevice(c->ctx->device));
  if (int e = spp_ensure_ctx_consts(c->ctx)) return e;
  Workspace* wp;
  if (int e = take_sized_workspace(c, count, false, &wp)) return e;
  Workspace& w = *wp;
  if (stream) *stream = w.st;
  const size_t need = spp_audit_scratch_bytes(count);
  if (need > w.audit_scratch_cap) {
    HIP_TRY(hipStreamSynchronize(w.st));
    if (w.audit_scratch) HIP_TRY(hipFree(w.audit_scratch));
    w.audit_scratch = nullptr;
    w.audit_scratch_cap = 0;
    HIP_TRY(hipMalloc(&w.audit_scratch, need));
    w.audit_scratch_cap = need;
  }
  if (int e = spp_audit_inputs_enqueue(c->ctx, w.st, w.audit_scratch, (const uint32_t*)d_pk_a, (const uint32_t*)d_pk_b, (uint32_t)count,
                                       (const uint8_t*)d_sk, (const int8_t*)d_r, (const int8_t*)d_e1, (const int8_t*)d_e2, w.d_inputs, (uint32_t*)d_c0,
                                       (uint32_t*)d_c1))
    return e;
  // one piece, no cut into body and tail (batch_tail): the cut would change which kernels a 2 049-proof audit batch runs
  return prove_on_device(c, w, count, w.d_inputs, BatchIO{(const uint8_t*)d_rs, (uint8_t*)d_proofs, (uint8_t*)d_pws, (uint32_t*)d_status});
}
extern "C" int spp_prove_audit_from_secrets_device(spp_circuit* c, size_t count, const void* d_pk_a, const void* d_pk_b, const void* d_sk,
                                                   const void* d_r, const void* d_e1, const void* d_e2, const void* d_rs, void* d_proofs,
                                                   void* d_pws, void* d_status) {
  return prove_audit_from_secrets(c, count, d_pk_a, d_pk_b, d_sk, d_r, d_e1, d_e2, d_rs, d_proofs, d_pws, d_status, nullptr, nullptr);
}
// The same with the record's third part: the ciphertext (generate_audit.py:590-606 writes it next to the proof).
extern "C" int spp_prove_audit_records_device(spp_circuit* c, size_t count, const void* d_pk_a, const void* d_pk_b, const void* d_sk,
                                              const void* d_r, const void* d_e1, const void* d_e2, const void* d_rs, void* d_proofs, void* d_pws,
                                              void* d_status, void* d_c0, void* d_c1) {
  if (!d_c0 || !d_c1) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  return prove_audit_from_secrets(c, count, d_pk_a, d_pk_b, d_sk, d_r, d_e1, d_e2, d_rs, d_proofs, d_pws, d_status, d_c0, d_c1);
}
// Host form: chunks of at most 2 048 records take turns on two sets of device buffers, so the uploads of chunk k + 1 and the
// input pipeline in front of its solver overlap the MSMs of chunk k; the results of chunk k are fetched once chunk k + 1 is
// enqueued (as spp_prove_batch does).  status and the zeroing of refused proofs follow spp_prove_batch.
extern "C" int spp_prove_audit_records(spp_circuit* c, const uint32_t* pk_a, const uint32_t* pk_b, size_t count, const uint8_t* sk,
                                       const int8_t* r, const int8_t* e1, const int8_t* e2, const uint8_t* rs, uint8_t* proofs, uint8_t* pws,
                                       int32_t* status, uint32_t* c0, uint32_t* c1) {
  if (!c || !pk_a || !pk_b || !sk || !r || !e1 || !e2 || !proofs || !pws || !c0 || !c1) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (c->circ.id != SPP_CIRCUIT_AUDIT || c->circ.n_inputs() != 3360) return fail(SPP_ERR_BAD_INPUT, "not the audit circuit");
  if (count == 0) return SPP_OK;
  if (count > (1u << 24)) return fail(SPP_ERR_BAD_INPUT, "too many records in one call");
  for (int i = 0; i < 1024; i++)
    if (pk_a[i] >= 167772161u || pk_b[i] >= 167772161u) return fail(SPP_ERR_BAD_INPUT, "public key coefficient not in [0, q)");
  std::vector<uint8_t> rnd;
  if (!rs) {
    if (int e = os_blinding(rnd, count)) return e;
    rs = rnd.data();
  }
  HIP_TRY(hipSetDevice(c->ctx->device));
  const size_t chunk = std::min<size_t>(count, 2048), pwl = c->pw_stride;
  struct CopyStream {   // the copies of this call, beside whatever else runs on the context; the proving streams are the library's
    hipStream_t s = nullptr;
    ~CopyStream() { if (s) hipStreamDestroy(s); }
  } copy;
  HIP_TRY(hipStreamCreateWithFlags(&copy.s, hipStreamNonBlocking));
  hipStream_t st = copy.s;
  struct Set {
    DevBuf sk, r, e1, e2, rs, proofs, pws, status, c0, c1;
    hipStream_t proving = nullptr;
    size_t off = 0, n = 0;
  } sets[2];
  DevBuf da, db;
  UP(da, pk_a, 4096);
  UP(db, pk_b, 4096);
  for (Set& s : sets) {
    HIP_TRY(s.sk.alloc(chunk * 32)); HIP_TRY(s.r.alloc(chunk * 1024)); HIP_TRY(s.e1.alloc(chunk * 64)); HIP_TRY(s.e2.alloc(chunk * 1024));
    HIP_TRY(s.rs.alloc(chunk * 64)); HIP_TRY(s.proofs.alloc(chunk * SPP_PROOF_LEN)); HIP_TRY(s.pws.alloc(chunk * pwl));
    HIP_TRY(s.status.alloc(chunk * 4)); HIP_TRY(s.c0.alloc(chunk * 64 * 4)); HIP_TRY(s.c1.alloc(chunk * 1024 * 4));
    if (count <= chunk) break;       // one chunk: one set
  }
  std::vector<uint32_t> stat(count);
  auto fetch = [&](Set& s) -> int {
    HIP_TRY(hipStreamSynchronize(s.proving));
    HIP_TRY(hipMemcpyAsync(proofs + (size_t)SPP_PROOF_LEN * s.off, s.proofs.p, (size_t)SPP_PROOF_LEN * s.n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(pws + pwl * s.off, s.pws.p, pwl * s.n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(stat.data() + s.off, s.status.p, 4 * s.n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(c0 + 64 * s.off, s.c0.p, 64 * 4 * s.n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(c1 + 1024 * s.off, s.c1.p, 1024 * 4 * s.n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    s.n = 0;
    return 0;
  };
  int k = 0;
  for (size_t off = 0; off < count; off += chunk, k ^= 1) {
    Set& s = sets[k];
    if (s.n)
      if (int e = fetch(s)) return e;
    const size_t n = std::min(chunk, count - off);
    HIP_TRY(hipMemcpyAsync(s.sk.p, sk + 32 * off, 32 * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s.r.p, r + 1024 * off, 1024 * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s.e1.p, e1 + 64 * off, 64 * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s.e2.p, e2 + 1024 * off, 1024 * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s.rs.p, rs + 64 * off, 64 * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    s.off = off;
    s.n = n;
    if (int e = prove_audit_from_secrets(c, n, da.p, db.p, s.sk.p, s.r.p, s.e1.p, s.e2.p, s.rs.p, s.proofs.p, s.pws.p, s.status.p, s.c0.p, s.c1.p,
                                         &s.proving))
      return e;
  }
  for (int j = 0; j < 2; j++) {      // the older chunk first
    Set& s = sets[k ^ j];
    if (s.n)
      if (int e = fetch(s)) return e;
  }
  int rc = SPP_OK;
  for (size_t i = 0; i < count; i++) {
    const int32_t v = stat[i] ? SPP_ERR_UNSAT : SPP_OK;
    if (status) status[i] = v;
    if (v && rc == SPP_OK) rc = fail(SPP_ERR_UNSAT, "record %zu: inputs do not satisfy the circuit", i);
    if (v) memset(proofs + (size_t)SPP_PROOF_LEN * i, 0, SPP_PROOF_LEN);
  }
  return rc;
}
// Withdraw proofs from notes against the resident tree (include/spp.h).  The rows are gathered on the TREE's stream (ctx->stream),
// not on the proving stream: spp_merkle_tree_insert runs there and may reallocate the level arrays (mt_reserve), so an insert
// made right after this call is stream-ordered behind the gather and every proof of the call is against the root at call time.
// Under the context lock: (1) ctx->stream waits until the workspace's previous batch has loaded its rows (ev_in), (2) the rows
// kernel writes into the workspace's d_inputs, (3) the proving stream waits for it (ev_rows).  A batch that is not a multiple
// of the wave width is split into body and tail as in spp_prove_batch_device; the tail's rows go to the tail workspace's own
// d_inputs, so each workspace's rows are only ever read by its own stream.
static int withdraw_notes_args(spp_circuit* c, spp_merkle_tree* t) {
  if (c->circ.id != SPP_CIRCUIT_WITHDRAW) return fail(SPP_ERR_BAD_INPUT, "not a withdraw circuit");
  if (t->ctx != c->ctx) return fail(SPP_ERR_BAD_INPUT, "the tree belongs to another context");
  if (c->circ.n_inputs() != 10 + t->depth)
    return fail(SPP_ERR_BAD_INPUT, "the circuit takes %u inputs, a withdraw row over a depth-%u tree has %u", c->circ.n_inputs(), t->depth,
                10 + t->depth);
  return SPP_OK;
}
// size == SPP_TREE_SIZE_NOW: the tree as it stands, the launches spp_prove_withdraw_notes_device always made.  Any other size: the
// first `size` leaves (merkle_prefix.hpp) -- k_merkle_frontier, then the as-of rows kernel for body and tail, all on the tree's
// stream in order; the size is checked under the lock, before a workspace is taken.
static int prove_withdraw_notes_device(spp_circuit* c, spp_merkle_tree* t, uint64_t size, size_t count, const void* d_notes, const void* d_rs,
                                       void* d_proofs, void* d_pws, void* d_status) {
  if (!c || !t || !d_notes || !d_rs || !d_proofs || !d_pws || !d_status) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (int e = withdraw_notes_args(c, t)) return e;
  const bool asof = size != SPP_TREE_SIZE_NOW;
  if (count == 0 && !asof) return SPP_OK;
  if (count > (1u << 20)) return fail(SPP_ERR_BAD_INPUT, "batch too large");
  spp_ctx* ctx = c->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  if (int e = spp_ensure_ctx_consts(ctx)) return e;
  if (asof && size > t->n_leaves) return spp_tree_frontier_enqueue(t, &size);   // the refusal, also for count == 0
  if (count == 0) return SPP_OK;
  Workspace* wp;
  if (int e = take_sized_workspace(c, count, c->generic_solver, &wp)) return e;
  Workspace &w = *wp, &wt = c->ws[c->next_ws];
  const size_t tail = batch_tail(c, count), body = count - tail;
  const uint8_t* notes = (const uint8_t*)d_notes;
  HIP_TRY(hipStreamWaitEvent(ctx->stream, w.ev_in, 0));
  if (tail) HIP_TRY(hipStreamWaitEvent(ctx->stream, wt.ev_in, 0));
  if (asof) {
    if (int e = spp_tree_frontier_enqueue(t, &size)) return e;
    launch_withdraw_rows_at(ctx->stream, ctx->gk_table, ctx->hc, t->dev, size, t->d_frontier, notes, w.d_inputs, (uint32_t)body);
    if (tail)
      launch_withdraw_rows_at(ctx->stream, ctx->gk_table, ctx->hc, t->dev, size, t->d_frontier, notes + body * SPP_NOTE_LEN, wt.d_inputs,
                              (uint32_t)tail);
  } else {
    launch_withdraw_rows(ctx->stream, ctx->gk_table, ctx->hc, t->dev, notes, w.d_inputs, (uint32_t)body);
    if (tail) launch_withdraw_rows(ctx->stream, ctx->gk_table, ctx->hc, t->dev, notes + body * SPP_NOTE_LEN, wt.d_inputs, (uint32_t)tail);
  }
  HIP_TRY(hipEventRecord(w.ev_rows, ctx->stream));
  HIP_TRY(hipStreamWaitEvent(w.st, w.ev_rows, 0));
  if (tail) HIP_TRY(hipStreamWaitEvent(wt.st, w.ev_rows, 0));
  const BatchIO io{(const uint8_t*)d_rs, (uint8_t*)d_proofs, (uint8_t*)d_pws, (uint32_t*)d_status};
  if (int e = prove_on_device(c, w, body, w.d_inputs, io)) return e;
  if (!tail) return SPP_OK;
  return prove_on_device(c, wt, tail, wt.d_inputs, io.at(c, body));
}
extern "C" int spp_prove_withdraw_notes_device(spp_circuit* c, spp_merkle_tree* t, size_t count, const void* d_notes, const void* d_rs,
                                               void* d_proofs, void* d_pws, void* d_status) {
  return prove_withdraw_notes_device(c, t, SPP_TREE_SIZE_NOW, count, d_notes, d_rs, d_proofs, d_pws, d_status);
}
extern "C" int spp_prove_withdraw_notes_at_device(spp_circuit* c, spp_merkle_tree* t, uint64_t size, size_t count, const void* d_notes,
                                                  const void* d_rs, void* d_proofs, void* d_pws, void* d_status) {
  return prove_withdraw_notes_device(c, t, size, count, d_notes, d_rs, d_proofs, d_pws, d_status);
}
// Host form: all rows are built (one gather, one root) before spp_prove_batch proves them in chunks.
extern "C" int spp_prove_withdraw_notes(spp_circuit* c, spp_merkle_tree* t, size_t count, const uint8_t* notes, const uint8_t* rs, uint8_t* proofs,
                                        uint8_t* pws, int32_t* status) {
  if (!c || !t || !notes || !proofs || !pws) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (int e = withdraw_notes_args(c, t)) return e;
  if (count == 0) return SPP_OK;
  if (count > (1u << 24)) return fail(SPP_ERR_BAD_INPUT, "too many notes in one call");
  std::vector<uint8_t> rows(count * c->in_stride);
  if (int e = spp_withdraw_rows_from_tree(t, count, notes, rows.data())) return e;
  return spp_prove_batch(c, count, rows.data(), rs, proofs, pws, status);
}
extern "C" int spp_prove_withdraw_notes_at(spp_circuit* c, spp_merkle_tree* t, uint64_t size, size_t count, const uint8_t* notes, const uint8_t* rs,
                                           uint8_t* proofs, uint8_t* pws, int32_t* status) {
  if (size == SPP_TREE_SIZE_NOW) return spp_prove_withdraw_notes(c, t, count, notes, rs, proofs, pws, status);
  if (!c || !t || !notes || !proofs || !pws) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (int e = withdraw_notes_args(c, t)) return e;
  if (count > (1u << 24)) return fail(SPP_ERR_BAD_INPUT, "too many notes in one call");
  std::vector<uint8_t> rows(std::max<size_t>(count, 1) * c->in_stride);
  if (int e = spp_withdraw_rows_from_tree_at(t, size, count, notes, rows.data())) return e;   // refuses a size past the tree, also for count == 0
  if (count == 0) return SPP_OK;
  return spp_prove_batch(c, count, rows.data(), rs, proofs, pws, status);
}
// Deposit proofs from records against the resident tree (include/spp.h): spp_prove_withdraw_notes_device's scheme with k_deposit_rows
// as the rows kernel -- gathered on the tree's stream under the context lock, body and tail into their own workspaces' d_inputs.
// The range check reads the tree's size under that lock, before a workspace is taken.
static int deposit_args(spp_circuit* c, spp_merkle_tree* t) {
  if (c->circ.id != SPP_CIRCUIT_DEPOSIT) return fail(SPP_ERR_BAD_INPUT, "not a deposit circuit");
  if (t->ctx != c->ctx) return fail(SPP_ERR_BAD_INPUT, "the tree belongs to another context");
  if (c->circ.n_inputs() != SPP_DEPOSIT_INPUTS || t->depth != SPP_TREE_DEPTH)
    return fail(SPP_ERR_BAD_INPUT, "the circuit takes %u inputs and the tree has depth %u; a deposit row has %d fields over a depth-%d tree",
                c->circ.n_inputs(), t->depth, SPP_DEPOSIT_INPUTS, SPP_TREE_DEPTH);
  return SPP_OK;
}
extern "C" int spp_prove_deposits_device(spp_circuit* c, spp_merkle_tree* t, uint64_t first_index, size_t count, const void* d_deposits,
                                         const void* d_rs, void* d_proofs, void* d_pws, void* d_status) {
  if (!c || !t || !d_deposits || !d_rs || !d_proofs || !d_pws || !d_status) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (int e = deposit_args(c, t)) return e;
  if (count > (1u << 20)) return fail(SPP_ERR_BAD_INPUT, "batch too large");
  spp_ctx* ctx = c->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int e = spp_check_deposit_range(t, first_index, count)) return e;
  if (count == 0) return SPP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  if (int e = spp_ensure_ctx_consts(ctx)) return e;
  Workspace* wp;
  if (int e = take_sized_workspace(c, count, c->generic_solver, &wp)) return e;
  Workspace &w = *wp, &wt = c->ws[c->next_ws];
  const size_t tail = batch_tail(c, count), body = count - tail;
  const uint8_t* deposits = (const uint8_t*)d_deposits;
  HIP_TRY(hipStreamWaitEvent(ctx->stream, w.ev_in, 0));
  if (tail) HIP_TRY(hipStreamWaitEvent(ctx->stream, wt.ev_in, 0));
  launch_deposit_rows(ctx->stream, ctx->gk_table, ctx->hc, t->dev, first_index, deposits, w.d_inputs, (uint32_t)body);
  if (tail)
    launch_deposit_rows(ctx->stream, ctx->gk_table, ctx->hc, t->dev, first_index + body, deposits + body * SPP_DEPOSIT_LEN, wt.d_inputs, (uint32_t)tail);
  HIP_TRY(hipEventRecord(w.ev_rows, ctx->stream));
  HIP_TRY(hipStreamWaitEvent(w.st, w.ev_rows, 0));
  if (tail) HIP_TRY(hipStreamWaitEvent(wt.st, w.ev_rows, 0));
  const BatchIO io{(const uint8_t*)d_rs, (uint8_t*)d_proofs, (uint8_t*)d_pws, (uint32_t*)d_status};
  if (int e = prove_on_device(c, w, body, w.d_inputs, io)) return e;
  if (!tail) return SPP_OK;
  return prove_on_device(c, wt, tail, wt.d_inputs, io.at(c, body));
}
// Host form: all rows are built (one launch) before spp_prove_batch proves them in chunks.
extern "C" int spp_prove_deposits(spp_circuit* c, spp_merkle_tree* t, uint64_t first_index, size_t count, const uint8_t* deposits, const uint8_t* rs,
                                  uint8_t* proofs, uint8_t* pws, int32_t* status) {
  if (!c || !t || (count && (!deposits || !proofs || !pws))) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (int e = deposit_args(c, t)) return e;
  if (count > (1u << 24)) return fail(SPP_ERR_BAD_INPUT, "too many deposits in one call (%zu; at most 2^24)", count);
  std::vector<uint8_t> rows(std::max<size_t>(count, 1) * c->in_stride);
  if (int e = spp_deposit_rows_from_tree(t, first_index, count, deposits, rows.data())) return e;   // the field and range refusals, also for count == 0
  if (count == 0) return SPP_OK;
  return spp_prove_batch(c, count, rows.data(), rs, proofs, pws, status);
}
extern "C" int spp_commitment_challenge(spp_circuit* c, size_t count, const uint8_t* inputs, uint8_t* challenges) {
  if (!c || !inputs || !challenges) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count == 0) return SPP_OK;
  if (count > 4096) return fail(SPP_ERR_BAD_INPUT, "at most 4096 rows per call");
  if (c->CB.N == 0) return fail(SPP_ERR_BAD_INPUT, "the circuit has no commitment");
  std::lock_guard<std::mutex> lk(c->ctx->mu);
  HIP_TRY(hipSetDevice(c->ctx->device));
  Workspace& w = c->ws[c->next_ws];
  if (int e = ensure_workspace(c, w, count)) return e;
  hipStream_t st = w.st;
  const uint32_t P = (uint32_t)count;
  HIP_TRY(hipMemcpyAsync(w.d_inputs, inputs, c->in_stride * count, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(w.d_rs, 0, 64 * count, st));
  launch_load_inputs(st, w.d_inputs, w.d_rs, w.W, c->circ.n_inputs(), c->circ.n_wires, P);
  // whatever the program computes before the commitment (nothing for an all-inputs system), then commit and hash
  for (const SolveStep& s : c->schedule) {
    if (s.kind == SolveStep::COMMIT) break;
    switch (s.kind) {
      case SolveStep::SEQ: launch_solve(st, c->dc, w.W, w.scratch, s.a, s.b, P); break;
      case SolveStep::BATCH_DIV: launch_batch_div(st, c->dc, w.W, w.scratch, s.a, s.b, P); break;
      case SolveStep::COUNT8: launch_count8(st, c->dc, w.W, w.counters, s.a, s.b, s.c, P); break;
      default: break;
    }
  }
  run_msm(c, w, c->CB, w.CB, P, false);
  launch_challenge(st, w.CB.out, w.W, c->circ.challenge_wire, P, w.commit_affine, w.d_status);
  std::vector<Fr> out(count);
  HIP_TRY(hipMemcpyAsync(out.data(), w.W + (size_t)c->circ.challenge_wire * P, sizeof(Fr) * count, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (size_t i = 0; i < count; i++) out[i].to_bytes_be(challenges + 32 * i);
  return SPP_OK;
}
extern "C" int spp_sync(spp_circuit* c) {
  if (!c) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  HIP_TRY(hipSetDevice(c->ctx->device));
  for (auto& w : c->ws)
    if (w.st) HIP_TRY(hipStreamSynchronize(w.st));
  return SPP_OK;
}
extern "C" int spp_last_timings(spp_circuit* c, float ms[9]) { return spp_timings(c, 0, ms); }
extern "C" int spp_timings(spp_circuit* c, int which, float ms[9]) {
  if (!c || !ms) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  HIP_TRY(hipSetDevice(c->ctx->device));
  Workspace& w = c->ws[which ? c->prev_ws : c->last_ws];
  if (w.cap == 0) return fail(SPP_ERR_BAD_INPUT, "no such batch");
  HIP_TRY(hipStreamSynchronize(w.st));
  for (int i = 0; i < 6; i++) {
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, w.ev[i], w.ev[i + 1]));
    ms[i] = t;
  }
  float tot = 0;
  HIP_TRY(hipEventElapsedTime(&tot, w.ev[0], w.ev[6]));
  ms[6] = tot;
  float sum = 0;
  for (size_t i = 0; i < w.msm_ev_used; i++) {
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, w.msm_ev[i].first, w.msm_ev[i].second));
    sum += t;
  }
  ms[7] = w.msm_ev_used ? sum / (float)w.msm_ev_used : 0.f;
  ms[8] = (float)w.msm_ev_used;
  return SPP_OK;
}

// per-launch durations of the MSM kernels of one batch, in launch order: commitment (CB), A, B1, K, Z, PoK (CS), then the G2 set.
// The table walks alone: the byte-bucket kernels of the lookup-inverse wires (msm_lookup.hpp) are not in A or K here; their time
// is in stage 3 of spp_timings (msm_g1, ev[3] .. ev[4]) with the walks, the folds and the Horner launches.
extern "C" int spp_msm_kernel_ms(spp_circuit* c, int which, float ms[7]) {
  if (!c || !ms) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  HIP_TRY(hipSetDevice(c->ctx->device));
  Workspace& w = c->ws[which ? c->prev_ws : c->last_ws];
  if (w.cap == 0) return fail(SPP_ERR_BAD_INPUT, "no such batch");
  HIP_TRY(hipStreamSynchronize(w.st));
  HIP_TRY(hipStreamSynchronize(w.st2));
  if (w.own_st2p) HIP_TRY(hipStreamSynchronize(w.own_st2p));
  for (int i = 0; i < 7; i++) ms[i] = 0.f;
  for (size_t i = 0; i < w.msm_ev_used && i < 6; i++) HIP_TRY(hipEventElapsedTime(&ms[i], w.msm_ev[i].first, w.msm_ev[i].second));
  if (c->B2.N) HIP_TRY(hipEventElapsedTime(&ms[6], w.g2_ev.first, w.g2_ev.second));
  return SPP_OK;
}
// on = 1: both batch workspaces and the G2 MSM run on ONE stream (kernel durations are then not stretched by another stream
// sharing the chip: what a roofline figure needs); on = 0: the pipelined default.  Drains the device first.
extern "C" int spp_set_serial(spp_circuit* c, int on) {
  if (!c) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  std::lock_guard<std::mutex> lk(c->ctx->mu);
  HIP_TRY(hipSetDevice(c->ctx->device));
  HIP_TRY(hipDeviceSynchronize());
  for (int k = 0; k < SPP_NWS; k++) {
    Workspace& w = c->ws[k];
    w.st = on ? c->ws[0].own_st : w.own_st;
    w.st2 = on ? w.st : w.own_st2;
  }
  return SPP_OK;
}

extern "C" int spp_prove_batch(spp_circuit* c, size_t count, const uint8_t* inputs, const uint8_t* rs, uint8_t* proofs, uint8_t* pws,
                               int32_t* status) {
  if (!c || !inputs || !proofs || !pws) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count == 0) return SPP_OK;
  std::vector<uint8_t> rnd;
  if (!rs) {
    if (int e = os_blinding(rnd, count)) return e;
    rs = rnd.data();
  }
  std::vector<uint32_t> st(count);
  {
    // Large host batches are cut into chunks that alternate between the two workspaces / proving streams, so the
    // copies and the solver of chunk k+1 overlap the MSMs of chunk k exactly as consecutive spp_prove_batch_device calls
    // do, and the workspaces never grow beyond one chunk.
    std::lock_guard<std::mutex> lk(c->ctx->mu);
    HIP_TRY(hipSetDevice(c->ctx->device));
    const size_t pref = c->circ.n_wires <= 16384 ? 4096 : 2048;  // batch sizes at which the per-launch overheads are amortised
    const size_t chunk = count <= pref + pref / 2 ? count : pref;
    const size_t inl = c->in_stride, pwl = c->pw_stride;
    // copies back to pageable host memory block the caller until their stream has drained, so the results of chunk k are
    // fetched only after chunk k+1 has been enqueued on the other stream
    auto fetch = [&](Workspace& w, size_t off, size_t n) -> int {
      hipStream_t s = w.st;
      HIP_TRY(hipMemcpyAsync(proofs + (size_t)SPP_PROOF_LEN * off, w.d_proofs, (size_t)SPP_PROOF_LEN * n, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(pws + pwl * off, w.d_pws, pwl * n, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(st.data() + off, w.d_status, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      return 0;
    };
    Workspace* prev_w = nullptr;
    size_t prev_off = 0, prev_n = 0;
    // chunk list: a last chunk that is not a multiple of the wave width is cut into a 64-aligned body and a tail (see
    // batch_tail); the two alternate workspaces like any other pair of chunks
    std::vector<std::pair<size_t, size_t>> chunks;
    for (size_t off = 0; off < count; off += chunk) {
      const size_t n = std::min(chunk, count - off), t = batch_tail(c, n);
      if (t) {
        chunks.push_back({off, n - t});
        chunks.push_back({off + n - t, t});
      } else chunks.push_back({off, n});
    }
    for (const auto& ch : chunks) {
      const size_t off = ch.first, n = ch.second;
      Workspace& w = take_workspace(c, 2);
      if (int e = ensure_workspace(c, w, n)) return e;   // the chunk's own workspace only, sized to the chunk
      hipStream_t s = w.st;
      HIP_TRY(hipMemcpyAsync(w.d_inputs, inputs + inl * off, inl * n, hipMemcpyHostToDevice, s));
      HIP_TRY(hipMemcpyAsync(w.d_rs, rs + 64 * off, 64 * n, hipMemcpyHostToDevice, s));
      if (int e = prove_on_device(c, w, (uint32_t)n, w.d_inputs, w.d_rs, w.d_proofs, w.d_pws, w.d_status)) return e;
      if (prev_w)
        if (int e = fetch(*prev_w, prev_off, prev_n)) return e;
      prev_w = &w;
      prev_off = off;
      prev_n = n;
    }
    if (prev_w)
      if (int e = fetch(*prev_w, prev_off, prev_n)) return e;
    for (auto& w : c->ws)
      if (w.st) HIP_TRY(hipStreamSynchronize(w.st));
  }
  int rc = SPP_OK;
  for (size_t i = 0; i < count; i++) {
    int32_t v = st[i] ? SPP_ERR_UNSAT : SPP_OK;
    if (status) status[i] = v;
    if (v && rc == SPP_OK) rc = fail(SPP_ERR_UNSAT, "proof %zu: inputs do not satisfy the circuit", i);
    if (v) memset(proofs + (size_t)SPP_PROOF_LEN * i, 0, SPP_PROOF_LEN);
  }
  return rc;
}

// -----------------------------------------------------------------------------------------------------
// Withdrawals from notes: both proofs, one audit record per new identity (include/spp.h; the plan is withdrawal_plan.hpp)
// -----------------------------------------------------------------------------------------------------
namespace {
void wipe_bytes(void* p, size_t bytes) {
  volatile uint8_t* v = (volatile uint8_t*)p;
  for (size_t i = 0; i < bytes; i++) v[i] = 0;
}
struct WipedI8 {   // host scratch that held noise or secret keys
  std::vector<int8_t> v;
  ~WipedI8() { wipe_bytes(v.data(), v.size()); }
};
// n coefficients uniform in [-3, 3] from OS randomness: three bits of a byte, the value 7 rejected (scripts/generate_audit.py:469-506
// draws randint(-3, 3))
int os_noise(int8_t* out, size_t n) {
  FILE* f = fopen("/dev/urandom", "rb");
  if (!f) return fail(SPP_ERR_IO, "cannot read /dev/urandom");
  uint8_t buf[4096];
  size_t done = 0;
  int rc = SPP_OK;
  while (done < n && rc == SPP_OK) {
    if (fread(buf, 1, sizeof buf, f) != sizeof buf) rc = fail(SPP_ERR_IO, "cannot read /dev/urandom");
    for (size_t k = 0; k < sizeof buf && done < n && rc == SPP_OK; k++) {
      const int v = buf[k] & 7;
      if (v != 7) out[done++] = (int8_t)(v - 3);
    }
  }
  wipe_bytes(buf, sizeof buf);
  fclose(f);
  return rc;
}
}  // namespace

// The withdraw side of spp_prove_withdrawals: rows resident in the call's own device buffer (complete: the tree's stream has been
// waited for), proved in the chunks spp_prove_batch cuts, on the circuit's proving streams.  Unlike spp_prove_batch the context is
// locked per chunk, for the enqueue only, so that the audit batch of the same call gets its turns; therefore the outputs of a chunk
// go to buffers of the call, not to the workspace's, which another caller may take over in between.
static int prove_resident_rows(spp_circuit* c, size_t count, const uint8_t* d_rows, const uint8_t* rs, uint8_t* proofs, uint8_t* pws,
                               std::vector<uint32_t>& stat) {
  HIP_TRY(hipSetDevice(c->ctx->device));
  const size_t pref = c->circ.n_wires <= 16384 ? 4096 : 2048;
  const size_t chunk = count <= pref + pref / 2 ? count : pref;
  const size_t inl = c->in_stride, pwl = c->pw_stride;
  struct CopyStream {
    hipStream_t s = nullptr;
    ~CopyStream() { if (s) hipStreamDestroy(s); }
  } copy;
  HIP_TRY(hipStreamCreateWithFlags(&copy.s, hipStreamNonBlocking));
  hipStream_t st = copy.s;
  struct Set {
    DevBuf rs, proofs, pws, status;
    hipStream_t proving = nullptr;
    size_t off = 0, n = 0;
  } sets[2];
  std::vector<std::pair<size_t, size_t>> chunks;   // as spp_prove_batch: a last chunk that is no multiple of the wave width is body + tail
  for (size_t off = 0; off < count; off += chunk) {
    const size_t n = std::min(chunk, count - off), t = batch_tail(c, n);
    if (t) {
      chunks.push_back({off, n - t});
      chunks.push_back({off + n - t, t});
    } else chunks.push_back({off, n});
  }
  for (size_t k = 0; k < std::min<size_t>(2, chunks.size()); k++) {
    Set& s = sets[k];
    HIP_TRY(s.rs.alloc(chunk * 64)); HIP_TRY(s.proofs.alloc(chunk * SPP_PROOF_LEN)); HIP_TRY(s.pws.alloc(chunk * pwl)); HIP_TRY(s.status.alloc(chunk * 4));
  }
  auto fetch = [&](Set& s) -> int {
    HIP_TRY(hipStreamSynchronize(s.proving));
    HIP_TRY(hipMemcpyAsync(proofs + (size_t)SPP_PROOF_LEN * s.off, s.proofs.p, (size_t)SPP_PROOF_LEN * s.n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(pws + pwl * s.off, s.pws.p, pwl * s.n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(stat.data() + s.off, s.status.p, 4 * s.n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    s.n = 0;
    return 0;
  };
  int k = 0;
  for (const auto& ch : chunks) {
    Set& s = sets[k];
    k ^= 1;
    if (s.n)
      if (int e = fetch(s)) return e;
    const size_t off = ch.first, n = ch.second;
    HIP_TRY(hipMemcpyAsync(s.rs.p, rs + 64 * off, 64 * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    s.off = off;
    s.n = n;
    std::lock_guard<std::mutex> lk(c->ctx->mu);
    Workspace& w = take_workspace(c, 2);
    if (int e = ensure_workspace(c, w, n)) return e;
    s.proving = w.st;
    if (int e = prove_on_device(c, w, n, d_rows + inl * off, BatchIO{s.rs.as<uint8_t>(), s.proofs.as<uint8_t>(), s.pws.as<uint8_t>(), s.status.as<uint32_t>()}))
      return e;
  }
  for (int j = 0; j < 2; j++) {      // the older chunk first
    Set& s = sets[k ^ j];
    if (s.n)
      if (int e = fetch(s)) return e;
  }
  return SPP_OK;
}

extern "C" int spp_prove_withdrawals(spp_circuit* withdraw, spp_circuit* audit, spp_merkle_tree* t, spp_pool* pool, uint64_t size,
                                     const uint32_t* pk_a, const uint32_t* pk_b, size_t count, const uint8_t* notes, const int8_t* r,
                                     const int8_t* e1, const int8_t* e2, const uint8_t* rs_withdraw, const uint8_t* rs_audit, uint8_t* proofs,
                                     uint8_t* pws, int32_t* status, uint32_t* audit_of, uint32_t* audit_note, uint32_t* n_audits,
                                     size_t audit_cap, uint8_t* audit_proofs, uint8_t* audit_pws, int32_t* audit_status, uint32_t* c0,
                                     uint32_t* c1) {
  if (!withdraw || !audit || !t || !pk_a || !pk_b || !n_audits || (count && (!notes || !proofs || !pws || !audit_of)) ||
      (count && audit_cap && (!audit_note || !audit_proofs || !audit_pws || !c0 || !c1)))
    return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if ((r != nullptr) != (e1 != nullptr) || (r != nullptr) != (e2 != nullptr))
    return fail(SPP_ERR_BAD_INPUT, "r, e1 and e2: all three, or all three NULL for noise from the operating system");
  if (int e = withdraw_notes_args(withdraw, t)) return e;
  if (audit->circ.id != SPP_CIRCUIT_AUDIT || audit->circ.n_inputs() != 3360) return fail(SPP_ERR_BAD_INPUT, "not the audit circuit");
  spp_ctx* ctx = withdraw->ctx;
  if (audit->ctx != ctx) return fail(SPP_ERR_BAD_INPUT, "the audit circuit belongs to another spp_ctx than the withdraw circuit");
  if (pool && spp_pool_view(pool, nullptr, nullptr) != ctx) return fail(SPP_ERR_BAD_INPUT, "the pool belongs to another spp_ctx than the circuits");
  if (count > SPP_WITHDRAWALS_MAX) return fail(SPP_ERR_BAD_INPUT, "too many notes in one call (%zu; at most 2^20)", count);
  for (int i = 0; i < 1024; i++)
    if (pk_a[i] >= 167772161u || pk_b[i] >= 167772161u) return fail(SPP_ERR_BAD_INPUT, "public key coefficient not in [0, q)");
  if (int e = spp_check_notes(count, notes)) return e;
  for (size_t i = 0; i < count; i++) {
    bool sk_zero = true;
    for (int b = 0; b < 32; b++) sk_zero &= notes[SPP_NOTE_LEN * i + 64 + b] == 0;
    if (sk_zero) return fail(SPP_ERR_BAD_INPUT, "note %zu: secret_key is 0", i);
  }
  *n_audits = 0;
  const bool asof = size != SPP_TREE_SIZE_NOW;
  const size_t inl = withdraw->in_stride;
  DevBuf drows;
  uint32_t n = 0;
  std::vector<uint32_t> note(count);
  {
    // rows and plan on the tree's stream, in order with inserts and the pool's commits; the plan is read back
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    if (int e = spp_ensure_ctx_consts(ctx)) return e;
    if (asof && size > t->n_leaves) return spp_tree_frontier_enqueue(t, &size);   // the refusal, also for count == 0
    if (count == 0) return SPP_OK;
    hipStream_t st = ctx->stream;
    DevBuf dnotes, dscratch, dplan;
    UP(dnotes, notes, count * SPP_NOTE_LEN);
    HIP_TRY(drows.alloc(count * inl));
    HIP_TRY(dscratch.alloc(spp_withdrawal_plan_scratch_bytes(count)));
    HIP_TRY(dplan.alloc((2 * count + 1) * sizeof(uint32_t)));
    if (asof) {
      if (int e = spp_tree_frontier_enqueue(t, &size)) return e;
      launch_withdraw_rows_at(st, ctx->gk_table, ctx->hc, t->dev, size, t->d_frontier, dnotes.as<uint8_t>(), drows.as<uint8_t>(), (uint32_t)count);
    } else {
      launch_withdraw_rows(st, ctx->gk_table, ctx->hc, t->dev, dnotes.as<uint8_t>(), drows.as<uint8_t>(), (uint32_t)count);
    }
    uint32_t *d_of = dplan.as<uint32_t>(), *d_note = d_of + count, *d_n = d_note + count;
    if (int e = spp_withdrawal_plan_enqueue(ctx, pool, drows.as<uint8_t>() + 4 * 32, inl, count, dscratch.p, d_of, d_note, d_n)) return e;
    HIP_TRY(hipMemcpyAsync(audit_of, d_of, count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(note.data(), d_note, count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&n, d_n, sizeof n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipGetLastError());
  }
  *n_audits = n;
  if (std::min<size_t>(n, audit_cap)) memcpy(audit_note, note.data(), std::min<size_t>(n, audit_cap) * sizeof(uint32_t));
  if (n > audit_cap)
    return fail(SPP_ERR_BAD_INPUT, "the batch needs %u audit records, audit_cap is %zu", n, audit_cap);

  // the representatives' secrets in slot order
  WipedI8 sk, gr, ge1, ge2;
  std::vector<uint8_t> grs;
  sk.v.resize((size_t)n * 32);
  gr.v.resize((size_t)n * 1024); ge1.v.resize((size_t)n * 64); ge2.v.resize((size_t)n * 1024);
  for (size_t s = 0; s < n; s++) memcpy(sk.v.data() + 32 * s, notes + SPP_NOTE_LEN * note[s] + 64, 32);
  if (r) {
    for (size_t s = 0; s < n; s++) {
      memcpy(gr.v.data() + 1024 * s, r + (size_t)1024 * note[s], 1024);
      memcpy(ge1.v.data() + 64 * s, e1 + (size_t)64 * note[s], 64);
      memcpy(ge2.v.data() + 1024 * s, e2 + (size_t)1024 * note[s], 1024);
    }
  } else {
    if (int e = os_noise(gr.v.data(), gr.v.size())) return e;
    if (int e = os_noise(ge1.v.data(), ge1.v.size())) return e;
    if (int e = os_noise(ge2.v.data(), ge2.v.size())) return e;
  }
  if (rs_audit) {
    grs.resize((size_t)n * 64);
    for (size_t s = 0; s < n; s++) memcpy(grs.data() + 64 * s, rs_audit + (size_t)64 * note[s], 64);
  }
  std::vector<uint8_t> rnd;
  if (!rs_withdraw) {
    if (int e = os_blinding(rnd, count)) return e;
    rs_withdraw = rnd.data();
  }

  // both batches in flight together: the audit records on a host thread of their own (spp_prove_audit_records as it is, which locks
  // the context for each enqueue only), the withdraw chunks on this one
  int rc_audit = SPP_OK;
  char audit_err[sizeof g_spp_err] = {0};
  std::thread audit_thread;
  if (n)
    audit_thread = std::thread([&] {
      rc_audit = spp_prove_audit_records(audit, pk_a, pk_b, n, (const uint8_t*)sk.v.data(), gr.v.data(), ge1.v.data(), ge2.v.data(),
                                         rs_audit ? grs.data() : nullptr, audit_proofs, audit_pws, audit_status, c0, c1);
      if (rc_audit) memcpy(audit_err, g_spp_err, sizeof audit_err);   // the message is thread-local
    });
  std::vector<uint32_t> stat(count);
  const int rc_rows = prove_resident_rows(withdraw, count, drows.as<uint8_t>(), rs_withdraw, proofs, pws, stat);
  if (audit_thread.joinable()) audit_thread.join();
  if (rc_rows) return rc_rows;
  if (rc_audit && rc_audit != SPP_ERR_UNSAT) {
    memcpy(g_spp_err, audit_err, sizeof audit_err);
    return rc_audit;
  }
  int rc = SPP_OK;
  for (size_t i = 0; i < count; i++) {
    const int32_t v = stat[i] ? SPP_ERR_UNSAT : SPP_OK;
    if (status) status[i] = v;
    if (v && rc == SPP_OK) rc = fail(SPP_ERR_UNSAT, "note %zu: inputs do not satisfy the circuit", i);
    if (v) memset(proofs + (size_t)SPP_PROOF_LEN * i, 0, SPP_PROOF_LEN);
  }
  if (rc == SPP_OK && rc_audit) {
    memcpy(g_spp_err, audit_err, sizeof audit_err);
    rc = rc_audit;
  }
  return rc;
}

extern "C" int spp_prove_withdraw(spp_circuit* c, const spp_withdraw_inputs* in, const uint8_t rs_seed[64], uint8_t proof[SPP_PROOF_LEN],
                                  uint8_t pw[SPP_WITHDRAW_PW_LEN]) {
  if (!c || !in || !proof || !pw) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (c->circ.id != SPP_CIRCUIT_WITHDRAW) return fail(SPP_ERR_BAD_INPUT, "not a withdraw circuit");
  if (c->circ.n_inputs() != 10 + SPP_TREE_DEPTH) return fail(SPP_ERR_BAD_INPUT, "this entry point serves the depth-16 circuit; use spp_prove_batch");
  std::vector<uint8_t> buf(26 * 32, 0);
  auto put = [&](int i, const uint8_t* v) { memcpy(buf.data() + 32 * i, v, 32); };
  auto put64 = [&](int i, uint64_t v) { for (int k = 0; k < 8; k++) buf[32 * i + 31 - k] = (uint8_t)(v >> (8 * k)); };
  put(0, in->root); put(1, in->nullifier); put(2, in->recipient); put64(3, in->amount); put(4, in->wa_commitment);
  put(5, in->secret_key); put(6, in->owner_x); put(7, in->owner_y); put(8, in->randomness); put64(9, in->index);
  for (int i = 0; i < SPP_TREE_DEPTH; i++) put(10 + i, in->siblings[i]);
  int32_t st = 0;
  return spp_prove_batch(c, 1, buf.data(), rs_seed, proof, pw, &st);
}

extern "C" int spp_debug_witness(spp_circuit* c, uint8_t* out, size_t n_wires) {
  if (!c || !out) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  std::lock_guard<std::mutex> lk(c->ctx->mu);
  Workspace& w = c->ws[c->last_ws];
  if (w.cap == 0) return fail(SPP_ERR_BAD_INPUT, "no batch has been proved yet");
  HIP_TRY(hipSetDevice(c->ctx->device));
  HIP_TRY(hipStreamSynchronize(w.st));
  size_t P = w.last_P;   // column 0 of W at the stride of the last batch
  std::vector<Fr> col(std::min<size_t>(n_wires, c->circ.n_wires));
  for (size_t i = 0; i < col.size(); i++) HIP_TRY(hipMemcpy(&col[i], w.W + i * P, sizeof(Fr), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < col.size(); i++) col[i].to_bytes_be(out + 32 * i);
  return SPP_OK;
}
