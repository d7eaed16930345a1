// What the units that load a circuit (spp_plan.cpp, spp_load.cpp) and prove with it (spp_prove.cpp) share: the circuit object,
// its MSM sets and batch workspaces, the experiment switches.  Private, like spp_internal.hpp.
#pragma once
#include "spp_internal.hpp"
#include "msm_classes.hpp"
#include "msm_lookup.hpp"
#include "coop_plan.hpp"   // SolveStep, the schedule and the cooperative solver's items

template <class F>
struct MsmSet {
  uint32_t N = 0;
  Affine<F>* table = nullptr;
  uint32_t* rows = nullptr;
  bool from_h = false;   // scalars come from the h array instead of the witness
  uint32_t c = 0;        // window bits of this set's table
  uint32_t Wt = 0;       // table rows per base: msm_windows(c) = one per window (no passes), 1 = one row and msm_windows(c) passes
  // flat sets (Wt = 1): start and entry count of every 64-row block of the table (msm_ragged.hpp); `narrow`: some block is shorter
  // than 2^(c-1) entries, i.e. the table only serves scalars within the classes of the set's wires
  MsmBlock* blocks = nullptr;
  bool narrow = false;
};
template <class F>
struct MsmBuf {
  XYZZ<F>* partial = nullptr;
  XYZZ<F>* out = nullptr;
  size_t partial_cap = 0;   // elements allocated in `partial`
  MsmPlan plan{};           // lane layout of the last launch (the fold needs it)
};
struct Workspace {
  hipStream_t st = nullptr;
  hipStream_t st2 = nullptr;          // side stream: the G2 MSM only needs the witness, so it runs beside matrix eval / NTT / G1 MSMs
  hipStream_t own_st = nullptr, own_st2 = nullptr;   // the streams of the pipelined mode (st / st2 point at them unless serialised)
  hipStream_t own_st2p = nullptr;                    // side stream with a priority of its own: used by batches (see its creation)
  std::pair<hipEvent_t, hipEvent_t> g2_ev{nullptr, nullptr};   // dispatch timestamps of the G2 MSM kernel
  hipEvent_t ev_w = nullptr, ev_b2 = nullptr;
  // withdraw rows from notes (spp_prove_withdraw_notes_device): ev_in is recorded on `st` once a batch has loaded its input rows
  // (d_inputs may then be overwritten), ev_rows on the tree's stream once the next rows are written
  hipEvent_t ev_in = nullptr, ev_rows = nullptr;
  size_t cap = 0, last_P = 0;
  Fr *W = nullptr, *abc = nullptr, *scratch = nullptr;
  G1Affine* commit_affine = nullptr;
  uint8_t *d_inputs = nullptr, *d_rs = nullptr, *d_proofs = nullptr, *d_pws = nullptr;
  uint32_t* d_status = nullptr;
  uint32_t* counters = nullptr;   // [256][P] lookup histogram
  MsmBuf<Fq> A, B1, K, Z, CB, CS;
  MsmBuf<Fq> sA, rB;                  // small batches: s*Ar and r*Bs1 as table sums over the scaled witness (Ws, Wr)
  Fr *Ws = nullptr, *Wr = nullptr;
  MsmBuf<Fq2> B2;
  // signed-digit planes of the scalars of one MSM (k_msm_digits): dig1 is shared by the G1 sets, which run one after the
  // other on `st`; the G2 set runs beside them on the side stream and has its own
  int16_t *dig1 = nullptr, *dig2 = nullptr;
  size_t dig1_cap = 0, dig2_cap = 0;
  int16_t* small = nullptr;           // [sm_nslots][P]: byte-ranged wires as integers (small rows of the matrix evaluation)
  // byte-bucket sums of the lookup-inverse wires (msm_lookup.hpp, kernels_msm_lookup.hip); lk_bkt = nullptr: not allocated
  XYZZ<Fq>*lk_bkt = nullptr, *lk_win = nullptr, *lk_sum = nullptr;
  Fr* lk_inv = nullptr;
  int8_t* lk_dig = nullptr;
  uint8_t* lk_bytes = nullptr;
  void* audit_scratch = nullptr;      // temporaries of the audit input pipeline (spp_prove_audit_from_secrets_device), P = cap
  size_t audit_scratch_cap = 0;
  std::vector<void*> owned;
  hipEvent_t ev[8] = {};
  std::vector<std::pair<hipEvent_t, hipEvent_t>> msm_ev;
  size_t msm_ev_used = 0;
};

template <class F>
struct PendingTable {
  std::vector<Affine<F>> pts;
  Affine<F>* table;
  uint32_t c, Wt;
  MsmRagged layout;              // flat sets; empty: the uniform layout
  const MsmBlock* blocks;        // its copy on the device
};
// Experiment and diagnostic switches that steer the proving path.  Read from the environment by read_switches (spp_load.cpp)
// every time a circuit is loaded; nothing below the load reads the environment.
struct Switches {
  // How h = (A B - C) / Z reaches Krs (SPP_H_MODE, default 2):
  //   0  gnark's computeH: 3 inverse + 3 coset-forward + 1 coset-inverse transform, h coefficients against pk.G1.Z
  //   1  the H bases moved to the evaluation basis on the coset g*H at load: six transforms
  //   2  product form: h is the HIGH HALF of the product polynomial A(X) B(X) (A B = h (X^n - 1) + C with deg C < n), whose
  //      coefficients are a linear functional of its values on the 2n-th roots of unity H u zeta*H.  On H the values are a_i b_i =
  //      c_i = <C_i, w> -- linear in the witness, folded into per-wire bases at load; on zeta*H they need the transforms of A and
  //      B only: FOUR transforms, no transform of C, the same group element (spp_load_circuit, "product form")
  int h_mode = 2;
  bool no_coop = false;           // SPP_NO_COOP=1 (diagnostic): always the one-lane-per-proof solver
  bool trace_items = false;       // SPP_COOP_TRACE=1 (diagnostic): one launch per item of the cooperative solver
  bool one_track = false;         // SPP_COOP_ONE_TRACK=1 (diagnostic): the independent tracks of a stretch one after the other
  bool no_level_stream = false;   // SPP_NO_LEVEL_STREAM=1 (diagnostic): table-driven level items instead of the LDS-staged stream
  // batches up to this size are solved by one wave per proof (k_solve_coop); above it the wave-per-64-proofs solver has the
  // better throughput (a cooperative wave runs ~1/3 of the dependent instructions, but 64 times as many waves)
  uint32_t coop_max_batch = 1024;   // SPP_COOP_MAX (experiment) overrides
  // the same threshold for a program of generic solver instructions (a decoded gnark system: ~7 800 dependency levels of one to
  // four rows, profiles/generic_coop_probe.json); load_program copies it into coop_max_batch unless SPP_COOP_MAX is set
  uint32_t coop_max_batch_generic = 1024;
  bool no_side = false;           // SPP_NO_SIDE=1 (experiment): the G2 sum of a small batch on the batch's own stream
  int forced_depth = 0;           // SPP_DEPTH (experiment): batches in flight, 1 .. SPP_NWS; 0: by batch size (ws_depth)
  bool no_split = false;          // SPP_NO_SPLIT=1 (experiment): no cut of a batch into a 64-aligned body and a tail
  bool ragged = true;             // SPP_RAGGED=0 (comparison, fallback): every base wide -- full table rows for all, the windows that affords
  // Lookup-inverse wires summed by byte bucket (msm_lookup.hpp).  Unset: circuits with at least LKB_MIN_LOOKUPS such wires, batches
  // from LKB_MIN_BATCH proofs.  SPP_LOOKUP_BUCKETS=N (experiment, tests): every circuit that has such a wire, batches from N
  // proofs (at least 64); 0: never -- the library then runs the table walks alone, as before the path existed
  uint32_t lookup_min_batch = LKB_MIN_BATCH;
  bool lookup_forced = false;
  MsmTuning msm;                  // SPP_MSM_WAVES, SPP_MSM_WAVES_SMALL (experiment): rounds of resident waves per table walk (msm_plan.hpp)
};
// Up to a batch size that depends on the circuit s*Ar and r*Bs1 are two more fixed-base sums (sets A and B1 over the witness scaled by s and r) instead of
// 254 doublings on one lane each: 3 ms of a single proof's 9.  The sums cost a third of a proof's table additions, so a batch
// keeps the per-lane multiplication (its latency is shared by the whole batch).
// Measured (profiles/batch_size_sweep.py): the two extra sums cost ~15 us per withdraw proof and ~60 us per audit proof, the
// per-lane multiplication 3.3 ms per batch whatever its size -- so the switch is on the number of scaled scalars, P * (N_A + N_B1).
static constexpr uint64_t SCALED_BLIND_MAX_SCALARS = 1500000;
inline uint32_t scaled_blind_max_batch(uint32_t n_a, uint32_t n_b1) {
  const uint64_t n = (uint64_t)n_a + n_b1;
  return n ? (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(1024, SCALED_BLIND_MAX_SCALARS / n)) : 1;
}
struct spp_circuit {
  spp_ctx* ctx = nullptr;
  std::vector<SolveStep> schedule;
  Circuit circ;
  DevCircuit dc{};
  uint32_t c_bits = 10, n = 0, logn = 0;
  uint32_t max_batch_div = SOLVE_SCRATCH_MIN_ROWS;
  DevCoop coop{};
  uint32_t coop_item_count[COOP_KINDS] = {}, coop_stream_chunks = 0;   // what coop_plan made: items per COOP_* kind, chunks of the level stream (spp_circuit_plan_stats)
  uint32_t coop_generic_rows = 0, coop_generic_divs = 0;   // OP_SOLVE_ROW rows in level items, those with a run-time division
  Switches sw;
  bool generic_solver = false;    // the program is the solver of a decoded gnark system (OP_SOLVE_ROW ...): above the cooperative
                                  // solver's threshold ~12 K dependent row solves per proof on one lane -- a batch's solver phase
                                  // outlasts the rest of it, so three batches take turns
  uint32_t row_r = 0, row_s = 0, row_rs = 0, n_rows = 0;
  size_t in_stride = 0, pw_stride = 0;   // bytes of one proof's input row and of its public witness (blinding: 64, proof: SPP_PROOF_LEN)
  uint64_t table_bytes = 0;
  MsmSet<Fq> A, B1, K, Z, CB, CS;
  MsmSet<Fq2> B2;
  // lookup-inverse wires on the flat A (index 0) and K (1) sets (msm_lookup.hpp): lk_n of them (0: the path is off for this
  // circuit), the hint row of each, its base's index in the set, and the set's rows with MSM_ROW_ZERO for these bases
  uint32_t lk_n = 0;
  uint32_t* lk_hints = nullptr;
  uint32_t *lk_pos[2] = {nullptr, nullptr}, *lk_rows[2] = {nullptr, nullptr};
  Fr *tw_fwd = nullptr, *tw_inv = nullptr, *coset_br = nullptr, *coset_inv_br = nullptr;
  Fr zinv;
  // device copies owned here
  std::vector<void*> owned;
  Workspace ws[SPP_NWS];
  int next_ws = 0, last_ws = 0, prev_ws = 0;   // prev_ws: the workspace of the batch before the last one (spp_timings which = 1)
  std::vector<PendingTable<Fq>> pending1;    // tables allocated but not yet built (spp_load_circuit)
  std::vector<PendingTable<Fq2>> pending2;
};

template <class T>
static int own_upload(spp_circuit* c, T** dst, const std::vector<T>& src) {
  HIP_TRY(dev_upload(dst, src));
  c->owned.push_back((void*)*dst);
  return 0;
}

// shared between the units above; not part of the ABI
#pragma GCC visibility push(hidden)
int coop_plan(spp_circuit* c);                                   // spp_plan.cpp
int row_paths_plan(spp_circuit* c);
void destroy_circuit(spp_circuit* c);                            // spp_load.cpp
void free_workspace(Workspace& w);
#pragma GCC visibility pop
