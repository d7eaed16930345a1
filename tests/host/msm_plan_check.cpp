// csrc/msm_plan.hpp against tests/golden/msm_plan.json (the answers of the planner it was moved out of, see
// tests/golden/make_msm_plan.py): every plan field, the partial-sum capacity of a workspace and the slices left after the trim in
// workspaces sized for 2 048 and 4 096 proofs; then the clamps of the two tuning variables.
//   g++ -O2 -std=c++17 -I csrc tests/host/msm_plan_check.cpp -o msm_plan_check && ./msm_plan_check tests/golden/msm_plan.json
#include <cctype>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "msm_plan.hpp"

using namespace spp;

static int bad = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      if (bad++ < 20) { printf(__VA_ARGS__); printf("\n"); } \
    }                                            \
  } while (0)

static uint32_t slices_in_workspace(const MsmPlan& pl, uint32_t N, uint32_t P, uint32_t c, uint32_t Wt, uint32_t occ, const MsmTuning& t,
                                    size_t ws_P) {
  MsmPlan q = pl;
  q.fit(P, msm_partial_cap(N, ws_P, c, Wt, occ, t));
  return q.Sg;
}

int main(int argc, char** argv) {
  if (argc < 2) { printf("usage: msm_plan_check msm_plan.json\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { printf("cannot read %s\n", argv[1]); return 2; }
  std::string txt;
  char buf[4096];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) txt.append(buf, n);
  fclose(f);
  // the rows are the last member of the document: arrays of 17 unsigned integers
  const size_t at = txt.find("\"rows\"");
  if (at == std::string::npos) { printf("no rows in %s\n", argv[1]); return 2; }
  std::vector<unsigned long long> v;
  for (const char* p = txt.c_str() + at; *p;) {
    if (isdigit((unsigned char)*p)) {
      char* e;
      v.push_back(strtoull(p, &e, 10));
      p = e;
    } else p++;
  }
  const size_t COLS = 17;
  if (v.empty() || v.size() % COLS) { printf("malformed rows: %zu numbers\n", v.size()); return 2; }
  const size_t nrows = v.size() / COLS;
  for (size_t r = 0; r < nrows; r++) {
    const unsigned long long* x = &v[r * COLS];
    const uint32_t N = (uint32_t)x[0], P = (uint32_t)x[1], c = (uint32_t)x[2], Wt = (uint32_t)x[3], occ = (uint32_t)x[4];
    MsmTuning t;
    t.rounds = (uint32_t)x[5];
    t.rounds_small = (uint32_t)x[6];
    const MsmPlan pl = msm_plan(N, P, c, Wt, occ, t);
    const unsigned long long got[10] = {pl.W, pl.Wt, pl.R, pl.Q, pl.Wq, pl.Sg, pl.Pp, msm_partial_cap(N, P, c, Wt, occ, t),
                                        slices_in_workspace(pl, N, P, c, Wt, occ, t, 2048), slices_in_workspace(pl, N, P, c, Wt, occ, t, 4096)};
    static const char* name[10] = {"W", "Wt", "R", "Q", "Wq", "Sg", "Pp", "partial cap", "Sg in a 2048 workspace", "Sg in a 4096 workspace"};
    for (int k = 0; k < 10; k++)
      CHECK(got[k] == x[7 + k], "row %zu (N=%u P=%u c=%u Wt=%u occ=%u tuning %u/%u): %s = %llu, fixture %llu", r, N, P, c, Wt, occ, t.rounds,
            t.rounds_small, name[k], got[k], x[7 + k]);
    // the helpers the plan is built from, and the sizes derived from them
    CHECK(pl.Pp == msm_padded_batch(P) && pl.W == msm_windows(c), "row %zu: Pp / W disagree with msm_padded_batch / msm_windows", r);
    CHECK(msm_digit_elems(N, P, c) == (size_t)pl.W * N * pl.Pp, "row %zu: msm_digit_elems", r);
    CHECK(msm_table_elems(N, c, Wt) == msm_table_rows(N, pl.Wt) << (c - 1), "row %zu: msm_table_elems", r);
    CHECK(msm_table_rows(N, pl.Wt) % 64 == 0 && msm_table_rows(N, pl.Wt) >= (size_t)N * pl.Wt && msm_table_rows(N, pl.Wt) < (size_t)N * pl.Wt + 64,
          "row %zu: msm_table_rows", r);
    CHECK(pl.partial_elems(P) <= msm_partial_cap(N, P, c, Wt, occ, t), "row %zu: a workspace sized for P does not hold the plan at P", r);
  }
  // padding rule at the wave boundary
  CHECK(msm_padded_batch(0) == 0 && msm_padded_batch(1) == 1 && msm_padded_batch(63) == 63 && msm_padded_batch(64) == 64 &&
            msm_padded_batch(65) == 128 && msm_padded_batch(4096) == 4096 && msm_padded_batch(4097) == 4160,
        "msm_padded_batch");
  CHECK(msm_table_rows(0, 1) == 0 && msm_table_rows(1, 1) == 64 && msm_table_rows(1, 32) == 64 && msm_table_rows(2, 32) == 64 &&
            msm_table_rows(65, 1) == 128 && msm_table_rows(3, 29) == 128,
        "msm_table_rows");
  // the two variables: SPP_MSM_WAVES accepted in 1..16, else 4; SPP_MSM_WAVES_SMALL in 1..64, else 2
  struct { const char* s; uint32_t want; } w[] = {{nullptr, 4}, {"0", 4}, {"17", 4}, {"16", 16}, {"abc", 4}, {"1", 1}},
                                            ws[] = {{nullptr, 2}, {"0", 2}, {"65", 2}, {"64", 64}, {"1", 1}};
  for (auto& k : w) CHECK(msm_tuning_from_env(k.s, nullptr).rounds == k.want, "SPP_MSM_WAVES=%s -> %u", k.s ? k.s : "(unset)", msm_tuning_from_env(k.s, nullptr).rounds);
  for (auto& k : ws) CHECK(msm_tuning_from_env(nullptr, k.s).rounds_small == k.want, "SPP_MSM_WAVES_SMALL=%s -> %u", k.s ? k.s : "(unset)", msm_tuning_from_env(nullptr, k.s).rounds_small);
  CHECK(msm_tuning_from_env("16", "64").rounds == 16 && msm_tuning_from_env("16", "64").rounds_small == 64, "both variables");
  CHECK(MsmTuning{}.rounds == 4 && MsmTuning{}.rounds_small == 2, "defaults");
  if (bad) { printf("FAILED %d checks\n", bad); return 1; }
  printf("OK msm_plan %zu rows\n", nrows);
  return 0;
}
