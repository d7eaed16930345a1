#!/usr/bin/env python3
"""Writes tests/golden/msm_plan.json: what the MSM planner of commit 5a103d0 -- the last one before the planner moved into
csrc/msm_plan.hpp -- answers on a grid of cases.  tests/host/msm_plan_check.cpp holds the header to these rows.

    python tests/golden/make_msm_plan.py          (in a git checkout that has 5a103d0, with libspp.so and the oracle built)

The planner is not restated here: lines 40-99 of that commit's csrc/kernels_msm.hip (msm_windows, msm_plan) are taken from git
and compiled with g++ as they stand, next to a copy of its MsmPlan struct, the three lines of its ws_set (spp_prove.cpp:15-19:
the capacity of the partial-sum buffer of a workspace) and the one line of its run_msm (spp_prove.cpp:67: the trim).  That
planner read its tuning from SPP_MSM_WAVES / SPP_MSM_WAVES_SMALL into statics, so the program runs once per tuning.  The set
sizes are those of the proving keys of the two fixture circuits of tests/conftest.py (oracle setup, seeds 7 and 9), their window
bits what spp_plan_windows gives each circuit alone under the default 240 GB budget."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd"))
PARENT = "5a103d0"

DRIVER = r"""
#include <stdint.h>
#include <stddef.h>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdio>
struct MsmPlan { uint32_t W, Wt, R, Q, Wq, Sg, Pp; size_t partial_elems(uint32_t P) const { return (size_t)R * Sg * P; } };
MsmPlan msm_plan(uint32_t N, uint32_t P, uint32_t c, uint32_t Wt, uint32_t occ = 2);
#include "parent_planner.inc"
static size_t ws_cap(uint32_t N, size_t P, uint32_t c, uint32_t Wt, uint32_t occ) {   // ws_set
  const uint32_t R = msm_plan(N, (uint32_t)P, c, Wt, occ).R;
  size_t partial_cap = (size_t)256 * 4 * 8 * 64 + 65536 + (size_t)(R + 1) * (P + 64);
  for (size_t q = P; q >= 1; q /= 2)
    partial_cap = std::max(partial_cap, msm_plan(N, (uint32_t)q, c, Wt, occ).partial_elems((uint32_t)q));
  return partial_cap;
}
static uint32_t trimmed(MsmPlan pl, uint32_t P, size_t partial_cap) {                  // run_msm
  while (pl.Sg > 1 && pl.partial_elems(P) > partial_cap) pl.Sg--;
  return pl.Sg;
}
int main() {
  unsigned N, P, c, Wt, occ;
  while (scanf("%u %u %u %u %u", &N, &P, &c, &Wt, &occ) == 5) {
    const MsmPlan p = msm_plan(N, P, c, Wt, occ);
    printf("%u %u %u %u %u %u %u %zu %u %u\n", p.W, p.Wt, p.R, p.Q, p.Wq, p.Sg, p.Pp, ws_cap(N, P, c, Wt, occ),
           trimmed(p, P, ws_cap(N, 2048, c, Wt, occ)), trimmed(p, P, ws_cap(N, 4096, c, Wt, occ)));
  }
  return 0;
}
"""

BATCHES = [1, 8, 63, 64, 65, 128, 256, 257, 768, 769, 1024, 1025, 2048, 3000, 4096]
OCC = [2, 2, 2, 2, 2, 2, 1]   # A, B1, K, Z, CB, CS (G1) and B2 (G2)


def windows(c):
    return (254 + c - 1) // c


def fixture_sets(tmp):
    import spp
    from oracle import native
    lib = spp.load_library()
    rl = json.load(open(os.path.join(HERE, "rlwe_pk.json")))
    out = {}
    for name, cid, seed, aux in (("withdraw", 1, b"\x07" * 32, None), ("audit", 2, b"\x09" * 32, list(rl["a"]) + list(rl["b"]))):
        sppc, pk, vk = (os.path.join(tmp, name + e) for e in (".sppc", ".pk", ".vk"))
        spp.build_circuit(cid, sppc, aux=aux) if aux else spp.build_circuit(cid, sppc)
        native.setup(sppc, seed, pk, vk)
        sizes, bits = (ctypes.c_uint32 * 7)(), (ctypes.c_uint32 * 7)()
        assert lib.spp_pk_msm_sizes(pk.encode(), sizes) == 0
        assert lib.spp_plan_windows(ctypes.c_uint32(1), sizes, ctypes.c_double(240e9), bits) == 0
        out[name] = {"order": ["A", "B1", "K", "Z", "CB", "CS", "B2"], "sizes": list(sizes), "bits": list(bits)}
    return out


def grid(sets):
    """(N, P, c, Wt, occ, rounds, rounds_small); Wt = 1: the flat layout, Wt = windows(c): a table row per window"""
    cases = []
    for name in ("audit", "withdraw"):
        for s in range(7):
            n, c = sets[name]["sizes"][s], sets[name]["bits"][s]
            for p in BATCHES:
                cases.append((n, p, c, 1, OCC[s], 4, 2))
                cases.append((n, p, 8, windows(8), OCC[s], 4, 2))
            if s in (4, 5):   # the commitment sets as they are loaded: a row per window at their 9 bits
                for p in BATCHES:
                    cases.append((n, p, c, windows(c), OCC[s], 4, 2))
    for n in (0, 1, 3, 4, 5, 63, 64):
        for p in BATCHES:
            for occ in (1, 2):
                cases.append((n, p, 16, 1, occ, 4, 2))
                cases.append((n, p, 8, windows(8), occ, 4, 2))
    for n in (1 << 18, 1 << 19):   # where the lane-sharing branch is not taken at P = 1: the occupancy reaches Sg
        for occ in (1, 2):
            cases.append((n, 1, 8, windows(8), occ, 4, 2))
            cases.append((n, 1, 16, 1, occ, 4, 2))
    for tuning in ((1, 1), (16, 64)):
        for s in range(7):
            n, c = sets["audit"]["sizes"][s], sets["audit"]["bits"][s]
            for p in (1, 128, 256, 257, 2048, 4096):
                cases.append((n, p, c, 1, OCC[s]) + tuning)
                cases.append((n, p, 8, windows(8), OCC[s]) + tuning)
    seen, uniq = set(), []
    for k in cases:
        if k not in seen:
            seen.add(k)
            uniq.append(k)
    return uniq


def main():
    with tempfile.TemporaryDirectory() as tmp:
        sets = fixture_sets(tmp)
        src = subprocess.run(["git", "-C", ROOT, "show", PARENT + ":shielded-pool-pinocchio-solana_amd/csrc/kernels_msm.hip"],
                             check=True, capture_output=True, text=True).stdout.split("\n")
        open(os.path.join(tmp, "parent_planner.inc"), "w").write("\n".join(src[39:99]) + "\n")
        open(os.path.join(tmp, "driver.cpp"), "w").write(DRIVER)
        exe = os.path.join(tmp, "driver")
        subprocess.run(["g++", "-O2", "-std=c++17", "-I", tmp, os.path.join(tmp, "driver.cpp"), "-o", exe], check=True)
        cases = grid(sets)
        rows = []
        for tuning in sorted({k[5:] for k in cases}):
            sub = [k for k in cases if k[5:] == tuning]
            env = dict(os.environ, SPP_MSM_WAVES=str(tuning[0]), SPP_MSM_WAVES_SMALL=str(tuning[1]))
            out = subprocess.run([exe], input="".join("%d %d %d %d %d\n" % k[:5] for k in sub), env=env, check=True, capture_output=True,
                                 text=True).stdout.strip().split("\n")
            assert len(out) == len(sub)
            rows += [list(k) + [int(v) for v in line.split()] for k, line in zip(sub, out)]
    doc = {"what": "answers of the MSM planner of commit %s (make_msm_plan.py); Wt = 1 is the flat layout" % PARENT,
           "columns": ["N", "P", "c", "Wt_in", "occ", "rounds", "rounds_small", "W", "Wt", "R", "Q", "Wq", "Sg", "Pp",
                       "partial_cap_of_a_workspace_for_P", "Sg_in_a_workspace_for_2048", "Sg_in_a_workspace_for_4096"],
           "sets": sets}
    text = json.dumps(doc)[:-1] + ', "rows": [\n' + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]}\n"
    open(os.path.join(HERE, "msm_plan.json"), "w").write(text)
    print("%d rows, %d bytes" % (len(rows), len(text)))


if __name__ == "__main__":
    main()
