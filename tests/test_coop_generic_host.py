"""The cooperative solver's plan for programs with the generic solver instructions, checked without a GPU: tests/host/
coop_generic_check.cpp builds the plan with csrc/coop_plan.hpp (the header the library's loader uses), executes its items on the CPU
in an order that exposes a missed dependency (tracks and the rows of a level in reverse), and compares every wire with the program
run instruction by instruction; it also refuses a level that reads what the same or a later level of its item writes."""
import os
import subprocess
import pytest
from conftest import GOLDEN

import synth_circuits as S
import synth_generic as SG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "csrc")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("coop_generic") / "coop_generic_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tests", "host", "coop_generic_check.cpp"),
                    os.path.join(CSRC, "circuit.cpp"), "-o", exe], check=True)

    def run(sppc, *args):
        out = subprocess.run([exe, sppc] + list(args), capture_output=True, text=True)
        assert out.returncode == 0, (out.stdout, out.stderr)
        f = out.stdout.split()
        return {f[i]: int(f[i + 1]) for i in range(0, len(f), 2)}
    return run


def test_reference_system_plan_keeps_every_dependency(check, tmp_path):
    """the solved container of the reference's own R1CS: all 12 131 OP_SOLVE_ROW rows land in level items, 752 of them divide at run
    time, the histogram is an item of its own, and the items executed out of order give the program's wires"""
    from spp import acir, ccs
    program = acir.load_program(os.path.join(GOLDEN, "reference_withdraw_acir.json"))
    c = ccs.load_ccs(os.path.join(GOLDEN, "reference_withdraw.ccs"))
    sppc = str(tmp_path / "solved.sppc")
    assert ccs.to_sppc_solved(ccs.decode_system(c), c, program, sppc)[0] == 12452
    for args in ((), ("no_level_stream",)):
        st = check(sppc, *args)
        assert st["generic_ops"] == 1 and st["generic_rows"] == 12131 and st["generic_divs"] == 752, st
        assert st["mismatches"] == 0 and st["items_countn"] == 1 and st["items_par"] >= 1 and st["tracks"] >= 1, st
        if args:
            assert st["items_level_stream"] == 0 and st["items_levels"] > 0, st
        else:
            assert st["items_level_stream"] > 0, st


@pytest.mark.parametrize("name", sorted(SG.CASES))
def test_synthetic_generic_plans_keep_every_dependency(check, tmp_path, name):
    g = SG.CASES[name]()
    sppc = str(tmp_path / (name + ".sppc"))
    S.write_sppc(g.desc, sppc)
    for args in ((), ("no_level_stream",)):
        st = check(sppc, *args)
        assert st["mismatches"] == 0, st
        assert st["generic_rows"] == g.expect["generic_rows"] and st["generic_divs"] == g.expect["generic_divs"], st
        assert st["items_levels"] + st["items_level_stream"] > 0, st
    if name == "tracks":
        assert st["tracks"] >= 2, st
    if name == "longrow":
        assert check(sppc)["items_levels"] == 1


@pytest.mark.parametrize("name", ["chain40", "tracks32", "bigrow", "ops4", "div63"])
def test_native_plans_through_the_same_header(check, tmp_path, name):
    """circuits without a generic instruction go through the same planner: no generic rows, the same wires"""
    g = S.CASES[name]()
    sppc = str(tmp_path / (name + ".sppc"))
    S.write_sppc(g.desc, sppc)
    st = check(sppc)
    assert st["generic_ops"] == 0 and st["generic_rows"] == 0 and st["generic_divs"] == 0 and st["mismatches"] == 0, st
    model = S.plan_model(g.desc)
    assert (st["items_par"], st["items_levels"], st["items_level_stream"], st["stream_chunks"]) == \
        (model["items_par"], model["items_levels"], model["items_level_stream"], model["stream_chunks"]), (st, model)


def test_model_matches_the_oracle_solver_on_a_native_circuit():
    """the big-integer model of synth_generic against oracle.circuit.solve where both know the instructions (OP_SOLVE_C, OP_MASK)"""
    from oracle import circuit as C
    g = S.CASES["chain40"]()
    row = g.inputs(3)
    want = C.solve(S._as_circuit(g.desc), row, lambda w: 12345, rs=(5, 6))
    assert SG.model(g.desc, row, challenge=12345, rs=(5, 6)) == want
