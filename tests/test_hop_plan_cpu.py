"""The stencil planner (blockcg_amd/csrc/hop_plan.cpp) against the committed table of expected plans.

tests/golden/hop_plan_table.json holds, for every case of hop_plan_cases.py, what the launcher decided before the planner
existed (kernel instantiation, LDS bytes, pacing window, fold, grid, walk, window -- or "declined"), recorded from that
launcher, not from the planner.  The one kind of request where the planner answers differently on purpose is listed under
"unreached": a fused Gram product asked of a form that has none, which the old launcher dropped silently and the planner
declines; no caller makes such a request.  tests/cpp/hop_plan_probe.cpp is host code: no GPU."""
import os
import shutil
import subprocess

import pytest

import hop_plan_cases as hpc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blockcg_amd", "csrc")

@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the probe is compiled with the compiler that builds the library")
    out = tmp_path_factory.mktemp("hop_plan_probe")
    obj = os.path.join(ROOT, "blockcg_amd", "_build", "hop_plan.o")
    subprocess.run(["make", "-C", CSRC, "-s", "../_build/hop_plan.o"], check=True)  # (built with the library; here if it is not)
    exe = str(out / "hop_plan_probe")
    main = str(out / "hop_plan_probe.o")
    subprocess.run([hipcc, "-O1", "-std=c++17", "-Wall", "-c", os.path.join(ROOT, "tests", "cpp", "hop_plan_probe.cpp"), "-o", main],
                   check=True)
    subprocess.run([hipcc, main, obj, "-o", exe], check=True)
    return exe, out


def test_planner_decides_what_the_table_records(probe):
    exe, out = probe
    cases = list(hpc.cases())
    want, _ = hpc.load_table()
    assert len(want) == len(cases), "the table and hop_plan_cases.py list different cases"
    infile = out / "cases.txt"
    infile.write_text("".join(hpc.line(c) + "\n" for c in cases))
    got = subprocess.run([exe, str(infile)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(got) == len(cases)
    wrong = [(hpc.label(c), g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not wrong, f"{len(wrong)} of {len(cases)} plans differ; first: {wrong[:3]}"
    # the table is not trivially "declined": every form, the register-capped interior entry, pacing and the fold occur
    for needle in ("k_hop4<", "k_hop4c<", "k_hop4c_interior<", "k_hop4b<", ",false,true> ", "HOP_RESID", "HOP_FACT1", "HOP_FACT2",
                   "fold=1", "pace=4", "pace=1", "pace=0"):
        assert any(needle in w for w in want), needle


def test_unreached_requests_are_gram_products_and_declined():
    cases = list(hpc.cases())
    want, unreached = hpc.load_table()
    assert unreached
    for i in unreached:
        assert cases[i]["gram"] == 1 and want[i] == "declined", hpc.label(cases[i])
