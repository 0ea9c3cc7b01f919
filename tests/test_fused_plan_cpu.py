"""The stencil planner (blockcg_amd/csrc/hop_plan.cpp) for the two requests of the factored pair with phase B inside the
second factor: HOP_FACT1G (the first factor with its Gram product) and HOP_FACT2B (the fused launch).  Both are bundle plans
exactly where the factored pair's are; the fused launch asks for the sweep's LDS and 8 192 B for its two matrices, which makes
two blocks a CU's 160 KB.  Host code only (tests/cpp/fused_plan_probe.cpp): no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blockcg_amd", "csrc")
PLAIN, SHIFTED, RESID, FACT1, FACT2, FACT1G, FACT2B = range(7)
BUNDLE = 3  # HOP_FORM_BUNDLE
SWEEP_LDS = 73728
DEFAULT = dict(patch=(0, 8, 8), blocks=512)
SMALL = dict(patch=(16, 2, 2), blocks=32)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the probe is compiled with the compiler that builds the library")
    out = tmp_path_factory.mktemp("fused_plan_probe")
    subprocess.run(["make", "-C", CSRC, "-s", "../_build/hop_plan.o"], check=True)
    exe = str(out / "fused_plan_probe")
    main = str(out / "fused_plan_probe.o")  # (compiled and linked in two steps: hipcc takes every input of a .cpp line as source)
    subprocess.run([hipcc, "-O1", "-std=c++17", "-Wall", "-c", os.path.join(ROOT, "tests", "cpp", "fused_plan_probe.cpp"), "-o", main],
                   check=True)
    subprocess.run([hipcc, main, os.path.join(ROOT, "blockcg_amd", "_build", "hop_plan.o"), "-o", exe], check=True)

    def ask(dims, mode, gram=1, m=16, tune=SMALL, bundle=1, cls=0, x3n=0, ring=0, cb=0):
        line = " ".join(str(v) for v in [m, *dims, *tune["patch"], tune["blocks"], bundle, cls, x3n, ring, cb, mode, gram])
        form, lds, grid = subprocess.run([exe], input=line + "\n", check=True, capture_output=True, text=True).stdout.split()
        return int(form), int(lds), int(grid)
    return ask


@pytest.mark.parametrize("dims,tune,grid", [([64, 64, 64, 64], DEFAULT, 512), ([16, 8, 8, 8], SMALL, 32), ([32, 8, 8, 6], SMALL, 32),
                                            ([32, 4, 4, 3], SMALL, 32)])
def test_both_requests_are_bundle_plans(plan, dims, tune, grid):
    assert plan(dims, FACT1G, tune=tune) == (BUNDLE, SWEEP_LDS, grid)
    assert plan(dims, FACT2B, tune=tune) == (BUNDLE, SWEEP_LDS + 8192, grid)
    assert 2 * (SWEEP_LDS + 8192) == 160 * 1024
    # the pair's own requests are what they were
    assert plan(dims, FACT1, gram=0, tune=tune) == (BUNDLE, SWEEP_LDS, grid)
    assert plan(dims, FACT2, tune=tune) == (BUNDLE, SWEEP_LDS, grid)
    assert plan(dims, FACT1, gram=1, tune=tune)[0] == 0  # (the table's request: still declined)


@pytest.mark.parametrize("mode", [FACT1G, FACT2B])
def test_declined_elsewhere(plan, mode):
    dims = [16, 8, 8, 8]
    assert plan(dims, mode, gram=0)[0] == 0                      # always with their Gram products
    assert plan(dims, mode, m=8)[0] == 0 and plan(dims, mode, m=32)[0] == 0
    assert plan(dims, mode, x3n=6, ring=8)[0] == 0               # no ring
    assert plan([8, 8, 8, 8], mode, cb=1)[0] == 0                # no half fields
    assert plan(dims, mode, cls=1)[0] == 0                       # whole launches only
    assert plan(dims, mode, bundle=0)[0] == 0                    # the bundle sweep only: never a column or row plan
    assert plan([16, 8, 8, 8], mode, tune=DEFAULT)[0] == 0       # a lattice the default walk does not tile
