"""The stencil planner (blockcg_amd/csrc/hop_plan.cpp) for the two requests of the factored pair with phase B inside the
second factor: HOP_FACT1G (the first factor with its Gram product) and HOP_FACT2B (the fused launch).  Both are bundle plans
exactly where the factored pair's are; the fused launch asks for the sweep's LDS and 8 192 B for its two matrices, which makes
two blocks a CU's 160 KB.  And the pair planner (hop_plan_pair), which spells the requests of both uses of the pair for the
library: its plans are hop_plan's for those requests, and the pair is taken exactly when both are bundle plans.
Host code only (tests/cpp/fused_plan_probe.cpp): no GPU."""
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
def probe(tmp_path_factory):
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

    def run(what, *values):
        line = " ".join(str(int(v)) for v in values)
        return [int(v) for v in subprocess.run([exe, *what], input=line + "\n", check=True, capture_output=True, text=True).stdout.split()]
    return run


@pytest.fixture(scope="module")
def plan(probe):
    def ask(dims, mode, gram=1, m=16, tune=SMALL, bundle=1, cls=0, x3n=0, ring=0, cb=0):
        return tuple(probe([], m, *dims, *tune["patch"], tune["blocks"], bundle, cls, x3n, ring, cb, mode, gram))
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


# ---- the pair planner ------------------------------------------------------------------------------------------------------
# the four lattices of test_both_requests_are_bundle_plans, then the declined cases that mean something for a pair
PAIR_CASES = {"64^4": dict(dims=[64, 64, 64, 64], tune=DEFAULT), "16x8x8x8": dict(dims=[16, 8, 8, 8]), "32x8x8x6": dict(dims=[32, 8, 8, 6]),
              "32x4x4x3": dict(dims=[32, 4, 4, 3]), "m8": dict(dims=[16, 8, 8, 8], m=8, taken=False),
              "m32": dict(dims=[16, 8, 8, 8], m=32, taken=False), "bundle0": dict(dims=[16, 8, 8, 8], bundle=0, taken=False),
              "default-walk": dict(dims=[16, 8, 8, 8], tune=DEFAULT, taken=False)}
FIELDS = 14  # form, LDS, grid, tiles, p0, p1, p2, xcd_split, super, paced, window, stride, limit, folds (print_plan)


@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("with_phase_b", [0, 1], ids=["operator-form", "phase-B-inside"])
@pytest.mark.parametrize("case", sorted(PAIR_CASES))
def test_pair_plans_are_hop_plans_for_the_requests_as_spelled(probe, case, with_phase_b, fold):
    kw = dict(PAIR_CASES[case])
    dims, m, tune, bundle, taken = kw["dims"], kw.get("m", 16), kw.get("tune", SMALL), kw.get("bundle", 1), kw.get("taken", True)
    head = [m, *dims, *tune["patch"], tune["blocks"], bundle]
    got = probe(["pair"], *head, with_phase_b, fold)
    assert len(got) == 1 + 2 * FIELDS
    f1, f2 = got[1:1 + FIELDS], got[1 + FIELDS:]
    # whole launches over all slices, no ring, full fields; the first factor of the operator form has no Gram product and
    # is no fold target, every other launch carries its product and folds where the caller asked
    if with_phase_b:
        want1 = probe(["full"], *head, 0, 0, 0, 0, FACT1G, 1, fold)
        want2 = probe(["full"], *head, 0, 0, 0, 0, FACT2B, 1, fold)
    else:
        want1 = probe(["full"], *head, 0, 0, 0, 0, FACT1, 0, 0)
        want2 = probe(["full"], *head, 0, 0, 0, 0, FACT2, 1, fold)
    assert f1 == want1 and f2 == want2
    assert got[0] == int(f1[0] == BUNDLE and f2[0] == BUNDLE) == int(taken)
    if taken:  # the fields are live: a folded launch where asked, and the long sweep of 64^4 is the paced one
        assert f2[13] == fold and f1[13] == (fold if with_phase_b else 0)
        assert f1[9] == f2[9] == int(case == "64^4")
