"""The planners of the per-slice calls (blockcg_amd/csrc/slice_plan.cpp: slice_gram_plan, basis_slice_plan,
basis_slice_axpy_plan) against the committed table of expected plans.

tests/golden/slice_plan_table.json holds, for every case of slice_plan_cases.py, every field of the plan -- momenta per
launch, groups, blocks per slice, chunk, table length and directions, or "no plan" -- that the three planners gave while each
still lived beside its kernels, recorded from those, not from slice_plan.cpp.  The figures that the docstrings of
tests/test_slice_gram.py, tests/test_basis_slice.py and tests/test_basis_slice_axpy.py state in prose are asserted here from
the planner, so that prose and planner cannot drift.  tests/cpp/slice_plan_probe.cpp is host code: no GPU."""
import os
import shutil
import subprocess

import pytest

import slice_plan_cases as spc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blockcg_amd", "csrc")
ZERO = (0, 0, 0, 0)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """(cases, the probe's plan of each)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the probe is compiled with the compiler that builds the library")
    out = tmp_path_factory.mktemp("slice_plan_probe")
    obj = os.path.join(ROOT, "blockcg_amd", "_build", "slice_plan.o")
    subprocess.run(["make", "-C", CSRC, "-s", "../_build/slice_plan.o"], check=True)  # (built with the library; here if it is not)
    exe = str(out / "slice_plan_probe")
    main = str(out / "slice_plan_probe.o")
    subprocess.run([hipcc, "-O1", "-std=c++17", "-Wall", "-c", os.path.join(ROOT, "tests", "cpp", "slice_plan_probe.cpp"), "-o", main],
                   check=True)
    subprocess.run([hipcc, main, obj, "-o", exe], check=True)
    cases = list(spc.cases())
    infile = out / "cases.txt"
    infile.write_text("".join(spc.line(c) + "\n" for c in cases))
    got = subprocess.run([exe, str(infile)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(got) == len(cases)
    return cases, got


def test_planners_decide_what_the_table_records(plans):
    cases, got = plans
    want = spc.load_table()
    assert len(want) == len(cases), "the table and slice_plan_cases.py list different cases"
    wrong = [(spc.label(c), g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not wrong, f"{len(wrong)} of {len(cases)} plans differ; first: {wrong[:3]}"
    # the table is not trivially one-sided: plans and refusals of every planner, both forms, every momentum count
    for kind in (spc.GRAM, spc.BASIS, spc.AXPY):
        mine = [w for c, w in zip(cases, want) if c["kind"] == kind]
        assert "no plan" in mine and any(w != "no plan" for w in mine), kind
    for needle in ("pc=1 ", "pc=2 ", "pc=4 ", "pc_mfma=1 ", "pc_mfma=2 ", "pc_mfma=4 ", "pc_generic=1 ", "pc_generic=2 ",
                   "groups=1:", "groups=0:", ";0:", ";1:", "cols=12 ", "kb=1 ", "kb=2 ", "kb=3 ", "kb=4 "):
        assert any(needle in w for w in want), needle


def _plan(plans, **want):
    cases, got = plans
    return spc.fields(got[spc.find(cases, **want)])


def _blocks(plans, **want):
    p = _plan(plans, **want)
    return int(p["nbps"]), int(p["chunk"])


@pytest.mark.parametrize("dims,m,widths,per_slice", [([16, 16, 16, 4], 16, [32, 32], {3: 192, 0: 48}),
                                                     ([16, 16, 8, 4], 32, [32], {3: 96, 0: 24})], ids=["m16", "m32"])
def test_several_blocks_per_slice_as_the_gpu_tests_say(plans, dims, m, widths, per_slice):
    """test_slice_gram_with_several_blocks_per_slice, test_basis_slice_with_several_blocks_per_slice and
    test_basis_slice_axpy_with_several_blocks_per_slice: the blocks per slice they name, chunks of 64 rows."""
    for direction, nbps in per_slice.items():
        lat = dict(dims=dims, origin=ZERO, parity=-1, dir=direction)
        for n_mom in (0, 3):
            assert _blocks(plans, kind=spc.GRAM, m=m, mfma=1, n_mom=n_mom, half=spc.HALF, **lat) == (nbps, 64)
            assert _blocks(plans, kind=spc.BASIS, widths=widths, m=m, fast=1, n_mom=n_mom, half=spc.HALF, **lat) == (nbps, 64)
        if m == 16:
            for n_slices in (2, dims[direction]):
                assert _blocks(plans, kind=spc.AXPY, n_slices=n_slices, **lat) == (nbps, 64)


@pytest.mark.parametrize("widths,m", [([32, 32, 16], 16), ([32, 16], 32)], ids=["m16", "m32"])
def test_blocks_per_slice_on_8x8x8x8(plans, widths, m):
    """test_basis_slice_on_8x8x8x8: with three momenta and with none the same 24 blocks per slice (12 for a half field along
    direction 3) and the same chunk, though the groups differ."""
    for parity, direction, nbps in ((-1, 0, 24), (-1, 3, 24), (1, 3, 12)):
        lat = dict(dims=[8, 8, 8, 8], origin=ZERO, parity=parity, dir=direction)
        with_mom = _plan(plans, kind=spc.BASIS, widths=widths, m=m, fast=1, n_mom=3, half=spc.HALF, **lat)
        without = _plan(plans, kind=spc.BASIS, widths=widths, m=m, fast=1, n_mom=0, half=spc.HALF, **lat)
        assert (int(with_mom["nbps"]), int(with_mom["chunk"])) == (int(without["nbps"]), int(without["chunk"])) == (nbps, 64)
        assert with_mom["groups"] != without["groups"]


def test_group_counts_where_the_scratch_is_short(plans):
    """test_the_group_shrinks_where_the_scratch_is_short: [2048] along direction 0, V = 2 x 32 at m = 16: two groups of 2 blocks
    without momenta, four of 1 block with one; one block per slice.  And test_more_slices_than_blocks_aimed_at: 2048 listed
    slices get one block each."""
    lat = dict(dims=[2048], origin=ZERO, parity=-1, dir=0)
    for n_mom, groups in ((0, 2), (1, 4)):
        p = _plan(plans, kind=spc.BASIS, widths=[32, 32], m=16, fast=1, n_mom=n_mom, half=spc.HALF, **lat)
        assert p["groups"].count(";") == groups and int(p["kb"]) == 4 // groups and int(p["nbps"]) == 1, p
    assert _plan(plans, kind=spc.BASIS, widths=[32, 32], m=16, fast=1, n_mom=0, half=spc.HALF // 4, **lat) is None
    halved = _plan(plans, kind=spc.BASIS, widths=[12, 12, 12], m=32, fast=1, n_mom=2, half=spc.HALF, **lat)
    assert (halved["cols"], halved["pc_generic"], halved["groups"]) == ("12", "1", "0:0:1:12:0;0:1:1:12:12;0:2:1:12:24;")
    assert _blocks(plans, kind=spc.AXPY, n_slices=2048, **lat) == (1, 16)
