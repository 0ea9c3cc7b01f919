"""The C++ drop-in headers (blockcg_amd/include/blockcg/*.hpp) with the reference's names.

CPU: they compile with a plain host compiler against the C ABI, and their std::rand()-based setRandom
draws exactly the reference's values (so srand(k) reproduces the reference's lattices and sources).
GPU: this repository's drivers on the headers (n-D lattices, any width, half-volume form; a benchmark.cpp-shaped driver) and
the reference's own unmodified drivers and solver templates pass."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INC = os.path.join(ROOT, "blockcg_amd", "include")
LIBDIR = os.path.join(ROOT, "blockcg_amd", "_build")
OUT = os.path.join(ROOT, "examples", "_build")


def _compile(src, exe, link=True):
    os.makedirs(OUT, exist_ok=True)
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I", INC, src, "-o", os.path.join(OUT, exe)]
    if link:
        cmd += ["-L", LIBDIR, "-lblockcg_hip", f"-Wl,-rpath,{LIBDIR}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return os.path.join(OUT, exe)


@pytest.fixture(scope="module")
def built():
    import blockcg_amd
    if not os.path.exists(blockcg_amd.LIB_PATH):
        blockcg_amd.build()
    return {"test": _compile(os.path.join(ROOT, "examples", "nd_lattice_solve.cpp"), "nd_lattice_solve"),
            "bench": _compile(os.path.join(ROOT, "examples", "solver_comparison.cpp"), "solver_comparison")}


def test_headers_compile_with_host_compiler(built):
    assert os.path.exists(built["test"]) and os.path.exists(built["bench"])


def test_setrandom_reproduces_reference_draws():
    """The drop-in headers draw the reference's std::rand() sequence: against the reference's draws stored in
    tests/golden/extra/ref1d_v16_setrandom.npz (and, where oracle/_ref is built, against the live reference too)."""
    import oracle
    exe = _compile(os.path.join(ROOT, "tests", "cpp", "random_probe.cpp"), "random_probe", link=False)
    V = 16
    raw = np.frombuffer(subprocess.run([exe, "5", str(V)], capture_output=True).stdout, dtype=np.float64)
    U = raw[:V * 18].view(np.complex128).reshape(V, 1, 3, 3)
    B = raw[V * 18:].view(np.complex128).reshape(V, 4, 3)
    g = np.load(os.path.join(ROOT, "tests", "golden", "extra", "ref1d_v16_setrandom.npz"))
    Uref, Bref = g["U"], g["B"]         # srand(5); dirac_op D(V, mass); rand() state continues into B.setRandom()
    if oracle.ref_available():
        R = oracle.Reference()
        assert np.array_equal(R.make_dirac_1d(V, 0.1, 5), Uref) and np.array_equal(R.field_random(4, V), Bref)
    assert np.array_equal(U, Uref)
    assert np.array_equal(B, Bref)


@pytest.mark.gpu
def test_nd_lattices_through_the_headers(built):
    """examples/nd_lattice_solve.cpp: what the headers add to the reference's interface -- 4-D and 3-D lattices, widths 16, 5
    and 7, the half-volume form, host element access -- each solve to the reference's acceptance criterion (true residual
    < 2 eps for every shift and right-hand side, recomputed with the operator).  The reference's own 1-D test configuration
    is run by the reference's own files (test_unmodified_reference_unit_tests_pass_on_the_gpu, the solver-templates probe)."""
    r = subprocess.run([built["test"]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("passed") == 5 and "FAILED" not in r.stdout, r.stdout
    assert "N_rhs=5" in r.stdout and "N_rhs=7" in r.stdout and "two half-volume solves" in r.stdout


@pytest.mark.gpu
def test_benchmark_driver_matches_reference_run(built):
    """`./benchmark 100 0.1 1e-10` of the unmodified reference (built here from /root/reference) printed
      SCG residuals 9.834652e-11 ..., SBCGrQ residuals 6.416677e-11 ..., SCG_iterations 2142, SBCGrQ_iterations 360.
    The driver built on the drop-in headers draws the same lattice and sources from std::rand() (the headers keep the
    GPU runtime off the caller's rand() sequence), so it must reproduce that run up to rounding: identical block
    iteration count, SCG within one iteration per column, residuals of the same size; and two runs must agree bitwise."""
    outs = []
    for _ in range(2):
        r = subprocess.run([built["bench"], "100", "0.1", "1e-10"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    out = outs[0]
    assert int(re.search(r"SBCGrQ_iterations:\s+(\d+)", out).group(1)) == 360
    assert abs(int(re.search(r"SCG_iterations:\s+(\d+)", out).group(1)) - 2142) <= 12
    res = [float(x) for x in re.search(r"SBCGrQ residuals:\s+(.*)", out).group(1).split()]
    ref = [6.416677e-11, 6.416697e-11, 6.416718e-11, 6.416649e-11, 6.414947e-11, 6.399223e-11, 6.245456e-11, 7.270243e-12,
           2.186446e-15]
    assert len(res) == 9 and np.allclose(res[:8], ref[:8], rtol=0.15)
    res_scg = [float(x) for x in re.search(r"SCG residuals:\s+(.*)", out).group(1).split()]
    ref_scg = [9.834652e-11, 9.834652e-11, 9.834590e-11, 9.834536e-11, 9.823971e-11, 9.728676e-11, 8.827295e-11]
    assert len(res_scg) == 9 and np.allclose(res_scg[:7], ref_scg, rtol=0.05)


# ---- the reference's UNMODIFIED drivers (north_star: "drops in for benchmark.cpp") ---------------------------------
REF = "/root/reference"
DROPIN = {k: os.path.join(ROOT, "oracle", "_ref", k) for k in ("dropin_benchmark", "dropin_tests", "dropin_solver_templates")}


def test_unmodified_reference_drivers_compile_against_dropin_headers():
    """/root/reference/benchmark.cpp and /root/reference/test/{main,solvers}.cpp, compiled WHERE THEY LIE with only the
    drop-in headers on the include path (oracle/Makefile, target `dropin`): nothing of the reference's inc/ is used and
    nothing is copied.  Covers benchmark.cpp:100 (diagonal().real().array() / ... .maxCoeff())."""
    if not os.path.isdir(os.path.join(REF, "inc")):
        pytest.skip("/root/reference is not present on this machine")
    import blockcg_amd
    if not os.path.exists(blockcg_amd.LIB_PATH):
        blockcg_amd.build()
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "-j2", "dropin"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert all(os.path.exists(p) for p in DROPIN.values())
    # the include path really has no reference header on it
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    rule = mk[mk.index("_ref/dropin_benchmark:"):mk.index("clean:")]
    # (the one reference header that IS read is the solver templates' own file, named explicitly: the probe pre-defines the
    #  guards of the reference's fields.hpp / dirac_op.hpp, so those two resolve to the drop-in types)
    assert "-I$(REFERENCE)/inc" not in rule and rule.count("$(REFERENCE)/inc/") == 2 and "$(REFERENCE)/inc/block_solvers.hpp" in rule


def test_eigen_style_residual_expressions():
    """The expression chains of benchmark.cpp:100-101 and inc/block_solvers.hpp:20,42,62,83 on the drop-in matrix type."""
    exe = _compile(os.path.join(ROOT, "tests", "cpp", "expr_probe.cpp"), "expr_probe", link=False)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_unmodified_reference_benchmark_runs_on_the_gpu():
    """`./benchmark 100 0.1 1e-10` of the unmodified reference driver over the drop-in headers reproduces the CPU
    reference's run (SCG_iterations 2142, SBCGrQ_iterations 360; see test_benchmark_driver_matches_reference_run)."""
    if not os.path.exists(DROPIN["dropin_benchmark"]):
        pytest.skip("oracle/_ref/dropin_benchmark was not built (needs /root/reference at build time)")
    r = subprocess.run([DROPIN["dropin_benchmark"], "100", "0.1", "1e-10"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert "# Benchmark of SBCGrQ vs SCG solver: V = 100, N_rhs = 12" in out
    assert int(re.search(r"SBCGrQ_iterations:\s+(\d+)", out).group(1)) == 360
    assert abs(int(re.search(r"SCG_iterations:\s+(\d+)", out).group(1)) - 2142) <= 12
    res = [float(x) for x in re.search(r"SBCGrQ residuals:\s+(.*)", out).group(1).split()]
    ref = [6.416677e-11, 6.416697e-11, 6.416718e-11, 6.416649e-11, 6.414947e-11, 6.399223e-11, 6.245456e-11, 7.270243e-12]
    assert len(res) == 9 and np.allclose(res[:8], ref, rtol=0.15)


@pytest.mark.gpu
def test_unmodified_reference_unit_tests_pass_on_the_gpu():
    """The reference's own Catch suite (test/solvers.cpp: CG, SCG, BCG, BCGrQ, SBCGrQ at V=128, true residual < 2 eps)
    linked against the drop-in headers and libblockcg_hip.so."""
    if not os.path.exists(DROPIN["dropin_tests"]):
        pytest.skip("oracle/_ref/dropin_tests was not built (needs /root/reference at build time)")
    r = subprocess.run([DROPIN["dropin_tests"]], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert re.search(r"All tests passed \(\d+ assertions? in \d+ test cases?\)", r.stdout), r.stdout[-2000:]


@pytest.mark.gpu
def test_reference_solver_templates_run_over_the_dropin_types():
    """The reference's OWN solver templates (inc/block_solvers.hpp: SBCGrQ, BCGrQ, BCG -- unmodified, compiled where they lie)
    instantiated over the drop-in block_fermion_field / block_matrix / dirac_op: every field primitive they call is a C-ABI
    call, every m x m expression (fullPivLu().solve, rowwise().norm().array(), Eigen::Array, llt) the drop-in matrix type.
    What a user solver written in the reference's style gets: the reference's test configuration converges in its 41-44
    iterations to the reference's acceptance criterion and agrees with the library's own solver."""
    if not os.path.exists(DROPIN["dropin_solver_templates"]):
        pytest.skip("oracle/_ref/dropin_solver_templates was not built (needs /root/reference at build time)")
    r = subprocess.run([DROPIN["dropin_solver_templates"]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(" ok") == 3 and "FAILED" not in r.stdout, r.stdout


# ---- native multi-GPU driver (examples/multi_gpu_solver.cpp: drop-in headers + libblockcg_rccl.so, no Python) --------
def _build_multi_gpu_driver(transport="blockcg_rccl"):
    """transport = "blockcg_rccl_mock": the same driver linked against the test-only twin of the transport (several ranks
    on one GPU)."""
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "multi_gpu_solver" + ("_mock" if transport.endswith("mock") else ""))
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I", INC, os.path.join(ROOT, "examples", "multi_gpu_solver.cpp"),
           "-o", exe, "-L", LIBDIR, f"-l{transport}", "-lblockcg_hip", f"-Wl,-rpath,{LIBDIR}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_multi_gpu_driver_builds():
    import blockcg_amd
    blockcg_amd.build()  # libblockcg_hip.so and libblockcg_rccl.so
    assert os.path.exists(_build_multi_gpu_driver())


@pytest.mark.gpu
def test_multi_gpu_driver_world_of_one(tmp_path):
    """The C++ multi-process driver with one rank: RCCL communicator of one, (1,1,1,1) grid, capacity ring on and off."""
    exe = _build_multi_gpu_driver()
    for ring in ("0", "4"):
        idfile = str(tmp_path / f"id{ring}")
        env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
        r = subprocess.run([exe, idfile, "16", "8", "8", "16", "1", "1", "1", "1", "0.3", "1e-9", ring], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "SBCGrQ_iterations" in r.stdout
        res = [float(x) for x in re.search(r"SBCGrQ residuals:\s+(.*)", r.stdout).group(1).split()]
        assert len(res) == 4 and max(res) < 2e-9
        assert not os.path.exists(idfile)  # the rendezvous file is single-use: rank 0 removed it


@pytest.mark.gpu
def test_multi_gpu_driver_two_ranks_same_idfile_twice(tmp_path):
    """tools/launch_ranks.sh + the C++ driver with TWO ranks (both on GPU 0, over the host-staged stand-in for RCCL), run
    twice with the SAME rendezvous path, the second time with a stale id file of a dead launch planted there: every launch
    has its own run token, so the ranks of launch 2 cannot pick up an old id (they would wait for ever in the
    communicator's initialisation), and each launch removes its own file."""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "blockcg_amd", "csrc"), "-s", "mock"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    exe = _build_multi_gpu_driver("blockcg_rccl_mock")
    idfile = str(tmp_path / "bcg.id")
    env = dict(os.environ, BCG_LOCAL_RANK_OVERRIDE="0", BCG_HOP_BLOCKS="8", BCG_HOP_PATCH="16,2,2")
    iters = []
    for launch in range(2):
        if launch == 1:
            with open(idfile, "wb") as f:
                f.write(b"bcg_mock_stale_id".ljust(128, b"\0"))
        r = subprocess.run(["bash", os.path.join(ROOT, "tools", "launch_ranks.sh"), "2", exe, idfile, "32", "4", "4", "8",
                            "1", "1", "1", "2", "0.3", "1e-9"], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        res = [float(x) for x in re.search(r"SBCGrQ residuals:\s+(.*)", r.stdout).group(1).split()]
        assert len(res) == 4 and max(res) < 2e-9
        iters.append(int(re.search(r"SBCGrQ_iterations:\s+(\d+)", r.stdout).group(1)))
        left = [f for f in os.listdir(tmp_path) if f.startswith("bcg.id.")]
        assert not left, left
    assert iters[0] == iters[1]
    import glob
    import shutil
    for d in glob.glob("/dev/shm/bcg_mock_*"):
        shutil.rmtree(d, ignore_errors=True)


@pytest.mark.gpu
def test_multi_gpu_driver_half_volume_two_ranks(tmp_path):
    """The C++ driver's half-volume option on a lattice divided over two ranks (x1), x3 whole and swept in chunks of five
    slices: blockcg::SBCGrQ_half_volume through the headers, half ghost faces and the overlapped exchanges through
    libblockcg_rccl's split form (over the stand-in), residuals by the full-volume operator (benchmark.cpp:93-103)."""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "blockcg_amd", "csrc"), "-s", "mock"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    exe = _build_multi_gpu_driver("blockcg_rccl_mock")
    env = dict(os.environ, BCG_LOCAL_RANK_OVERRIDE="0", BCG_HOP_BLOCKS="32", BCG_HOP_PATCH="16,2,2", BCG_HALF_CHUNK="5")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "launch_ranks.sh"), "2", exe, str(tmp_path / "bcg.id"), "64", "16", "8",
                        "12", "1", "2", "1", "1", "0.3", "1e-9", "0", "1"], env=env, capture_output=True, text=True, timeout=300)
    import glob
    import shutil
    for d in glob.glob("/dev/shm/bcg_mock_*"):
        shutil.rmtree(d, ignore_errors=True)
    assert r.returncode == 0, r.stdout + r.stderr
    res = [float(x) for x in re.search(r"SBCGrQ residuals:\s+(.*)", r.stdout).group(1).split()]
    assert len(res) == 4 and max(res) < 2e-9


@pytest.mark.gpu
def test_half_volume_solve_through_the_headers():
    """blockcg::SBCGrQ_half_volume (two solves on half fields, one per site parity) passes the reference's acceptance test
    evaluated with the full-volume operator."""
    exe = _compile(os.path.join(ROOT, "tests", "cpp", "half_volume_probe.cpp"), "half_volume_probe")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "HALF_VOLUME_OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_field_multiplier_overloads_on_the_gpu():
    """Every (double | N x N) multiplier combination of add / rescale_add (inc/fields.hpp:69-90) and a write through
    operator[] (:37) on the drop-in field type, against the same expressions evaluated on the host site by site."""
    exe = _compile(os.path.join(ROOT, "tests", "cpp", "overload_probe.cpp"), "overload_probe")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OVERLOADS_OK" in r.stdout, r.stdout + r.stderr
