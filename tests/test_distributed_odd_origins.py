"""Divided lattices whose ranks start at ODD coordinates.

Every kernel that needs the global parity of a site adds the rank's origin to the local coordinate: the staggered phase
eta_mu(x) = (-1)^(x_0 + ... + x_{mu-1}) of the stencil kernels (og0, og1, og2), of both forms of the covariant shift sum and
of the force kernel; the parity filter of the wall sources; the noise generator's global site; the momentum phases of
slice_gram and basis_slice_dot and their `origin + t` slice folds; the index_of[t - origin] maps of basis_slice_axpy and
basis_slice_rotate.  An origin is coords * L_local, and every other multi-rank test divides its lattice into even local
extents, so there a kernel that dropped an origin term, or added the wrong direction's, would pass.  Here a divided
direction has local extent 3.

What an odd origin can reach is limited (tests/test_odd_origins_plans_cpu.py holds the planner to it): half fields are
refused at an odd local extent, so full fields only; an odd local L0 takes the general stencil kernel; an odd local L1 or L2
takes the row form k_hop4 in every tile class and window; the column sweep k_hop4c and the bundle sweep k_hop4b are never
planned at an odd origin.

1. Operator, Gram matrix and solve: a case is one process of tests/dist_threads_worker.py (ranks as threads over the native
   transport's stand-in in its synchronous mode, set up as in test_distributed_default_tuning.py).  Every rank checks the
   operator (< 2e-13), the all-reduced Gram matrix (< 1e-13) and four fixed iterations of SBCGrQ with three shifts
   (coefficients < 1e-10, solutions < 1e-11) of its sub-lattice against the CPU oracle on the whole lattice.  The miniature
   tuning of the other multi-rank tests (BCG_HOP_PATCH = one tile x 2 x 2, 32 blocks), once the shipped one.
2. The site-parity kernels outside the solver: the gloo workers of the test_*_distributed.py files on lattices with local
   extent 3 in the divided directions.  Their half-field parts run only where every local extent is even, so not here.

Shown once on a scratch copy: with the origin terms taken out of k_hop_generic, k_hop4 and
k_shift_generic every stencil case but the og3 one fails its operator assertion on the ranks
test_odd_origins_plans_cpu.py names (and, through the ghost faces of the second application of D, on their neighbours),
and the shift_sum and force cases fail."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from test_distributed_default_tuning import TUNING_PREFIXES, _forms
from test_distributed_gpu import _mock_transport, _sweep_mock_files

pytestmark = pytest.mark.gpu

WHOLE, SPLIT = (0,), (1,)
STENCIL_CASES = [
    # global dims,      grid,         m,  ring, overlap settings, shipped tuning
    ([6, 4, 4, 4], [2, 1, 1, 1], 5, 0, SPLIT, False),           # og0 = 3: eta_1, eta_2, eta_3 flip on rank 1; general stencil, generic rows
    ([6, 4, 4, 4], [2, 1, 1, 1], 16, 0, WHOLE, False),          # the same with MFMA row kernels over the general stencil
    ([6, 6, 4, 4], [2, 2, 1, 1], 5, 0, SPLIT, False),           # four ranks, og0 and og1 odd together (sum even, eta_1 still flips)
    ([16, 6, 4, 4], [1, 2, 1, 1], 16, 0, WHOLE + SPLIT, False),  # og1 = 3 in k_hop4: whole launch, then interior + boundary list; fused Gram
    ([16, 4, 6, 4], [1, 1, 2, 1], 16, 0, SPLIT, False),         # og2 = 3: eta_3 alone flips
    ([16, 4, 4, 6], [1, 1, 1, 2], 16, 0, SPLIT, False),         # og3 = 3: must change nothing in eta; generator and ghost layout at odd L3
    ([16, 6, 6, 4], [1, 2, 2, 1], 16, 0, SPLIT, False),         # four ranks with origins (0,3,.), (3,0,.), (3,3,.)
    ([32, 6, 4, 4], [1, 2, 1, 1], 8, 0, SPLIT, False),          # m = 8 row form, Gram declined
    ([8, 4, 6, 4], [1, 1, 2, 1], 32, 0, SPLIT, False),          # m = 32
    ([16, 6, 4, 12], [1, 2, 1, 1], 16, 12, WHOLE, False),       # k_hop4 with ring addressing at og1 = 3
    ([16, 9, 4, 4], [1, 3, 1, 1], 16, 0, SPLIT, False),         # three ranks wide: origins 0, 3, 6; the + and - neighbours are different peers
    ([16, 6, 4, 4], [1, 2, 1, 1], 16, 0, SPLIT, True),          # shipped tuning: every BCG_HOP_*, BCG_ROW_*, BCG_RING_* removed from the child
]
STENCIL_PARAMS = [pytest.param(d, g, m, r, o, s, id=f"{'x'.join(map(str, d))}-grid{'x'.join(map(str, g))}-m{m}-ring{r}-overlap{o}"
                               + ("-shipped" if s else ""))
                  for d, g, m, r, os_, s in STENCIL_CASES for o in os_]


def _child_env(dims, grid, m, ring, overlap, shipped):
    env = {k: v for k, v in os.environ.items() if not k.startswith(TUNING_PREFIXES)}
    env.update(BCG_TEST_DIMS=",".join(map(str, dims)), BCG_TEST_GRID=",".join(map(str, grid)), BCG_TEST_M=str(m),
               BCG_TEST_RING=str(ring), BCG_TEST_OVERLAP=str(overlap), BCG_TEST_JOIN_TIMEOUT="240", OMP_NUM_THREADS="1",
               BCG_MOCK_SYNC="1", BCG_RCCL_LIB=_mock_transport())
    if not shipped:  # the miniature the other multi-rank tests pin
        env.update(BCG_HOP_PATCH=f"{4 * (64 // m) if m in (8, 16, 32) else 16},2,2", BCG_HOP_BLOCKS="32")
    return env


def test_child_environment(monkeypatch):
    """The miniature tuning replaces whatever the caller's environment holds; the shipped-tuning case carries none."""
    for k in ("BCG_HOP_PATCH", "BCG_HOP_BLOCKS", "BCG_HOP_BLOCKS_OVERLAP", "BCG_HOP_BUNDLE", "BCG_ROW_BATCHED", "BCG_RING_CHUNK"):
        monkeypatch.setenv(k, "1")
    env = _child_env([16, 6, 4, 4], [1, 2, 1, 1], 16, 0, 1, True)
    assert not [k for k in env if k.startswith(TUNING_PREFIXES)]
    env = _child_env([32, 6, 4, 4], [1, 2, 1, 1], 8, 0, 1, False)
    assert {k: v for k, v in env.items() if k.startswith(TUNING_PREFIXES)} == {"BCG_HOP_PATCH": "32,2,2", "BCG_HOP_BLOCKS": "32"}
    assert env["BCG_MOCK_SYNC"] == "1" and env["OMP_NUM_THREADS"] == "1" and env["BCG_TEST_JOIN_TIMEOUT"] == "240"


@pytest.mark.parametrize("dims,grid,m,ring,overlap,shipped", STENCIL_PARAMS)
def test_operator_gram_and_solve_at_odd_origins(dims, grid, m, ring, overlap, shipped):
    """Operator, Gram matrix and fixed-work solve of every rank against the whole-lattice oracle (the worker's assertions),
    and the stencil forms that ran, from the profile's stencil_form_* counters rank by rank: the row form k_hop4 alone where
    the local L0 is a multiple of the tile, no specialised form at all where it is odd."""
    world = 1
    for g in grid:
        world *= g
    L = [d // g for d, g in zip(dims, grid)]
    assert any(c * l % 2 for l, g in zip(L, grid) for c in range(g)), "no rank of this case starts at an odd coordinate"
    env = _child_env(dims, grid, m, ring, overlap, shipped)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dist_threads_worker.py")], env=env, capture_output=True,
                         text=True, timeout=300)
    _sweep_mock_files()
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-6000:]
    assert f"DIST_THREADS_OK {world} " in out.stdout, out.stdout[-3000:]
    forms = _forms(out.stdout, world)
    print(next(ln for ln in out.stdout.splitlines() if ln.startswith("DIST_THREADS_OK"))[:200])
    tiled = m in (8, 16, 32) and L[0] % (4 * (64 // m)) == 0
    for rank, f in enumerate(forms):
        if tiled:
            assert f.get("k_hop4", 0) > 0 and set(f) == {"k_hop4"}, (rank, f)
        else:  # the general kernel is no planned form: nothing is counted
            assert not f, (rank, f)


def _launch(worker, world, port, ok, **env):
    env = dict(os.environ, OMP_NUM_THREADS="1", **env)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", worker)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    print(out.stdout[-1000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert ok in out.stdout


# [16,6,6,6]: local extent 3 in the divided direction; at m = 16 and 32 the shift sum takes its tile form with ghost reads (the
# worker asserts it at m = 32), so the tile kernel's p1, p2, p3 see odd og1 and og2.  [6,4,4,4]: the generic form at og0 = 3.
GRID_SETS = [
    # world, global dims, grids of one launch
    (2, [16, 6, 6, 6], "1,2,1,1;1,1,2,1;1,1,1,2"),
    (2, [6, 4, 4, 4], "2,1,1,1"),
    (4, [16, 6, 6, 6], "1,2,2,1"),
]
GRID_IDS = ["2-ranks-x1-x2-x3", "2-ranks-x0", "4-ranks-x1x2"]
WORKERS = [
    # worker,                       widths,    what it prints,       first master port
    ("dist_shift_sum_worker.py", "5,16,32", "DIST_SHIFT_SUM_OK", 29310),
    ("dist_sources_worker.py", "5,16", "DIST_SOURCES_OK", 29320),
    ("dist_slice_gram_worker.py", "5,16", "DIST_SLICE_GRAM_OK", 29330),
]


@pytest.mark.parametrize("world,dims,grids", GRID_SETS, ids=GRID_IDS)
@pytest.mark.parametrize("worker,widths,ok,port", WORKERS, ids=[w[0][5:-10] for w in WORKERS])
def test_site_parity_kernels_at_odd_origins(worker, widths, ok, port, world, dims, grids):
    """shift_sum, smear and laplacian (generic and tile form); noise, point and wall sources -- the walls also with the parity
    filter on a full field -- and slice_dot; slice_gram with momentum projection: every rank against the single-rank call on
    the whole lattice, with the workers' own tolerances."""
    _launch(worker, world, port + GRID_SETS.index((world, dims, grids)), ok, BCG_TEST_DIMS=",".join(map(str, dims)),
            BCG_TEST_GRIDS=grids, BCG_TEST_WIDTHS=widths)


FORCE_CASES = [
    # dims,          grid
    ([16, 6, 4, 4], [1, 2, 1, 1]),   # og1 = 3: eta_2, eta_3 of the outer products, the specialised stencil (k_hop4) for Y
    ([16, 4, 6, 4], [1, 1, 2, 1]),   # og2 = 3
    ([6, 4, 4, 4], [2, 1, 1, 1]),    # og0 = 3, general stencil
    ([16, 6, 6, 4], [1, 2, 2, 1]),   # 4 ranks
]


@pytest.mark.parametrize("m", [5, 16])
@pytest.mark.parametrize("dims,grid", FORCE_CASES, ids=lambda v: "x".join(map(str, v)))
def test_force_at_odd_origins(dims, grid, m):
    """Each rank's F, plain and projected, is its part of the single-rank F to 1e-13 (tests/dist_force_worker.py)."""
    world = 1
    for g in grid:
        world *= g
    _launch("dist_force_worker.py", world, 29340 + 2 * FORCE_CASES.index((dims, grid)) + (m == 16), "DIST_FORCE_OK",
            BCG_TEST_DIMS=",".join(map(str, dims)), BCG_TEST_GRID=",".join(map(str, grid)), BCG_TEST_M=str(m),
            BCG_HOP_BLOCKS="8", BCG_HOP_PATCH="16,2,2" if m == 16 else "8,2,2")


def test_basis_slice_dot_at_odd_origins():
    """V(t)^dagger b by slice with momentum projection on [16,6,6,6]: x1 divided (the phases of a spatial direction at
    og1 = 3) and x3 divided (the fold to slice origin + t = 3 + t)."""
    _launch("dist_basis_slice_worker.py", 2, 29350, "DIST_BASIS_SLICE_OK", BCG_TEST_DIMS="16,6,6,6", BCG_TEST_GRIDS="1,2,1,1;1,1,1,2")


def test_basis_slice_axpy_at_odd_origins():
    """y += w V C(t) on [16,6,6,10]: x1 divided at local extent 3, x3 divided at local extent 5, where the worker's listed
    slices 6 and 1 (which want a slice direction of 7 or more) are rank 1's local slice index_of[6 - 5] and rank 0's."""
    _launch("dist_basis_slice_axpy_worker.py", 2, 29351, "DIST_BASIS_SLICE_AXPY_OK", BCG_TEST_DIMS="16,6,6,10",
            BCG_TEST_GRIDS="1,2,1,1;1,1,1,2")


def test_laplacian_modes_at_odd_origins():
    """basis_slice_rotate and laplacian_modes on [8,6,6,8], x1 and x2 divided at local extent 3: the smallest lattice the
    worker's parameters allow (listed slices 6 and 1 in directions 0 and 3; the numpy restatement of the eigensolver
    converges in 8 outer iterations there, against 6 on [8,4,4,8])."""
    _launch("dist_laplacian_modes_worker.py", 2, 29352, "DIST_LAPLACIAN_MODES_OK", BCG_TEST_DIMS="8,6,6,8",
            BCG_TEST_GRIDS="1,2,1,1;1,1,2,1")
