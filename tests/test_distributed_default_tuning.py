"""Divided lattices under the stencil's SHIPPED tuning (HopTuning, kernels_mfma.hpp: patches of one tile x 8 x 8, 512 blocks,
the XCD patch walk with 64 tiles per class, the paced interior class, the boundary class dealt from its tile list).

Every other multi-rank GPU test pins BCG_HOP_PATCH=16,2,2 and BCG_HOP_BLOCKS to 8 or 32, and the shipped tuning otherwise runs on
one rank only (test_fullsize_parity.py), so ghost rows met the production forms nowhere: a row that crosses a 16 x 8 x 8 patch
face and takes its x1 or x2 neighbour from the ghost face, the x0 edge lanes of a tile that is not the first of its patch.
Here nothing about the tuning is set -- every BCG_HOP_*, BCG_ROW_* and BCG_RING_* variable is taken out of the child's
environment -- on the smallest local lattices that still plan the production forms (8 patches: [32,16,16,L3] at m = 16;
tests/test_default_tuning_plans_cpu.py holds the planner to that, so these cases cannot quietly turn into tests of the row form).

A case is one process of tests/dist_threads_worker.py: the ranks are threads, each with a context, a stream and the native
transport over its host-staged stand-in in the synchronous mode.  Every rank checks the operator (< 2e-13), the all-reduced
Gram matrix (< 1e-13) and four fixed iterations of SBCGrQ with three shifts (coefficients < 1e-10, solutions < 1e-11) of its
sub-lattice against the CPU oracle on the whole lattice.  This file adds which stencil forms ran, from the profile's
stencil_form_* counters over operator and solve, rank by rank -- not how often: that depends on the modes the solver asks for.

The paced launches (k_hop4c with pace = 4) cannot hang when several ranks share one GPU and a block's XCD class is not
resident: the wait in kernels_stencil.hip gives up after sync_limit ticks (HopSync::limit_ticks, 50 us) and the block goes
on unpaced."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT
from test_distributed_gpu import _mock_transport, _sweep_mock_files

pytestmark = pytest.mark.gpu

TUNING_PREFIXES = ("BCG_HOP_", "BCG_ROW_", "BCG_RING_")

WHOLE, SPLIT = (0,), (1,)
CASES = [
    # global dims,       grid,         m,  ring, overlap settings
    ([64, 16, 16, 4], [2, 1, 1, 1], 16, 0, WHOLE + SPLIT),   # x0 divided: edge lanes, U_0 ghost in tiles not first in their patch
    ([32, 32, 16, 4], [1, 2, 1, 1], 16, 0, WHOLE + SPLIT),   # x1 ghost rows across patch faces
    ([32, 16, 32, 4], [1, 1, 2, 1], 16, 0, WHOLE + SPLIT),   # x2
    ([32, 16, 16, 8], [1, 1, 1, 2], 16, 0, WHOLE + SPLIT),   # x3 divided, local L3 = 4
    ([64, 32, 16, 4], [2, 2, 1, 1], 16, 0, SPLIT),           # 4 ranks, two divided directions: corner tiles in the boundary list
    ([128, 16, 16, 4], [2, 1, 1, 1], 8, 0, WHOLE + SPLIT),   # m = 8: 32-site tiles, shifted + Gram on the column form
    ([16, 32, 16, 4], [1, 2, 1, 1], 32, 0, WHOLE + SPLIT),   # m = 32
    ([64, 16, 16, 12], [2, 1, 1, 1], 16, 12, WHOLE),         # capacity ring, serial form: ten-slice windows, ring addressing + ghosts
]
PARAMS = [pytest.param(d, g, m, r, o, id=f"{'x'.join(map(str, d))}-grid{'x'.join(map(str, g))}-m{m}-ring{r}-overlap{o}")
          for d, g, m, r, os_ in CASES for o in os_]


def _child_env(dims, grid, m, ring, overlap):
    env = {k: v for k, v in os.environ.items() if not k.startswith(TUNING_PREFIXES)}
    env.update(BCG_TEST_DIMS=",".join(map(str, dims)), BCG_TEST_GRID=",".join(map(str, grid)), BCG_TEST_M=str(m),
               BCG_TEST_RING=str(ring), BCG_TEST_OVERLAP=str(overlap), BCG_TEST_JOIN_TIMEOUT="240", OMP_NUM_THREADS="1",
               BCG_MOCK_SYNC="1", BCG_RCCL_LIB=_mock_transport())
    return env


def _forms(stdout, world):
    """{form: launches} per rank, from the worker's DIST_THREADS_OK line."""
    line = next(ln for ln in stdout.splitlines() if ln.startswith(f"DIST_THREADS_OK {world} "))
    ranks = dict(re.findall(r"rank(\d+):(\S*)", line.split(" forms ", 1)[1]))
    assert sorted(map(int, ranks)) == list(range(world)), line
    return [{k: int(v) for k, v in (kv.split("=") for kv in ranks[str(r)].split(",") if kv)} for r in range(world)]


def test_child_environment_carries_no_tuning(monkeypatch):
    """What this file is about: the child sees the library's defaults, whatever the caller's environment holds."""
    for k in ("BCG_HOP_PATCH", "BCG_HOP_BLOCKS", "BCG_HOP_BLOCKS_OVERLAP", "BCG_HOP_BUNDLE", "BCG_ROW_BATCHED", "BCG_RING_CHUNK",
              "BCG_RING_OVERLAP"):
        monkeypatch.setenv(k, "1")
    env = _child_env([64, 16, 16, 4], [2, 1, 1, 1], 16, 0, 1)
    left = [k for k in env if k.startswith(TUNING_PREFIXES)]
    assert not left, left
    assert env["BCG_MOCK_SYNC"] == "1" and env["OMP_NUM_THREADS"] == "1" and env["BCG_TEST_JOIN_TIMEOUT"] == "240"


@pytest.mark.parametrize("dims,grid,m,ring,overlap", PARAMS)
def test_divided_lattice_under_default_tuning(dims, grid, m, ring, overlap):
    """Operator, Gram matrix and fixed-work solve of every rank against the whole-lattice oracle with nothing about the
    stencil's tuning set, and the forms that ran: the bundle sweep k_hop4b for whole launches (overlap 0), the paced column
    sweep k_hop4c for the interior class and the row form k_hop4 over the boundary tile list (overlap 1), bundle and column
    windows with ring addressing in capacity mode.  (The paced launches give up waiting after 50 us -- see the module's
    docstring -- so ranks sharing the GPU cannot hang each other.)"""
    world = 1
    for g in grid:
        world *= g
    env = _child_env(dims, grid, m, ring, overlap)
    left = [k for k in env if k.startswith(TUNING_PREFIXES)]
    assert not left, left
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dist_threads_worker.py")], env=env, capture_output=True,
                         text=True, timeout=300)
    _sweep_mock_files()
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-6000:]
    assert f"DIST_THREADS_OK {world} " in out.stdout, out.stdout[-3000:]
    forms = _forms(out.stdout, world)
    print(f"{dims} grid {grid} m = {m} ring {ring} overlap {overlap}: {forms}")
    for rank, f in enumerate(forms):
        assert "general" not in f, (rank, f)
        if ring:
            assert f.get("k_hop4b", 0) > 0 and f.get("k_hop4c", 0) > 0, (rank, f)
        elif overlap:
            assert f.get("k_hop4c", 0) > 0 and f.get("k_hop4", 0) > 0, (rank, f)
        else:
            assert f.get("k_hop4b", 0) > 0, (rank, f)
