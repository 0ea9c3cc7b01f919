"""Stout smearing and the plaquette on a lattice divided over ranks (tests/dist_stout_smear_worker.py): 2 and 4 gloo ranks
share the one GPU.  [8,4,4,8] on the grids (2,1,1,1), (1,1,1,2) and (2,2,1,1); the last has the link U_nu(x-nu+mu) across two
divided directions at once, which reaches a rank only inside the backward staple its neighbour computes.  Each rank's result
equals its local rows of the single-rank result to 1e-13 (spatial weights and the full asymmetric table, 1 and 3 steps); the
plaquette equals the single-rank one and is bitwise equal across ranks; a smeared container used at once in the Laplacian has
its stale ghost refreshed; a context without a bcg_comm returns BCG_ERR_COMM.  One launch per world size."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

DIMS = [8, 4, 4, 8]
CASES = [(2, "2,1,1,1;1,1,1,2"), (4, "2,2,1,1")]


@pytest.mark.parametrize("world,grids", CASES, ids=["2-ranks", "4-ranks"])
def test_stout_smear_on_a_divided_lattice(world, grids):
    env = dict(os.environ, BCG_TEST_DIMS=",".join(map(str, DIMS)), BCG_TEST_GRIDS=grids, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
           "127.0.0.1", "--master-port", str(29820 + world), os.path.join(ROOT, "tests", "dist_stout_smear_worker.py")]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "DIST_STOUT_SMEAR_OK" in out.stdout
