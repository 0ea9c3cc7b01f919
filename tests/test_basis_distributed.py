"""Products with a basis of another width and the deflated solve on a lattice divided over ranks
(tests/dist_basis_worker.py): 2 and 4 gloo ranks share the one GPU.  V as widths [32, 16] at m = 16 (the MFMA form, full fields
and one half field) and [5, 7] at m = 5 (the generic form): basis_dot is identical on all ranks and equals the single-rank
result to 1e-13 of |V_i||b_j|; basis_axpy and SBCGrQ_deflated equal the single-rank fields to TOL_KERNEL and TOL_SOLUTION.
One launch per world size, so at most four rank processes run at a time."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

DIMS = [8, 4, 4, 8]
CASES = [(2, "2,1,1,1"), (4, "2,2,1,1")]


@pytest.mark.parametrize("world,grids", CASES, ids=["2-ranks", "4-ranks"])
def test_basis_on_a_divided_lattice(world, grids):
    env = dict(os.environ, BCG_TEST_DIMS=",".join(map(str, DIMS)), BCG_TEST_GRIDS=grids, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
           "127.0.0.1", "--master-port", str(29740 + world), os.path.join(ROOT, "tests", "dist_basis_worker.py")]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "DIST_BASIS_OK" in out.stdout
