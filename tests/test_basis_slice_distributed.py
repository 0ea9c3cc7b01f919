"""Per-slice products with a basis on a lattice divided over ranks (tests/dist_basis_slice_worker.py): 2 and 4 gloo ranks share
the one GPU.  V = 32 + 16 columns against m = 16 on full fields and on one half field (the MFMA form, a group that is split
by the momenta), V = 5 + 7 against m = 5 (the generic form); a divided and an undivided slice direction; three momenta with
non-zero components along the divided directions: the result is identical on all ranks and equals the single-rank result to
1e-13 of |V_i||b_j| per slice.  One launch per world size (the grids of one size share it)."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

DIMS = [8, 4, 4, 8]
CASES = [(2, "2,1,1,1;1,1,1,2"), (4, "2,2,1,1")]


@pytest.mark.parametrize("world,grids", CASES, ids=["2-ranks", "4-ranks"])
def test_basis_slice_dot_on_a_divided_lattice(world, grids):
    env = dict(os.environ, BCG_TEST_DIMS=",".join(map(str, DIMS)), BCG_TEST_GRIDS=grids, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
           "127.0.0.1", "--master-port", str(29960 + world), os.path.join(ROOT, "tests", "dist_basis_slice_worker.py")]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "DIST_BASIS_SLICE_OK" in out.stdout
