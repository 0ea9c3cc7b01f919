"""The covariant nearest-neighbour sum and smearing on a lattice divided over ranks (tests/dist_shift_sum_worker.py): 2 and 4
gloo ranks share the one GPU.  [8,4,4,8] on the grids (2,1,1,1), (1,1,1,2) and (2,2,1,1), m = 5, 16 and 32 (at m = 32 the grid
(1,1,1,2) takes the tile form with ghost reads), full and half fields: a random-coefficient shift_sum, smear(3) on full fields
and a link container whose ghost is stale.  Each rank's result equals its local part of the single-rank result to 1e-13.  One
launch per world size (the grids of one size share it) to keep the start-up cost of the ranks down."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

DIMS = [8, 4, 4, 8]
CASES = [(2, "2,1,1,1;1,1,1,2"), (4, "2,2,1,1")]


@pytest.mark.parametrize("world,grids", CASES, ids=["2-ranks", "4-ranks"])
def test_shift_sum_on_a_divided_lattice(world, grids):
    env = dict(os.environ, BCG_TEST_DIMS=",".join(map(str, DIMS)), BCG_TEST_GRIDS=grids, BCG_TEST_WIDTHS="5,16,32",
               OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
           "127.0.0.1", "--master-port", str(29940 + world), os.path.join(ROOT, "tests", "dist_shift_sum_worker.py")]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "DIST_SHIFT_SUM_OK" in out.stdout
