"""The fermion force on a divided lattice when one rank cannot allocate (tests/dist_force_worker.py, failing_rank_check): the
ranks agree on the outcome of their allocations before the first exchange, so every rank returns BCG_ERR_HIP with F unchanged
instead of waiting for faces that never come."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_one_rank_failing_its_allocation_leaves_no_rank_waiting():
    """Rank 2 of four has room for its X_s only (BCG_DEBUG_FIELD_BUDGET), so the work field of n_work = 0 cannot be allocated
    there.  Without the agreement the other ranks would wait in the first exchange until the time limit."""
    dims, grid, m = [8, 8, 4, 4], [2, 2, 1, 1], 16
    env = dict(os.environ, BCG_TEST_DIMS=",".join(map(str, dims)), BCG_TEST_GRID=",".join(map(str, grid)), BCG_TEST_M=str(m),
               OMP_NUM_THREADS="1", BCG_HOP_BLOCKS="8", BCG_HOP_PATCH="16,2,2", BCG_TEST_FAIL_RANK="2")
    env.pop("BCG_DEBUG_FIELD_BUDGET", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=4", "--master-addr", "127.0.0.1",
           "--master-port", "29661", os.path.join(ROOT, "tests", "dist_force_worker.py")]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "DIST_FORCE_OK" in out.stdout and "failed its allocation" in out.stdout
