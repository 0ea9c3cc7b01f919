"""The fermion force on a lattice divided over ranks (tests/dist_force_worker.py): 2 and 4 gloo ranks share the one GPU; each
rank's F, plain and projected, full and half fields, must be its slice of the single-rank F."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CASES = [
    # dims,          grid,          m
    ([16, 4, 4, 8], [1, 1, 1, 2], 16),   # x3 divided, the specialised stencil for Y
    ([16, 4, 4, 4], [2, 1, 1, 1], 16),   # x0 divided (half faces compact in x1)
    ([8, 8, 4, 4], [2, 2, 1, 1], 16),    # 4 ranks, x0 and x1 divided
    ([8, 8, 4, 4], [2, 2, 1, 1], 3),     # generic width
    ([8, 4, 4, 8], [1, 1, 1, 2], 32),
]


@pytest.mark.parametrize("dims,grid,m", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_force_on_a_divided_lattice(dims, grid, m):
    world = 1
    for g in grid:
        world *= g
    env = dict(os.environ, BCG_TEST_DIMS=",".join(map(str, dims)), BCG_TEST_GRID=",".join(map(str, grid)), BCG_TEST_M=str(m),
               OMP_NUM_THREADS="1", BCG_HOP_BLOCKS="8", BCG_HOP_PATCH="16,2,2" if m == 16 else "8,2,2")
    port = 29500 + (hash((tuple(dims), tuple(grid), m)) % 150)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "dist_force_worker.py")]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "DIST_FORCE_OK" in out.stdout
