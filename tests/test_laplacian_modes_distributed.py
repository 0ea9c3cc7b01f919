"""The per-slice rotation and the Laplacian modes on a lattice divided over ranks (tests/dist_laplacian_modes_worker.py):
2 and 4 gloo ranks share the one GPU.  [8,4,4,8], slices of direction 3, grids that divide a spatial direction, the slice
direction itself, and two spatial directions.  The rotation of each rank's sites equals the single-rank call's to TOL_KERNEL
(MFMA and generic widths, a divided and an undivided direction, all slices and two listed ones of which a rank may hold both,
one or none) and leaves the slices that are not listed bit-identical.  laplacian_modes with V as widths [32, 16], 32 wanted,
unitary links, upper_bound 12, degree 16 and tol 1e-10 (the restatement converges in 6 outer iterations on this lattice):
status, iteration count, Ritz values and residuals identical on every rank; the Ritz values equal the single-rank run's to
1e-12 of the bound; the span of the wanted vectors of every slice equals the single-rank span to 1e-8 (the cosines of the
principal angles).  One launch per world size."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

DIMS = [8, 4, 4, 8]
CASES = [(2, "2,1,1,1;1,1,1,2"), (4, "2,2,1,1")]


@pytest.mark.parametrize("world,grids", CASES, ids=["2-ranks", "4-ranks"])
def test_laplacian_modes_on_a_divided_lattice(world, grids):
    env = dict(os.environ, BCG_TEST_DIMS=",".join(map(str, DIMS)), BCG_TEST_GRIDS=grids, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
           "127.0.0.1", "--master-port", str(29790 + world), os.path.join(ROOT, "tests", "dist_laplacian_modes_worker.py")]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "DIST_LAPLACIAN_MODES_OK" in out.stdout
