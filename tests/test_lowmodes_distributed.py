"""The low-mode eigensolver on a lattice divided over ranks (tests/dist_lowmodes_worker.py): 2 and 4 gloo ranks share the one
GPU.  [8,4,4,8], V as widths [32, 16], 32 wanted: return code, spectral bound, iteration count, Ritz values and residuals
are identical on every rank; the Ritz values equal the single-rank run's to 1e-12 of the bound, and the span of the wanted
vectors the single-rank span to 1e-8 (the cosines of the principal angles; the spectrum is two-fold degenerate, so single
vectors are not comparable).  Degree 64, tol 1e-8: the 48 lowest eigenvalues lie within 0.0100 .. 0.0123 of a spectrum that
reaches 15.5.  One launch per world size."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

DIMS = [8, 4, 4, 8]
CASES = [(2, "2,1,1,1"), (4, "2,2,1,1")]


@pytest.mark.parametrize("world,grids", CASES, ids=["2-ranks", "4-ranks"])
def test_lowest_modes_on_a_divided_lattice(world, grids):
    env = dict(os.environ, BCG_TEST_DIMS=",".join(map(str, DIMS)), BCG_TEST_GRIDS=grids, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
           "127.0.0.1", "--master-port", str(29760 + world), os.path.join(ROOT, "tests", "dist_lowmodes_worker.py")]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "DIST_LOWMODES_OK" in out.stdout
