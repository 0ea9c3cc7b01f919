"""A basis put onto slices of a lattice divided over ranks (tests/dist_basis_slice_axpy_worker.py): 2 and 4 gloo ranks share
the one GPU.  V = 32 + 16 columns against m = 16 on full fields and on one half field (the MFMA form), V = 5 + 7 against m = 5
(the generic form); a divided and an undivided slice direction; all slices, and one listed slice in the second rank's half
with one in the first's (so that a rank may hold one, both or none of them); a momentum with non-zero components along the
divided directions; beta 1, 0 and -0.5.  Each rank's result equals its sites of the single-rank result to TOL_KERNEL, the
sites that are not listed are bit-identical to the start at beta = 1 and exact zeros at beta = 0.  One launch per world size
(the grids of one size share it): at most four rank processes at a time."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

DIMS = [8, 4, 4, 8]
CASES = [(2, "2,1,1,1;1,1,1,2"), (4, "2,2,1,1")]


@pytest.mark.parametrize("world,grids", CASES, ids=["2-ranks", "4-ranks"])
def test_basis_slice_axpy_on_a_divided_lattice(world, grids):
    env = dict(os.environ, BCG_TEST_DIMS=",".join(map(str, DIMS)), BCG_TEST_GRIDS=grids, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
           "127.0.0.1", "--master-port", str(29970 + world), os.path.join(ROOT, "tests", "dist_basis_slice_axpy_worker.py")]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "DIST_BASIS_SLICE_AXPY_OK" in out.stdout
