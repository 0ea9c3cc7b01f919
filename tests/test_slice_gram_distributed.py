"""Per-slice Gram matrices with momentum projection on a lattice divided over ranks (tests/dist_slice_gram_worker.py): 2 and 4
gloo ranks share the one GPU.  Full and half fields, a divided and an undivided slice direction, momenta with non-zero
components along the divided directions: the result is identical on all ranks and equals the single-rank result to 1e-13 of
|a_i||b_j| per slice.  One launch per world size (the grids of one size share it) to keep the start-up cost of the ranks down."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

DIMS = [8, 4, 4, 8]
CASES = [(2, "2,1,1,1;1,1,1,2"), (4, "2,2,1,1")]


@pytest.mark.parametrize("world,grids", CASES, ids=["2-ranks", "4-ranks"])
def test_slice_gram_on_a_divided_lattice(world, grids):
    env = dict(os.environ, BCG_TEST_DIMS=",".join(map(str, DIMS)), BCG_TEST_GRIDS=grids, BCG_TEST_WIDTHS="5,16",
               OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
           "127.0.0.1", "--master-port", str(29720 + world), os.path.join(ROOT, "tests", "dist_slice_gram_worker.py")]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "DIST_SLICE_GRAM_OK" in out.stdout
