"""Baryon elementals on a lattice divided over ranks (tests/dist_basis_slice_triple_worker.py): 2 and 4 gloo ranks share the one
GPU.  One list of 32 + 16 columns three times on full fields and on one half field (the MFMA form, identical lists), lists of
5 + 7, 5 and 3 columns (the generic form); a divided and an undivided slice direction; all slices, and two listed slices that
leave the ranks of the lower half without one; three momenta with non-zero components along the divided directions.  [6,4,4,6]
on (2,1,1,2): local extents of 3, ranks at odd origins.  The result is bit-identical on all ranks and within the tolerance of
tests/test_basis_slice_triple.py of the single-rank call.  One launch per world size: at most four rank processes at a time."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CASES = [(2, "8,4,4,8:2,1,1,1;8,4,4,8:1,1,1,2"), (4, "8,4,4,8:2,2,1,1;6,4,4,6:2,1,1,2")]


@pytest.mark.parametrize("world,runs", CASES, ids=["2-ranks", "4-ranks"])
def test_basis_slice_triple_on_a_divided_lattice(world, runs):
    env = dict(os.environ, BCG_TEST_RUNS=runs, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
           "127.0.0.1", "--master-port", str(29980 + world), os.path.join(ROOT, "tests", "dist_basis_slice_triple_worker.py")]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "DIST_BASIS_SLICE_TRIPLE_OK" in out.stdout
