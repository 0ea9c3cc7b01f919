"""Worker for tests/test_lowmodes_distributed.py: one rank of a divided lattice running the low-mode eigensolver.  Several
ranks share GPU 0 and all-reduce through gloo.  Links and Gaussian noise depend on the global site only, so each rank also
holds the whole lattice on a context of its own and compares with the single-rank result."""
import os
import sys

import numpy as np
import torch  # noqa: F401  -- before the library: one HIP runtime (tests/conftest.py)
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import blockcg_amd as bc  # noqa: E402
from blockcg_amd.comm import TorchDistComm, coords_of  # noqa: E402
from dist_shift_sum_worker import local_rows  # noqa: E402

# [8,4,4,8] with random links has its 48 lowest eigenvalues of dirac_op::op within 0.0100 .. 0.0123 of a spectrum that reaches
# 15.5: degree 16 does not separate them in 120 outer iterations of the numpy restatement, degree 64 does in 26 at tol 1e-10
WIDTHS, WANT, DEGREE, TOL, MASS, LIMIT = [32, 16], 32, 64, 1e-8, 0.1, 100


def run(c, comm=None):
    D = bc.dirac_op(c, MASS, seed=5)
    ub = bc.spectral_bound(D, 10, 9)
    V = [bc.block_fermion_field(c, w).setGaussian(60 + k) for k, w in enumerate(WIDTHS)]
    try:
        r = bc.lowest_modes(V, D, WANT, ub, DEGREE, TOL, LIMIT)
        code = 0
    except bc.BlockCGError as e:
        r, code = None, e.code
    if comm is not None and comm.error:
        raise comm.error
    return ub, V, r, code


def main():
    gdims = [int(x) for x in os.environ["BCG_TEST_DIMS"].split(",")]
    grids = [[int(x) for x in g.split(",")] for g in os.environ["BCG_TEST_GRIDS"].split(";")]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    whole = bc.Context(gdims, device=0)
    wub, wV, wr, wcode = run(whole)
    assert wcode == 0 and wr["resid"][:WANT].max() <= TOL * wub, (wcode, wr)
    worst = [0.0, 0.0]
    for grid in grids:
        assert int(np.prod(grid)) == world
        comm = TorchDistComm(0)
        ctx = bc.Context(gdims, device=0, grid=grid, coords=coords_of(rank, grid), stream=comm.stream_ptr)
        comm.attach(ctx)
        ub, V, r, code = run(ctx, comm)
        # the same on every rank: return code, bound, iteration count, Ritz values and residuals, bit for bit
        mine = (code, ub, None if r is None else (r["iterations"], r["applications"], r["evals"].tobytes(), r["resid"].tobytes()))
        gathered = [None] * world
        dist.all_gather_object(gathered, mine)
        assert all(g == gathered[0] for g in gathered), (rank, grid, gathered)
        assert code == 0, (rank, grid, code)
        assert abs(ub - wub) <= 1e-12 * wub, (ub, wub)
        assert r["resid"][:WANT].max() <= TOL * ub
        e = float(np.abs(r["evals"][:WANT] - wr["evals"][:WANT]).max())
        assert e <= 1e-12 * wub, (rank, grid, e)
        worst[0] = max(worst[0], e / wub)
        # The wanted block against the single-rank vectors.  Every eigenvalue of dirac_op::op is two-fold degenerate (the two
        # parity blocks have the same spectrum), so a vector is fixed only up to a rotation inside its pair and the diagonal
        # of W^dagger V says nothing (0.03 .. 1 here).  The projectors are compared instead: the singular values of W^dagger V
        # are the cosines of the principal angles between the two spans; the 32 wanted columns end between two pairs.
        rows = local_rows(gdims, ctx, None)
        W0 = bc.block_fermion_field(ctx, WIDTHS[0], host=wV[0].download()[rows])
        d = np.linalg.svd(bc.basis_dot([W0], V[0]), compute_uv=False)
        if comm.error:
            raise comm.error
        assert np.abs(d - 1.0).max() <= 1e-8, (rank, grid, d)
        worst[1] = max(worst[1], float(np.abs(d - 1.0).max()))
        dist.barrier()
    if rank == 0:
        print("DIST_LOWMODES_OK", world, grids, "iterations %d (single rank %d)" % (r["iterations"], wr["iterations"]),
              "max err evals %.2e of the bound, vectors %.2e" % tuple(worst))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
