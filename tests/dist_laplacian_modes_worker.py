"""Worker for tests/test_laplacian_modes_distributed.py: one rank of a divided lattice rotating a basis slice by slice and
computing the Laplacian modes of every slice.  Several ranks share GPU 0 and all-reduce through gloo.  Gaussian noise depends
on the global site only and the links are cut out of one host array, so each rank also holds the whole lattice on a context of
its own and compares with the single-rank result."""
import os
import sys

import numpy as np
import torch  # noqa: F401  -- before the library: one HIP runtime (tests/conftest.py)
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import blockcg_amd as bc  # noqa: E402
import shift_sum_ref as ss  # noqa: E402
from blockcg_amd.comm import TorchDistComm, coords_of  # noqa: E402
from dist_shift_sum_worker import local_rows  # noqa: E402

TOL_KERNEL = 1e-13  # tests/conftest.py
DIR = 3
SLICES = [6, 1]  # one in the second rank's half of a divided direction of 8, one in the first's
ROTATIONS = ([32, 16], [5, 7])  # the MFMA form and the generic one
# [8,4,4,8] with unitary links: a slice has 384 dimensions, its eigenvalues 32 and 33 are 0.02 .. 0.04 apart and the numpy
# restatement converges in 6 outer iterations at the degree and tolerance of the single-rank tests
WIDTHS, WANT, DEGREE, TOL, UB, LIMIT = [32, 16], 32, 16, 1e-10, 12.0, 100
LINK_SEED = 4242


def run(c, U, comm=None):
    links = bc.gauge_field(c).upload(U)
    V = [bc.block_fermion_field(c, w).setGaussian(60 + k) for k, w in enumerate(WIDTHS)]
    try:
        r = bc.laplacian_modes(V, links, DIR, WANT, UB, DEGREE, TOL, LIMIT)
        code = 0
    except bc.BlockCGError as e:
        r, code = None, e.code
    if comm is not None and comm.error:
        raise comm.error
    return V, r, code


def main():
    gdims = [int(x) for x in os.environ["BCG_TEST_DIMS"].split(",")]
    grids = [[int(x) for x in g.split(",")] for g in os.environ["BCG_TEST_GRIDS"].split(";")]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    whole = bc.Context(gdims, device=0)
    U = ss.unitary_links(np.random.default_rng(LINK_SEED), gdims)  # the same on every rank
    wV, wr, wcode = run(whole, U)
    assert wcode == 0 and wr["resid"][:, :WANT].max() <= TOL * UB, (wcode, wr)
    x_dir = ss.coordinates(gdims)[:, DIR]
    rng = np.random.default_rng(79)  # the same draws on every rank
    worst = [0.0, 0.0, 0.0]
    for grid in grids:
        assert int(np.prod(grid)) == world
        comm = TorchDistComm(0)
        ctx = bc.Context(gdims, device=0, grid=grid, coords=coords_of(rank, grid), stream=comm.stream_ptr)
        comm.attach(ctx)
        rows = local_rows(gdims, ctx, None)

        # ---- the rotation: each rank's sites against the single-rank call; the slices that are not listed keep their bits
        for widths in ROTATIONS:
            K = sum(widths)
            V = [bc.block_fermion_field(ctx, w).setGaussian(5 + k) for k, w in enumerate(widths)]
            WV = [bc.block_fermion_field(whole, w).setGaussian(5 + k) for k, w in enumerate(widths)]
            start, wstart = [v.download() for v in V], [v.download() for v in WV]
            for direction in (0, DIR):
                t_mine = ss.coordinates(gdims)[rows, direction]
                for slices in (None, SLICES):
                    S = gdims[direction] if slices is None else len(slices)
                    Q = rng.standard_normal((S, K, K)) + 1j * rng.standard_normal((S, K, K))
                    listed = np.isin(t_mine, range(gdims[direction]) if slices is None else slices)
                    for v, h in zip(V + WV, start + wstart):
                        v.upload(h)
                    bc.basis_slice_rotate(V, Q, direction, slices)
                    bc.basis_slice_rotate(WV, Q, direction, slices)
                    if comm.error:
                        raise comm.error
                    for v, wv, h in zip(V, WV, start):
                        got, want = v.download(), wv.download()[rows]
                        err = float(np.linalg.norm(got - want) / np.linalg.norm(want))
                        assert err <= TOL_KERNEL, (rank, grid, widths, direction, slices, err)
                        worst[0] = max(worst[0], err)
                        assert np.array_equal(got[~listed].view(np.uint64), h[~listed].view(np.uint64)), (rank, grid, widths, direction, slices)

        # ---- the eigensolver
        V, r, code = run(ctx, U[rows], comm)
        # the same on every rank: return code, iteration count, Ritz values and residuals, bit for bit
        mine = (code, None if r is None else (r["iterations"], r["applications"], r["evals"].tobytes(), r["resid"].tobytes()))
        gathered = [None] * world
        dist.all_gather_object(gathered, mine)
        assert all(g == gathered[0] for g in gathered), (rank, grid, gathered)
        assert code == 0, (rank, grid, code)
        assert r["resid"][:, :WANT].max() <= TOL * UB
        e = float(np.abs(r["evals"][:, :WANT] - wr["evals"][:, :WANT]).max())
        assert e <= 1e-12 * UB, (rank, grid, e)
        worst[1] = max(worst[1], e / UB)
        # The wanted block against the single-rank vectors, slice by slice: the singular values of W(t)^dagger V(t) are the
        # cosines of the principal angles between the two spans (single vectors are fixed up to a phase only, and up to a
        # rotation where eigenvalues coincide)
        W0 = bc.block_fermion_field(ctx, WIDTHS[0], host=wV[0].download()[rows])
        for t, M in enumerate(bc.basis_slice_dot([W0], V[0], DIR)):
            d = np.linalg.svd(M, compute_uv=False)
            assert np.abs(d - 1.0).max() <= 1e-8, (rank, grid, t, d)
            worst[2] = max(worst[2], float(np.abs(d - 1.0).max()))
        if comm.error:
            raise comm.error
        dist.barrier()
    if rank == 0:
        print("DIST_LAPLACIAN_MODES_OK", world, grids, "iterations %d (single rank %d)" % (r["iterations"], wr["iterations"]),
              "max err rotation %.2e, evals %.2e of the bound, spans %.2e" % tuple(worst))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
