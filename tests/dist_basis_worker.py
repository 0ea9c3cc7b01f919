"""Worker for tests/test_basis_distributed.py: one rank of a divided lattice taking products with a basis of another width
and running the deflated solve.  Several ranks share GPU 0 and all-reduce through gloo.  Links and Gaussian noise depend on the
global site only, so each rank also holds the whole lattice on a context of its own and compares with the single-rank result."""
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
from dist_shift_sum_worker import local_rows, rel_err  # noqa: E402

EPS_DOT = 1e-13
TOL_KERNEL = 1e-13
TOL_SOLUTION = 1e-8
CASES = (([32, 16], 16), ([5, 7], 5))  # (widths of V, m): the MFMA form and the generic one
MASS, SIGMA, EPS = 0.1, [0.0, 0.05, 0.5], 1e-10


def orthonormal_basis(c, D, widths):
    """Gaussian fields orthonormalised with the library's own calls (thinQR within a field, deflate against the fields before
    it), and their Ritz values of dirac_op::op.  The same calls on the whole lattice give the same basis to rounding."""
    V = []
    for k, w in enumerate(widths):
        f = bc.block_fermion_field(c, w).setGaussian(40 + k)
        f.thinQR()
        for _ in range(2):
            if V:
                bc.deflate(f, V)
            f.thinQR()
        V.append(f)
    ritz = []
    for f in V:
        Af = bc.block_fermion_field(c, f.N_rhs)
        D.op(Af, f)
        ritz.append(np.diag(bc.basis_dot([f], Af)).real)
    return V, np.concatenate(ritz)


def main():
    gdims = [int(x) for x in os.environ["BCG_TEST_DIMS"].split(",")]
    grids = [[int(x) for x in g.split(",")] for g in os.environ["BCG_TEST_GRIDS"].split(";")]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    whole = bc.Context(gdims, device=0)
    worst = [0.0, 0.0, 0.0]
    for grid in grids:
        assert int(np.prod(grid)) == world
        comm = TorchDistComm(0)
        ctx = bc.Context(gdims, device=0, grid=grid, coords=coords_of(rank, grid), stream=comm.stream_ptr)
        comm.attach(ctx)
        for widths, m in CASES:
            K = sum(widths)
            rng = np.random.default_rng(K + m)  # the same coefficients on every rank
            C = rng.standard_normal((K, m)) + 1j * rng.standard_normal((K, m))
            for parity in (None, 1) if m == 16 else (None,):
                rows = local_rows(gdims, ctx, parity)
                new = lambda c, w, seed: bc.block_fermion_field(c, w, parity=parity).setGaussian(seed)  # noqa: E731
                V, wV = ([new(c, w, 10 + k) for k, w in enumerate(widths)] for c in (ctx, whole))
                b, wb, y, wy = new(ctx, m, 30), new(whole, m, 30), new(ctx, m, 31), new(whole, m, 31)
                got = bc.basis_dot(V, b)
                if comm.error:
                    raise comm.error
                want = bc.basis_dot(wV, wb)
                scale = np.sqrt(np.outer(np.concatenate([np.diag(bc.basis_dot([v], v)).real for v in wV]),
                                         np.diag(bc.basis_dot([wb], wb)).real))
                err = float(np.max(np.abs(got - want) / scale))
                assert err <= EPS_DOT, (rank, grid, widths, m, parity, err)
                worst[0] = max(worst[0], err)
                gathered = [None] * world
                dist.all_gather_object(gathered, got.tobytes())
                assert all(g == gathered[0] for g in gathered), (rank, grid, widths, m, parity)
                assert bc.basis_dot(V, b).tobytes() == got.tobytes()
                for beta in (0.0, -0.5):
                    e = rel_err(bc.basis_axpy(y, V, C, beta).download(), bc.basis_axpy(wy, wV, C, beta).download()[rows])
                    assert e <= TOL_KERNEL, (rank, grid, widths, m, parity, beta, e)
                    worst[1] = max(worst[1], e)
        # the deflated solve, full fields, V as widths [32, 16] at m = 16
        widths, m = CASES[0]
        rows = local_rows(gdims, ctx, None)
        X = {}
        for c in (ctx, whole):
            D = bc.dirac_op(c, MASS, seed=5)
            V, ritz = orthonormal_basis(c, D, widths)
            B = bc.block_fermion_field(c, m).setGaussian(77)
            X[c] = [bc.block_fermion_field(c, m) for _ in SIGMA]
            bc.SBCGrQ_deflated(X[c], B, D, SIGMA, V, ritz, EPS, EPS)
            if comm.error:
                raise comm.error
        for s in range(len(SIGMA)):
            e = rel_err(X[ctx][s].download(), X[whole][s].download()[rows])
            assert e <= TOL_SOLUTION, (rank, grid, s, e)
            worst[2] = max(worst[2], e)
        dist.barrier()
    if rank == 0:
        print("DIST_BASIS_OK", world, grids, "max err dot %.2e update %.2e solve %.2e" % tuple(worst))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
