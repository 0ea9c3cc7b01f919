"""Worker for tests/test_basis_slice_axpy_distributed.py: one rank of a divided lattice putting a basis onto slices.  Several
ranks share GPU 0.  The call is purely local and Gaussian noise depends on the global site only, so each rank also does the
call on the whole lattice, on a context of its own, and compares its own sites."""
import os
import sys

import numpy as np
import torch  # noqa: F401  -- before the library: one HIP runtime (tests/conftest.py)
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import blockcg_amd as bc  # noqa: E402
from blockcg_amd.comm import TorchDistComm, coords_of  # noqa: E402

TOL_KERNEL = 1e-13  # tests/conftest.py
# non-zero components along every direction a grid divides (0, 1 and 3), beyond the extents and negative
MOMENTUM = {0: [0, -5, 2, 9], 3: [-9, 3, 2, 0]}
SLICES = [6, 1]  # one in the second rank's half of a divided direction of 8, one in the first's
# (widths of V, m, parity)
CASES = (([32, 16], 16, None), ([32, 16], 16, 1), ([5, 7], 5, None))


def main():
    gdims = [int(x) for x in os.environ["BCG_TEST_DIMS"].split(",")]
    grids = [[int(x) for x in g.split(",")] for g in os.environ["BCG_TEST_GRIDS"].split(";")]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    whole = bc.Context(gdims, device=0)
    par_of_site = np.indices(gdims[::-1]).sum(axis=0) & 1  # [x3, x2, x1, x0]
    x_of_site = np.indices(gdims[::-1])[::-1]              # x_of_site[mu] is [x3, x2, x1, x0] -> x_mu
    rng = np.random.default_rng(77)  # the same draws on every rank
    worst = 0.0
    for grid in grids:
        assert int(np.prod(grid)) == world
        comm = TorchDistComm(0)
        ctx = bc.Context(gdims, device=0, grid=grid, coords=coords_of(rank, grid), stream=comm.stream_ptr)
        comm.attach(ctx)
        sl = tuple(slice(o, o + n) for o, n in zip(ctx.origin, ctx.local_dims))[::-1]

        def mine(host, m, parity):
            """this rank's sites of a host array of the whole lattice (or of its half of one parity)"""
            if parity is None:
                return host.reshape(gdims[::-1] + [m, 3])[sl].reshape(-1, m, 3)
            full = np.zeros(gdims[::-1] + [m, 3], dtype=np.complex128)
            full[par_of_site == parity] = host
            return full[sl][par_of_site[sl] == parity]

        # half fields need every local extent even (the library refuses them otherwise): full fields only at an odd one
        halves = all(n % 2 == 0 for n in ctx.local_dims)
        for widths, m, parity in CASES:
            if parity is not None and not halves:
                continue
            new = lambda c, w, seed: bc.block_fermion_field(c, w, parity=parity).setGaussian(seed)  # noqa: E731
            V, y = [new(ctx, w, 5 + k) for k, w in enumerate(widths)], new(ctx, m, 15)
            WV, wy = [new(whole, w, 5 + k) for k, w in enumerate(widths)], new(whole, m, 15)
            start, wstart = y.download(), wy.download()
            assert np.array_equal(start, mine(wstart, m, parity))
            K = sum(widths)
            for direction in (0, 3):
                t_mine = x_of_site[direction][sl].reshape(-1) if parity is None else x_of_site[direction][sl][par_of_site[sl] == parity]
                for slices in (None, SLICES):
                    S = gdims[direction] if slices is None else len(slices)
                    C = rng.standard_normal((S, K, m)) + 1j * rng.standard_normal((S, K, m))
                    listed = np.isin(t_mine, range(gdims[direction]) if slices is None else slices)
                    for mom in (None, MOMENTUM[direction]):
                        for beta in (1.0, 0.0, -0.5):
                            y.upload(np.full_like(start, np.nan) if beta == 0.0 else start)
                            wy.upload(wstart)
                            bc.basis_slice_axpy(y, V, C, direction, slices, mom, beta)
                            bc.basis_slice_axpy(wy, WV, C, direction, slices, mom, beta)
                            if comm.error:
                                raise comm.error
                            got, want = y.download(), mine(wy.download(), m, parity)
                            what = (rank, grid, widths, m, parity, direction, slices, mom, beta)
                            nw = np.linalg.norm(want)
                            err = float(np.linalg.norm(got - want) / (nw if nw > 0 else 1.0))
                            assert err <= TOL_KERNEL, what + (err,)
                            worst = max(worst, err)
                            if beta == 1.0:  # the sites that are not listed keep their bits
                                assert np.array_equal(got[~listed].view(np.float64), start[~listed].view(np.float64)), what
                            if beta == 0.0:
                                assert not np.isnan(got).any() and np.all(got[~listed] == 0), what
        dist.barrier()
    if rank == 0:
        print("DIST_BASIS_SLICE_AXPY_OK", world, grids, "max err %.2e" % worst)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
