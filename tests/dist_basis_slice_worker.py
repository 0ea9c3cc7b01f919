"""Worker for tests/test_basis_slice_distributed.py: one rank of a divided lattice taking per-slice products with a basis.
Several ranks share GPU 0 and all-reduce through gloo.  Gaussian noise depends on the global site only, so each rank also
fills the whole lattice on a context of its own and compares with the single-rank result."""
import os
import sys

import numpy as np
import torch  # noqa: F401  -- before the library: one HIP runtime (tests/conftest.py)
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import blockcg_amd as bc  # noqa: E402
from blockcg_amd.comm import TorchDistComm, coords_of  # noqa: E402

EPS_DOT = 1e-13
# non-zero components along every direction a grid divides (0, 1 and 3), beyond the extents and negative
MOMENTA = {0: [[0, 1, -1, 3], [0, -5, 2, 9], [0, 0, 1, 0]], 3: [[1, 1, -1, 0], [-9, 3, 2, 0], [0, 0, 1, 0]]}
# (widths of V, m, parity)
CASES = (([32, 16], 16, None), ([32, 16], 16, 1), ([5, 7], 5, None))


def main():
    gdims = [int(x) for x in os.environ["BCG_TEST_DIMS"].split(",")]
    grids = [[int(x) for x in g.split(",")] for g in os.environ["BCG_TEST_GRIDS"].split(";")]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    whole = bc.Context(gdims, device=0)
    worst = 0.0
    for grid in grids:
        assert int(np.prod(grid)) == world
        comm = TorchDistComm(0)
        ctx = bc.Context(gdims, device=0, grid=grid, coords=coords_of(rank, grid), stream=comm.stream_ptr)
        comm.attach(ctx)
        # half fields need every local extent even (the library refuses them otherwise): full fields only at an odd one
        halves = all(n % 2 == 0 for n in ctx.local_dims)
        for widths, m, parity in CASES:
            if parity is not None and not halves:
                continue
            new = lambda c, w, seed: bc.block_fermion_field(c, w, parity=parity).setGaussian(seed)  # noqa: E731
            V, b = [new(ctx, w, 5 + k) for k, w in enumerate(widths)], new(ctx, m, 15)
            WV, wb = [new(whole, w, 5 + k) for k, w in enumerate(widths)], new(whole, m, 15)
            for direction in (0, 3):
                nv = np.concatenate([np.einsum("tii->ti", v.slice_gram(v, direction)).real for v in WV], axis=1)
                nb = np.einsum("tii->ti", wb.slice_gram(wb, direction)).real
                scale = np.sqrt(nv[:, :, None] * nb[:, None, :])
                for mom in (None, MOMENTA[direction]):
                    got = bc.basis_slice_dot(V, b, direction, mom)
                    if comm.error:
                        raise comm.error
                    want = bc.basis_slice_dot(WV, wb, direction, mom)
                    err = float(np.max(np.abs(got - want) / scale))
                    assert err <= EPS_DOT, (rank, grid, widths, m, parity, direction, mom, err)
                    worst = max(worst, err)
                    gathered = [None] * world
                    dist.all_gather_object(gathered, got.tobytes())
                    assert all(g == gathered[0] for g in gathered), (rank, grid, widths, m, parity, direction)
        dist.barrier()
    if rank == 0:
        print("DIST_BASIS_SLICE_OK", world, grids, "max err %.2e" % worst)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
