"""Worker for tests/test_slice_gram_distributed.py: one rank of a divided lattice taking per-slice Gram matrices with momentum
projection.  Several ranks share GPU 0 and all-reduce through gloo.  Gaussian noise depends on the global site only, so each
rank also fills the whole lattice on a context of its own and compares with the single-rank result."""
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
MOMENTA = {0: [[0, 1, -1, 3], [0, -5, 2, 9]], 3: [[1, 1, -1, 0], [-9, 3, 2, 0]]}


def main():
    gdims = [int(x) for x in os.environ["BCG_TEST_DIMS"].split(",")]
    grids = [[int(x) for x in g.split(",")] for g in os.environ["BCG_TEST_GRIDS"].split(";")]
    widths = [int(x) for x in os.environ["BCG_TEST_WIDTHS"].split(",")]
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
        parities = (None, 1) if all(n % 2 == 0 for n in ctx.local_dims) else (None,)
        for m in widths:
            for parity in parities:
                new = lambda c, seed: bc.block_fermion_field(c, m, parity=parity).setGaussian(seed)  # noqa: E731
                a, b, wa, wb = new(ctx, 5), new(ctx, 6), new(whole, 5), new(whole, 6)
                for direction in (0, 3):
                    na = np.einsum("tii->ti", wa.slice_gram(wa, direction)).real
                    nb = np.einsum("tii->ti", wb.slice_gram(wb, direction)).real
                    for x, y, wx, wy, ny in ((a, b, wa, wb, nb), (a, a, wa, wa, na)):
                        scale = np.sqrt(na[:, :, None] * ny[:, None, :])
                        for mom in (None, MOMENTA[direction]):
                            got = x.slice_gram(y, direction, mom)
                            if comm.error:
                                raise comm.error
                            want = wx.slice_gram(wy, direction, mom)
                            err = float(np.max(np.abs(got - want) / scale))
                            assert err <= EPS_DOT, (rank, grid, m, parity, direction, mom, err)
                            worst = max(worst, err)
                            gathered = [None] * world
                            dist.all_gather_object(gathered, got.tobytes())
                            assert all(g == gathered[0] for g in gathered), (rank, grid, m, parity, direction)
        dist.barrier()
    if rank == 0:
        print("DIST_SLICE_GRAM_OK", world, grids, "m", widths, "max err %.2e" % worst)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
