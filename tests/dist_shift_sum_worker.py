"""Worker for tests/test_shift_sum_distributed.py: one rank of a divided lattice applying the covariant nearest-neighbour sum
and smearing.  Several ranks share GPU 0 and exchange faces through gloo.  Links and Gaussian noise depend on the global site
only, so each rank also holds the whole lattice on a context of its own and compares its local part of the single-rank result."""
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
import shift_sum_ref as ref  # noqa: E402

TOL_KERNEL = 1e-13


def local_rows(gdims, ctx, parity):
    """Rows of the single-rank field (full, or the half field of `parity`) that this rank holds, in its own order."""
    lc = ref.coordinates(ctx.local_dims) + np.asarray(ctx.origin)
    strides = np.cumprod([1] + list(gdims[:-1]))
    gidx = lc @ strides
    if parity is None:
        return gidx
    held = ref.parity_mask(gdims, parity)
    return (np.cumsum(held) - 1)[gidx[lc.sum(axis=1) % 2 == parity]]


def rel_err(a, b):
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


def main():
    gdims = [int(x) for x in os.environ["BCG_TEST_DIMS"].split(",")]
    grids = [[int(x) for x in g.split(",")] for g in os.environ["BCG_TEST_GRIDS"].split(";")]
    widths = [int(x) for x in os.environ["BCG_TEST_WIDTHS"].split(",")]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    whole = bc.Context(gdims, device=0)
    nd = len(gdims)
    rng = np.random.default_rng(23)  # the same coefficients on every rank
    worst = 0.0
    for grid in grids:
        assert int(np.prod(grid)) == world
        comm = TorchDistComm(0)
        ctx = bc.Context(gdims, device=0, grid=grid, coords=coords_of(rank, grid), stream=comm.stream_ptr)
        comm.attach(ctx)
        D, wD = bc.dirac_op(ctx, 0.1, seed=5), bc.dirac_op(whole, 0.1, seed=5)
        # a link container refilled after its ghost was exchanged: the stale ghost must be refreshed
        G, wG = bc.gauge_field(ctx).setRandom(8), bc.gauge_field(whole).setRandom(9)
        # half fields need every local extent even (the library refuses them otherwise): full fields only at an odd one
        parities = (None, 0, 1) if all(n % 2 == 0 for n in ctx.local_dims) else (None,)
        for m in widths:
            for parity in parities:  # half fields: both directions, each with its own x0 offset and half ghost faces
                po = None if parity is None else 1 - parity
                rows = local_rows(gdims, ctx, po)
                a, wa = (bc.block_fermion_field(c, m, parity=parity).setGaussian(6) for c in (ctx, whole))
                out, wout = (bc.block_fermion_field(c, m, parity=po) for c in (ctx, whole))
                for eta in (False, True):
                    c0 = complex(rng.normal(), rng.normal()) if parity is None else 0.0
                    fw, bw = rng.normal(size=nd) + 1j * rng.normal(size=nd), rng.normal(size=nd) + 1j * rng.normal(size=nd)
                    ctx.profiling(True)
                    ctx.profile_reset()
                    got = bc.shift_sum(out, a, D, c0, fw, bw, eta).download()
                    prof = ctx.profile()
                    ctx.profiling(False)
                    if comm.error:
                        raise comm.error
                    want = bc.shift_sum(wout, wa, wD, c0, fw, bw, eta).download()[rows]
                    err = rel_err(got, want)
                    assert err <= TOL_KERNEL, (rank, grid, m, parity, eta, err)
                    worst = max(worst, err)
                    if m == 32 and parity is None and grid[0] == 1 and ctx.local_dims[0] % 8 == 0:
                        assert prof.get("shift_form_tile", {}).get("count", 0) == 1, sorted(prof)  # the tile form read ghosts
                if parity is None:
                    got = bc.smear(a, D, 3, 0.1, 3).download()
                    if comm.error:
                        raise comm.error
                    want = bc.smear(wa, wD, 3, 0.1, 3).download()[rows]
                    err = rel_err(got, want)
                    assert err <= TOL_KERNEL, (rank, grid, m, "smear", err)
                    worst = max(worst, err)
                    # stale ghost: G's ghost is exchanged for seed 8, then G is refilled with the whole lattice's seed 9
                    a.setGaussian(7), wa.setGaussian(7)
                    bc.laplacian(out, a, G)
                    G.setRandom(9)
                    got = bc.laplacian(out, a, G).download()
                    if comm.error:
                        raise comm.error
                    err = rel_err(got, bc.laplacian(wout, wa, wG).download()[rows])
                    assert err <= TOL_KERNEL, (rank, grid, m, "stale gauge ghost", err)
                    G.setRandom(8)
        dist.barrier()
    if rank == 0:
        print("DIST_SHIFT_SUM_OK", world, grids, "m", widths, "max err %.2e" % worst)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
