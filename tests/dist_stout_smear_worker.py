"""Worker for tests/test_stout_smear_distributed.py: one rank of a divided lattice smearing the links and taking the
plaquette.  Several ranks share GPU 0 and exchange faces through gloo.  The device generator's links depend on the global site
only, so each rank also holds the whole lattice on a context of its own and compares its local rows of the single-rank result."""
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
import shift_sum_ref as sref  # noqa: E402
import stout_ref as ref  # noqa: E402

TOL_KERNEL = 1e-13


def local_rows(gdims, ctx):
    """Sites of the whole lattice that this rank holds, in its own order."""
    lc = sref.coordinates(ctx.local_dims) + np.asarray(ctx.origin)
    return lc @ np.cumprod([1] + list(gdims[:-1]))


def main():
    gdims = [int(x) for x in os.environ["BCG_TEST_DIMS"].split(",")]
    grids = [[int(x) for x in g.split(",")] for g in os.environ["BCG_TEST_GRIDS"].split(";")]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    whole = bc.Context(gdims, device=0)
    nd = len(gdims)
    table = np.array([[0.12 + 0.01 * mu + 0.003 * nu for nu in range(nd)] for mu in range(nd)])
    wU = bc.gauge_field(whole).setRandom(5)
    wout = bc.gauge_field(whole)
    _, scale = ref.plaquette(ref.from_lib(wU.download()), gdims, with_scale=True)
    wP = bc.plaquette(wU)
    wpsi, wlap = bc.block_fermion_field(whole, 4).setGaussian(6), bc.block_fermion_field(whole, 4)
    worst = 0.0
    for grid in grids:
        assert int(np.prod(grid)) == world
        # without a bcg_comm: every rank is told so, and out keeps its contents
        bare = bc.Context(gdims, device=0, grid=grid, coords=coords_of(rank, grid))
        a, b = bc.gauge_field(bare).setRandom(5), bc.gauge_field(bare).setRandom(6)
        keep = b.download()
        for call in (lambda: bc.stout_smear(b, a, 0.1, 1), lambda: bc.plaquette(a)):
            try:
                call()
                raise AssertionError("no error without a bcg_comm")
            except bc.BlockCGError as e:
                assert e.code == 5, e
        assert np.array_equal(b.download(), keep)

        comm = TorchDistComm(0)
        ctx = bc.Context(gdims, device=0, grid=grid, coords=coords_of(rank, grid), stream=comm.stream_ptr)
        comm.attach(ctx)
        rows = local_rows(gdims, ctx)
        U, out, work = bc.gauge_field(ctx).setRandom(5), bc.gauge_field(ctx), bc.gauge_field(ctx)
        for name, rho, d in (("spatial", 0.1, 3), ("table", table, None)):
            for n in (1, 3):
                got = bc.stout_smear(out, U, rho, n, dir=d, work=work if name == "table" else None).download()
                if comm.error:
                    raise comm.error
                want = bc.stout_smear(wout, wU, rho, n, dir=d).download()[rows]
                err = ref.rel_err(got, want)
                assert err <= TOL_KERNEL, (rank, grid, name, n, err)
                worst = max(worst, err)
        # the plaquette: the single-rank value, and the same bits on every rank
        P = bc.plaquette(U)
        if comm.error:
            raise comm.error
        assert np.all(np.abs(P - wP) <= TOL_KERNEL * scale), (rank, grid, P, wP)
        gathered = [torch.zeros(nd * nd, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(gathered, torch.from_numpy(P.reshape(-1).copy()))
        assert all(np.array_equal(g.numpy().view(np.uint64), P.reshape(-1).view(np.uint64)) for g in gathered), (rank, grid)
        # a smeared container used at once: its stale gauge ghost is refreshed (out held other links a moment ago)
        psi, lap = bc.block_fermion_field(ctx, 4).setGaussian(6), bc.block_fermion_field(ctx, 4)
        bc.laplacian(lap, psi, out)  # exchanges out's ghost for its current contents
        bc.stout_smear(out, U, 0.1, 2, dir=3)
        got = bc.laplacian(lap, psi, out, dir=3).download()
        if comm.error:
            raise comm.error
        bc.stout_smear(wout, wU, 0.1, 2, dir=3)
        err = ref.rel_err(got, bc.laplacian(wlap, wpsi, wout, dir=3).download()[rows])
        assert err <= TOL_KERNEL, (rank, grid, "stale gauge ghost", err)
        worst = max(worst, err)
        dist.barrier()
    if rank == 0:
        print("DIST_STOUT_SMEAR_OK", world, grids, "max err %.2e" % worst)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
