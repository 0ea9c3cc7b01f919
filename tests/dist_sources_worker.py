"""Worker for tests/test_sources_sinks_distributed.py: one rank of a divided lattice filling noise and source fields and taking
slice dots.  Several ranks share GPU 0 and all-reduce through gloo.  Every value depends on the global site only, so each rank
also builds the whole lattice on a context of its own and compares its part."""
import os
import sys

import numpy as np
import torch  # noqa: F401  -- before the library: one HIP runtime (tests/conftest.py)
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import blockcg_amd as bc  # noqa: E402
from blockcg_amd.comm import TorchDistComm, coords_of  # noqa: E402


def fields(ctx, m, parity, pts, col, sl):
    """The fields under test on this context: three kinds of noise, point sources, walls along 0 and 3."""
    new = lambda: bc.block_fermion_field(ctx, m, parity=parity)  # noqa: E731
    f = [new().setGaussian(5), new().setZ2(6), new().setZ4(7), new().setPointSources(pts, col),
         new().setWallSources(0, sl[0], col, -1), new().setWallSources(3, sl[3], col, -1 if parity is None else parity)]
    if parity is None:  # the parity filter on a full field: the walls' even and odd sites by their GLOBAL coordinates
        f += [new().setWallSources(mu, sl[mu], col, par) for mu in (0, 3) for par in (0, 1)]
    return f


def main():
    gdims = [int(x) for x in os.environ["BCG_TEST_DIMS"].split(",")]
    grids = [[int(x) for x in g.split(",")] for g in os.environ["BCG_TEST_GRIDS"].split(";")]
    widths = [int(x) for x in os.environ["BCG_TEST_WIDTHS"].split(",")]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    whole = bc.Context(gdims, device=0)
    par_of_site = np.indices(gdims[::-1]).sum(axis=0) & 1  # [x3, x2, x1, x0]
    worst = 0.0
    for grid in grids:
        assert int(np.prod(grid)) == world
        comm = TorchDistComm(0)
        ctx = bc.Context(gdims, device=0, grid=grid, coords=coords_of(rank, grid), stream=comm.stream_ptr)
        comm.attach(ctx)
        sl = tuple(slice(o, o + n) for o, n in zip(ctx.origin, ctx.local_dims))[::-1]
        # half fields need every local extent even (the library refuses them otherwise): full fields only at an odd one
        parities = (None, 0, 1) if all(n % 2 == 0 for n in ctx.local_dims) else (None,)
        for m in widths:
            rng = np.random.default_rng(100 + m)  # the same draws on every rank
            for parity in parities:
                pts = [[int(rng.integers(0, d)) for d in gdims] for _ in range(m)]
                if parity is not None:
                    for p in pts:
                        if sum(p) % 2 != parity:
                            p[0] ^= 1
                col = [int(c) for c in rng.integers(0, 3, m)]
                sls = {mu: [int(s) for s in rng.integers(0, gdims[mu], m)] for mu in (0, 3)}
                mine, all_of_it = fields(ctx, m, parity, pts, col, sls), fields(whole, m, parity, pts, col, sls)
                for k, (f, w) in enumerate(zip(mine, all_of_it)):
                    wh = w.download()
                    if parity is None:
                        full = wh.reshape(gdims[::-1] + [m, 3])
                        want = full[sl].reshape(-1, m, 3)
                    else:  # scatter the half field into the whole lattice, cut, gather this rank's sites of the parity
                        full = np.zeros(gdims[::-1] + [m, 3], dtype=np.complex128)
                        full[par_of_site == parity] = wh
                        want = full[sl][par_of_site[sl] == parity]
                    assert np.array_equal(f.download(), want), (rank, grid, m, parity, k)
                a, b = mine[0], mine[2]
                wa, wb = all_of_it[0], all_of_it[2]
                na = wa.slice_dot(wa, 0).real.sum(axis=0)  # whole-lattice column norms, for the scale of the sums over t
                for direction in (0, 3):
                    for x, y, wx, wy in ((a, b, wa, wb), (a, a, wa, wa)):
                        got = x.slice_dot(y, direction)
                        if comm.error:
                            raise comm.error
                        want = wx.slice_dot(wy, direction)
                        scale = np.sqrt(wx.slice_dot(wx, direction).real * wy.slice_dot(wy, direction).real)
                        err = float(np.max(np.abs(got - want) / scale))
                        assert err <= 1e-13, (rank, grid, m, parity, direction, err)
                        worst = max(worst, err)
                        gathered = [None] * world
                        dist.all_gather_object(gathered, got.tobytes())
                        assert all(g == gathered[0] for g in gathered), (rank, grid, m, parity, direction)
                assert np.all(na > 0)
        dist.barrier()
    if rank == 0:
        print("DIST_SOURCES_OK", world, grids, "m", widths, "max slice-dot err %.2e" % worst)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
