"""Worker for tests/test_force_distributed.py: one rank of a divided lattice computing the fermion force (bcg_force_accumulate)
of full and half fields.  Several ranks share GPU 0 and exchange faces through gloo.  Every input comes from the counter-based
generator (its values depend on the global site only), so each rank also builds the whole lattice on a context of its own
and checks that its F is its slice of the single-rank F."""
import os
import sys

import numpy as np
import torch  # noqa: F401  -- before the library: one HIP runtime (tests/conftest.py)
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import blockcg_amd as bc  # noqa: E402
from blockcg_amd.comm import TorchDistComm, coords_of  # noqa: E402


def forces(ctx, m, parity, residues):
    """(plain F with two work fields, projected F with the library's own) from the generator's links, X_s and F."""
    D = bc.dirac_op(ctx, 0.3, seed=3)
    X = [bc.block_fermion_field(ctx, m, parity=parity).setRandom(seed=10 + s) for s in range(len(residues))]
    F = bc.gauge_field(ctx).setRandom(seed=20)
    P = bc.gauge_field(ctx).setRandom(seed=21)
    bc.fermion_force(F, X, D, residues, 0.7, work=[bc.block_fermion_field(ctx, m, parity=parity) for _ in range(2)])
    bc.fermion_force(P, X, D, residues, 0.7, project=True)
    return F.download(), P.download()


def failing_rank_check(ctx, comm, m, rank, fail_rank):
    """One rank cannot allocate the call's work field (n_work = 0): the ranks agree on that before the first exchange, so every
    rank returns BCG_ERR_HIP (none waits for a face that never comes) and F is unchanged on all of them."""
    D = bc.dirac_op(ctx, 0.3, seed=3)
    X = [bc.block_fermion_field(ctx, m).setRandom(seed=10 + s) for s in range(3)]
    F = bc.gauge_field(ctx).setRandom(seed=20)
    before = F.download()
    try:
        bc.fermion_force(F, X, D, [0.9, -1.1, 0.4], 0.7)
    except bc.BlockCGError as e:
        assert e.code == 3, (rank, str(e))
        if rank != fail_rank:
            assert "another rank of the process grid could not allocate" in str(e), (rank, str(e))
    else:
        raise AssertionError(f"rank {rank}: the call succeeded although rank {fail_rank} could not allocate")
    if comm.error:
        raise comm.error
    assert np.array_equal(F.download(), before), rank


def main():
    gdims = [int(x) for x in os.environ["BCG_TEST_DIMS"].split(",")]
    grid = [int(x) for x in os.environ["BCG_TEST_GRID"].split(",")]
    m = int(os.environ["BCG_TEST_M"])
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert int(np.prod(grid)) == world
    nd = len(gdims)
    comm = TorchDistComm(0, overlap=os.environ.get("BCG_TEST_OVERLAP", "1") == "1")
    fail_rank = int(os.environ.get("BCG_TEST_FAIL_RANK", "-1"))
    if rank == fail_rank:  # room for the caller's three fields X_s only: the call's own work field cannot be allocated
        V_local = int(np.prod(gdims)) // world
        os.environ["BCG_DEBUG_FIELD_BUDGET"] = str(3 * V_local * 48 * m)
    ctx = bc.Context(gdims, device=0, grid=grid, coords=coords_of(rank, grid), stream=comm.stream_ptr)
    os.environ.pop("BCG_DEBUG_FIELD_BUDGET", None)
    comm.attach(ctx)
    if fail_rank >= 0:
        failing_rank_check(ctx, comm, m, rank, fail_rank)
        dist.barrier()
        if rank == 0:
            print("DIST_FORCE_OK", world, grid, "m", m, "rank", fail_rank, "failed its allocation; every rank returned")
        dist.destroy_process_group()
        return
    whole = bc.Context(gdims, device=0)
    L, og = ctx.local_dims, ctx.origin
    sl = tuple(slice(o, o + n) for o, n in zip(og, L))[::-1]

    def local(a):  # [V, nd, 3, 3] of the whole lattice -> this rank's sites in local lexicographic order
        return np.ascontiguousarray(a.reshape(gdims[::-1] + [nd, 3, 3])[sl]).reshape(-1, nd, 3, 3)

    residues = [0.9, -1.1, 0.4]  # three shifts with two work fields: launches of two and one
    worst = 0.0
    # half fields need every local extent even (the library refuses them otherwise): full fields only at an odd one
    for parity in (None, 0, 1) if all(n % 2 == 0 for n in L) else (None,):
        got = forces(ctx, m, parity, residues)
        if comm.error:
            raise comm.error
        want = forces(whole, m, parity, residues)
        for g, w, what in zip(got, want, ("plain", "projected")):
            wl = local(w)
            err = np.max(np.abs(g - wl)) / np.max(np.abs(wl))
            assert err <= 1e-13, (rank, parity, what, err)
            worst = max(worst, err)
    dist.barrier()
    if rank == 0:
        print("DIST_FORCE_OK", world, grid, "m", m, "max rel err %.2e" % worst)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
