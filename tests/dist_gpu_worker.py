"""Worker for tests/test_distributed_gpu.py: one rank of a domain-decomposed SBCGrQ run.  Several ranks
share GPU 0 and talk through gloo (host-staged), which exercises everything of the multi-GPU path except
the RCCL transport itself: ghost-face packing, the halo callbacks, ghost reads in the stencil kernels, the
gauge ghost, and the all-reduced Gram matrices.  Each rank checks its sub-lattice against the CPU oracle
run on the whole lattice."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import blockcg_amd as bc  # noqa: E402
import oracle  # noqa: E402
from blockcg_amd.comm import TorchDistComm, coords_of  # noqa: E402


def main():
    gdims = [int(x) for x in os.environ["BCG_TEST_DIMS"].split(",")]
    grid = [int(x) for x in os.environ["BCG_TEST_GRID"].split(",")]
    m = int(os.environ["BCG_TEST_M"])
    generic = os.environ.get("BCG_TEST_GENERIC", "0") == "1"
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert int(np.prod(grid)) == world
    nd = len(gdims)
    coords = coords_of(rank, grid)
    if os.environ.get("BCG_TEST_TRANSPORT", "torch") == "native":
        # the native transport (libblockcg_rccl*.so; BCG_RCCL_LIB selects the host-staged twin for ranks sharing a GPU)
        from blockcg_amd import rccl
        uid = [rccl.get_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(uid, src=0)
        ctx = bc.Context(gdims, device=0, grid=grid, coords=coords)
        comm = rccl.RcclComm(ctx, uid[0], rank, world)
        if os.environ.get("BCG_TEST_OVERLAP", "1") != "1":  # blocking exchange only: drop the split callbacks
            cb = comm.callbacks
            from blockcg_amd import _lib
            blocking = _lib.bcg_comm(cb.user, cb.halo_exchange, cb.allreduce_sum, _lib.HALO_CB(), _lib.HALO_END_CB())
            ctx.set_comm(blocking, comm)
    else:
        comm = TorchDistComm(0, overlap=os.environ.get("BCG_TEST_OVERLAP", "1") == "1")
        ctx = bc.Context(gdims, device=0, grid=grid, coords=coords, stream=comm.stream_ptr)
        comm.attach(ctx)
    ctx.force_generic(generic)
    ctx.capacity_mode(int(os.environ.get("BCG_TEST_RING", "0")))
    mass, shifts, iters = 0.1, [0.0, 1e-3, 1e-1], 4
    D = bc.dirac_op(ctx, mass, seed=3)
    B = bc.block_fermion_field(ctx, m).setRandom(seed=4)
    # operator alone
    out = bc.block_fermion_field(ctx, m)
    ctx.profiling(True)
    D.op(out, B)
    prof = ctx.profile()
    ctx.profiling(False)
    if comm.error:
        raise comm.error
    if os.environ.get("BCG_TEST_EXPECT_RING_OVERLAP") == "1":  # capacity mode took the overlapped form: split exchanges per chunk
        assert prof.get("halo_exchange_begin", {}).get("count", 0) >= 2 and "hop_ring" in prof, prof
        assert prof["halo_exchange_end"]["count"] == prof["halo_exchange_begin"]["count"], prof
        assert "halo_exchange" not in prof, sorted(prof)  # the source's faces travel in the split form too: nothing blocks
    orc = oracle.Oracle()
    V = int(np.prod(gdims))
    U = orc.fill_gauge(gdims, 3)
    Bh = orc.fill_field(m, V, 4)
    L, og = ctx.local_dims, ctx.origin
    sl = tuple(slice(o, o + l) for o, l in zip(og, L))[::-1]

    def local(a):  # [V, m, 3] global -> this rank's sites in local lexicographic order
        return np.ascontiguousarray(a.reshape(gdims[::-1] + [m, 3])[sl]).reshape(-1, m, 3)

    def rel(a, b):
        return np.linalg.norm(a - b) / np.linalg.norm(b)

    assert np.array_equal(B.download(), local(Bh))
    e_op = rel(out.download(), local(orc.dirac_apply(U, gdims, mass, Bh)))
    assert e_op < 2e-13, ("op", rank, e_op)
    # Gram matrix over all ranks
    G = B.hermitian_dot(out)
    Gw = orc.hermitian_dot(Bh, orc.dirac_apply(U, gdims, mass, Bh))
    assert rel(G, Gw) < 1e-13
    # solver, fixed work
    X = [bc.block_fermion_field(ctx, m) for _ in shifts]
    info = bc.SBCGrQ(X, B, D, shifts, 0.0, 0.0, max_iterations=iters, trace_limit=iters, return_info=True)
    if comm.error:
        raise comm.error
    o = orc.sbcgrq(U, gdims, mass, Bh, shifts, 0.0, 0.0, max_iterations=iters, trace_limit=iters)
    for key in ("alpha", "rho", "delta", "alpha_s", "beta_s"):
        assert rel(info["trace"][key], o["trace"][key]) < 1e-10, (key, rank)
    for s in range(len(shifts)):
        e = rel(X[s].download(), local(o["X"][s]))
        assert e < 1e-11, ("X", s, rank, e)
    if os.environ.get("BCG_TEST_HALF") == "1":
        half_volume_checks(ctx, comm, orc, D, B, U, Bh, gdims, mass, m, local, rel)
    if os.environ.get("BCG_TEST_STANDARD") == "1":
        standard_solver_checks(ctx, comm, orc, D, B, U, Bh, gdims, mass, iters, local, rel)
    dist.barrier()
    if rank == 0:
        print("DIST_GPU_OK", world, grid, "generic" if generic else "fast", "op err %.2e" % e_op)
    dist.destroy_process_group()


def standard_solver_checks(ctx, comm, orc, D, B, U, Bh, gdims, mass, iters, local, rel):
    """SCG and BCG on a lattice divided over ranks (tests/test_standard_solvers.py has them on one rank): the all-reduce under
    real_dot and the Gram matrices, the halo exchange of apply_shifted.  A fixed number of iterations, this rank's sites
    against the whole-lattice oracle."""
    shifts = [0.0, 1e-3, 0.5]
    V = int(np.prod(gdims))
    bh = orc.fill_field(1, V, 8)
    b = bc.block_fermion_field(ctx, 1).setRandom(seed=8)
    xs = [bc.block_fermion_field(ctx, 1) for _ in shifts]
    it = bc.SCG(xs, b, D, shifts, 0.0, 0.0, max_iterations=iters)
    if comm.error:
        raise comm.error
    xo, ito = orc.scg(U, gdims, mass, bh, shifts, 0.0, 0.0, iters)
    assert it == ito == iters
    for s in range(len(shifts)):
        e = rel(xs[s].download(), local_of(xo[s], gdims, ctx, 1))
        assert e < 1e-11, ("SCG x", s, e)
    X = bc.block_fermion_field(ctx, B.N_rhs)
    it = bc.BCG(X, B, D, 0.0, max_iterations=iters)
    if comm.error:
        raise comm.error
    Xo, ito = orc.bcg(U, gdims, mass, Bh, 0.0, iters)
    assert it == ito == iters
    e = rel(X.download(), local(Xo))
    assert e < 1e-11, ("BCG X", e)


def local_of(a, gdims, ctx, m):
    """[V, m, 3] global -> this rank's sites in local lexicographic order (main's `local` for another width)"""
    sl = tuple(slice(o, o + l) for o, l in zip(ctx.origin, ctx.local_dims))[::-1]
    return np.ascontiguousarray(a.reshape(gdims[::-1] + [m, 3])[sl]).reshape(-1, m, 3)


HALF_SHIFTS, HALF_EPS = [0.0, 1e-3, 5e-2], 1e-10


def half_volume_oracle(orc, U, Bh, gdims, mass):
    """What half_volume_checks compares with, on the whole lattice (computed once per process)."""
    pre = {"Dh": orc.hop(U, gdims, Bh), "Ah": orc.dirac_apply(U, gdims, mass, Bh), "Gw": orc.hermitian_dot(Bh, Bh)}
    # the oracle's own converged solve of the whole lattice is minutes of single-thread CPU per rank on the larger lattices:
    # there the solve is judged by the reference's acceptance test alone (true residuals through the operator this worker has
    # just checked against the oracle on the same decomposition)
    if os.environ.get("BCG_TEST_HALF_ORACLE_SOLVE", "1") == "1":
        pre["ref"] = orc.sbcgrq(U, gdims, mass, Bh, HALF_SHIFTS, HALF_EPS, HALF_EPS)
    return pre


def half_volume_checks(ctx, comm, orc, D, B, U, Bh, gdims, mass, m, local, rel, pre=None):
    """Half-volume fields on a lattice divided over ranks (half ghost faces: kernels_generic.hip k_pack_faces_half): the
    operator blocks and the two-half-solves solve of this rank's sites against the whole-lattice oracle."""
    pre = pre or half_volume_oracle(orc, U, Bh, gdims, mass)
    L = ctx.local_dims
    idx = np.arange(ctx.V)
    par = np.zeros(ctx.V, dtype=np.int64)
    for ext in L:  # x0 fastest; the local origin is even in every direction (even local extents)
        par += idx % ext
        idx = idx // ext
    masks = [(par % 2) == q for q in (0, 1)]
    Dh = local(pre["Dh"])
    Ah = local(pre["Ah"])
    halves = B.split_parity()
    ctx.profiling(True)
    for q, half in enumerate(halves):
        assert np.array_equal(half.download(), local(Bh)[masks[q]])
        out = bc.block_fermion_field(ctx, m, parity=q)
        D.op(out, half)
        e = rel(out.download(), Ah[masks[q]])
        assert e < 2e-13, ("half op", q, e)
        other = bc.block_fermion_field(ctx, m, parity=1 - q)
        D.D(other, half)
        e = rel(other.download(), Dh[masks[1 - q]])
        assert e < 2e-13, ("half D", q, e)
    prof = ctx.profile()
    ctx.profiling(False)
    if os.environ.get("BCG_TEST_EXPECT_CHECKERBOARD") == "1":  # the bundle sweep's checkerboard form ran, ghost rows and all
        assert prof.get("stencil_form_k_hop4b_checkerboard", {}).get("count", 0) >= 4, sorted(prof)
    if os.environ.get("BCG_TEST_EXPECT_HALF_CHUNKED") == "1":
        # x3 whole and the split exchange on offer: the operator sweeps x3 in chunks (BCG_HALF_CHUNK) with every exchange --
        # the source's faces in two windows, tmp's per chunk -- begun and ended around stencil launches, none blocking
        ctx.profiling(True)
        ctx.profile_reset()
        out = bc.block_fermion_field(ctx, m, parity=0)
        D.op(out, halves[0])
        prof = ctx.profile()
        ctx.profiling(False)
        chunk = int(os.environ["BCG_HALF_CHUNK"])
        chunks = (L[3] + chunk - 1) // chunk
        assert "halo_exchange" not in prof, sorted(prof)
        assert prof["halo_exchange_begin"]["count"] == chunks + 2 == prof["halo_exchange_end"]["count"], prof
        assert prof["stencil_form_k_hop4b_checkerboard"]["count"] >= 2 * chunks, prof
    if comm.error:
        raise comm.error
    Gw = pre["Gw"]
    G = halves[0].hermitian_dot(halves[0]) + halves[1].hermitian_dot(halves[1])  # each all-reduced over the ranks
    assert rel(G, Gw) < 1e-13
    shifts, eps = HALF_SHIFTS, HALF_EPS
    X = [bc.block_fermion_field(ctx, m) for _ in shifts]
    its = bc.SBCGrQ_half_volume(X, B, D, shifts, eps, eps)
    if comm.error:
        raise comm.error
    if "ref" in pre:
        ref = pre["ref"]
        for s in range(len(shifts)):
            e = rel(X[s].download(), local(ref["X"][s]))
            assert e < 1e-8, ("half solve X", s, e)
        assert max(its) <= ref["iterations"] + 1, (its, ref["iterations"])
    assert bc.true_residuals(X, B, D, shifts).max() < 2 * eps  # the reference's acceptance test (test/solvers.cpp:104-116)


if __name__ == "__main__":
    main()
