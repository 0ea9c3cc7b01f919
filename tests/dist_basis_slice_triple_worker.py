"""Worker for tests/test_basis_slice_triple_distributed.py: one rank of a divided lattice computing baryon elementals.  Several
ranks share GPU 0.  Gaussian noise depends on the global site only, so each rank also does the call on the whole lattice, on a
context of its own: the divided result is within the tolerance of tests/test_basis_slice_triple.py of it (EPS_DOT of the scale
sum_x |A_i(x)| |B_j(x)| |C_k(x)| of tests/basis_slice_triple_ref.py), and bit-identical on all ranks."""
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
import basis_slice_triple_ref as ref  # noqa: E402

EPS_DOT = 1e-13
# three momenta with non-zero components along every direction a grid divides (0, 1 and 3), beyond the extents and negative
MOMENTA = {0: [[0, -5, 2, 9], [0, 1, 0, -1], [0, 0, 0, 0]], 3: [[-9, 3, 2, 0], [1, -1, 0, 0], [0, 0, 0, 0]]}
IDENTICAL = "identical"
# (widths of A, B, C or IDENTICAL, parity)
CASES = ((([32, 16], IDENTICAL, IDENTICAL), None), (([32, 16], IDENTICAL, IDENTICAL), 1), (([5, 7], [5], [3]), None))


def main():
    # "dims:grid;dims:grid;..."
    runs = [([int(x) for x in d.split(",")], [int(x) for x in g.split(",")])
            for d, g in (r.split(":") for r in os.environ["BCG_TEST_RUNS"].split(";"))]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    worst = 0.0
    wholes = {}
    for gdims, grid in runs:
        assert int(np.prod(grid)) == world
        whole = wholes.setdefault(tuple(gdims), bc.Context(gdims, device=0))
        comm = TorchDistComm(0)
        ctx = bc.Context(gdims, device=0, grid=grid, coords=coords_of(rank, grid), stream=comm.stream_ptr)
        comm.attach(ctx)
        # half fields need every local extent even (the library refuses them otherwise): full fields only at an odd one
        halves = all(n % 2 == 0 for n in ctx.local_dims)
        for spec, parity in CASES:
            if parity is not None and not halves:
                continue

            def lists(c):
                new = lambda w, seed: bc.block_fermion_field(c, w, parity=parity).setGaussian(seed)  # noqa: E731
                A = [new(w, 5 + k) for k, w in enumerate(spec[0])]
                if spec[1] == IDENTICAL:
                    return A, A, A
                return A, [new(w, 25 + k) for k, w in enumerate(spec[1])], [new(w, 45 + k) for k, w in enumerate(spec[2])]

            mine, theirs = lists(ctx), lists(whole)
            hosts = tuple([f.download() for f in fl] for fl in theirs)
            for direction in (0, 3):
                L = gdims[direction]
                # all slices; two slices of the upper half in descending order: where `direction` is divided, the ranks of the
                # lower half hold neither
                for slices in (None, [L - 2, L - 3]):
                    _, scale = ref.basis_slice_triple(*hosts, gdims, direction, slices, None, parity)
                    for mom in (None, MOMENTA[direction]):
                        got = bc.basis_slice_triple(*mine, direction, slices, mom)
                        if comm.error:
                            raise comm.error
                        want = bc.basis_slice_triple(*theirs, direction, slices, mom)
                        what = (rank, gdims, grid, spec, parity, direction, slices, mom is not None)
                        assert got.shape == want.shape, what
                        sc = np.broadcast_to(scale, got.shape)
                        assert not np.any(got[sc == 0]) and not np.any(want[sc == 0]), what
                        err = float(np.max(np.abs(got - want)[sc > 0] / sc[sc > 0]))
                        assert err <= EPS_DOT, what + (err,)
                        worst = max(worst, err)
                        # the same bits on every rank
                        t = torch.from_numpy(np.ascontiguousarray(got).view(np.float64).reshape(-1).copy())
                        hi, lo = t.clone(), t.clone()
                        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
                        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
                        assert torch.equal(hi, t) and torch.equal(lo, t), what
                        if spec[1] == IDENTICAL:  # antisymmetric on a divided lattice too: the all-reduce adds images to images
                            ax = (0, 2, 1, 3) if mom is None else (0, 1, 3, 2, 4)
                            assert np.array_equal(got, -got.transpose(ax)), what
        dist.barrier()
    if rank == 0:
        print("DIST_BASIS_SLICE_TRIPLE_OK", world, runs, "max err %.2e" % worst)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
