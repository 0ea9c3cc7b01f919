"""Rerun reproducibility: the Gram products are reduced in a fixed order whatever the order in which the blocks finish
(mfma_common.hpp: gram_fold, the block partials of the stencil and of phase B; launch_reduce_partials for hermitian_dot), so
the same solve gives the same bits on every run.  A stale or missed partial in the fold would not fail a convergence test --
CG absorbs a wrong Gram matrix as extra iterations -- but it shows up here as a coefficient that differs between runs.
Each case runs the same seeded work in a first context, in a second, fresh one, and once more in the first."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHIFTS = [0.0, 1e-3, 0.1, 2.0]
KEYS = ("alpha", "rho", "delta", "alpha_s", "beta_s", "residual", "residual_shift")


@pytest.fixture(scope="module")
def bc():
    import blockcg_amd
    return blockcg_amd


def _solve(bc, ctx, m, iters, seed):
    D = bc.dirac_op(ctx, 0.2, seed=seed)
    B = bc.block_fermion_field(ctx, m).setRandom(seed=seed + 1)
    X = [bc.block_fermion_field(ctx, m) for _ in SHIFTS]
    info = bc.SBCGrQ(X, B, D, SHIFTS, 0.0, 0.0, max_iterations=iters, trace_limit=iters, return_info=True)
    assert info["iterations"] == iters
    return info, X


# 32^4 at m = 16: phase B (batched) and the stencil's fused Gram product fold the partials of hundreds of blocks; the ragged
# lattice (3V = 11340 rows, a partial last tile) runs k_phaseB at m = 32 over the default grid
@pytest.mark.parametrize("m,dims,iters", [(16, [32, 32, 32, 32], 20), (32, [18, 10, 7, 3], 8)], ids=["m16-32^4", "m32-18x10x7x3"])
def test_solve_is_bitwise_reproducible(bc, m, dims, iters):
    """Gap 4: the same seeded fixed-work solve in two fresh contexts and once more in the first: every trace entry, every X_s
    and the residual equal bit for bit."""
    ctx1 = bc.Context(dims)
    first, X1 = _solve(bc, ctx1, m, iters, seed=81)
    X1h = [x.download() for x in X1]
    del X1
    assert 0 < first["residual"] < 1.0  # the solve did something
    ctx2 = bc.Context(dims)
    for which, ctx in (("fresh context", ctx2), ("first context again", ctx1)):
        info, X = _solve(bc, ctx, m, iters, seed=81)
        assert info["residual"] == first["residual"], which
        for key in KEYS:
            assert np.array_equal(info["trace"][key], first["trace"][key]), (which, key)
        for s in range(len(SHIFTS)):
            assert np.array_equal(X[s].download(), X1h[s]), (which, s)
        del X
    ctx2.close()
    ctx1.close()


@pytest.mark.parametrize("m,dims", [(16, [32, 32, 32, 32]), (32, [18, 10, 7, 3])], ids=["m16-32^4", "m32-18x10x7x3"])
def test_hermitian_dot_is_bitwise_reproducible(bc, m, dims):
    """Gap 4: hermitian_dot of a large field twice in one context and once in another: the same bits."""
    ctx1 = bc.Context(dims)
    a = bc.block_fermion_field(ctx1, m).setRandom(seed=91)
    b = bc.block_fermion_field(ctx1, m).setRandom(seed=92)
    G = [a.hermitian_dot(b), a.hermitian_dot(b), a.hermitian_dot(a)]
    ctx2 = bc.Context(dims)
    a2 = bc.block_fermion_field(ctx2, m).setRandom(seed=91)
    b2 = bc.block_fermion_field(ctx2, m).setRandom(seed=92)
    G2 = [a2.hermitian_dot(b2), a2.hermitian_dot(a2)]
    assert np.abs(G[0]).max() > 0
    assert np.array_equal(G[0], G[1]) and np.array_equal(G[0], G2[0]) and np.array_equal(G[2], G2[1])
    ctx2.close()
    ctx1.close()
