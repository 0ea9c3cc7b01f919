"""The Gram product of the factored pair's second factor as a self-product (mfma_common.hpp: gram_self_step,
gram_self_block_store): G = W^dagger W with Im G = C - C^T, C = x^T y, and Re G = P - (C + C^T),
P = (x + y)^T (x + y) -- two real matrix products per colour instead of four (three, Re G = x^T x + y^T y, in builds with
-DBCG_SELF_GRAM_3M).  The kernel antisymmetrises Im G in every block partial, so the matrix the device sums is Hermitian
with a real diagonal before the host touches it.  These tests hold for either form at the same bounds.

Shapes and patches as in test_factored_stencil.py: 16 x 8 x 8 x 8 and 32 x 8 x 8 x 6 (an x3 extent that is no multiple of
the pacing window) with BCG_HOP_PATCH=16,2,2, so that the bundle sweep and the factored pair are taken.

Bounds.  Against bcg_dirac_apply (the unfactored kernels) and hermitian_dot: TOL_KERNEL = 1e-13, the project's constant
for one kernel's output against another route to the same numbers.  Against BCG_HOP_FACTORED=0 over 6 iterations:
FORM_BOUND = 9e-14 of test_factored_stencil.py (ten times the oracle's own drift between its summation orders at these
inputs), imported from there so that the two files cannot drift apart."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import TOL_KERNEL, rel_err
from test_factored_stencil import FORM_BOUND, ITERS, KEYS, M, SHAPES, SHIFTS, _count, _env, _inputs
from test_factored_stencil import _solve as _solve_form

pytestmark = pytest.mark.gpu

MASSES = (0.2, 1e-3)


def _context(dims, factored=True):
    import blockcg_amd as bc
    with _env(BCG_HOP_FACTORED=int(factored), BCG_HOP_PATCH="16,2,2", BCG_HOP_BLOCKS="32"):
        ctx = bc.Context(dims)
    ctx.profiling(True)
    return ctx


def _raw_gram(ctx):
    """The Gram matrix of the last phase A as the device summed it (no mirror, no diagonal fix), G[i, j] = G(i, j)."""
    G = np.zeros((M, M), dtype=np.complex128)  # column-major from the library
    fn = ctx.lib.bcg_debug_phase_a_gram_raw
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    assert fn(ctx.h, M, G.ctypes.data_as(ctypes.c_void_p)) == 0
    return G.T.copy()


def _assert_factored_bundle(prof, n_min):
    """From the profile's kernel classes: every application was the factored pair, both passes on the bundle sweep."""
    n = _count(prof, "hop")
    assert n >= n_min and _count(prof, "hop_shifted_gram") == n, sorted(prof)
    assert _count(prof, "stencil_form_factored_pair") == n, sorted(prof)
    assert _count(prof, "stencil_form_k_hop4b") == 2 * n and "stencil_form_k_hop4c" not in prof, sorted(prof)


@functools.lru_cache(maxsize=None)
def _first_iteration(shape, mass):
    """One iteration of SBCGrQ: (raw device G of its phase A, P_0^dagger (A + sigma_0) P_0 by the unfactored route, profile)."""
    import blockcg_amd as bc
    dims, U, Bh = _inputs(shape, M)
    ctx = _context(dims)
    D = bc.dirac_op(ctx, mass, U=U)
    B = bc.block_fermion_field(ctx, M, Bh)
    X = [bc.block_fermion_field(ctx, M) for _ in SHIFTS]
    bc.SBCGrQ(X, B, D, list(SHIFTS), 0.0, 0.0, max_iterations=1)
    prof = ctx.profile()
    G = _raw_gram(ctx)
    # the independent route: P_0 = Q of B = Q rho, T = (m^2 - D^2) P_0 by bcg_dirac_apply, G = P_0^dagger T + sigma_0 P_0^dagger P_0
    P = bc.block_fermion_field(ctx, M, Bh)
    P.thinQR()
    T = bc.block_fermion_field(ctx, M)
    D.op(T, P)
    G_ref = P.hermitian_dot(T)
    if SHIFTS[0] != 0.0:
        G_ref = G_ref + SHIFTS[0] * P.hermitian_dot(P)
    return G, G_ref, prof


@functools.lru_cache(maxsize=None)
def _solve_raw(shape, mass, run):
    """ITERS iterations, factored pair on: (X_s, trace, profile, raw device G of the last phase A).  `run` tells two
    solves of the same inputs apart."""
    import blockcg_amd as bc
    dims, U, Bh = _inputs(shape, M)
    ctx = _context(dims)
    D = bc.dirac_op(ctx, mass, U=U)
    B = bc.block_fermion_field(ctx, M, Bh)
    X = [bc.block_fermion_field(ctx, M) for _ in SHIFTS]
    info = bc.SBCGrQ(X, B, D, list(SHIFTS), 0.0, 0.0, max_iterations=ITERS, trace_limit=ITERS, return_info=True)
    return [x.download() for x in X], info["trace"], ctx.profile(), _raw_gram(ctx)


@pytest.mark.parametrize("mass", MASSES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_raw_device_gram_is_hermitian_by_construction(shape, mass):
    for G, prof, n in ((_first_iteration(shape, mass)[0], _first_iteration(shape, mass)[2], 1),
                       (_solve_raw(shape, mass, 0)[3], _solve_raw(shape, mass, 0)[2], ITERS)):
        _assert_factored_bundle(prof, n)
        d = np.diagonal(G)
        print(f"{shape} mass {mass}: max |Im G_ii| = {np.abs(d.imag).max():.3e}, max |G - G^dagger| = {np.abs(G - G.conj().T).max():.3e}")
        assert np.all(d.imag == 0.0)
        assert np.array_equal(G, G.conj().T)
        assert np.all(d.real > 0.0) and np.any(G.imag != 0.0)  # (a matrix was read, and a complex one)


@pytest.mark.parametrize("mass", MASSES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_first_gram_against_the_unfactored_route(shape, mass):
    G, G_ref, prof = _first_iteration(shape, mass)
    _assert_factored_bundle(prof, 1)
    e = rel_err(G, G_ref)
    print(f"{shape} mass {mass}: |G - P0^dagger T| / |P0^dagger T| = {e:.3e}")
    assert e <= TOL_KERNEL


@pytest.mark.parametrize("mass", MASSES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_two_solves_are_bit_identical(shape, mass):
    a, b = _solve_raw(shape, mass, 0), _solve_raw(shape, mass, 1)
    _assert_factored_bundle(a[2], ITERS)
    _assert_factored_bundle(b[2], ITERS)
    for s in range(len(SHIFTS)):
        assert np.array_equal(a[0][s], b[0][s]), s
    for key in KEYS:
        assert np.array_equal(a[1][key], b[1][key]), key
    assert np.array_equal(a[3], b[3])


@pytest.mark.parametrize("mass", MASSES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_solve_against_the_unfactored_form(shape, mass):
    on = _solve_raw(shape, mass, 0)
    _assert_factored_bundle(on[2], ITERS)
    off = _solve_form(shape, mass, SHIFTS, False)
    assert "stencil_form_factored_pair" not in off[2]
    worst = 0.0
    for key in KEYS:
        e = rel_err(on[1][key], off[1][key])
        print(f"{shape} mass {mass} self-product vs unfactored {key}: {e:.3e}")
        worst = max(worst, e)
    for s in range(len(SHIFTS)):
        e = rel_err(on[0][s], off[0][s])
        print(f"{shape} mass {mass} self-product vs unfactored X[{s}]: {e:.3e}")
        worst = max(worst, e)
    assert 0.0 < worst < FORM_BOUND
