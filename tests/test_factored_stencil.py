"""Phase A at m = 16 as the factored stencil pair (capi_operator.hip: plan_pair, pair_first_factor, pair_second_factor):
A + sigma_0 = mu^2 - D^2 = (mu + D)(mu - D), W = (mu - D) P_0, T = (mu + D) W, G = W^dagger W, so that the second stencil pass
reads no P_0.  BCG_HOP_FACTORED=0 keeps the other form (tmp = D P_0, T = (m^2 + sigma_0) P_0 - D tmp, G = P_0^dagger T).

Shapes: 16 x 8 x 8 x 8 with patches of 16 x 2 x 2 -- every site is next to a periodic wrap, a patch border or the first or
last x3 slice -- and 32 x 8 x 8 x 6: two tiles in x0, an x3 extent that is no power of two.

Bound between the two forms (on against off): how far two legitimately different roundings of the same solve drift in
6 iterations at these inputs, measured on the CPU with the oracle, times 10.  The oracle's operator has one term order, but
its site sums have three: the reference's sequential order, 8 host threads (set_threads) and pairwise sums
(set_gram_arith(1)).  Against the sequential order, over both shapes, both masses and both sets of shifts, the traces
and X_s differ by 5.5e-15 to 9.0e-15 (threads) and 5.7e-15 to 7.8e-15 (pairwise): FORM_BOUND = 10 x 9.0e-15.
Measured on the GPU, on against off: 5e-17 to 8e-16."""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest

from conftest import TOL_COEFF, rel_err

pytestmark = pytest.mark.gpu

M = 16
SHAPES = {"16x8x8x8": [16, 8, 8, 8], "32x8x8x6": [32, 8, 8, 6]}
SHIFTS = (0.0, 1e-3, 0.1)
ITERS = 6
KEYS = ("alpha", "rho", "delta", "alpha_s", "beta_s")
FORM_BOUND = 9e-14
SEED_U, SEED_B = 171, 172


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _inputs(shape, m):
    import oracle
    orc = oracle.Oracle()
    dims = SHAPES.get(shape) or [int(d) for d in shape.split("x")]
    U = orc.fill_gauge(dims, SEED_U)
    Bh = orc.fill_field(m, int(np.prod(dims)), SEED_B)
    for a in (U, Bh):
        a.setflags(write=False)
    return dims, U, Bh


@functools.lru_cache(maxsize=None)
def _oracle(shape, mass, shifts):
    import oracle
    dims, U, Bh = _inputs(shape, M)
    return oracle.Oracle().sbcgrq(U, dims, mass, Bh, list(shifts), 0.0, 0.0, max_iterations=ITERS, trace_limit=ITERS)


@functools.lru_cache(maxsize=None)
def _solve(shape, mass, shifts, factored, m=M, ring=0):
    """ITERS iterations of SBCGrQ with the switch as given: (X_s, trace, profile, G of the last phase A)."""
    import blockcg_amd as bc
    dims, U, Bh = _inputs(shape, m)
    with _env(BCG_HOP_FACTORED=int(factored), BCG_HOP_PATCH="16,2,2", BCG_HOP_BLOCKS="32"):
        ctx = bc.Context(dims)
    ctx.capacity_mode(ring)
    ctx.profiling(True)
    D = bc.dirac_op(ctx, mass, U=U)
    B = bc.block_fermion_field(ctx, m, Bh)
    X = [bc.block_fermion_field(ctx, m) for _ in shifts]
    info = bc.SBCGrQ(X, B, D, list(shifts), 0.0, 0.0, max_iterations=ITERS, trace_limit=ITERS, return_info=True)
    G = np.zeros((m, m), dtype=np.complex128)  # column-major from the library: G[j, i] here is G(i, j)
    ctx.lib.bcg_debug_phase_a_gram.restype = ctypes.c_int
    ctx.lib.bcg_debug_phase_a_gram.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    assert ctx.lib.bcg_debug_phase_a_gram(ctx.h, m, G.ctypes.data_as(ctypes.c_void_p)) == 0
    return [x.download() for x in X], info["trace"], ctx.profile(), G.T.copy()


def _count(prof, key):
    return prof.get(key, {}).get("count", 0)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_factored_pair_runs_when_on_and_not_when_off(shape):
    on, off = (_solve(shape, 0.2, SHIFTS, f)[2] for f in (True, False))
    for prof in (on, off):  # the same profile classes either way, one launch of each per application, all on the bundle sweep
        n = _count(prof, "hop")
        assert n >= ITERS and _count(prof, "hop_shifted_gram") == n, sorted(prof)
        assert _count(prof, "stencil_form_k_hop4b") == 2 * n and "stencil_form_k_hop4c" not in prof
    n = _count(on, "hop")
    assert _count(off, "hop") == n and _count(on, "stencil_form_factored_pair") == n
    assert "stencil_form_factored_pair" not in off
    # the second pass is booked with the first pass's streams: two field passes and the links, not three
    assert on["hop_shifted_gram"]["bytes"] == on["hop"]["bytes"] == off["hop"]["bytes"]
    V = int(np.prod(SHAPES[shape]))
    assert off["hop_shifted_gram"]["bytes"] - on["hop_shifted_gram"]["bytes"] == pytest.approx(n * V * 48.0 * M, rel=1e-12)


@pytest.mark.parametrize("mass", [0.2, 1e-3])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_factored_pair_against_the_oracle(shape, mass):
    X, trace, prof, _ = _solve(shape, mass, SHIFTS, True)
    assert _count(prof, "stencil_form_factored_pair") >= ITERS
    o = _oracle(shape, mass, SHIFTS)
    for key in KEYS:
        e = rel_err(trace[key], o["trace"][key])
        print(f"{shape} mass {mass} factored vs oracle {key}: {e:.3e}")
        assert e < TOL_COEFF, key
    for s in range(len(SHIFTS)):
        e = rel_err(X[s], o["X"][s])
        print(f"{shape} mass {mass} factored vs oracle X[{s}]: {e:.3e}")
        assert e < 1e-10, s


@pytest.mark.parametrize("mass", [0.2, 1e-3])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_factored_pair_against_the_other_form(shape, mass):
    on, off = (_solve(shape, mass, SHIFTS, f) for f in (True, False))
    worst = 0.0
    for key in KEYS:
        e = rel_err(on[1][key], off[1][key])
        print(f"{shape} mass {mass} on vs off {key}: {e:.3e}")
        worst = max(worst, e)
    for s in range(len(SHIFTS)):
        e = rel_err(on[0][s], off[0][s])
        print(f"{shape} mass {mass} on vs off X[{s}]: {e:.3e}")
        worst = max(worst, e)
    assert 0.0 < worst < FORM_BOUND  # (not bit-identical: another rounding of the same operator)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_gram_matrix_of_the_factored_pair_is_hermitian_positive(shape):
    """G = W^dagger W as the host used it in the last phase A (bcg_debug_phase_a_gram): exactly Hermitian with an exactly
    real, positive diagonal -- the lower triangle is mirrored and the imaginary rounding residue of the self-product's
    diagonal dropped -- and positive definite.  It is the matrix the solver inverted (the last alpha of the trace, to the
    rounding of an m x m inversion: 16 m eps cond(G)), and the other form's P_0^dagger T of the same iteration to the
    bound between the two forms."""
    _, trace, _, G = _solve(shape, 0.2, SHIFTS, True)
    assert np.array_equal(G, G.conj().T)
    d = np.diagonal(G)
    assert np.all(d.imag == 0.0) and np.all(d.real > 0.0)
    assert np.linalg.eigvalsh(G).min() > 0.0
    tol = 16 * M * np.finfo(np.float64).eps * np.linalg.cond(G)
    e = np.linalg.norm(trace["alpha"][-1] @ G - np.eye(M))
    print(f"{shape}: |alpha G - 1| = {e:.3e}, bound {tol * np.sqrt(M):.3e}")
    assert e < tol * np.sqrt(M)  # (Frobenius norm of the identity: sqrt(m))
    G_off = _solve(shape, 0.2, SHIFTS, False)[3]
    assert np.array_equal(np.triu(G_off, 1), np.conj(np.tril(G_off, -1)).T)
    e = rel_err(G, G_off)
    print(f"{shape}: G on vs off {e:.3e}, largest |Im G_ii| / |G_ii| of the other form {np.abs(np.diagonal(G_off).imag / np.diagonal(G_off).real).max():.3e}")
    assert 0.0 < e < FORM_BOUND


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_factored_pair_with_a_positive_first_shift(shape):
    """sigma_0 > 0: mu = sqrt(m^2 + sigma_0) is not the mass."""
    shifts, mass = (0.05, 0.3), 0.2
    X, trace, prof, _ = _solve(shape, mass, shifts, True)
    assert _count(prof, "stencil_form_factored_pair") >= ITERS
    o = _oracle(shape, mass, shifts)
    for key in KEYS:
        assert rel_err(trace[key], o["trace"][key]) < TOL_COEFF, key
    for s in range(len(shifts)):
        assert rel_err(X[s], o["X"][s]) < 1e-10, s
    Xoff, toff, _, _ = _solve(shape, mass, shifts, False)
    assert max(rel_err(trace[k], toff[k]) for k in KEYS) < FORM_BOUND
    assert max(rel_err(X[s], Xoff[s]) for s in range(len(shifts))) < FORM_BOUND


@pytest.mark.parametrize("shape,m,ring", [("16x8x4x8", 8, 0), ("16x8x8x8", 16, 4)], ids=["m8", "capacity-ring4"])
def test_other_widths_and_capacity_mode_keep_their_kernels(shape, m, ring):
    on, off = (_solve(shape, 0.2, SHIFTS, f, m, ring) for f in (True, False))
    assert "stencil_form_factored_pair" not in on[2] and "stencil_form_factored_pair" not in off[2]
    for s in range(len(SHIFTS)):
        assert np.array_equal(on[0][s], off[0][s]), s
    for key in KEYS:
        assert np.array_equal(on[1][key], off[1][key]), key
