"""numpy restatement of bcg_laplacian_modes (include/blockcg_hip.h), step for step as blockcg_amd/csrc/capi_lowmodes.hip
composes it: lowmodes_ref.ortho_ritz slice by slice, residuals by slice, and ONE Chebyshev filter for all slices on the
interval [max_t theta_last(t), ub] scaled at min_t theta_1(t).  The operator is the dense A = -Lap_dir of
shift_sum_ref.laplacian ([n, n], n = 3 x sites, rows as basis_ref.to_vec orders them); a block is an [n, K] array and slice t
owns the rows rows[t]."""
import functools

import numpy as np

import basis_ref as ref
import lowmodes_ref as lm
import shift_sum_ref as ss
from basis_slice_axpy_ref import slice_of_sites


def dense_minus_laplacian(U, dims, direction):
    """A = -Lap_dir as a dense (3 V, 3 V) matrix, column by column through shift_sum_ref.laplacian"""
    n = 3 * int(np.prod(dims))
    eye = ref.to_field(np.eye(n, dtype=np.complex128))
    return -ref.to_vec(ss.laplacian(U, list(dims), eye, direction))


def slice_rows(dims, direction):
    """rows[t]: the row indices 3 x + c of the sites of slice t, ascending"""
    t = slice_of_sites(list(dims), direction)
    return [np.flatnonzero(np.repeat(t == s, 3)) for s in range(dims[direction])]


def chfsi(A, rows, V0, n_want, degree, ub, tol, max_iterations, L=None, nv=1, guard=None, per_slice_intervals=False):
    """Returns dict(V, evals [L_dir, K], resid [L_dir, K], iterations, applications).  per_slice_intervals: every slice filtered
    on its own interval [theta_last(t), ub] scaled at theta_1(t) -- what the device does NOT do, kept for the comparison of
    the iteration counts."""
    V = np.array(V0, dtype=np.complex128)
    K = V.shape[1]
    g = lm.guard_columns(K, n_want)
    if g:
        assert guard is not None and guard.shape == (V.shape[0], g)
        V, nv = np.concatenate([V, guard], axis=1), nv + 1
    blocks = [A[np.ix_(r, r)] for r in rows]
    theta = np.zeros((len(rows), V.shape[1]))
    resid = np.zeros_like(theta)
    iterations = 0
    while True:
        for t, r in enumerate(rows):
            V[r], theta[t] = lm.ortho_ritz(blocks[t], V[r], None if L is None else L[r])
            resid[t] = np.linalg.norm(blocks[t] @ V[r] - V[r] * theta[t][None, :], axis=0)
        if resid[:, :n_want].max() <= tol * ub or iterations >= max_iterations:
            break
        if per_slice_intervals:
            for t, r in enumerate(rows):
                V[r] = lm.chebyshev_filter(blocks[t], V[r], degree, theta[t, 0], theta[t, -1], ub)
        else:
            V = lm.chebyshev_filter(A, V, degree, theta[:, 0].min(), theta[:, -1].max(), ub)
        iterations += 1
    return dict(V=V[:, :K], evals=theta[:, :K].copy(), resid=resid[:, :K].copy(), iterations=iterations,
                applications=nv * (2 * (iterations + 1) + degree * iterations))


# ---- the shared inputs -----------------------------------------------------------------------------------------------------
WIDTHS = (32, 16)
WANT = 32
DEGREE = 16
TOL = 1e-10
SEED = 8111
CASES = (((4, 4, 4, 3), 3), ((3, 4, 4, 4), 0))


@functools.lru_cache(maxsize=None)
def problem(dims, direction, unitary=True):
    """links, the dense A, the rows and all eigenvalues of every slice, the bound and the start blocks V0 (first stage), V1
    (the locked stage and the guard block), computed once per case.  Unitary links: ub = 4 (ndim - 1) = 12; general links:
    1.02 lambda_max."""
    rng = np.random.default_rng(SEED + direction + (0 if unitary else 100))
    U = ss.unitary_links(rng, list(dims)) if unitary else ss.random_links(rng, list(dims))
    A = dense_minus_laplacian(U, dims, direction)
    rows = slice_rows(dims, direction)
    evals = np.stack([np.linalg.eigvalsh(0.5 * (A[np.ix_(r, r)] + A[np.ix_(r, r)].conj().T)) for r in rows])
    n, K = A.shape[0], sum(WIDTHS)
    V0 = rng.standard_normal((n, K)) + 1j * rng.standard_normal((n, K))
    V1 = rng.standard_normal((n, K)) + 1j * rng.standard_normal((n, K))
    ub = 4.0 * (len(dims) - 1) if unitary else 1.02 * evals.max()
    return dict(U=U, A=A, rows=rows, evals=evals, ub=ub, V0=V0, V1=V1)


@functools.lru_cache(maxsize=None)
def first_stage(dims, direction, unitary=True):
    p = problem(dims, direction, unitary)
    return chfsi(p["A"], p["rows"], p["V0"], WANT, DEGREE, p["ub"], TOL, 100, nv=len(WIDTHS))
