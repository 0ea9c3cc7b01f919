"""numpy restatement of the low-mode eigensolver (include/blockcg_hip.h: bcg_basis_rotate, bcg_spectral_bound,
bcg_lowest_modes), step for step as blockcg_amd/csrc/capi_lowmodes.hip composes it.  The operator is a dense Hermitian
matrix A ([n, n], n = 3 x sites, rows as basis_ref.to_vec orders them), a block is an [n, K] array; the input and the layouts
are those of basis_ref."""
import functools

import numpy as np

import basis_ref as ref


def rotate(V, Q):
    """host fields V (a list of [sites, w, 3]) times Q ([K, K]): the fields of V Q, same widths"""
    out = np.einsum("xic,ij->xjc", ref.concat(V), np.asarray(Q))
    return ref.split_columns(out, [v.shape[1] for v in V])


def lanczos_bound(A, v0, steps):
    """theta_max(T_k) + beta_k after k = steps Lanczos steps from v0 (Zhou & Saad's safeguarded bound)"""
    v = v0 / np.linalg.norm(v0)
    vp = np.zeros_like(v)
    alpha, beta = [], []
    for j in range(steps):
        w = A @ v
        if j > 0:
            w = w - beta[-1] * vp
        alpha.append(np.vdot(v, w).real)
        w = w - alpha[-1] * v
        beta.append(np.linalg.norm(w))
        if beta[-1] <= 1e-14 * abs(alpha[0]):
            break
        vp, v = v, w / beta[-1]
    k = len(alpha)
    T = np.diag(alpha) + np.diag(beta[:k - 1], 1) + np.diag(beta[:k - 1], -1)
    return np.linalg.eigvalsh(T)[-1] + beta[-1]


def _herm(M):
    return 0.5 * (M + M.conj().T)


def ortho_ritz(A, V, L=None):
    """project out L, Cholesky-orthonormalise; the same again with the reduced eigenproblem in the second rotation"""
    for p in range(2):
        if L is not None:
            V = V - L @ (L.conj().T @ V)
        G = _herm(V.conj().T @ V)
        R = np.linalg.cholesky(G).conj().T  # upper, G = R^dagger R
        Rinv = np.linalg.inv(R)
        if p == 0:
            V = V @ Rinv
            continue
        H = _herm(V.conj().T @ (A @ V))
        theta, Z = np.linalg.eigh(Rinv.conj().T @ H @ Rinv)
        V = V @ (Rinv @ Z)
    return V, theta


def chebyshev_filter(A, V, degree, theta_1, lo, ub):
    c, e = 0.5 * (ub + lo), 0.5 * (ub - lo)
    sigma1 = e / (theta_1 - c)
    prev, cur = V, (sigma1 / e) * (A @ V - c * V)
    sigma = sigma1
    for _ in range(2, degree + 1):
        sigma_n = 1.0 / (2.0 / sigma1 - sigma)
        prev, cur = cur, (2.0 * sigma_n / e) * (A @ cur - c * cur) - (sigma * sigma_n) * prev
        sigma = sigma_n
    return cur


def guard_columns(K, n_want):
    """the guard block a call carries when the caller brings no spare columns (n_want == K): min(16, 64 - K) columns"""
    return min(16, 64 - K) if n_want == K else 0


def chfsi(A, V0, n_want, degree, ub, tol, max_iterations, L=None, nv=1, guard=None):
    """Returns dict(V, evals, resid, iterations, applications, cond): iterations counts filter applications, applications the
    calls of the block operator for a basis held as nv fields, cond the largest cond(V^dagger V) met in a first pass.
    guard: the [n, guard_columns(K, n_want)] start of the guard block (the device draws noise); it is carried behind V as one
    more field and dropped at the end, V keeps the lowest K Ritz vectors."""
    V = np.array(V0, dtype=np.complex128)
    K = V.shape[1]
    g = guard_columns(K, n_want)
    if g:
        assert guard is not None and guard.shape == (V.shape[0], g)
        V, nv = np.concatenate([V, guard], axis=1), nv + 1
    iterations, worst_cond = 0, 1.0
    while True:
        worst_cond = max(worst_cond, np.linalg.cond(V.conj().T @ V))
        V, theta = ortho_ritz(A, V, L)
        resid = np.linalg.norm(A @ V - V * theta[None, :], axis=0)
        if resid[:n_want].max() <= tol * ub or iterations >= max_iterations:
            break
        V = chebyshev_filter(A, V, degree, theta[0], theta[-1], ub)
        iterations += 1
    V, theta, resid = V[:, :K], theta[:K], resid[:K]
    return dict(V=V, evals=theta, resid=resid, iterations=iterations,
                applications=nv * (2 * (iterations + 1) + degree * iterations), cond=worst_cond)


# ---- the shared input: basis_ref.deflation_problem() and one start block ---------------------------------------------------
LOWMODES_WIDTHS = (32, 16)
LOWMODES_WANT = 32
LOWMODES_DEGREE = 16
LOWMODES_TOL = 1e-10
LOWMODES_STEPS = 10
LOWMODES_SEED = 4711


@functools.lru_cache(maxsize=1)
def lowmodes_problem():
    """A, all its eigenvalues, the 10-step bound and the start blocks of the first stage (V0) and of the locked second
    stage (V1), computed once."""
    p = ref.deflation_problem()
    A = p["A"]
    n = A.shape[0]
    rng = np.random.default_rng(LOWMODES_SEED)
    v0 = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    K = sum(LOWMODES_WIDTHS)
    V0 = rng.standard_normal((n, K)) + 1j * rng.standard_normal((n, K))
    V1 = rng.standard_normal((n, K)) + 1j * rng.standard_normal((n, K))
    return dict(A=A, U=p["U"], evals=np.linalg.eigvalsh(A), ub=lanczos_bound(A, v0, LOWMODES_STEPS), V0=V0, V1=V1)


@functools.lru_cache(maxsize=1)
def first_stage():
    p = lowmodes_problem()
    return chfsi(p["A"], p["V0"], LOWMODES_WANT, LOWMODES_DEGREE, p["ub"], LOWMODES_TOL, 100, nv=len(LOWMODES_WIDTHS))
