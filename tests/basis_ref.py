"""numpy restatement of the products with a basis of another width (include/blockcg_hip.h: bcg_basis_dot, bcg_basis_axpy,
bcg_field_copy_columns) and of the deflated solve built on them.  Host arrays are the ABI's: a field is [V, m, 3]
([site, column, colour]); K x m matrices are ordinary (row, column) arrays.  The basis is the concatenation of the host
arrays of V along the column axis; the products are one einsum each."""
import functools

import numpy as np


def concat(V):
    return np.concatenate([np.asarray(v) for v in V], axis=1)


def basis_dot(V, b):
    """C[i, j] = sum_{x, c} conj(V_i(x, c)) b_j(x, c), (K, m)"""
    return np.einsum("xic,xjc->ij", np.conj(concat(V)), b)


def basis_axpy(y, V, C, beta=1.0):
    """beta y + V C; beta == 0 does not read y"""
    vc = np.einsum("xic,ij->xjc", concat(V), np.asarray(C))
    return vc if beta == 0 else beta * y + vc


def dot_scale(V, b):
    """sqrt(|V_i|^2 |b_j|^2), (K, m): what an entry of basis_dot is small or large against"""
    W = concat(V)
    nv = np.einsum("xic,xic->i", np.conj(W), W).real
    nb = np.einsum("xjc,xjc->j", np.conj(b), b).real
    return np.sqrt(np.outer(nv, nb))


def random_field(rng, V, m):
    return rng.uniform(-1, 1, (V, m, 3)) + 1j * rng.uniform(-1, 1, (V, m, 3))


def random_links(rng, V, ndim):
    """every real component uniform in [-1, 1), as gauge_field.setRandom draws them"""
    return rng.uniform(-1, 1, (V, ndim, 3, 3)) + 1j * rng.uniform(-1, 1, (V, ndim, 3, 3))


def split_columns(W, widths):
    """[V, K, 3] -> contiguous fields of the given widths"""
    out, o = [], 0
    for w in widths:
        out.append(np.ascontiguousarray(W[:, o:o + w]))
        o += w
    assert o == W.shape[1]
    return out


# ---- the deflated solve ------------------------------------------------------------------------------------------------
def to_vec(f):
    """[V, m, 3] -> [3 V, m], row index 3 x + c"""
    return np.ascontiguousarray(f.transpose(0, 2, 1)).reshape(f.shape[0] * 3, f.shape[1])


def to_field(v):
    return np.ascontiguousarray(v.reshape(v.shape[0] // 3, 3, v.shape[1]).transpose(0, 2, 1))


def dense_operator(U, dims, mass, hop_by_lines):
    """A = mass^2 - D^2 (dirac_op::op) as a dense (3 V, 3 V) matrix from the hop given (conftest.hop_by_lines)"""
    V = int(np.prod(dims))
    n = 3 * V
    eye = to_field(np.eye(n, dtype=np.complex128))
    D = to_vec(hop_by_lines(U, list(dims), eye))
    return mass * mass * np.eye(n) - D @ D


def bcgrq(A, B, eps, max_iterations=10000):
    """inc/block_solvers.hpp:50-86 with numpy's QR: X, operator applications.  The residual measure is the reference's:
    row norms of delta against those of the first delta."""
    X = np.zeros_like(B)
    Q, delta = np.linalg.qr(B)
    P = Q.copy()
    norms = np.linalg.norm(delta, axis=1)
    it, residual = 0, 1.0
    while residual > eps and it < max_iterations:
        T = A @ P
        it += 1
        alpha = np.linalg.inv(P.conj().T @ T)
        Q, rho = np.linalg.qr(Q - T @ alpha)
        X += P @ (alpha @ delta)
        P = P @ rho.conj().T + Q
        delta = rho @ delta
        residual = np.max(np.linalg.norm(delta, axis=1) / norms)
    return X, it


def deflated_bcgrq(A, B, W, evals, sigma, eps):
    """(A + sigma)^-1 B with the span of the orthonormal W ([n, K], eigenvalues evals of A) taken out of the Krylov solve"""
    C = W.conj().T @ B
    X, it = bcgrq(A + sigma * np.eye(A.shape[0]), B - W @ C, eps)
    return X + W @ (C / (evals + sigma)[:, None]), it


DEFLATION_DIMS = (4, 4, 4, 2)
DEFLATION_M = 8
DEFLATION_WIDTHS = (32, 16)
DEFLATION_MASS = 0.05
DEFLATION_SIGMA = (0.0, 0.05, 0.5)
DEFLATION_EPS = 1e-10
DEFLATION_SEED = 20261


@functools.lru_cache(maxsize=1)
def deflation_problem():
    """The input shared by tests/test_basis_cpu.py and tests/test_basis.py: links, the dense operator, its lowest
    K = sum(DEFLATION_WIDTHS) eigenpairs and a right-hand side."""
    from conftest import hop_by_lines
    rng = np.random.default_rng(DEFLATION_SEED)
    V = int(np.prod(DEFLATION_DIMS))
    U = random_links(rng, V, len(DEFLATION_DIMS))
    B = random_field(rng, V, DEFLATION_M)
    A = dense_operator(U, DEFLATION_DIMS, DEFLATION_MASS, hop_by_lines)
    A = 0.5 * (A + A.conj().T)
    evals, vecs = np.linalg.eigh(A)
    K = sum(DEFLATION_WIDTHS)
    return dict(U=U, B=B, A=A, evals=evals[:K].copy(), W=np.ascontiguousarray(vecs[:, :K]))
