"""numpy restatement of the covariant nearest-neighbour sum (include/blockcg_hip.h: bcg_dirac_shift_sum) by explicit
global coordinates:

    (S psi)(x) = c0 psi(x) + sum_mu s_mu(x) [ f_mu U_mu(x) psi(x+mu) + b_mu U_mu(x-mu)^dagger psi(x-mu) ]

Host layouts: psi [V, m, 3], U [V, ndim, 3, 3] with U[x, mu, k, r] = U_mu(x)(r, k), sites lexicographic with x_0 fastest.
Neighbours are gathered through a table built from coordinate tuples; no site-index stride is shared with the kernels."""
import itertools

import numpy as np


def coordinates(dims):
    """[V, ndim]: row s = the coordinates of site s (x_0 fastest)."""
    c = np.array(list(itertools.product(*[range(d) for d in reversed(dims)])), dtype=np.int64).reshape(-1, len(dims))[:, ::-1]
    return np.ascontiguousarray(c)


def neighbours(dims, mu, step):
    """site index of x + step * mu-hat (periodic), looked up by coordinate tuple."""
    coords = coordinates(dims)
    index = {tuple(c): s for s, c in enumerate(coords)}
    out = np.empty(len(coords), dtype=np.int64)
    for s, c in enumerate(coords):
        y = list(c)
        y[mu] = (y[mu] + step) % dims[mu]
        out[s] = index[tuple(y)]
    return out


def _vec(v, nd):
    if v is None:
        return np.zeros(nd, dtype=np.complex128)
    a = np.asarray(v, dtype=np.complex128)
    return np.full(nd, complex(a)) if a.ndim == 0 else a


def shift_sum(U, dims, psi, c0=0.0, fwd=None, bwd=None, eta=False):
    nd = len(dims)
    fwd, bwd = _vec(fwd, nd), _vec(bwd, nd)
    coords = coordinates(dims)
    out = complex(c0) * psi if complex(c0) != 0 else np.zeros_like(psi)
    for mu in range(nd):
        if fwd[mu] == 0 and bwd[mu] == 0:
            continue
        s = np.where(coords[:, :mu].sum(axis=1) % 2 == 1, -1.0, 1.0) if eta else np.ones(len(coords))
        if fwd[mu] != 0:
            xf = neighbours(dims, mu, +1)
            # (U psi)[x, j, r] = sum_k U(r, k) psi[x+mu, j, k] = sum_k U[x, mu, k, r] psi[xf, j, k]
            out = out + (fwd[mu] * s)[:, None, None] * np.einsum("xkr,xjk->xjr", U[:, mu], psi[xf])
        if bwd[mu] != 0:
            xb = neighbours(dims, mu, -1)
            # (U^dagger psi)[x, j, r] = sum_k conj(U_b(k, r)) psi[x-mu, j, k] = sum_k conj(U[xb, mu, r, k]) psi[xb, j, k]
            out = out + (bwd[mu] * s)[:, None, None] * np.einsum("xrk,xjk->xjr", np.conj(U[xb, mu]), psi[xb])
    return out


def laplacian(U, dims, psi, dir=-1):
    hop = np.ones(len(dims), dtype=np.complex128)
    if dir >= 0:
        hop[dir] = 0
    return shift_sum(U, dims, psi, -2.0 * (len(dims) - (1 if dir >= 0 else 0)), hop, hop)


def smear(U, dims, psi, dir, kappa, n_iter):
    hop = np.full(len(dims), kappa, dtype=np.complex128)
    if dir >= 0:
        hop[dir] = 0
    c0 = 1.0 - 2.0 * kappa * (len(dims) - (1 if dir >= 0 else 0))
    for _ in range(n_iter):
        psi = shift_sum(U, dims, psi, c0, hop, hop)
    return psi


def parity_mask(dims, parity):
    """sites of global parity `parity` in lexicographic order: the sites a half field of that parity holds, in its order."""
    return coordinates(dims).sum(axis=1) % 2 == parity


def random_field(rng, V, m):
    return rng.normal(size=(V, m, 3)) + 1j * rng.normal(size=(V, m, 3))


def random_links(rng, dims):
    V = int(np.prod(dims))
    return rng.uniform(-1, 1, size=(V, len(dims), 3, 3)) + 1j * rng.uniform(-1, 1, size=(V, len(dims), 3, 3))


def unitary_links(rng, dims):
    V = int(np.prod(dims))
    z = rng.normal(size=(V, len(dims), 3, 3)) + 1j * rng.normal(size=(V, len(dims), 3, 3))
    q, _ = np.linalg.qr(z)
    return np.ascontiguousarray(q)
