"""numpy restatement of stout link smearing and the plaquette (include/blockcg_hip.h, "gauge links: stout smearing and
plaquettes"), the yardstick of test_stout_smear*.py.  Links are arrays M[site, mu, r, c] of mathematical matrices (row r,
column c); the library's host layout is [site, mu, c, r] (column-major), so to_lib / from_lib swap the last two axes.  Sites
are lexicographic, direction 0 fastest, periodic.

One step with three interchangeable exponentials of i Q (Q Hermitian, traceless): exp_eigh (eigendecomposition),
exp_taylor (scaling and squaring of the Taylor series) and exp_ch (Cayley-Hamilton, Morningstar and Peardon 2004, the form
the device kernel uses)."""
import numpy as np


def to_lib(M):
    return np.ascontiguousarray(np.swapaxes(M, -1, -2))


from_lib = to_lib


def dagger(M):
    return np.conj(np.swapaxes(M, -1, -2))


def _grid(dims):
    dims = list(dims)
    return dims, int(np.prod(dims))


def shift(F, dims, mu, sign):
    """F[x] -> F[x + sign * mu] for an array whose first axis is the site index"""
    dims, V = _grid(dims)
    shape = tuple(reversed(dims))  # axis of direction mu is ndim - 1 - mu
    A = F.reshape(shape + F.shape[1:])
    return np.roll(A, -sign, axis=len(dims) - 1 - mu).reshape(F.shape)


def rho_table(rho, ndim, dir=None):
    """scalar rho (on all pairs not involving dir) or an ndim x ndim table -> table with a zero diagonal"""
    r = np.asarray(rho, dtype=np.float64)
    if r.ndim == 0:
        t = np.full((ndim, ndim), float(r))
        if dir is not None and dir >= 0:
            t[dir, :] = 0.0
            t[:, dir] = 0.0
    else:
        t = r.reshape(ndim, ndim).copy()
    t[np.arange(ndim), np.arange(ndim)] = 0.0
    return t


# ---- exp(iQ) three ways -----------------------------------------------------------------------------------------
def exp_eigh(Q):
    w, v = np.linalg.eigh(Q)
    return np.einsum("...ik,...k,...jk->...ij", v, np.exp(1j * w), np.conj(v))


def exp_taylor(Q, terms=24):
    """exp(iQ) = (sum_k (iQ / 2^s)^k / k!)^(2^s), s chosen so that ||Q / 2^s|| <= 1/2"""
    Q = np.asarray(Q, dtype=np.complex128)
    nrm = np.sqrt(np.sum(np.abs(Q) ** 2, axis=(-1, -2)))
    big = float(nrm.max()) if nrm.size else 0.0
    s = max(0, int(np.ceil(np.log2(max(big, 1e-300) / 0.5)))) if big > 0.5 else 0
    A = 1j * Q / (2.0 ** s)
    one = np.broadcast_to(np.eye(3, dtype=np.complex128), Q.shape)
    E = one.copy()
    T = one.copy()
    for k in range(1, terms + 1):
        T = T @ A / k
        E = E + T
    for _ in range(s):
        E = E @ E
    return E


def ch_coefficients(Q):
    """f0, f1, f2 with exp(iQ) = f0 + f1 Q + f2 Q^2, by the guards of the header comment"""
    Q = np.asarray(Q, dtype=np.complex128)
    Q2 = Q @ Q
    c0 = np.real(
        Q[..., 0, 0] * (Q[..., 1, 1] * Q[..., 2, 2] - Q[..., 1, 2] * Q[..., 2, 1])
        - Q[..., 0, 1] * (Q[..., 1, 0] * Q[..., 2, 2] - Q[..., 1, 2] * Q[..., 2, 0])
        + Q[..., 0, 2] * (Q[..., 1, 0] * Q[..., 2, 1] - Q[..., 1, 1] * Q[..., 2, 0]))
    c1 = 0.5 * np.real(Q2[..., 0, 0] + Q2[..., 1, 1] + Q2[..., 2, 2])
    c1 = np.maximum(c1, 0.0)
    third = c1 / 3.0
    c0max = 2.0 * third * np.sqrt(third)
    neg = c0 < 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(c0max > 0.0, np.abs(c0) / np.where(c0max > 0.0, c0max, 1.0), 0.0)
    theta = np.arccos(np.clip(ratio, 0.0, 1.0))
    u = np.sqrt(third) * np.cos(theta / 3.0)
    w = np.sqrt(c1) * np.sin(theta / 3.0)
    u2, w2 = u * u, w * w
    small = np.abs(w) < 0.05
    with np.errstate(divide="ignore", invalid="ignore"):
        xi0 = np.where(small, 1.0 - w2 / 6.0 * (1.0 - w2 / 20.0 * (1.0 - w2 / 42.0)), np.sin(w) / np.where(small, 1.0, w))
    cw = np.cos(w)
    e2 = np.exp(2j * u)
    em = np.exp(-1j * u)
    h0 = (u2 - w2) * e2 + em * (8.0 * u2 * cw + 2j * u * (3.0 * u2 + w2) * xi0)
    h1 = 2.0 * u * e2 - em * (2.0 * u * cw - 1j * (3.0 * u2 - w2) * xi0)
    h2 = e2 - em * (cw + 3j * u * xi0)
    den = 9.0 * u2 - w2
    ok = (c0max > 0.0) & (den > 0.0)
    sden = np.where(ok, den, 1.0)
    f0 = np.where(ok, h0 / sden, 1.0)
    f1 = np.where(ok, h1 / sden, 0.0)
    f2 = np.where(ok, h2 / sden, 0.0)
    f0 = np.where(neg, np.conj(f0), f0)
    f1 = np.where(neg, -np.conj(f1), f1)
    f2 = np.where(neg, np.conj(f2), f2)
    return f0, f1, f2, Q2


def exp_ch(Q):
    f0, f1, f2, Q2 = ch_coefficients(Q)
    one = np.eye(3, dtype=np.complex128)
    return f0[..., None, None] * one + f1[..., None, None] * Q + f2[..., None, None] * Q2


# ---- the step ------------------------------------------------------------------------------------------------------
def staple_sum(U, rho, dims, mu):
    """C_mu(x) = sum_{nu != mu} rho[mu][nu] [U_nu(x) U_mu(x+nu) U_nu(x+mu)^dagger + U_nu(x-nu)^dagger U_mu(x-nu) U_nu(x-nu+mu)]"""
    dims, V = _grid(dims)
    ndim = len(dims)
    C = np.zeros((V, 3, 3), dtype=np.complex128)
    for nu in range(ndim):
        if nu == mu or rho[mu, nu] == 0.0 or dims[nu] == 1:
            continue
        Un, Um = U[:, nu], U[:, mu]
        fwd = Un @ shift(Um, dims, nu, +1) @ dagger(shift(Un, dims, mu, +1))
        W = dagger(Un) @ Um @ shift(Un, dims, mu, +1)
        C += rho[mu, nu] * (fwd + shift(W, dims, nu, -1))
    return C


def stout_step(U, rho, dims, exp=exp_eigh):
    dims, V = _grid(dims)
    ndim = len(dims)
    rho = rho_table(rho, ndim)
    out = U.copy()
    for mu in range(ndim):
        live = [nu for nu in range(ndim) if nu != mu and rho[mu, nu] != 0.0 and dims[nu] > 1]
        if dims[mu] == 1 or not live:
            continue
        C = staple_sum(U, rho, dims, mu)
        Om = C @ dagger(U[:, mu])
        A = dagger(Om) - Om
        tr = A[:, 0, 0] + A[:, 1, 1] + A[:, 2, 2]
        Q = 0.5j * A - (1j / 6.0) * tr[:, None, None] * np.eye(3)
        out[:, mu] = exp(Q) @ U[:, mu]
    return out


def stout_smear(U, rho, dims, n_steps=1, dir=None, exp=exp_eigh):
    rho = rho_table(rho, len(list(dims)), dir)
    for _ in range(n_steps):
        U = stout_step(U, rho, dims, exp=exp)
    return U


def plaquette_sites(U, dims, mu, nu):
    """tr[U_mu(x) U_nu(x+mu) U_mu(x+nu)^dagger U_nu(x)^dagger] per site"""
    P = U[:, mu] @ shift(U[:, nu], dims, mu, +1) @ dagger(shift(U[:, mu], dims, nu, +1)) @ dagger(U[:, nu])
    return P[:, 0, 0] + P[:, 1, 1] + P[:, 2, 2]


def plaquette(U, dims, with_scale=False):
    """P[mu, nu] = P[nu, mu] = Re sum_x tr(...) / (3 V); with_scale: also sum_x |tr(...)| / (3 V), the size the rounding
    error of the sum is measured against"""
    dims, V = _grid(dims)
    ndim = len(dims)
    P = np.zeros((ndim, ndim))
    S = np.zeros((ndim, ndim))
    for mu in range(ndim):
        for nu in range(mu + 1, ndim):
            if dims[mu] == 1 or dims[nu] == 1:
                continue
            t = plaquette_sites(U, dims, mu, nu)
            P[mu, nu] = P[nu, mu] = np.sum(t.real) / (3.0 * V)
            S[mu, nu] = S[nu, mu] = np.sum(np.abs(t)) / (3.0 * V)
    return (P, S) if with_scale else P


# ---- test fields -----------------------------------------------------------------------------------------------------
def random_hermitian_traceless(shape, rng):
    A = rng.standard_normal(tuple(shape) + (3, 3)) + 1j * rng.standard_normal(tuple(shape) + (3, 3))
    H = 0.5 * (A + dagger(A))
    tr = (H[..., 0, 0] + H[..., 1, 1] + H[..., 2, 2]) / 3.0
    return H - tr[..., None, None] * np.eye(3)


def random_su3(shape, eps, rng):
    """exp(i eps H), H random traceless Hermitian"""
    return exp_eigh(eps * random_hermitian_traceless(shape, rng))


def random_links(shape, rng):
    """general complex links, real and imaginary parts uniform in [-1, 1)"""
    return rng.uniform(-1, 1, tuple(shape) + (3, 3)) + 1j * rng.uniform(-1, 1, tuple(shape) + (3, 3))


def gauge_transform(U, g, dims):
    """U_mu(x) -> g(x) U_mu(x) g(x+mu)^dagger"""
    out = np.empty_like(U)
    for mu in range(U.shape[1]):
        out[:, mu] = g @ U[:, mu] @ dagger(shift(g, dims, mu, +1))
    return out


def laplacian(psi, U, dims, dir=-1):
    """sum_{mu != dir} [U_mu(x) psi(x+mu) + U_mu(x-mu)^dagger psi(x-mu) - 2 psi(x)], psi[site, colour, column]"""
    out = np.zeros_like(psi)
    for mu in range(U.shape[1]):
        if mu == dir:
            continue
        out += U[:, mu] @ shift(psi, dims, mu, +1) + shift(dagger(U[:, mu]) @ psi, dims, mu, -1) - 2.0 * psi
    return out


def rel_err(a, b):
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))
