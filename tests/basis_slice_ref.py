"""numpy restatement of bcg_basis_slice_dot (include/blockcg_hip.h) for tests/test_basis_slice*.py: V^dagger b resolved by slice,
with momentum projection.  Host layout: a field is [V, m, 3] over the sites it holds, site index lexicographic with x0
fastest; the basis is the concatenation of the host arrays of V along the column axis (basis_ref.concat), the weights are
those of slice_gram_ref.phases, and each (p, t) is one einsum."""
import numpy as np

from basis_ref import concat
from slice_gram_ref import phases
from sources_ref import coords, parity_mask


def basis_slice_dot(V, b, dims, direction, momenta=None, parity=None):
    """([P, L_dir, K, m] sums with entry (i, j) = sum w_p conj(V_i) b_j, [L_dir, K, m] scale sqrt(|V_i|^2_slice |b_j|^2_slice)).
    momenta None: the single momentum 0."""
    moms = [[0, 0, 0, 0]] if momenta is None else momenta
    W = concat(V)
    t = coords(dims)[parity_mask(dims, parity), direction]
    w = phases(dims, moms, direction, parity)
    L, K, m = dims[direction], W.shape[1], b.shape[1]
    out = np.zeros((len(moms), L, K, m), dtype=np.complex128)
    scale = np.zeros((L, K, m))
    for s in range(L):
        sel = t == s
        ws, bs = W[sel], b[sel]
        nw = (np.abs(ws) ** 2).sum(axis=(0, 2))
        nb = (np.abs(bs) ** 2).sum(axis=(0, 2))
        scale[s] = np.sqrt(np.outer(nw, nb))
        for p in range(len(moms)):
            out[p, s] = np.einsum("xic,xjc->ij", np.conj(ws), bs * w[p, sel][:, None, None])
    return out, scale


def by_sites(V, b, dims, direction, momenta=None, parity=None):
    """The same sums by a plain loop over the sites held: every site adds w_p(x) conj(V_i(x, c)) b_j(x, c) to its slice."""
    moms = [[0, 0, 0, 0]] if momenta is None else momenta
    d = list(dims) + [1] * (4 - len(dims))
    W = concat(V)
    x = coords(dims)[parity_mask(dims, parity)]
    out = np.zeros((len(moms), dims[direction], W.shape[1], b.shape[1]), dtype=np.complex128)
    for s in range(len(x)):
        for p, n in enumerate(moms):
            n = list(n) + [0] * (4 - len(n))
            frac = sum(((int(n[mu]) * int(x[s, mu])) % d[mu]) / d[mu] for mu in range(4))
            wgt = np.exp(-2j * np.pi * frac)
            for c in range(3):
                out[p, x[s, direction]] += wgt * np.outer(np.conj(W[s, :, c]), b[s, :, c])
    return out
