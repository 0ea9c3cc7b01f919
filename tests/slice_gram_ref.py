"""numpy restatement of bcg_field_slice_gram (include/blockcg_hip.h) for tests/test_slice_gram*.py: per-slice Gram matrices with
momentum projection.  Host layout: field [V, m, 3] over the sites the field holds, site index lexicographic with x0 fastest."""
import numpy as np

from sources_ref import coords, parity_mask


def phases(dims, momenta, direction, parity=None):
    """[P, sites held] weights exp(-2 pi i sum_mu ((n_mu x_mu) mod L_mu) / L_mu) from the global coordinates; the component
    along `direction` must be 0."""
    d = list(dims) + [1] * (4 - len(dims))
    x = coords(dims)[parity_mask(dims, parity)]
    out = np.empty((len(momenta), len(x)), dtype=np.complex128)
    for p, n in enumerate(momenta):
        n = list(n) + [0] * (4 - len(n))
        assert n[direction] == 0
        frac = np.zeros(len(x))
        for mu in range(4):
            frac = frac + ((int(n[mu]) * x[:, mu]) % d[mu]) / d[mu]
        out[p] = np.exp(-2j * np.pi * frac)
    return out


def slice_gram(a, b, dims, direction, momenta=None, parity=None):
    """([P, L_dir, m, m] sums with entry (i, j) = sum w_p conj(a_i) b_j, [L_dir, m, m] scale sqrt(|a_i|^2_slice |b_j|^2_slice)).
    momenta None: the single momentum 0."""
    moms = [[0, 0, 0, 0]] if momenta is None else momenta
    t = coords(dims)[parity_mask(dims, parity), direction]
    w = phases(dims, moms, direction, parity)
    L, m = dims[direction], a.shape[1]
    out = np.zeros((len(moms), L, m, m), dtype=np.complex128)
    scale = np.zeros((L, m, m))
    for s in range(L):
        sel = t == s
        as_, bs = a[sel], b[sel]
        na = (np.abs(as_) ** 2).sum(axis=(0, 2))
        nb = (np.abs(bs) ** 2).sum(axis=(0, 2))
        scale[s] = np.sqrt(np.outer(na, nb))
        for p in range(len(moms)):
            out[p, s] = np.einsum("xic,xjc->ij", np.conj(as_), bs * w[p, sel][:, None, None])
    return out, scale
