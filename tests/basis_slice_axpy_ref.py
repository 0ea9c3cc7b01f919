"""numpy restatement of bcg_basis_slice_axpy (include/blockcg_hip.h) for tests/test_basis_slice_axpy*.py: a basis put onto
slices, the adjoint of basis_slice_ref.basis_slice_dot.  Host layout: a field is [V, m, 3] over the sites it holds, site index
lexicographic with x0 fastest; the basis is the concatenation of the host arrays of V along the column axis
(basis_ref.concat), the weights are the conjugates of slice_gram_ref.phases, and each listed slice is one einsum."""
import numpy as np

from basis_ref import concat
from slice_gram_ref import phases
from sources_ref import coords, parity_mask


def slice_of_sites(dims, direction, parity=None):
    """the global x_dir of every site held"""
    return coords(dims)[parity_mask(dims, parity), direction]


def basis_slice_axpy(y, V, C, dims, direction, slices=None, momentum=None, beta=1.0, parity=None):
    """beta y + w V C[s] on the sites of slice slices[s], beta y on the others; beta == 0 does not read y (zeros off the listed
    slices).  C [S, K, m]; slices None: all slices in ascending order; momentum None: w = 1."""
    W = concat(V)
    C = np.asarray(C)
    sl = list(range(dims[direction])) if slices is None else list(slices)
    assert C.shape[0] == len(sl) and len(set(sl)) == len(sl)
    t = slice_of_sites(dims, direction, parity)
    out = np.zeros((W.shape[0], C.shape[2], 3), dtype=np.complex128) if beta == 0 else beta * np.asarray(y)
    w = None if momentum is None else np.conj(phases(dims, [momentum], direction, parity)[0])
    for s, ts in enumerate(sl):
        sel = t == ts
        vc = np.einsum("xic,ij->xjc", W[sel], C[s])
        out[sel] += vc if w is None else vc * w[sel][:, None, None]
    return out


def by_sites(y, V, C, dims, direction, slices=None, momentum=None, beta=1.0, parity=None):
    """The same update by a plain loop over the sites held."""
    d = list(dims) + [1] * (4 - len(dims))
    W = concat(V)
    sl = list(range(dims[direction])) if slices is None else list(slices)
    x = coords(dims)[parity_mask(dims, parity)]
    n = [0, 0, 0, 0] if momentum is None else list(momentum) + [0] * (4 - len(momentum))
    K, m = W.shape[1], np.asarray(C).shape[2]
    out = np.zeros((len(x), m, 3), dtype=np.complex128)
    for s in range(len(x)):
        if beta != 0:
            out[s] = beta * y[s]
        if int(x[s, direction]) not in sl:
            continue
        Cs = C[sl.index(int(x[s, direction]))]
        frac = sum(((int(n[mu]) * int(x[s, mu])) % d[mu]) / d[mu] for mu in range(4))
        wgt = np.exp(+2j * np.pi * frac)
        for j in range(m):
            for c in range(3):
                acc = 0.0
                for i in range(K):
                    acc += W[s, i, c] * Cs[i, j]
                out[s, j, c] += wgt * acc
    return out
