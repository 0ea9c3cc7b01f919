"""numpy restatement of bcg_basis_slice_rotate (include/blockcg_hip.h) for tests/test_basis_slice_rotate.py,
tests/test_laplacian_modes*.py: V(x) <- V(x) Q[s] on the sites of slice slices[s], every other site as it was.  Host layout as
in basis_ref and basis_slice_axpy_ref: a field is [V, w, 3] over the sites it holds, the basis the concatenation of the fields
along the column axis; each listed slice is one einsum."""
import numpy as np

from basis_ref import concat, split_columns
from basis_slice_axpy_ref import slice_of_sites
from sources_ref import coords, parity_mask


def basis_slice_rotate(V, Q, dims, direction, slices=None, parity=None):
    """the fields of V Q[s] on the listed slices (same widths); Q [S, K, K]; slices None: all slices in ascending order.
    Sites that are not listed are copied, so a NaN there stays a NaN and nothing of it leaks into a listed slice."""
    W = concat(V)
    Q = np.asarray(Q)
    sl = list(range(dims[direction])) if slices is None else list(slices)
    assert Q.shape == (len(sl), W.shape[1], W.shape[1]) and len(set(sl)) == len(sl)
    t = slice_of_sites(dims, direction, parity)
    out = W.copy()
    for s, ts in enumerate(sl):
        sel = t == ts
        out[sel] = np.einsum("xic,ij->xjc", W[sel], Q[s])
    return split_columns(out, [np.asarray(v).shape[1] for v in V])


def by_sites(V, Q, dims, direction, slices=None, parity=None):
    """The same rotation by a plain loop over the sites held."""
    W = concat(V)
    sl = list(range(dims[direction])) if slices is None else list(slices)
    x = coords(dims)[parity_mask(dims, parity)]
    K = W.shape[1]
    out = W.copy()
    for s in range(len(x)):
        ts = int(x[s, direction])
        if ts not in sl:
            continue
        Qs = Q[sl.index(ts)]
        for j in range(K):
            for c in range(3):
                acc = 0.0
                for i in range(K):
                    acc += W[s, i, c] * Qs[i, j]
                out[s, j, c] = acc
    return split_columns(out, [np.asarray(v).shape[1] for v in V])
