"""numpy restatement of bcg_basis_slice_triple (include/blockcg_hip.h) for tests/test_basis_slice_triple*.py: the baryon
elementals of three lists of fields, T_p(s; i, j, k) = sum over the sites x of slice slices[s] of w_p(x) det[A_i(x), B_j(x),
C_k(x)].  Host layout: a field is [V, m, 3] over the sites the field holds, site index lexicographic with x0 fastest.  The
diquark D_ij(x) = A_i(x) x B_j(x) is formed by the three cross-product lines, then one einsum per (p, s) and 256 sites."""
import itertools

import numpy as np

from basis_ref import concat
from slice_gram_ref import phases
from sources_ref import coords, parity_mask


SITES = 256  # of a slice per einsum


def basis_slice_triple(A, B, C, dims, direction, slices=None, momenta=None, parity=None):
    """([P, S, Ka, Kb, Kc] sums, [S, Ka, Kb, Kc] scale sum_x |A_i(x)| |B_j(x)| |C_k(x)| with the colour 2-norms of each site).
    slices None: all in ascending order; momenta None: the single momentum 0."""
    a, b, c = concat(A), concat(B), concat(C)
    moms = [[0, 0, 0, 0]] if momenta is None else momenta
    sl = list(range(dims[direction])) if slices is None else list(slices)
    t = coords(dims)[parity_mask(dims, parity), direction]
    w = phases(dims, moms, direction, parity)
    out = np.zeros((len(moms), len(sl), a.shape[1], b.shape[1], c.shape[1]), dtype=np.complex128)
    scale = np.zeros(out.shape[1:])
    for s, ts in enumerate(sl):
        sel = np.flatnonzero(t == ts)
        for x0 in range(0, len(sel), SITES):  # a bounded D: [sites, Ka, Kb, 3]
            x = sel[x0:x0 + SITES]
            as_, bs, cs = a[x], b[x], c[x]
            ai, bj = as_[:, :, None, :], bs[:, None, :, :]
            D = np.empty((len(x), a.shape[1], b.shape[1], 3), dtype=np.complex128)
            D[..., 0] = ai[..., 1] * bj[..., 2] - ai[..., 2] * bj[..., 1]
            D[..., 1] = ai[..., 2] * bj[..., 0] - ai[..., 0] * bj[..., 2]
            D[..., 2] = ai[..., 0] * bj[..., 1] - ai[..., 1] * bj[..., 0]
            na, nb, nc = (np.sqrt((np.abs(f) ** 2).sum(axis=2)) for f in (as_, bs, cs))
            scale[s] += np.einsum("xi,xj,xk->ijk", na, nb, nc, optimize=True)
            for p in range(len(moms)):
                out[p, s] += np.einsum("xija,xka->ijk", D, cs * w[p, x][:, None, None], optimize=True)
    return out, scale


def by_sites(A, B, C, dims, direction, slices=None, momenta=None, parity=None):
    """The same sums by the epsilon tensor, one site at a time: what the restatement is checked against."""
    a, b, c = concat(A), concat(B), concat(C)
    moms = [[0, 0, 0, 0]] if momenta is None else momenta
    sl = list(range(dims[direction])) if slices is None else list(slices)
    t = coords(dims)[parity_mask(dims, parity), direction]
    w = phases(dims, moms, direction, parity)
    eps = np.zeros((3, 3, 3))
    for perm in itertools.permutations(range(3)):
        eps[perm] = np.linalg.det(np.eye(3)[list(perm)])
    out = np.zeros((len(moms), len(sl), a.shape[1], b.shape[1], c.shape[1]), dtype=np.complex128)
    for x in range(a.shape[0]):
        if t[x] not in sl:
            continue
        det = np.einsum("abc,ia,jb,kc->ijk", eps, a[x], b[x], c[x])
        for p in range(len(moms)):
            out[p, sl.index(t[x])] += w[p, x] * det
    return out
