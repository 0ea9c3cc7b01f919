"""numpy restatement of the device's sources and sinks (include/blockcg_hip.h: noise, point / wall sources, slice dot) for
tests/test_sources_sinks*.py.  Host layout throughout: field [V, m, 3], site index lexicographic with x0 fastest."""
import numpy as np

GAUSSIAN, Z2, Z4 = 0, 1, 2


def noise_from_uniforms(u, kind):
    """u: output of oracle.fill_field (real part a, imaginary part b, both in [-1, 1))."""
    a, b = u.real, u.imag
    if kind == GAUSSIAN:
        w = (1.0 - a) / 2.0
        return np.sqrt(-np.log(w)) * (np.cos(np.pi * b) + 1j * np.sin(np.pi * b))
    if kind == Z2:
        return np.where(a < 0, -1.0, 1.0) + 0j
    if kind == Z4:
        return (np.where(a < 0, -1.0, 1.0) + 1j * np.where(b < 0, -1.0, 1.0)) / np.sqrt(2.0)
    raise ValueError(kind)


def coords(dims):
    """[V, 4] coordinates of every site (entries beyond len(dims) are 0)."""
    d = list(dims) + [1] * (4 - len(dims))
    idx = np.arange(int(np.prod(d)))
    x = np.zeros((len(idx), 4), dtype=np.int64)
    for mu in range(4):
        x[:, mu] = idx % d[mu]
        idx = idx // d[mu]
    return x


def parity_mask(dims, parity):
    x = coords(dims)
    if parity is None:
        return np.ones(len(x), dtype=bool)
    return (x.sum(axis=1) & 1) == parity


def point_sources(dims, m, pts, colours, parity=None):
    d = list(dims) + [1] * (4 - len(dims))
    f = np.zeros((int(np.prod(d)), m, 3), dtype=np.complex128)
    for j in range(m):
        x = list(pts[j]) + [0] * (4 - len(pts[j]))
        site = x[0] + d[0] * (x[1] + d[1] * (x[2] + d[2] * x[3]))
        f[site, j, colours[j]] = 1.0
    return f[parity_mask(dims, parity)]


def wall_sources(dims, m, direction, slices, colours, site_parity=-1, parity=None):
    x = coords(dims)
    f = np.zeros((len(x), m, 3), dtype=np.complex128)
    par = x.sum(axis=1) & 1
    for j in range(m):
        on = x[:, direction] == slices[j]
        if site_parity >= 0:
            on &= par == site_parity
        f[on, j, colours[j]] = 1.0
    return f[parity_mask(dims, parity)]


def slice_dot(a, b, dims, direction, parity=None):
    """([L_dir, m] sums, [L_dir, m] products of the slice norms of a and b)."""
    t = coords(dims)[parity_mask(dims, parity), direction]
    L = dims[direction]
    m = a.shape[1]
    out = np.zeros((L, m), dtype=np.complex128)
    na = np.zeros((L, m))
    nb = np.zeros((L, m))
    p = (np.conj(a) * b).sum(axis=2)
    pa = (np.abs(a) ** 2).sum(axis=2)
    pb = (np.abs(b) ** 2).sum(axis=2)
    for s in range(L):
        sel = t == s
        out[s] = p[sel].sum(axis=0)
        na[s] = pa[sel].sum(axis=0)
        nb[s] = pb[sel].sum(axis=0)
    return out, np.sqrt(na * nb)
