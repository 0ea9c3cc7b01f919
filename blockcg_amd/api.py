"""Python mirror of the reference's header-level interface over the C ABI.

Names and argument meaning follow the reference so that parity tests read like its own tests
(test/solvers.cpp): block_fermion_field(V-or-context, N_rhs), dirac_op(context, mass),
SBCGrQ(X, B, D, sigma, eps, eps_shifts, max_iterations) -> number of operator applications.
Host arrays are numpy complex128 in the reference's layout: field [V, m, 3]; gauge
[V, ndim, 3, 3] with [.., k, r] = U(r, k); m x m matrices as ordinary (row, col) numpy arrays.
"""
import ctypes
import json

import numpy as np

from . import _lib
from ._lib import c_dbl_p

NOISE_GAUSSIAN, NOISE_Z2, NOISE_Z4 = 0, 1, 2  # BCG_NOISE_* of include/blockcg_hip.h

SUPPORTED_WIDTHS = tuple(range(1, 33))  # the reference's N_rhs is any int (inc/fields.hpp:19-26)

_STATUS = {1: "BCG_ERR_INVALID", 2: "BCG_ERR_UNSUPPORTED", 3: "BCG_ERR_HIP", 4: "BCG_ERR_NO_DEVICE", 5: "BCG_ERR_COMM",
           6: "BCG_ERR_NUMERIC"}


class BlockCGError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{_STATUS.get(code, code)}: {msg}")
        self.code = code


def _dp(a):
    return a.ctypes.data_as(c_dbl_p)


def _mat_in(M, m):
    M = np.asarray(M, dtype=np.complex128)
    if M.shape != (m, m):
        raise ValueError(f"expected a {m}x{m} matrix")
    return np.ascontiguousarray(M.T)  # column-major buffer


def _ivec(v, n=4, fill=1):
    v = list(v) + [fill] * (n - len(v))
    return (ctypes.c_int * n)(*v)


class Context:
    """One GPU = one rank of the process grid over a periodic lattice of up to 4 dimensions."""

    def __init__(self, dims, device=0, grid=None, coords=None, stream=None):
        self.lib = _lib.load()
        self.dims = [int(d) for d in dims]
        self.ndim = len(self.dims)
        self.grid = [int(g) for g in grid] if grid is not None else [1] * self.ndim
        self.coords = [int(x) for x in coords] if coords is not None else [0] * self.ndim
        h = ctypes.c_void_p()
        rc = self.lib.bcg_context_create(ctypes.byref(h), device, stream, self.ndim, _ivec(self.dims), _ivec(self.grid),
                                         _ivec(self.coords, fill=0))
        if rc != 0:
            raise BlockCGError(rc, self.lib.bcg_last_error(None).decode())
        self.h = h
        self._comm_keepalive = None
        ld = (ctypes.c_int * 4)()
        og = (ctypes.c_int * 4)()
        self.lib.bcg_local_dims(self.h, ld, og)
        self.local_dims = list(ld)[:self.ndim]
        self.origin = list(og)[:self.ndim]
        self.V = int(self.lib.bcg_local_volume(self.h))

    def check(self, rc):
        if rc != 0:
            raise BlockCGError(rc, self.lib.bcg_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.bcg_context_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        self.check(self.lib.bcg_synchronize(self.h))

    def profiling(self, enable=True):
        self.check(self.lib.bcg_profiling(self.h, 1 if enable else 0))

    def profile_reset(self):
        self.check(self.lib.bcg_profile_reset(self.h))

    def profile(self):
        return json.loads(self.lib.bcg_profile_json(self.h).decode())

    def force_generic(self, enable=True):
        self.check(self.lib.bcg_force_generic(self.h, 1 if enable else 0))

    def capacity_mode(self, ring_slices):
        """Keep dirac_op::op's intermediate field as a ring of `ring_slices` x3 slices (0: whole field)."""
        self.check(self.lib.bcg_capacity_mode(self.h, int(ring_slices)))

    def sbcgrq_device_bytes(self, m, n_shifts, consume_B=False):
        n = ctypes.c_size_t()
        self.check(self.lib.bcg_sbcgrq_device_bytes(self.h, m, n_shifts, 1 if consume_B else 0, ctypes.byref(n)))
        return n.value

    def sbcgrq_device_bytes_half(self, m, n_shifts, consume_B=False):
        n = ctypes.c_size_t()
        self.check(self.lib.bcg_sbcgrq_device_bytes_half(self.h, m, n_shifts, 1 if consume_B else 0, ctypes.byref(n)))
        return n.value

    def halo_buffers(self):
        s = ctypes.c_void_p()
        r = ctypes.c_void_p()
        n = ctypes.c_size_t()
        self.check(self.lib.bcg_halo_buffers(self.h, ctypes.byref(s), ctypes.byref(r), ctypes.byref(n)))
        return s.value, r.value, n.value

    def set_comm(self, comm_struct, keepalive):
        self._comm_keepalive = (comm_struct, keepalive)
        self.check(self.lib.bcg_context_set_comm(self.h, ctypes.byref(comm_struct)))

    def bytes_per_iteration(self, m, n_shifts):
        return float(self.lib.bcg_sbcgrq_bytes_per_iteration(self.h, m, n_shifts))


class block_fermion_field:
    """Device block field (inc/fields.hpp:25-147).  `N_rhs` is the reference's template parameter."""

    def __init__(self, ctx, N_rhs, host=None, parity=None):
        """parity = 0 / 1: a half-volume field, the ctx.V / 2 sites of that parity (include/blockcg_hip.h,
        bcg_field_create_half); every operation then takes operands of the same parity."""
        self.ctx = ctx
        self.N_rhs = int(N_rhs)
        self.parity = parity
        self.V = ctx.V if parity is None else ctx.V // 2
        h = ctypes.c_void_p()
        if parity is None:
            ctx.check(ctx.lib.bcg_field_create(ctx.h, self.N_rhs, ctypes.byref(h)))
        else:
            ctx.check(ctx.lib.bcg_field_create_half(ctx.h, self.N_rhs, int(parity), ctypes.byref(h)))
        self.h = h
        if host is not None:
            self.upload(host)

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.ctx.lib.bcg_field_destroy(self.h)
            self.h = None
        except Exception:
            pass

    # full field <-> its parity halves
    def split_parity(self):
        """(even, odd): new half-volume fields holding this field's sites of parity 0 and 1."""
        out = []
        for par in (0, 1):
            half = block_fermion_field(self.ctx, self.N_rhs, parity=par)
            self.ctx.check(self.ctx.lib.bcg_field_parity_copy(self.h, half.h, 1))
            out.append(half)
        return tuple(out)

    def merge_parity(self, even, odd):
        """This (full) field's sites of either parity <- the two half-volume fields."""
        for half in (even, odd):
            self.ctx.check(self.ctx.lib.bcg_field_parity_copy(self.h, half.h, 0))
        return self

    # host <-> device
    def pinned_array(self):
        """A (V, N_rhs, 3) complex128 array in pinned host memory (bcg_host_alloc): transfers to / from it run at the bus
        rate with no staging copy.  Freed when the array (and every view of it) is garbage-collected."""
        import ctypes
        import weakref
        n = self.V * self.N_rhs * 3 * 16
        p = ctypes.c_void_p()
        self.ctx.check(self.ctx.lib.bcg_host_alloc(n, ctypes.byref(p)))
        buf = (ctypes.c_char * n).from_address(p.value)
        a = np.frombuffer(buf, dtype=np.complex128).reshape(self.V, self.N_rhs, 3)
        weakref.finalize(buf, self.ctx.lib.bcg_host_free, p)
        return a

    def upload(self, host):
        a = np.ascontiguousarray(host, dtype=np.complex128)
        if a.shape != (self.V, self.N_rhs, 3):
            raise ValueError(f"expected host array of shape {(self.V, self.N_rhs, 3)}, got {a.shape}")
        self.ctx.check(self.ctx.lib.bcg_field_upload(self.h, _dp(a)))
        return self

    def download(self, out=None):
        """out: an existing (V, N_rhs, 3) complex128 array to fill (e.g. a view of pinned memory from pinned_array)."""
        a = np.empty((self.V, self.N_rhs, 3), dtype=np.complex128) if out is None else out
        if a.shape != (self.V, self.N_rhs, 3) or a.dtype != np.complex128 or not a.flags.c_contiguous:
            raise ValueError("download(out=...): expected a C-contiguous complex128 array of shape (V, N_rhs, 3)")
        self.ctx.check(self.ctx.lib.bcg_field_download(self.h, _dp(a)))
        return a

    def download_sites(self, sites):
        """Tiles of chosen local sites, [len(sites), N_rhs, 3] (operator[] read access, inc/fields.hpp:37-38)."""
        sites = np.ascontiguousarray(sites, dtype=np.int64)
        a = np.empty((len(sites), self.N_rhs, 3), dtype=np.complex128)
        self.ctx.check(self.ctx.lib.bcg_field_download_sites(self.h, len(sites),
                                                             sites.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _dp(a)))
        return a

    def copy_columns(self, dst_first, src, src_first, n):
        """Columns src_first .. src_first + n - 1 of src -> columns dst_first .. of this field; the other columns keep their
        bits.  The widths may differ (packing and unpacking a wide basis); full or half fields of one parity; src is not
        this field."""
        self.ctx.check(self.ctx.lib.bcg_field_copy_columns(self.h, int(dst_first), src.h, int(src_first), int(n)))
        return self

    def copy(self):
        f = block_fermion_field(self.ctx, self.N_rhs)
        self.ctx.check(self.ctx.lib.bcg_field_copy(f.h, self.h))
        return f

    def setZero(self):
        self.ctx.check(self.ctx.lib.bcg_field_set_zero(self.h))
        return self

    def setRandom(self, seed=1):
        self.ctx.check(self.ctx.lib.bcg_field_fill_random(self.h, seed))
        return self

    # sources and sinks on the device (include/blockcg_hip.h: noise, point / wall sources, slice sums)
    def _fill_noise(self, kind, seed):
        self.ctx.check(self.ctx.lib.bcg_field_fill_noise(self.h, kind, seed))
        return self

    def setGaussian(self, seed=1):
        """Complex Gaussian noise of density exp(-|z|^2) (<|z|^2> = 1) from the generator of setRandom."""
        return self._fill_noise(NOISE_GAUSSIAN, seed)

    def setZ2(self, seed=1):
        return self._fill_noise(NOISE_Z2, seed)

    def setZ4(self, seed=1):
        return self._fill_noise(NOISE_Z4, seed)

    def setPointSources(self, coords, colours):
        """Zero, then column j has a 1 at the GLOBAL site coords[j] (ndim entries each), colour colours[j]."""
        m = self.N_rhs
        xs = np.zeros((m, 4), dtype=np.intc)
        cs = np.asarray(coords, dtype=np.intc).reshape(m, -1)
        xs[:, :cs.shape[1]] = cs
        col = np.ascontiguousarray(np.asarray(colours, dtype=np.intc).reshape(m))
        self.ctx.check(self.ctx.lib.bcg_field_set_point_sources(self.h, xs.ctypes.data_as(_lib.c_int_p),
                                                                col.ctypes.data_as(_lib.c_int_p)))
        return self

    def setWallSources(self, dir, slices, colours, parity=-1):
        """Zero, then column j has a 1 in colour colours[j] on the sites with GLOBAL x_dir = slices[j] (parity: -1 all, 0 even,
        1 odd sites of the slice)."""
        m = self.N_rhs
        sl = np.ascontiguousarray(np.asarray(slices, dtype=np.intc).reshape(m))
        col = np.ascontiguousarray(np.asarray(colours, dtype=np.intc).reshape(m))
        self.ctx.check(self.ctx.lib.bcg_field_set_wall_sources(self.h, int(dir), sl.ctypes.data_as(_lib.c_int_p),
                                                               col.ctypes.data_as(_lib.c_int_p), int(parity)))
        return self

    def slice_dot(self, rhs, dir):
        """[L_dir global, N_rhs]: sum over the sites of slice x_dir = t and the colours of conj(this) * rhs, per column;
        summed over ranks.  Its sum over t is the diagonal of hermitian_dot(rhs)."""
        if not 0 <= int(dir) < self.ctx.ndim:
            raise BlockCGError(1, "slice_dot: direction outside the lattice")
        out = np.empty((self.ctx.dims[int(dir)], self.N_rhs), dtype=np.complex128)
        self.ctx.check(self.ctx.lib.bcg_field_slice_dot(self.h, rhs.h, int(dir), _dp(out)))
        return out

    def slice_gram(self, rhs, dir, momenta=None):
        """Per-slice Gram matrices: [L_dir global, N_rhs, N_rhs] with entry (t, i, j) = sum over the sites of slice x_dir = t
        and the colours of conj(this[.., i]) * rhs[.., j]; its sum over t is hermitian_dot(rhs), its diagonal slice_dot.
        momenta: a list of integer momenta (ndim or 4 entries each, the entry along dir 0) gives [P, L_dir, N_rhs, N_rhs]
        with the summand weighted by exp(-2 pi i sum_mu n_mu x_mu / L_mu) of the GLOBAL coordinates.  Summed over ranks."""
        if not 0 <= int(dir) < self.ctx.ndim:
            raise BlockCGError(1, "slice_gram: direction outside the lattice")
        m, L = self.N_rhs, self.ctx.dims[int(dir)]
        if momenta is None:
            out = np.empty((L, m, m), dtype=np.complex128)
            self.ctx.check(self.ctx.lib.bcg_field_slice_gram(self.h, rhs.h, int(dir), 0, None, _dp(out)))
            return np.ascontiguousarray(out.transpose(0, 2, 1))
        mom = [list(p) for p in momenta]
        if not mom or any(len(p) > 4 for p in mom):
            raise BlockCGError(1, "slice_gram: momenta is a non-empty list of up to 4 integers each")
        ns = np.zeros((len(mom), 4), dtype=np.intc)
        for k, p in enumerate(mom):
            ns[k, :len(p)] = p
        out = np.empty((len(mom), L, m, m), dtype=np.complex128)
        self.ctx.check(self.ctx.lib.bcg_field_slice_gram(self.h, rhs.h, int(dir), len(mom), ns.ctypes.data_as(_lib.c_int_p),
                                                         _dp(out)))
        return np.ascontiguousarray(out.transpose(0, 1, 3, 2))

    def __iadd__(self, rhs):
        self.ctx.check(self.ctx.lib.bcg_field_add_assign(self.h, rhs.h))
        return self

    def __isub__(self, rhs):
        self.ctx.check(self.ctx.lib.bcg_field_sub_assign(self.h, rhs.h))
        return self

    def add(self, rhs, rhs_multiplier):
        """this += rhs * rhs_multiplier  (scalar or m x m)  inc/fields.hpp:70-77"""
        if np.isscalar(rhs_multiplier):
            self.ctx.check(self.ctx.lib.bcg_field_add_scalar(self.h, rhs.h, float(rhs_multiplier)))
        else:
            M = _mat_in(rhs_multiplier, self.N_rhs)
            self.ctx.check(self.ctx.lib.bcg_field_add_matrix(self.h, rhs.h, _dp(M)))
        return self

    def rescale_add(self, lhs_multiplier, rhs, rhs_multiplier):
        """this = this * lhs_multiplier + rhs * rhs_multiplier  inc/fields.hpp:79-90"""
        if np.isscalar(lhs_multiplier):
            self.ctx.check(self.ctx.lib.bcg_field_rescale_add_scalar(self.h, float(lhs_multiplier), rhs.h,
                                                                     float(rhs_multiplier)))
        else:
            M = _mat_in(lhs_multiplier, self.N_rhs)
            self.ctx.check(self.ctx.lib.bcg_field_rescale_add_matrix(self.h, _dp(M), rhs.h, float(rhs_multiplier)))
        return self

    def hermitian_dot(self, rhs):
        m = self.N_rhs
        out = np.empty((m, m), dtype=np.complex128)
        self.ctx.check(self.ctx.lib.bcg_field_hermitian_dot(self.h, rhs.h, _dp(out)))
        return np.ascontiguousarray(out.T)

    def real_dot(self, rhs):
        out = ctypes.c_double()
        self.ctx.check(self.ctx.lib.bcg_field_real_dot(self.h, rhs.h, ctypes.byref(out)))
        return out.value

    def multiply_upper_triangular_inverse_RHS(self, R):
        M = _mat_in(R, self.N_rhs)
        self.ctx.check(self.ctx.lib.bcg_field_tri_solve_rhs(self.h, _dp(M)))
        return self

    def thinQR(self):
        """In place; returns R (the reference fills its argument, inc/fields.hpp:140-146)."""
        m = self.N_rhs
        out = np.empty((m, m), dtype=np.complex128)
        self.ctx.check(self.ctx.lib.bcg_field_thin_qr(self.h, _dp(out)))
        return np.ascontiguousarray(out.T)


class dirac_op:
    """inc/dirac_op.hpp:8-44 on a device lattice: public V, mass; op(lhs, rhs)."""

    def __init__(self, ctx, mass=0.1, U=None, seed=None):
        self.ctx = ctx
        self.V = ctx.V
        self.mass = float(mass)
        h = ctypes.c_void_p()
        ctx.check(ctx.lib.bcg_gauge_create(ctx.h, ctypes.byref(h)))
        self.h = h
        if U is not None:
            self.set_links(U)
        elif seed is not None:
            ctx.check(ctx.lib.bcg_gauge_fill_random(self.h, seed))

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.ctx.lib.bcg_gauge_destroy(self.h)
            self.h = None
        except Exception:
            pass

    def set_links(self, U):
        a = np.ascontiguousarray(U, dtype=np.complex128)
        if a.shape != (self.V, self.ctx.ndim, 3, 3):
            raise ValueError(f"expected links of shape {(self.V, self.ctx.ndim, 3, 3)}, got {a.shape}")
        self.ctx.check(self.ctx.lib.bcg_gauge_upload(self.h, _dp(a)))

    def op(self, lhs, rhs):
        self.ctx.check(self.ctx.lib.bcg_dirac_apply(self.ctx.h, self.h, self.mass, lhs.h, rhs.h))

    def D(self, lhs, rhs):
        """The reference's private hop (inc/dirac_op.hpp:14-21), exposed for tests.  Half-volume fields: lhs of the
        parity opposite to rhs's."""
        if getattr(rhs, "parity", None) is not None:
            self.ctx.check(self.ctx.lib.bcg_dirac_hop_half(self.ctx.h, self.h, lhs.h, rhs.h))
        else:
            self.ctx.check(self.ctx.lib.bcg_dirac_hop(self.ctx.h, self.h, lhs.h, rhs.h))


class gauge_field:
    """A link-shaped device field of the context: one 3 x 3 complex matrix per local site and direction, host arrays
    [V, ndim, 3, 3] in the layout dirac_op.set_links takes ([.., k, r] = M(r, k)).  fermion_force accumulates into one."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.V = ctx.V
        self.shape = (ctx.V, ctx.ndim, 3, 3)
        h = ctypes.c_void_p()
        ctx.check(ctx.lib.bcg_gauge_create(ctx.h, ctypes.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.ctx.lib.bcg_gauge_destroy(self.h)
            self.h = None
        except Exception:
            pass

    def setZero(self):
        self.ctx.check(self.ctx.lib.bcg_gauge_set_zero(self.h))
        return self

    def setRandom(self, seed=1):
        """i.i.d. uniform [-1,1) per real component (the generator of dirac_op(ctx, seed=...))"""
        self.ctx.check(self.ctx.lib.bcg_gauge_fill_random(self.h, seed))
        return self

    def upload(self, U):
        a = np.ascontiguousarray(U, dtype=np.complex128)
        if a.shape != self.shape:
            raise ValueError(f"expected an array of shape {self.shape}, got {a.shape}")
        self.ctx.check(self.ctx.lib.bcg_gauge_upload(self.h, _dp(a)))
        return self

    def download(self):
        a = np.empty(self.shape, dtype=np.complex128)
        self.ctx.check(self.ctx.lib.bcg_gauge_download(self.h, _dp(a)))
        return a


def fermion_force(F, X, D, residues, scale=1.0, project=False, work=None):
    """F += scale * sum_s residues[s] G(X_s), or TA(U G) per link with project=True (include/blockcg_hip.h,
    bcg_force_accumulate): the derivative of S = sum_s a_s B^dagger (A + sigma_s)^-1 B with respect to the links, from the
    shifted solutions X_s.  F: a gauge_field; X: fields of one width and parity; D: the dirac_op whose links are used.
    work: fields of X's width and parity for D X_s (None: the library allocates one); up to len(X) of them let several
    shifts share one pass over F."""
    ctx = D.ctx
    S = len(X)
    a = np.ascontiguousarray(residues, dtype=np.float64)
    if a.shape != (S,):
        raise ValueError("one residue per field X_s is needed")
    Xh = (ctypes.c_void_p * S)(*[x.h for x in X])
    work = list(work or [])
    Wh = (ctypes.c_void_p * max(1, len(work)))(*[w.h for w in work])
    ctx.check(ctx.lib.bcg_force_accumulate(ctx.h, D.h, Xh, S, _dp(a), float(scale), 1 if project else 0,
                                           Wh if work else None, len(work), F.h))
    return F


def _coefficients(v, ndim):
    """None, one complex number for every direction, or one per direction -> ndim x (re, im) doubles (None stays None)."""
    if v is None:
        return None
    a = np.asarray(v, dtype=np.complex128)
    if a.ndim == 0:
        a = np.full(ndim, complex(a))
    if a.shape != (ndim,):
        raise ValueError(f"expected one coefficient, or one per direction ({ndim})")
    return np.ascontiguousarray(a).view(np.float64)


def shift_sum(out, inp, links, c0=0.0, fwd=None, bwd=None, eta=False):
    """out(x) = c0 inp(x) + sum_mu s_mu(x) [fwd[mu] U_mu(x) inp(x+mu) + bwd[mu] U_mu(x-mu)^dagger inp(x-mu)]
    (include/blockcg_hip.h, bcg_dirac_shift_sum).  links: a dirac_op or a gauge_field.  c0, fwd[mu], bwd[mu] complex; fwd and
    bwd one number per direction, one for all, or None (all 0); s_mu = eta_mu when eta, else 1.  A term whose coefficient is
    exactly 0 is not evaluated.  Half fields: inp of parity p, out of parity 1 - p, c0 = 0."""
    ctx = links.ctx
    c = np.array([complex(c0)], dtype=np.complex128).view(np.float64)
    f, b = _coefficients(fwd, ctx.ndim), _coefficients(bwd, ctx.ndim)
    ctx.check(ctx.lib.bcg_dirac_shift_sum(ctx.h, links.h, out.h, inp.h, _dp(c), None if f is None else _dp(f),
                                          None if b is None else _dp(b), 1 if eta else 0))
    return out


def covariant_shift(out, inp, links, mu, sign=+1):
    """sign > 0: out(x) = U_mu(x) inp(x+mu);  sign < 0: out(x) = U_mu(x-mu)^dagger inp(x-mu).  Only direction mu's links and
    that one neighbour row are read."""
    ndim = links.ctx.ndim
    if not 0 <= int(mu) < ndim or sign == 0:
        raise ValueError("mu must be a direction of the lattice and sign non-zero")
    one = np.zeros(ndim, dtype=np.complex128)
    one[int(mu)] = 1.0
    return shift_sum(out, inp, links, 0.0, one if sign > 0 else None, one if sign < 0 else None)


def _but(ndim, dir, value):
    if not -1 <= int(dir) < ndim:
        raise ValueError(f"dir must be -1 or a direction of the lattice, got {dir}")
    v = np.full(ndim, value, dtype=np.complex128)
    if dir >= 0:
        v[int(dir)] = 0.0
    return v, ndim - (1 if dir >= 0 else 0)


def laplacian(out, inp, links, dir=-1):
    """out = sum_{mu != dir} [U_mu(x) inp(x+mu) + U_mu(x-mu)^dagger inp(x-mu) - 2 inp(x)]; dir = -1: every direction.
    dir = 3 on a 4-D lattice is the spatial covariant Laplacian (its links of direction 3 are not read)."""
    hop, n = _but(links.ctx.ndim, dir, 1.0)
    return shift_sum(out, inp, links, -2.0 * n, hop, hop)


def smear(f, links, dir, kappa, n_iter, work=None):
    """f <- (1 + kappa Lap_dir)^n_iter f in place (include/blockcg_hip.h, bcg_covariant_smear): n_iter calls of shift_sum with
    c0 = 1 - 2 kappa (number of smeared directions), fwd = bwd = kappa off dir, bit for bit.  work: a field of f's width
    (None: allocated for the call); overwritten."""
    ctx = links.ctx
    ctx.check(ctx.lib.bcg_covariant_smear(ctx.h, links.h, f.h, None if work is None else work.h, int(dir), float(kappa),
                                          int(n_iter)))
    return f


def _rho_table(rho, ndim, dir=None):
    """a scalar weight (on all pairs, or on all pairs not involving dir) or an ndim x ndim table -> ndim*ndim doubles"""
    r = np.asarray(rho, dtype=np.float64)
    d = -1 if dir is None else int(dir)
    if not -1 <= d < ndim:
        raise ValueError(f"dir must be None, -1 or a direction of the lattice, got {dir}")
    if r.ndim == 0:
        t = np.full((ndim, ndim), float(r))
        if d >= 0:
            t[d, :] = 0.0
            t[:, d] = 0.0
    else:
        if r.size != ndim * ndim:
            raise ValueError(f"expected one weight, or an {ndim} x {ndim} table")
        if d >= 0:
            raise ValueError("dir goes with a scalar rho; a table says itself which pairs it smears")
        t = r.reshape(ndim, ndim)
    return np.ascontiguousarray(t, dtype=np.float64)


def stout_smear(out, links, rho=0.1, n_steps=1, dir=None, work=None):
    """out = S^n_steps(links): stout smearing of the gauge links on the device (include/blockcg_hip.h,
    bcg_gauge_stout_smear).  out: a gauge_field; links: a dirac_op or a gauge_field (not written).  rho: one weight, or an
    ndim x ndim table rho[mu][nu] (diagonal ignored, a zero entry is not evaluated); a scalar rho with dir = t means rho on all
    pairs not involving t (dir = 3 on a 4-D lattice: spatial smearing, direction 3 copied bit for bit); dir None or -1: all
    pairs.  work: a gauge_field the steps alternate with (None: allocated for the call when n_steps >= 2); overwritten.
    Returns out."""
    ctx = links.ctx
    t = _rho_table(rho, ctx.ndim, dir)
    ctx.check(ctx.lib.bcg_gauge_stout_smear(ctx.h, out.h, links.h, _dp(t), int(n_steps), None if work is None else work.h))
    return out


def plaquette(links):
    """P[mu, nu] = P[nu, mu] = sum_x Re tr[U_mu(x) U_nu(x+mu) U_mu(x+nu)^dagger U_nu(x)^dagger] / (3 V_global) as an
    ndim x ndim array (include/blockcg_hip.h, bcg_gauge_plaquette); 0 on the diagonal and for directions of extent 1.  links:
    a dirac_op or a gauge_field.  Summed over all ranks, the same bits on every call."""
    ctx = links.ctx
    out = np.zeros((ctx.ndim, ctx.ndim), dtype=np.float64)
    ctx.check(ctx.lib.bcg_gauge_plaquette(ctx.h, links.h, _dp(out)))
    return out


def _basis_handles(V):
    V = list(V)
    if not V:
        raise ValueError("a basis is a non-empty list of fields")
    return (ctypes.c_void_p * len(V))(*[v.h for v in V]), len(V), sum(v.N_rhs for v in V)


def basis_dot(V, b):
    """C = V^dagger b as a (K, m) array: V a list of fields of any widths 1..32 (K the sum of the widths, basis column i the
    column i - offset_k of the field it falls in) of b's context, parity and site count.  Every entry is computed, nothing is
    mirrored; summed over ranks and identical on every rank (include/blockcg_hip.h, bcg_basis_dot).  b may be one of V."""
    Vh, nv, K = _basis_handles(V)
    out = np.empty((b.N_rhs, K), dtype=np.complex128)
    b.ctx.check(b.ctx.lib.bcg_basis_dot(Vh, nv, b.h, _dp(out)))
    return np.ascontiguousarray(out.T)


def basis_slice_dot(V, b, dir, momenta=None):
    """V^dagger b resolved by slice: [L_dir global, K, m] with entry (t, i, j) = sum over the sites of slice x_dir = t and the
    colours of conj(V_i) * b_j, V as in basis_dot; its sum over t is basis_dot(V, b).  momenta: a list of integer momenta (ndim
    or 4 entries each, the entry along dir 0) gives [P, L_dir, K, m] with the summand weighted by
    exp(-2 pi i sum_mu n_mu x_mu / L_mu) of the GLOBAL coordinates, as in block_fermion_field.slice_gram.  Summed over ranks and
    identical on every rank (include/blockcg_hip.h, bcg_basis_slice_dot).  b may be one of V."""
    Vh, nv, K = _basis_handles(V)
    if not 0 <= int(dir) < b.ctx.ndim:
        raise BlockCGError(1, "basis_slice_dot: direction outside the lattice")
    m, L = b.N_rhs, b.ctx.dims[int(dir)]
    if momenta is None:
        out = np.empty((L, m, K), dtype=np.complex128)
        b.ctx.check(b.ctx.lib.bcg_basis_slice_dot(Vh, nv, b.h, int(dir), 0, None, _dp(out)))
        return np.ascontiguousarray(out.transpose(0, 2, 1))
    mom = [list(p) for p in momenta]
    if not mom or any(len(p) > 4 for p in mom):
        raise BlockCGError(1, "basis_slice_dot: momenta is a non-empty list of up to 4 integers each")
    ns = np.zeros((len(mom), 4), dtype=np.intc)
    for k, p in enumerate(mom):
        ns[k, :len(p)] = p
    out = np.empty((len(mom), L, m, K), dtype=np.complex128)
    b.ctx.check(b.ctx.lib.bcg_basis_slice_dot(Vh, nv, b.h, int(dir), len(mom), ns.ctypes.data_as(_lib.c_int_p), _dp(out)))
    return np.ascontiguousarray(out.transpose(0, 1, 3, 2))


def basis_axpy(y, V, C, beta=1.0):
    """y <- beta y + V C with C a (K, m) array (bcg_basis_axpy).  beta exactly 0 does not read y.  y is none of V."""
    Vh, nv, K = _basis_handles(V)
    C = np.asarray(C, dtype=np.complex128)
    if C.shape != (K, y.N_rhs):
        raise ValueError(f"expected a {K}x{y.N_rhs} matrix")
    Ct = np.ascontiguousarray(C.T)  # column-major buffer
    y.ctx.check(y.ctx.lib.bcg_basis_axpy(y.h, Vh, nv, _dp(Ct), float(beta)))
    return y


def basis_slice_axpy(y, V, C, dir, slices=None, momentum=None, beta=1.0):
    """y <- beta y + w V C[s] on the sites with global x_dir = slices[s] and y <- beta y on every other site
    (bcg_basis_slice_axpy), the adjoint of basis_slice_dot.  C: an (S, K, m) array, one matrix per listed slice; slices: a
    list of distinct global slice indices (None: all L_dir slices in ascending order, so that basis_slice_dot's result goes
    straight in).  momentum: None (w = 1) or up to 4 integers, the entry along dir 0: w(x) = exp(+2 pi i sum_mu n_mu x_mu / L_mu)
    of the GLOBAL coordinates.  beta exactly 0 does not read y (the other slices become zeros), beta exactly 1 leaves the other
    slices alone.  Purely local.  y is none of V."""
    Vh, nv, K = _basis_handles(V)
    if not 0 <= int(dir) < y.ctx.ndim:
        raise BlockCGError(1, "basis_slice_axpy: direction outside the lattice")
    if slices is None:
        S, sl, n_slices = y.ctx.dims[int(dir)], None, 0
    else:
        arr = np.ascontiguousarray(list(slices), dtype=np.intc)
        if arr.ndim != 1 or arr.size == 0:
            raise BlockCGError(1, "basis_slice_axpy: slices is a non-empty list of slice indices")
        S, sl, n_slices = int(arr.size), arr.ctypes.data_as(_lib.c_int_p), int(arr.size)
    C = np.asarray(C, dtype=np.complex128)
    if C.shape != (S, K, y.N_rhs):
        raise ValueError(f"expected {S} matrices of {K}x{y.N_rhs}")
    Ct = np.ascontiguousarray(C.transpose(0, 2, 1))  # column-major blocks
    mp = None
    if momentum is not None:
        p = list(momentum)
        if len(p) > 4:
            raise BlockCGError(1, "basis_slice_axpy: a momentum has up to 4 integers")
        mom = np.zeros(4, dtype=np.intc)
        mom[:len(p)] = p
        mp = mom.ctypes.data_as(_lib.c_int_p)
    y.ctx.check(y.ctx.lib.bcg_basis_slice_axpy(y.h, Vh, nv, int(dir), n_slices, sl, _dp(Ct), mp, float(beta)))
    return y


def basis_slice_triple(A, B, C, dir, slices=None, momenta=None):
    """The baryon elementals of three lists of fields, slice by slice (include/blockcg_hip.h, bcg_basis_slice_triple):
    [S, Ka, Kb, Kc] with entry (s, i, j, k) = sum over the sites x of slice x_dir = slices[s] of det[A_i(x), B_j(x), C_k(x)], the
    colour determinant of three columns.  A, B, C as V in basis_dot, at most 64 columns each; they may share fields or be the
    same list, and the same list three times gives a result that is antisymmetric bit for bit.  slices: a list of distinct
    global slice indices (None: all L_dir slices in ascending order).  momenta as in basis_slice_dot: [P, S, Ka, Kb, Kc].
    Summed over ranks and identical on every rank."""
    A = list(A)
    (Ah, na, Ka), (Bh, nb, Kb), (Ch, nc, Kc) = _basis_handles(A), _basis_handles(B), _basis_handles(C)
    ctx = A[0].ctx
    if not 0 <= int(dir) < ctx.ndim:
        raise BlockCGError(1, "basis_slice_triple: direction outside the lattice")
    if slices is None:
        S, sl, n_slices = ctx.dims[int(dir)], None, 0
    else:
        arr = np.ascontiguousarray(list(slices), dtype=np.intc)
        if arr.ndim != 1 or arr.size == 0:
            raise BlockCGError(1, "basis_slice_triple: slices is a non-empty list of slice indices")
        S, sl, n_slices = int(arr.size), arr.ctypes.data_as(_lib.c_int_p), int(arr.size)
    if momenta is None:
        out = np.empty((S, Kc, Kb, Ka), dtype=np.complex128)
        ctx.check(ctx.lib.bcg_basis_slice_triple(Ah, na, Bh, nb, Ch, nc, int(dir), n_slices, sl, 0, None, _dp(out)))
        return np.ascontiguousarray(out.transpose(0, 3, 2, 1))
    mom = [list(p) for p in momenta]
    if not mom or any(len(p) > 4 for p in mom):
        raise BlockCGError(1, "basis_slice_triple: momenta is a non-empty list of up to 4 integers each")
    ns = np.zeros((len(mom), 4), dtype=np.intc)
    for k, p in enumerate(mom):
        ns[k, :len(p)] = p
    out = np.empty((len(mom), S, Kc, Kb, Ka), dtype=np.complex128)
    ctx.check(ctx.lib.bcg_basis_slice_triple(Ah, na, Bh, nb, Ch, nc, int(dir), n_slices, sl, len(mom), ns.ctypes.data_as(_lib.c_int_p),
                                             _dp(out)))
    return np.ascontiguousarray(out.transpose(0, 1, 4, 3, 2))


def deflate(B, V):
    """B <- B - V (V^dagger B) for an orthonormal basis V; returns C = V^dagger B, (K, m)."""
    C = basis_dot(V, B)
    basis_axpy(B, V, -C, 1.0)
    return C


def low_mode_solution(X, V, evals, C, sigma):
    """X_s += V (Lambda + sigma_s)^-1 C: the part of (A + sigma_s)^-1 B inside the span of V, for eigenvectors V of A with
    eigenvalues evals (K of them) and C = V^dagger B.  (A + sigma_s)^-1 is diagonal on eigenvectors of A for every shift at
    once, so one coefficient matrix per shift is all that changes."""
    ev = np.asarray(evals, dtype=np.float64)
    C = np.asarray(C, dtype=np.complex128)
    if ev.shape != (C.shape[0],) or len(sigma) != len(X):
        raise ValueError("one eigenvalue per basis column and one shift per X_s are needed")
    for x, s in zip(X, sigma):
        basis_axpy(x, V, C / (ev + float(s))[:, None], 1.0)
    return X


def SBCGrQ_deflated(X, B, D, sigma, V, evals, eps=1.e-15, eps_shifts=1.e-15, max_iterations=1000000, return_info=False):
    """(op + sigma_s) X_s = B with the span of V taken out of the Krylov solve: B is copied, the copy deflated
    (B - V V^dagger B), SBCGrQ run on it, and the low-mode part V (Lambda + sigma_s)^-1 V^dagger B added to every X_s.
    Contract: V is orthonormal and evals are its Ritz values of dirac_op::op.  With inexact eigenvectors the result is inexact
    by their residuals; true_residuals is the check.  Returns the operator applications of the inner solve (or its info)."""
    Bp = block_fermion_field(B.ctx, B.N_rhs, parity=B.parity)
    B.ctx.check(B.ctx.lib.bcg_field_copy(Bp.h, B.h))
    C = deflate(Bp, V)
    r = SBCGrQ(X, Bp, D, sigma, eps, eps_shifts, max_iterations, consume_B=True, return_info=return_info)
    low_mode_solution(X, V, evals, C, sigma)
    return r


BASIS_ROTATE_MAX_COLUMNS = 64


def basis_rotate(V, Q):
    """V <- V Q in place (bcg_basis_rotate): V a list of fields of widths 1..32 whose widths sum to K <= 64, Q a (K, K) array
    that need not be unitary; column j of the result is sum_i V_i Q[i, j].  One launch takes all K columns and needs no second
    copy of the basis.  Purely local."""
    Vh, nv, K = _basis_handles(V)
    Q = np.asarray(Q, dtype=np.complex128)
    if Q.shape != (K, K):
        raise ValueError(f"expected a {K}x{K} matrix")
    Qt = np.ascontiguousarray(Q.T)  # column-major buffer
    V[0].ctx.check(V[0].ctx.lib.bcg_basis_rotate(Vh, nv, _dp(Qt)))
    return V


def spectral_bound(D, steps=10, seed=1, parity=None):
    """An upper bound on the largest eigenvalue of D.op (parity None) or of its block of one parity (0 / 1): theta_max + beta
    of a `steps`-step Lanczos run from Gaussian noise (bcg_spectral_bound)."""
    out = ctypes.c_double()
    D.ctx.check(D.ctx.lib.bcg_spectral_bound(D.ctx.h, D.h, D.mass, -1 if parity is None else int(parity), int(steps), int(seed),
                                             ctypes.byref(out)))
    return out.value


def lowest_modes(V, D, n_want, upper_bound, degree=16, tol=1e-10, max_iterations=100, locked=None):
    """Chebyshev-filtered subspace iteration for the lowest eigenpairs of D.op (bcg_lowest_modes).  V: the start block (a list
    of fields, K <= 64 columns in all, filled by the caller), on return orthonormal Ritz vectors with ascending Ritz values;
    locked: converged orthonormal vectors V is kept orthogonal to.  Converged when the residuals of the first n_want columns
    are at most tol * upper_bound; reaching max_iterations is no error.  The top columns of the block the iteration carries
    sit on the edge of the interval the filter damps and converge slowly or not at all, so the wanted columns need columns
    beyond them; with n_want == K the call carries a guard block of min(16, 64 - K) columns of its own.  Returns a dict: evals and resid (K each), iterations
    (filter applications), applications (calls of the block operator)."""
    Vh, nv, K = _basis_handles(V)
    if locked:
        Lh, nl, _ = _basis_handles(locked)
    else:
        Lh, nl = None, 0
    evals = np.zeros(K)
    resid = np.zeros(K)
    it = ctypes.c_int()
    apps = ctypes.c_int64()
    D.ctx.check(D.ctx.lib.bcg_lowest_modes(D.ctx.h, D.h, D.mass, Vh, nv, Lh, nl, int(n_want), int(degree), float(upper_bound),
                                           float(tol), int(max_iterations), _dp(evals), _dp(resid), ctypes.byref(it),
                                           ctypes.byref(apps)))
    return dict(evals=evals, resid=resid, iterations=it.value, applications=apps.value)


def basis_slice_rotate(V, Q, dir, slices=None):
    """V(x) <- V(x) Q[s] in place on the sites with global x_dir = slices[s] (bcg_basis_slice_rotate): basis_rotate with one
    matrix per slice.  Q: an (S, K, K) array, one matrix per listed slice, none of them need be unitary; slices: a list of
    distinct global slice indices (None: all L_dir slices in ascending order).  The sites of the other slices are neither read
    nor written.  Purely local; no second copy of the basis."""
    Vh, nv, K = _basis_handles(V)
    ctx = V[0].ctx
    if not 0 <= int(dir) < ctx.ndim:
        raise BlockCGError(1, "basis_slice_rotate: direction outside the lattice")
    if slices is None:
        S, sl, n_slices = ctx.dims[int(dir)], None, 0
    else:
        arr = np.ascontiguousarray(list(slices), dtype=np.intc)
        if arr.ndim != 1 or arr.size == 0:
            raise BlockCGError(1, "basis_slice_rotate: slices is a non-empty list of slice indices")
        S, sl, n_slices = int(arr.size), arr.ctypes.data_as(_lib.c_int_p), int(arr.size)
    Q = np.asarray(Q, dtype=np.complex128)
    if Q.shape != (S, K, K):
        raise ValueError(f"expected {S} matrices of {K}x{K}")
    Qt = np.ascontiguousarray(Q.transpose(0, 2, 1))  # column-major blocks
    ctx.check(ctx.lib.bcg_basis_slice_rotate(Vh, nv, int(dir), n_slices, sl, _dp(Qt)))
    return V


def laplacian_modes(V, links, dir, n_want, upper_bound, degree=16, tol=1e-10, max_iterations=100, locked=None):
    """The lowest eigenpairs of -Lap_dir (the covariant Laplacian without direction dir, laplacian(..., dir) negated) on every
    slice of dir at once (bcg_laplacian_modes): a distillation basis.  links: a dirac_op or a gauge_field.  V: the start block
    (a list of full fields, K <= 64 columns in all, filled by the caller); on return V is orthonormal on every slice with
    ascending Ritz values per slice.  locked: vectors orthonormal per slice that V is kept orthogonal to, slice by slice.
    upper_bound: of the spectrum; 4 (ndim - 1) for unitary links.  n_want, degree, tol, max_iterations and the guard block of
    n_want == K as in lowest_modes; converged when every slice is.  Returns a dict: evals and resid ([L_dir, K] each),
    iterations (filter applications), applications (shift_sum calls)."""
    Vh, nv, K = _basis_handles(V)
    ctx = links.ctx
    if locked:
        Lh, nl, _ = _basis_handles(locked)
    else:
        Lh, nl = None, 0
    if not 0 <= int(dir) < ctx.ndim:
        raise BlockCGError(1, "laplacian_modes: direction outside the lattice")
    L = ctx.dims[int(dir)]
    evals = np.zeros((L, K))
    resid = np.zeros((L, K))
    it = ctypes.c_int()
    apps = ctypes.c_int64()
    ctx.check(ctx.lib.bcg_laplacian_modes(ctx.h, links.h, int(dir), Vh, nv, Lh, nl, int(n_want), int(degree), float(upper_bound),
                                          float(tol), int(max_iterations), _dp(evals), _dp(resid), ctypes.byref(it),
                                          ctypes.byref(apps)))
    return dict(evals=evals, resid=resid, iterations=it.value, applications=apps.value)


def _trace_buffers(trace_limit, S, m):
    if trace_limit <= 0:
        return None, None, None
    mats = np.zeros((trace_limit, 3 + 2 * S, m, m), dtype=np.complex128)
    rr = np.zeros((trace_limit, 1 + S), dtype=np.float64)
    return _lib.bcg_sbcgrq_trace(trace_limit, 0, _dp(mats), _dp(rr)), mats, rr


def _solve_info(it, res, tr, mats, rr, S):
    info = dict(iterations=it.value, residual=res.value, trace=None)
    if tr is not None:
        n = tr.recorded
        mt = np.ascontiguousarray(np.swapaxes(mats[:n], -1, -2))
        info["trace"] = dict(alpha=mt[:, 0], rho=mt[:, 1], delta=mt[:, 2], alpha_s=mt[:, 3:3 + S],
                             beta_s=mt[:, 3 + S:3 + 2 * S], residual=rr[:n, 0], residual_shift=rr[:n, 1:])
    return info


def SBCGrQ(X, B, D, sigma, eps=1.e-15, eps_shifts=1.e-15, max_iterations=1000000, trace_limit=0, consume_B=False,
           return_info=False):
    """inc/block_solvers.hpp:91-185.  X: list of fields (overwritten); returns operator applications."""
    ctx = B.ctx
    S = len(X)
    if len(sigma) != S:
        raise ValueError("number of shifts does not match number of solution vectors")  # :97-98
    sig = np.ascontiguousarray(sigma, dtype=np.float64)
    Xh = (ctypes.c_void_p * S)(*[x.h for x in X])
    it = ctypes.c_int(0)
    res = ctypes.c_double(0.0)
    tr, mats, rr = _trace_buffers(trace_limit, S, B.N_rhs)
    ctx.check(ctx.lib.bcg_sbcgrq_solve(ctx.h, D.h, D.mass, Xh, B.h, S, _dp(sig), eps, eps_shifts, int(max_iterations),
                                       1 if consume_B else 0, ctypes.byref(it), ctypes.byref(res),
                                       ctypes.byref(tr) if tr is not None else None))
    if not return_info:
        return it.value
    return _solve_info(it, res, tr, mats, rr, S)


def _sum_args(sigma, residues):
    sig = np.ascontiguousarray(sigma, dtype=np.float64)
    a = np.ascontiguousarray(residues, dtype=np.float64)
    if a.shape != sig.shape:
        raise ValueError("one residue per shift is needed")
    return sig, a


def SBCGrQ_sum(Y, B, D, sigma, residues, c0=0.0, eps=1.e-15, eps_shifts=1.e-15, max_iterations=1000000, trace_limit=0,
               consume_B=False, return_info=False):
    """Y = c0 B + sum_s residues[s] (A + sigma_s)^-1 B: the partial-fraction form of a rational function of the operator.
    The solve is SBCGrQ's (same iterations, coefficients and trace, bit for bit), but the shifted solutions are summed into
    the one field Y as they are updated instead of being kept (include/blockcg_hip.h, bcg_sbcgrq_solve_sum)."""
    ctx = B.ctx
    sig, a = _sum_args(sigma, residues)
    S = len(sig)
    it = ctypes.c_int(0)
    res = ctypes.c_double(0.0)
    tr, mats, rr = _trace_buffers(trace_limit, S, B.N_rhs)
    ctx.check(ctx.lib.bcg_sbcgrq_solve_sum(ctx.h, D.h, D.mass, Y.h, B.h, S, _dp(sig), _dp(a), float(c0), eps, eps_shifts,
                                           1 if consume_B else 0, int(max_iterations), ctypes.byref(it), ctypes.byref(res),
                                           ctypes.byref(tr) if tr is not None else None))
    if not return_info:
        return it.value
    return _solve_info(it, res, tr, mats, rr, S)


class SBCGrQState:
    """The solver as a resumable state machine (bcg_sbcgrq_begin / iterate / end): lets bench.py run
    W warm-up iterations, then time exactly K iterations of the hot loop."""

    def __init__(self, X, B, D, sigma, eps=0.0, eps_shifts=0.0, consume_B=False):
        self.ctx = B.ctx
        self._keep = (X, B, D)
        S = len(X)
        if len(sigma) != S:
            raise ValueError("number of shifts does not match number of solution vectors")
        sig = np.ascontiguousarray(sigma, dtype=np.float64)
        Xh = (ctypes.c_void_p * S)(*[x.h for x in X])
        st = ctypes.c_void_p()
        self.ctx.check(self.ctx.lib.bcg_sbcgrq_begin(self.ctx.h, D.h, D.mass, Xh, B.h, S, _dp(sig), eps, eps_shifts,
                                                     1 if consume_B else 0, ctypes.byref(st)))
        self.h = st
        self.iterations = 0
        self.residual = 1.0

    def iterate(self, n):
        it = ctypes.c_int(0)
        res = ctypes.c_double(0.0)
        self.ctx.check(self.ctx.lib.bcg_sbcgrq_iterate(self.h, int(n), ctypes.byref(it), ctypes.byref(res), None))
        self.iterations, self.residual = it.value, res.value
        return it.value

    def end(self):
        if self.h:
            self.ctx.lib.bcg_sbcgrq_end(self.h)
            self.h = None

    def __del__(self):
        try:
            self.end()
        except Exception:
            pass


class SBCGrQSumState(SBCGrQState):
    """SBCGrQState in sum mode (bcg_sbcgrq_begin_sum): Y accumulates c0 B + sum_s residues[s] X_s."""

    def __init__(self, Y, B, D, sigma, residues, c0=0.0, eps=0.0, eps_shifts=0.0, consume_B=False):
        self.ctx = B.ctx
        self._keep = (Y, B, D)
        sig, a = _sum_args(sigma, residues)
        st = ctypes.c_void_p()
        self.ctx.check(self.ctx.lib.bcg_sbcgrq_begin_sum(self.ctx.h, D.h, D.mass, Y.h, B.h, len(sig), _dp(sig), _dp(a),
                                                         float(c0), eps, eps_shifts, 1 if consume_B else 0, ctypes.byref(st)))
        self.h = st
        self.iterations = 0
        self.residual = 1.0


def true_residuals(X, B, D, sigma):
    """Reference acceptance measure (test/solvers.cpp:104-116) on the device; returns [n_shifts, N_rhs]."""
    ctx = B.ctx
    S = len(X)
    sig = np.ascontiguousarray(sigma, dtype=np.float64)
    Xh = (ctypes.c_void_p * S)(*[x.h for x in X])
    res = np.empty((S, B.N_rhs), dtype=np.float64)
    ctx.check(ctx.lib.bcg_true_residuals(ctx.h, D.h, D.mass, Xh, B.h, S, _dp(sig), _dp(res)))
    return res


def SBCGrQ_half_volume(X, B, D, sigma, eps=1.e-15, eps_shifts=1.e-15, max_iterations=1000000):
    """(op + sigma_s) X_s = B as two half-volume solves, one per site parity: dirac_op::D couples opposite parities only
    (inc/dirac_op.hpp:14-21), so op = mass^2 - D^2 (inc/dirac_op.hpp:36-43) is block diagonal in the parity.  X, B: full
    fields; each half solve runs inc/block_solvers.hpp:91-185 unchanged on half-volume fields (half the work fields'
    memory).  Returns the operator applications of the (even, odd) solve.  A caller short of memory keeps half fields
    only and calls SBCGrQ on them directly."""
    its = []
    halves = []
    for par, Bp in enumerate(B.split_parity()):
        Xp = [block_fermion_field(B.ctx, B.N_rhs, parity=par) for _ in X]
        its.append(SBCGrQ(Xp, Bp, D, sigma, eps, eps_shifts, max_iterations, consume_B=True))
        halves.append(Xp)
    for s, x in enumerate(X):
        x.merge_parity(halves[0][s], halves[1][s])
    return tuple(its)


def CG(x, b, D, eps=1.e-15, max_iterations=1000000):
    """src/standard_solvers.cpp:3-32"""
    it = ctypes.c_int(0)
    b.ctx.check(b.ctx.lib.bcg_cg_solve(b.ctx.h, D.h, D.mass, x.h, b.h, eps, int(max_iterations), ctypes.byref(it)))
    return it.value


def SCG(x, b, D, sigma, eps=1.e-15, eps_shifts=1.e-15, max_iterations=1000000):
    """src/standard_solvers.cpp:34-95"""
    S = len(x)
    if len(sigma) != S:
        raise ValueError("number of shifts does not match number of solution vectors")
    sig = np.ascontiguousarray(sigma, dtype=np.float64)
    xh = (ctypes.c_void_p * S)(*[v.h for v in x])
    it = ctypes.c_int(0)
    b.ctx.check(b.ctx.lib.bcg_scg_solve(b.ctx.h, D.h, D.mass, xh, b.h, S, _dp(sig), eps, eps_shifts, int(max_iterations),
                                        ctypes.byref(it)))
    return it.value


def BCG(X, B, D, eps=1.e-15, max_iterations=1000000):
    """inc/block_solvers.hpp:10-45"""
    it = ctypes.c_int(0)
    B.ctx.check(B.ctx.lib.bcg_bcg_solve(B.ctx.h, D.h, D.mass, X.h, B.h, eps, int(max_iterations), ctypes.byref(it)))
    return it.value


def BCGrQ(X, B, D, eps=1.e-15, max_iterations=1000000):
    """inc/block_solvers.hpp:50-86"""
    it = ctypes.c_int(0)
    B.ctx.check(B.ctx.lib.bcg_bcgrq_solve(B.ctx.h, D.h, D.mass, X.h, B.h, eps, int(max_iterations), ctypes.byref(it)))
    return it.value
