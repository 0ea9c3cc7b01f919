"""Every block width 1 .. 32 on every entry point that is instantiated or laid out per width: the covariant shift sum, the
fermion force, sources and slice sums, slice Gram matrices, the basis products and the column copy, the core primitives and a
short solve on half fields, and the sum form of the solve.  One test function per family and width, so a failure names both.

Two lattices, made once for the module: [4,2,4,2] (64 sites, 4-D, even extents, an extent of 2; full fields and both
parities of 32 sites) and [5,3,2] (30 sites, 90 rows, 3-D, odd extents; full fields only).  For most widths 64, 32 and 30
are no multiple of 256 // m, so the last block of the per-site kernels is partly filled, and 90 rows are no multiple of 16
or of any generic tile height.

References: the numpy restatements of the extension tests (shift_sum_ref, test_force_cpu.numpy_force, sources_ref,
slice_gram_ref, basis_ref) and the oracle.  Tolerances are the project's own: TOL_KERNEL, TOL_COEFF (conftest), EPS_DOT =
1e-13 of the norms (test_basis, test_slice_gram, test_sources_sinks), 1e-13 by test_force._close, 1e-14 for the Gaussian
noise (test_sources_sinks), 1e-12 for Q and the triangular solve and 1e-11 for X after fixed iterations
(test_gpu_parity.test_every_block_width, test_sum_mode.test_fixed_work_against_oracle)."""
import numpy as np
import pytest

import basis_ref
import shift_sum_ref
import slice_gram_ref
import sources_ref
from conftest import TOL_COEFF, TOL_KERNEL, rel_err
from test_force import _close, _expected, _gpu_force

pytestmark = pytest.mark.gpu

EPS_DOT = 1e-13
L4, L3 = (4, 2, 4, 2), (5, 3, 2)
MASS, SEED_U, SEED_B, SEED_Y = 0.2, 5, 6, 7  # the operator and the fields of test_gpu_parity.test_every_block_width
SHIFTS = [0.0, 1e-3, 0.5]
ITERATIONS = 3


@pytest.fixture(scope="module")
def bc():
    import blockcg_amd
    return blockcg_amd


class _Lattice:
    """Context, random links on the host and on the device, and the operators over them: never changed by a test."""

    def __init__(self, bc, orc, dims):
        self.dims = list(dims)
        self.ctx = bc.Context(self.dims)
        self.V, self.nd = self.ctx.V, len(dims)
        self.U = shift_sum_ref.random_links(np.random.default_rng(17 + len(dims)), self.dims)
        self.links = bc.gauge_field(self.ctx).upload(self.U)
        self.D = bc.dirac_op(self.ctx, 0.3, U=self.U)
        self.U_gen = orc.fill_gauge(self.dims, SEED_U)
        self.D_gen = bc.dirac_op(self.ctx, MASS, seed=SEED_U)
        self.parities = (None, 0, 1) if tuple(dims) == L4 else (None,)

    def mask(self, parity):
        return sources_ref.parity_mask(self.dims, parity)

    def field(self, bc, m, host=None, parity=None):
        return bc.block_fermion_field(self.ctx, m, host, parity=parity)


@pytest.fixture(scope="module")
def lattices(bc, orc):
    return {d: _Lattice(bc, orc, d) for d in (L4, L3)}


@pytest.fixture(scope="module")
def small_lattices(bc, orc):
    """The same two lattices with contexts made in the `small` environment of tests/test_force.py (the tuning is read when a
    context is made)."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("BCG_HOP_PATCH", "16,2,2")
        mp.setenv("BCG_HOP_BLOCKS", "32")
        return {d: _Lattice(bc, orc, d) for d in (L4, L3)}


def _bits(x):
    return np.ascontiguousarray(x).view(np.float64)


def _rand(rng, shape):
    return rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)


def _matrix(m):
    rng = np.random.default_rng(m)
    return rng.uniform(-1, 1, (m, m)) + 1j * rng.uniform(-1, 1, (m, m))


# ---- shift sum --------------------------------------------------------------------------------------------------------
def _coefficients(rng, nd):
    return (complex(rng.normal(), rng.normal()), rng.normal(size=nd) + 1j * rng.normal(size=nd),
            rng.normal(size=nd) + 1j * rng.normal(size=nd))


@pytest.mark.parametrize("m", range(1, 33))
def test_shift_sum(bc, lattices, m):
    worst = 0.0
    for lat in lattices.values():
        rng = np.random.default_rng(1000 + m)
        psi = shift_sum_ref.random_field(rng, lat.V, m)
        f, out = lat.field(bc, m, psi), lat.field(bc, m)
        for eta in (False, True):
            c0, fw, bw = _coefficients(rng, lat.nd)
            got = bc.shift_sum(out, f, lat.links, c0, fw, bw, eta).download()
            err = rel_err(got, shift_sum_ref.shift_sum(lat.U, lat.dims, psi, c0, fw, bw, eta))
            worst = max(worst, err)
            assert err <= TOL_KERNEL, (lat.dims, m, eta, err)
        assert np.array_equal(_bits(f.download()), _bits(psi))  # `in` untouched
        if len(lat.parities) == 1:
            continue
        halves = f.split_parity()
        for p in (0, 1):  # parity p into parity 1 - p, c0 = 0
            src, dst = halves[p], lat.field(bc, m, parity=1 - p)
            for eta in (False, True):
                _, fw, bw = _coefficients(rng, lat.nd)
                got = bc.shift_sum(dst, src, lat.links, 0.0, fw, bw, eta).download()
                want = shift_sum_ref.shift_sum(lat.U, lat.dims, psi, 0.0, fw, bw, eta)[shift_sum_ref.parity_mask(lat.dims, 1 - p)]
                err = rel_err(got, want)
                worst = max(worst, err)
                assert err <= TOL_KERNEL, (lat.dims, m, p, eta, err)
            assert np.array_equal(_bits(src.download()), _bits(psi[shift_sum_ref.parity_mask(lat.dims, p)]))
    print(f"shift sum, m = {m}: worst error {worst:.3e} relative")


# ---- force ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", range(1, 33))
def test_force(bc, small_lattices, m):
    worst, S = 0.0, 2
    for lat in small_lattices.values():
        rng = np.random.default_rng(2000 + m)
        for parity in (None, 1) if len(lat.parities) > 1 else (None,):
            n = lat.V if parity is None else lat.V // 2
            Xh = [_rand(rng, (n, m, 3)) for _ in range(S)]
            a, scale = rng.uniform(-2, 2, S), rng.uniform(0.5, 1.5)
            F0 = _rand(rng, (lat.V, lat.nd, 3, 3))
            for project in (False, True):
                got = _gpu_force(bc, lat.ctx, lat.D, Xh, a, scale, parity, F0=F0, project=project, n_work=S)
                want = F0 + _expected(lat.U, lat.dims, Xh, a, scale, parity, project)
                worst = max(worst, np.max(np.abs(got - want)) / np.max(np.abs(want)))
                _close(got, want)
    print(f"force, m = {m}: worst error {worst:.3e} of the largest entry")


# ---- sources and slice sums -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", range(1, 33))
def test_sources_and_slice_dot(bc, orc, lattices, m):
    worst_noise, worst_dot = 0.0, 0.0
    for lat in lattices.values():
        dims, nd = lat.dims, lat.nd
        for parity in lat.parities:
            f = lat.field(bc, m, parity=parity)
            # noise against the definition
            u = orc.fill_field(m, lat.V, 40 + m)[lat.mask(parity)]
            assert np.array_equal(f.setRandom(40 + m).download(), u)
            assert np.array_equal(f.setZ2(40 + m).download(), sources_ref.noise_from_uniforms(u, sources_ref.Z2))
            assert np.array_equal(f.setZ4(40 + m).download(), sources_ref.noise_from_uniforms(u, sources_ref.Z4))
            dev = np.max(np.abs(f.setGaussian(40 + m).download() - sources_ref.noise_from_uniforms(u, sources_ref.GAUSSIAN)))
            worst_noise = max(worst_noise, dev)
            assert dev <= 1e-14, (dims, m, parity, dev)
            # point and wall sources, bit for bit: colour j % 3, site and slice vary with j
            col = [j % 3 for j in range(m)]
            pts = [[(j * (mu + 1) + mu) % dims[mu] for mu in range(nd)] for j in range(m)]
            if parity is not None:
                for p in pts:
                    if sum(p) % 2 != parity:
                        p[0] ^= 1  # even extents: stays inside
            assert np.array_equal(f.setPointSources(pts, col).download(), sources_ref.point_sources(dims, m, pts, col, parity))
            for direction in range(nd):
                sl = [(j + direction) % dims[direction] for j in range(m)]
                for sp in ((-1, 0, 1) if parity is None else (-1, parity)):
                    got = f.setWallSources(direction, sl, col, sp).download()
                    assert np.array_equal(got, sources_ref.wall_sources(dims, m, direction, sl, col, sp, parity)), (dims, m, parity, direction, sp)
            # slice sums along direction 0 and along the last one, two operands and one
            a = lat.field(bc, m, parity=parity).setGaussian(11)
            b = lat.field(bc, m, parity=parity).setGaussian(12)
            ah, bh = a.download(), b.download()
            for x, xh, y, yh in ((a, ah, b, bh), (a, ah, a, ah)):
                for direction in (0, nd - 1):
                    got = x.slice_dot(y, direction)
                    want, scale = sources_ref.slice_dot(xh, yh, dims, direction, parity)
                    assert got.shape == want.shape
                    assert np.array_equal(got[scale == 0], want[scale == 0])  # slices a half field holds no site of
                    held = scale > 0
                    err = float(np.max(np.abs(got - want)[held] / scale[held]))
                    worst_dot = max(worst_dot, err)
                    assert err <= EPS_DOT, (dims, m, parity, direction, x is y, err)
    print(f"sources, m = {m}: Gaussian deviation {worst_noise:.3e}, slice dot {worst_dot:.3e} of |a||b| per slice")


# ---- slice Gram matrices ----------------------------------------------------------------------------------------------
def _check_gram(got, want, scale, what):
    """got, want [P, L, m, m]; scale [L, m, m].  Slices a half field holds no site of: exact zeros."""
    assert got.shape == want.shape, what
    sc = np.broadcast_to(scale, got.shape)
    assert np.array_equal(got[sc == 0], np.zeros_like(got[sc == 0])), what
    held = sc > 0
    err = float(np.max(np.abs(got - want)[held] / sc[held]))
    assert err <= EPS_DOT, (what, err)
    return err


@pytest.mark.parametrize("m", range(1, 33))
def test_slice_gram(bc, lattices, m):
    worst = 0.0
    for lat in lattices.values():
        dims, nd = lat.dims, lat.nd
        momenta = [[1, 0, 0, 0][:nd], [-1, 1, 0, 0][:nd]]
        for parity in lat.parities:
            a = lat.field(bc, m, parity=parity).setGaussian(21)
            b = lat.field(bc, m, parity=parity).setGaussian(22)
            ah, bh = a.download(), b.download()
            for x, xh, y, yh in ((a, ah, b, bh), (a, ah, a, ah)):
                what = (dims, m, parity, x is y)
                got = x.slice_gram(y, nd - 1, momenta)
                want, scale = slice_gram_ref.slice_gram(xh, yh, dims, nd - 1, momenta, parity)
                worst = max(worst, _check_gram(got, want, scale, what + ("last direction",)))
                got = x.slice_gram(y, 0)
                want, scale = slice_gram_ref.slice_gram(xh, yh, dims, 0, None, parity)
                worst = max(worst, _check_gram(got[None], want, scale, what + ("direction 0",)))
    print(f"slice gram, m = {m}: worst error {worst:.3e} of |a_i||b_j| per slice")


# ---- basis products ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", range(1, 33))
def test_basis_products(bc, lattices, m):
    """V = [33 - m, m] ([m] alone at m = 32) against b and y of width m: every width is a basis width and the block width.
    The column copy takes n = min(m, 33 - m) columns from column m // 3 on of a field of 32 columns (the one width that holds
    columns m // 3 .. m // 3 + n - 1 at every m) into the last n columns of the field of width m and, below m = 32, of the
    field of width 33 - m: every width is a target."""
    widths = [33 - m, m] if m < 32 else [m]
    K = sum(widths)
    worst_dot, worst_axpy = 0.0, 0.0
    for lat in lattices.values():
        for parity in lat.parities:
            what = (lat.dims, m, parity)
            V = [lat.field(bc, w, parity=parity).setGaussian(100 + k) for k, w in enumerate(widths)]
            b = lat.field(bc, m, parity=parity).setGaussian(150)
            y = lat.field(bc, m, parity=parity).setGaussian(151)
            Vh, bh, yh = [v.download() for v in V], b.download(), y.download()
            err = float(np.max(np.abs(bc.basis_dot(V, b) - basis_ref.basis_dot(Vh, bh)) / basis_ref.dot_scale(Vh, bh)))
            worst_dot = max(worst_dot, err)
            assert err <= EPS_DOT, (what, err)
            rng = np.random.default_rng(K * 100 + m)
            C = rng.standard_normal((K, m)) + 1j * rng.standard_normal((K, m))
            for beta in (0.0, -0.5):
                y.upload(np.full_like(yh, np.nan) if beta == 0.0 else yh)
                out = bc.basis_axpy(y, V, C, beta).download()
                assert np.isfinite(out).all(), (what, beta)
                err = rel_err(out, basis_ref.basis_axpy(yh, Vh, C, beta))
                worst_axpy = max(worst_axpy, err)
                assert err <= TOL_KERNEL, (what, beta, err)
            for v, vh in zip(V, Vh):
                assert np.array_equal(_bits(v.download()), _bits(vh)), what
            assert np.array_equal(_bits(b.download()), _bits(bh)), what
            # the column copy, bit for bit, the other columns of the target unchanged
            n, first = min(m, 33 - m), m // 3
            src = lat.field(bc, 32, parity=parity).setGaussian(152)
            sh = src.download()
            for target, th in ((b, bh),) + (((V[0], Vh[0]),) if m < 32 else ()):
                w = th.shape[1]
                want = th.copy()
                want[:, w - n:] = sh[:, first:first + n]
                target.copy_columns(w - n, src, first, n)
                assert np.array_equal(_bits(target.download()), _bits(want)), (what, w)
            assert np.array_equal(_bits(src.download()), _bits(sh)), what
    print(f"basis products, V widths {widths}, m = {m}: dot {worst_dot:.3e} of |V_i||b_j|, update {worst_axpy:.3e} relative")


# ---- core primitives on half fields -----------------------------------------------------------------------------------
@pytest.mark.parametrize("m", range(1, 33))
def test_core_primitives_on_half_fields(bc, orc, lattices, m):
    """[4,2,4,2], both parities, against the oracle on the arrays restricted to the parity (the pattern of
    tests/test_half_volume.py::test_half_fields_layout_operator_and_primitives, the tolerances of
    tests/test_gpu_parity.py::test_every_block_width)."""
    lat = lattices[L4]
    dims, D, U = lat.dims, lat.D_gen, lat.U_gen
    masks = [lat.mask(p) for p in (0, 1)]
    Bh, Yh = orc.fill_field(m, lat.V, SEED_B), orc.fill_field(m, lat.V, SEED_Y)
    Dh, Ah = orc.hop(U, dims, Bh), orc.dirac_apply(U, dims, MASS, Bh)
    M = _matrix(m)
    # split and merge, bit for bit
    halves = lat.field(bc, m, Bh).split_parity()
    for p in (0, 1):
        assert halves[p].V == lat.V // 2 and np.array_equal(_bits(halves[p].download()), _bits(Bh[masks[p]]))
    assert np.array_equal(_bits(lat.field(bc, m).merge_parity(*halves).download()), _bits(Bh))
    errs = {}

    def check(name, got, want, tol):
        e = rel_err(got, want)
        errs[name] = max(errs.get(name, 0.0), e)
        assert e < tol, (m, p, name, e)

    for p in (0, 1):
        Bp, Yp = np.ascontiguousarray(Bh[masks[p]]), np.ascontiguousarray(Yh[masks[p]])
        F = lambda a: lat.field(bc, m, a, parity=p)  # noqa: E731
        assert np.array_equal(_bits(F(Bp).download()), _bits(Bp))  # upload / download round trip
        other = lat.field(bc, m, parity=1 - p)
        D.D(other, F(Bp))  # (D B) at the sites of parity 1 - p only sees B's sites of parity p
        check("D", other.download(), Dh[masks[1 - p]], TOL_KERNEL)
        out = lat.field(bc, m, parity=p)
        D.op(out, F(Bp))
        check("op", out.download(), Ah[masks[p]], TOL_KERNEL)
        check("add scalar", F(Yp).add(F(Bp), 0.3).download(), orc.add_scalar(Yp, Bp, 0.3), TOL_KERNEL)
        check("add matrix", F(Yp).add(F(Bp), M).download(), orc.add_matrix(Yp, Bp, M), TOL_KERNEL)
        check("rescale_add scalar", F(Yp).rescale_add(-1.0, F(Bp), 0.25).download(), orc.rescale_add_scalar(Yp, -1.0, Bp, 0.25), TOL_KERNEL)
        check("rescale_add matrix", F(Yp).rescale_add(M, F(Bp), 1.0).download(), orc.rescale_add_matrix(Yp, M, Bp, 1.0), TOL_KERNEL)
        fy = F(Yp)
        fy += F(Bp)
        check("+=", fy.download(), orc.add_scalar(Yp, Bp, 1.0), TOL_KERNEL)
        fy = F(Yp)
        fy -= F(Bp)
        check("-=", fy.download(), orc.sub(Yp, Bp), TOL_KERNEL)
        check("hermitian_dot", F(Yp).hermitian_dot(F(Bp)), orc.hermitian_dot(Yp, Bp), TOL_KERNEL)
        q = F(Yp)
        R = q.thinQR()
        qo, Ro = orc.thin_qr(Yp)
        check("thinQR R", R, Ro, TOL_KERNEL)
        check("thinQR Q", q.download(), qo, 1e-12)
        check("tri solve", F(Bp).multiply_upper_triangular_inverse_RHS(Ro).download(), orc.tri_solve_rhs(Bp, Ro), 1e-12)
    name = max(errs, key=errs.get)
    print(f"half-field primitives, m = {m}: worst error {errs[name]:.3e} relative ({name})")


# ---- a short solve on half fields -------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", range(1, 33))
def test_short_solve_on_half_fields(bc, orc, lattices, m):
    """Three fixed iterations on parity 1 of [4,2,4,2] against the oracle on the full lattice with the source zero on parity
    0: op does not mix the parities, so the oracle's solve is the half solve with exact zeros on the other sites.

    A half field here has 96 rows.  The residual block of iteration k is orthogonal to the k m directions used so far, so
    once 4 m > 96 (m >= 25) the third thinQR (inc/block_solvers.hpp:152) factors a block of rank 96 - 3 m < m: the
    algorithm breaks down there, whatever computes it.  The oracle carries NaN in rho and delta of that iteration (at
    m = 32, where nothing but rounding is left, a rho of 1e-11); the library reports BCG_ERR_NUMERIC instead, before it
    updates X (tests/test_gpu_parity.py::test_degenerate_lattices: the same rule for a rank-deficient start).  X of all
    three iterations and every coefficient but the last rho and delta do not depend on that factor.  So at these widths
    the third iteration either is reported as a breakdown, or gives the oracle's X and those coefficients; and the two
    iterations before it are checked in full, like the three at the other widths."""
    lat = lattices[L4]
    mask = lat.mask(1)
    Bh = orc.fill_field(m, lat.V, SEED_B)
    Bh[~mask] = 0.0
    keys = ("alpha", "rho", "delta", "alpha_s", "beta_s")

    def run(iterations):
        X = [lat.field(bc, m, parity=1) for _ in SHIFTS]
        info = bc.SBCGrQ(X, lat.field(bc, m, Bh[mask], parity=1), lat.D_gen, SHIFTS, 0.0, 0.0, max_iterations=iterations,
                         trace_limit=iterations, return_info=True)
        o = orc.sbcgrq(lat.U_gen, lat.dims, MASS, Bh, SHIFTS, 0.0, 0.0, max_iterations=iterations, trace_limit=iterations)
        assert info["iterations"] == o["iterations"] == iterations
        assert np.isfinite(o["X"]).all() and not o["X"][:, ~mask].any()
        return rel_err(np.stack([x.download() for x in X]), o["X"][:, mask]), info["trace"], o["trace"]

    rank_deficient = 3 * (lat.V // 2) < (ITERATIONS + 1) * m
    if not rank_deficient:
        err_x, got, want = run(ITERATIONS)
        errs = {key: rel_err(got[key], want[key]) for key in keys}
        print(f"half solve, m = {m}: X {err_x:.3e}, coefficients {max(errs.values()):.3e} ({max(errs, key=errs.get)})")
    else:
        err_x, got, want = run(ITERATIONS - 1)
        errs = {key: rel_err(got[key], want[key]) for key in keys}
        try:
            err_3, got, want = run(ITERATIONS)
        except bc.BlockCGError as e:
            assert e.code == 6  # BCG_ERR_NUMERIC: the breakdown is reported
            third = "reported as a breakdown"
        else:
            err_x = max(err_x, err_3)
            for key in keys:
                n = ITERATIONS - 1 if key in ("rho", "delta") else ITERATIONS
                errs[key] = max(errs[key], rel_err(got[key][:n], want[key][:n]))
            third = "run"
        print(f"half solve, m = {m}: X {err_x:.3e}, coefficients {max(errs.values()):.3e} ({max(errs, key=errs.get)}); "
              f"third iteration (rank {max(0, 3 * (lat.V // 2) - ITERATIONS * m)} of {m}) {third}")
    assert err_x < 1e-11
    for key, e in errs.items():
        assert e < TOL_COEFF, (key, e)


# ---- the sum form -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", range(1, 33))
def test_sum_form(bc, orc, lattices, m):
    lat = lattices[L4]
    a, c0 = [1.0, 0.5, 0.25], 0.1
    Bh = orc.fill_field(m, lat.V, SEED_B)
    Y = lat.field(bc, m)
    it = bc.SBCGrQ_sum(Y, lat.field(bc, m, Bh), lat.D_gen, SHIFTS, a, c0, 0.0, 0.0, max_iterations=ITERATIONS)
    o = orc.sbcgrq(lat.U_gen, lat.dims, MASS, Bh, SHIFTS, 0.0, 0.0, max_iterations=ITERATIONS, trace_limit=ITERATIONS)
    assert it == o["iterations"] == ITERATIONS
    err = rel_err(Y.download(), c0 * Bh + sum(ak * x for ak, x in zip(a, o["X"])))
    print(f"sum form, m = {m}: Y {err:.3e} relative")
    assert err < 1e-11
