"""The fermion force of multi-shift solutions (bcg_force_accumulate, fermion_force, gauge_field) on the GPU:
F += scale sum_s a_s G(X_s) with G_mu(x) = eta_mu(x) sum_j [Y(x+mu) X(x)^dag - X(x+mu) Y(x)^dag], Y = D X.  The kernel against
the numpy formula (tests/test_force_cpu.py, Y by conftest.hop_by_lines), the convention against a finite difference of the
action, the projection, the work fields, the argument checks, the production geometry and the C++ drop-in.  Divided
lattices: tests/test_force_distributed.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_force_cpu import action, dense_D, derivative, from_vec, lattice_coords, numpy_force, ta, to_host, to_vec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bc():
    import blockcg_amd
    return blockcg_amd


@pytest.fixture
def small(monkeypatch):
    # a lattice this small needs small patches and few blocks for the column / bundle sweep
    monkeypatch.setenv("BCG_HOP_PATCH", "16,2,2")
    monkeypatch.setenv("BCG_HOP_BLOCKS", "32")
    return monkeypatch


def _rand(rng, shape):
    return rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)


def _parity_sites(dims, parity):
    return np.flatnonzero(lattice_coords(dims).sum(axis=1) % 2 == parity)


def _full(half, dims, parity):
    """a half field's host array -> the full field that is zero on the other parity"""
    V = int(np.prod(dims))
    f = np.zeros((V,) + half.shape[1:], dtype=np.complex128)
    f[_parity_sites(dims, parity)] = half
    return f


def _gpu_force(bc, ctx, D, Xh, a, scale, parity=None, F0=None, project=False, n_work=0):
    m = Xh[0].shape[1]
    X = [bc.block_fermion_field(ctx, m, x, parity=parity) for x in Xh]
    F = bc.gauge_field(ctx)
    if F0 is None:
        F.setZero()
    else:
        F.upload(F0)
    work = [bc.block_fermion_field(ctx, m, parity=parity) for _ in range(n_work)]
    bc.fermion_force(F, X, D, a, scale, project, work)
    return F.download()


def _expected(U, dims, Xh, a, scale, parity=None, project=False):
    X = Xh if parity is None else [_full(x, dims, parity) for x in Xh]
    return numpy_force(U, dims, X, a, scale, project)


def _close(got, want, tol=1e-13):
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    assert err <= tol, err


# ---- 1. the kernel against numpy ------------------------------------------------------------------------------------------
SHAPES = [
    # dims,             half fields possible
    ([64], True),               # the reference's 1-D operator
    ([6, 2, 5], False),         # 3-D, an extent 2 and an odd extent: full fields only
    ([4, 6, 2], True),          # 3-D with an extent 2
    ([8, 4, 2, 6], True),       # 4-D with an extent 2
    ([5, 4, 3, 4], False),      # 4-D, odd extents
    ([16, 4, 4, 4], True),      # 4-D, the specialised stencil at m = 8, 16, 32
]


@pytest.mark.parametrize("dims,halves", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
@pytest.mark.parametrize("m", [1, 3, 8, 12, 16, 32])
def test_kernel_against_numpy(bc, small, dims, halves, m):
    rng = np.random.default_rng(100 + m)
    ctx = bc.Context(dims)
    V, nd = ctx.V, len(dims)
    U = _rand(rng, (V, nd, 3, 3))
    D = bc.dirac_op(ctx, 0.3, U=U)
    for parity in [None, 0, 1] if halves else [None]:
        n = V if parity is None else V // 2
        for S in (1, 4):
            Xh = [_rand(rng, (n, m, 3)) for _ in range(S)]
            a = rng.uniform(-2, 2, S)
            scale = rng.uniform(0.5, 1.5)
            F0 = _rand(rng, (V, nd, 3, 3))
            got = _gpu_force(bc, ctx, D, Xh, a, scale, parity, F0=F0, n_work=S)
            _close(got, F0 + _expected(U, dims, Xh, a, scale, parity))


# ---- 2. the convention: finite difference of the action --------------------------------------------------------------------
def _fd_setup(seed=7):
    rng = np.random.default_rng(seed)
    dims, m, mass = [4, 4, 4, 4], 4, 2.0
    sigma, a = [0.0, 0.25, 1.0], [0.6, -0.9, 1.4]
    V = 256
    U, dU = _rand(rng, (V, 4, 3, 3)), _rand(rng, (V, 4, 3, 3))
    B = _rand(rng, (V, m, 3))
    return dims, m, mass, sigma, a, V, U, dU, B, dense_D(U, dims), dense_D(dU, dims)


def _fd(S, eps=1e-4):
    """dS/de at 0 by the fourth-order central difference.  (The second-order one at e = 1e-6 is limited to ~1e-7 by the rounding
    of S itself: |S| is a few hundred here, |dS| below one.)"""
    return (8 * (S(eps) - S(-eps)) - (S(2 * eps) - S(-2 * eps))) / (12 * eps)


@pytest.mark.parametrize("solver", ["dense", "sbcgrq"])
def test_finite_difference_full_fields(bc, small, solver):
    dims, m, mass, sigma, a, V, U, dU, B, D0, Dd = _fd_setup()
    ctx = bc.Context(dims)
    D = bc.dirac_op(ctx, mass, U=U)
    if solver == "dense":
        A = mass * mass * np.eye(3 * V) - D0 @ D0
        Xh = [from_vec(np.linalg.solve(A + s * np.eye(3 * V), to_vec(B)), V) for s in sigma]
        tol = 1e-7
    else:
        X = [bc.block_fermion_field(ctx, m) for _ in sigma]
        bc.SBCGrQ(X, bc.block_fermion_field(ctx, m, B), D, sigma, 1e-12, 1e-12)
        Xh = [x.download() for x in X]
        tol = 1e-6
    G = to_host(_gpu_force(bc, ctx, D, Xh, a, 1.0))
    dS = derivative(G, to_host(dU))
    fd = _fd(lambda e: action(D0 + e * Dd, mass, to_vec(B), sigma, a))
    assert abs(fd - dS) <= tol * abs(fd), (fd, dS)


@pytest.mark.parametrize("parity", [0, 1])
def test_finite_difference_half_fields(bc, small, parity):
    """The parity-p action S_p = sum_s a_s B_p^dag (A_pp + sigma_s)^-1 B_p, A_pp the dense A restricted to parity p."""
    dims, m, mass, sigma, a, V, U, dU, B, D0, Dd = _fd_setup(8 + parity)
    ctx = bc.Context(dims)
    D = bc.dirac_op(ctx, mass, U=U)
    sites = _parity_sites(dims, parity)
    rows = (3 * sites[:, None] + np.arange(3)).ravel()  # vector indices 3 x + c of the parity-p sites

    def action_p(Dm):
        A = (mass * mass * np.eye(3 * V) - Dm @ Dm)[np.ix_(rows, rows)]
        Bv = to_vec(B[sites])
        return sum(ak * np.trace(Bv.conj().T @ np.linalg.solve(A + s * np.eye(len(rows)), Bv)).real for s, ak in zip(sigma, a))

    App = (mass * mass * np.eye(3 * V) - D0 @ D0)[np.ix_(rows, rows)]
    Xh = [from_vec(np.linalg.solve(App + s * np.eye(len(rows)), to_vec(B[sites])), len(sites)) for s in sigma]
    G = to_host(_gpu_force(bc, ctx, D, Xh, a, 1.0, parity=parity))
    fd = _fd(lambda e: action_p(D0 + e * Dd))
    dS = derivative(G, to_host(dU))
    assert abs(fd - dS) <= 1e-7 * abs(fd), (fd, dS)


# ---- 3. projection ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", [None, 0])
@pytest.mark.parametrize("m", [3, 16])
def test_projection(bc, small, parity, m):
    rng = np.random.default_rng(21 + m)
    dims = [16, 4, 4, 4]
    ctx = bc.Context(dims)
    V = ctx.V
    U = _rand(rng, (V, 4, 3, 3))
    D = bc.dirac_op(ctx, 0.3, U=U)
    n = V if parity is None else V // 2
    Xh = [_rand(rng, (n, m, 3)) for _ in range(3)]
    a = [0.5, -1.5, 2.0]
    raw = to_host(_gpu_force(bc, ctx, D, Xh, a, 0.75, parity))
    proj = to_host(_gpu_force(bc, ctx, D, Xh, a, 0.75, parity, project=True))
    want = ta(to_host(U) @ raw)
    _close(proj, want)
    scale = np.max(np.abs(proj))
    assert np.max(np.abs(proj + np.conj(np.swapaxes(proj, -1, -2)))) <= 1e-14 * scale   # anti-Hermitian
    assert np.max(np.abs(np.trace(proj, axis1=-2, axis2=-1))) <= 1e-14 * scale          # traceless
    # the projected form accumulates too, and is that of the numpy force
    F0 = _rand(rng, (V, 4, 3, 3))
    _close(_gpu_force(bc, ctx, D, Xh, a, 0.75, parity, F0=F0, project=True), F0 + to_host(proj))
    _close(to_host(_expected(U, dims, Xh, a, 0.75, parity, project=True)), want)


# ---- 4. work fields ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", [None, 1])
def test_work_fields_do_not_change_the_result(bc, small, parity):
    rng = np.random.default_rng(31)
    dims, m, S = [16, 4, 4, 4], 16, 5
    ctx = bc.Context(dims)
    V = ctx.V
    D = bc.dirac_op(ctx, 0.3, seed=32)
    n = V if parity is None else V // 2
    Xh = [_rand(rng, (n, m, 3)) for _ in range(S)]
    a = rng.uniform(-1, 1, S)
    F0 = _rand(rng, (V, 4, 3, 3))
    ref = _gpu_force(bc, ctx, D, Xh, a, 1.3, parity, F0=F0, n_work=0)
    for n_work in (1, 2, S, 9):  # 2: a launch of two, two and one shift; 9: more than the shifts
        got = _gpu_force(bc, ctx, D, Xh, a, 1.3, parity, F0=F0, n_work=n_work)
        assert np.max(np.abs(got - ref)) <= 1e-14 * np.max(np.abs(ref)), n_work


def test_failed_allocation_leaves_F_untouched(bc, small):
    """BCG_DEBUG_FIELD_BUDGET (the library's stand-in for a full device): room for the caller's fields only, so the work
    field of n_work = 0 cannot be allocated -- a clean BCG_ERR_HIP, F as it was; with a work field passed the call runs."""
    dims, m = [16, 4, 4, 4], 8
    field = 16 * 4 * 4 * 4 * 3 * m * 16
    small.setenv("BCG_DEBUG_FIELD_BUDGET", str(3 * field))  # X_0, X_1 and W
    ctx = bc.Context(dims)
    D = bc.dirac_op(ctx, 0.3, seed=41)
    X = [bc.block_fermion_field(ctx, m).setRandom(seed=42 + s) for s in range(2)]
    W = bc.block_fermion_field(ctx, m)
    F = bc.gauge_field(ctx).setRandom(seed=44)
    before = F.download()
    with pytest.raises(bc.BlockCGError) as e:
        bc.fermion_force(F, X, D, [1.0, 2.0])
    assert e.value.code == 3
    assert np.array_equal(F.download(), before)
    bc.fermion_force(F, X, D, [1.0, 2.0], work=[W])
    assert not np.array_equal(F.download(), before)


# ---- 5. argument checks ----------------------------------------------------------------------------------------------------
def test_invalid_arguments(bc, small):
    from blockcg_amd.api import _dp
    dims, m = [8, 4, 4, 4], 8
    ctx = bc.Context(dims)
    other = bc.Context(dims)
    D = bc.dirac_op(ctx, 0.3, seed=51)
    X = [bc.block_fermion_field(ctx, m).setRandom(seed=52 + s) for s in range(2)]
    F = bc.gauge_field(ctx).setRandom(seed=54)
    before = F.download()
    good = np.array([1.0, -0.5])

    def call(Xs, res=good, scale=1.0, Fh=None, Uh=None, work=(), ctxh=None, n=None):
        Xa = (ctypes.c_void_p * max(1, len(Xs)))(*[x.h for x in Xs])
        Wa = (ctypes.c_void_p * max(1, len(work)))(*[w.h for w in work])
        return ctx.lib.bcg_force_accumulate(ctxh or ctx.h, Uh or D.h, Xa, len(Xs) if n is None else n,
                                            None if res is None else _dp(np.ascontiguousarray(res, dtype=np.float64)), scale, 0,
                                            Wa if work else None, len(work), Fh or F.h)

    wide = bc.block_fermion_field(ctx, m + 1)
    half0, half1 = bc.block_fermion_field(ctx, m, parity=0), bc.block_fermion_field(ctx, m, parity=1)
    foreign = bc.block_fermion_field(other, m)
    F_other, D_other = bc.gauge_field(other), bc.dirac_op(other, 0.3, seed=1)
    assert call(X, Fh=D.h) == 1                                   # F == U
    assert call(X, Fh=F_other.h) == 1                             # F of another context
    assert call(X, Uh=D_other.h) == 1                             # U of another context
    assert call([X[0], foreign]) == 1                             # an X of another context
    assert call([X[0], wide]) == 1                                # mixed widths
    assert call([X[0], half0]) == 1                               # mixed parities
    assert call([half0, half1]) == 1
    assert call(X, n=0) == 1                                      # n_shifts < 1
    assert call(X, res=[1.0, np.nan]) == 1                        # non-finite residue
    assert call(X, res=[np.inf, 1.0]) == 1
    assert call(X, res=None) == 1
    assert call(X, scale=np.nan) == 1                             # non-finite scale
    assert call(X, scale=-np.inf) == 1
    assert call(X, work=[wide]) == 1                              # work field of the wrong width
    assert call(X, work=[half0]) == 1                             # ... of the wrong parity
    assert call(X, work=[X[1]]) == 1                              # ... aliasing an X
    W = bc.block_fermion_field(ctx, m)
    assert call(X, work=[W, W]) == 1                              # ... listed twice
    assert call([half0, half0], work=[half1]) == 1                # half X, work of the other parity
    assert call(X, work=[foreign]) == 1                           # ... of another context
    assert np.array_equal(F.download(), before)
    with pytest.raises(ValueError):
        bc.fermion_force(F, X, D, [1.0])
    assert call(X, work=[W]) == 0                                 # and the context still works
    W0 = bc.block_fermion_field(ctx, m, parity=0)
    assert call([half0.setZero(), half0], work=[W0]) == 0


# ---- 6. production geometry -------------------------------------------------------------------------------------------------
def test_production_geometry_sampled(bc, orc, monkeypatch):
    """32^4, m = 16, S = 4 with the default tuning (the specialised stencil over the whole lattice): F at ~1000 sites (wrap
    corners, faces, tile borders, random) against the numpy formula on their neighbourhood, Y from the oracle's sampled
    evaluator of D on the counter-based generator's U and X (independent of the device stencil)."""
    from test_fullsize_parity import chosen_sites
    for k in ("BCG_HOP_BLOCKS", "BCG_HOP_PATCH", "BCG_PAIR_SHIFTS"):
        monkeypatch.delenv(k, raising=False)
    dims, m, seed_U = [32, 32, 32, 32], 16, 61
    seeds, a, scale = [62, 63, 64, 65], [0.9, -0.4, 1.6, 0.3], 0.8
    ctx = bc.Context(dims)
    D = bc.dirac_op(ctx, 0.3, seed=seed_U)
    X = [bc.block_fermion_field(ctx, m).setRandom(seed=s) for s in seeds]
    F = bc.gauge_field(ctx).setZero()
    ctx.profiling(True)
    bc.fermion_force(F, X, D, a, scale, work=[bc.block_fermion_field(ctx, m) for _ in seeds])
    prof = ctx.profile()
    assert prof["force"]["count"] == 1 and prof["hop"]["count"] == 4, sorted(prof)
    Fh = F.download()
    sites = chosen_sites(dims)
    c = np.stack([sites % 32, sites // 32 % 32, sites // 1024 % 32, sites // 32768], axis=1)
    strides = np.array([1, 32, 1024, 32768])
    G = np.zeros((len(sites), 4, 3, 3), dtype=np.complex128)
    for s, ak in zip(seeds, a):
        x0 = X[seeds.index(s)].download_sites(sites)
        y0 = orc.hop_sampled(m, dims, seed_U, s, sites)
        for mu in range(4):
            cp = c.copy()
            cp[:, mu] = (cp[:, mu] + 1) % 32
            nb = cp @ strides
            x1 = X[seeds.index(s)].download_sites(nb)
            y1 = orc.hop_sampled(m, dims, seed_U, s, nb)
            eta = (-1.0) ** (c[:, :mu].sum(axis=1) % 2)
            t = np.einsum("vjr,vjc->vrc", y1, x0.conj()) - np.einsum("vjr,vjc->vrc", x1, y0.conj())
            G[:, mu] += scale * ak * eta[:, None, None] * t
    _close(Fh[sites], to_host(G))


# ---- 7. the C++ drop-in ----------------------------------------------------------------------------------------------------
def test_cpp_dropin_force_probe(bc, small, tmp_path):
    from test_force_cpu import build_force_probe
    exe = build_force_probe()
    out = tmp_path / "force.bin"
    r = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, BCG_HOP_PATCH="16,2,2", BCG_HOP_BLOCKS="32"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FORCE_OK" in r.stdout, r.stdout
    dims, m = [8, 4, 4, 6], 8
    ctx = bc.Context(dims)
    D = bc.dirac_op(ctx, 0.3, seed=51)
    X = [bc.block_fermion_field(ctx, m).setRandom(seed=52 + s) for s in range(4)]
    a = [0.7, -1.3, 2.5, 0.25]
    F = bc.gauge_field(ctx).setRandom(seed=60)
    P = bc.gauge_field(ctx).setZero()
    bc.fermion_force(F, X, D, a, 0.5)
    bc.fermion_force(P, X, D, a, 0.5, project=True)
    cpp = np.fromfile(out, dtype=np.complex128).reshape(2, ctx.V, 4, 3, 3)
    _close(cpp[0], F.download(), 1e-14)
    _close(cpp[1], P.download(), 1e-14)
