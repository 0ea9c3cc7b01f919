"""The fused SBCGrQ row kernels at the edges of their work split, against the oracle and against exact sums.

Phase B (k_phaseB, k_phaseB8, k_phaseB_batched), phase C (k_phaseC, k_phaseC_p0[_batched], k_phaseC_multi and their SUM
forms) and the in-kernel Gram fold (mfma_common.hpp: gram_fold) split a field's 3V rows into 16-row tiles (and, in the
batched m = 16 kernels, 512-row chunks) and fold the block partials over 8 groups.  The solver tests elsewhere run them on
whole tiles and on the default grids only.  Here:
  1. row counts that end in a partial tile (3V % 16 != 0, or 3 V/2 % 16 != 0 for half fields) at m = 8, 16, 32, through
     every fused form the solver has: grouped shift updates, deferred X_0, deferred Q normalisation, sum mode;
  2. phase B / phase C grids of 1 ... 17 blocks (fewer than the fold's 8 groups, not a multiple of 8, groups of one block,
     chunks spread unevenly over the blocks of the batched kernels);
  3. the Gram product against host sums in extended precision, element by element, at row counts around tile and chunk edges;
  4. the fermion force at the lane-group widths with idle lanes and in calls split into several launches.
Rerun reproducibility: tests/test_reproducibility.py."""
import numpy as np
import pytest

from conftest import TOL_COEFF, rel_err
from test_force_cpu import lattice_coords, numpy_force

pytestmark = pytest.mark.gpu

SHIFTS = [0.0, 1e-3, 0.1, 2.0]
MASS = 0.2
COEFFS = ("alpha", "rho", "delta", "alpha_s", "beta_s")
SEED_U, SEED_B = 71, 72


@pytest.fixture(scope="module")
def bc():
    import blockcg_amd
    return blockcg_amd


@pytest.fixture
def env(monkeypatch):
    monkeypatch.setenv("BCG_HOP_PATCH", "16,2,2")  # small lattices: small patches wherever the specialised stencil applies
    return monkeypatch


def _rows(dims, parity=None):
    V = int(np.prod(dims))
    return 3 * (V if parity is None else V // 2)


def _parity_mask(dims, parity):
    return lattice_coords(dims).sum(axis=1) % 2 == parity


_ORACLE = {}


def _oracle(orc, m, dims, iters, shifts=SHIFTS, parity=None):
    """Oracle solve with a fixed number of iterations (cached per module).  parity: B zero on the other parity -- the
    full-volume solve then stays on one parity and is the half-volume solve (op = mass^2 - D^2 keeps the parity)."""
    key = (m, tuple(dims), iters, tuple(shifts), parity)
    if key not in _ORACLE:
        V = int(np.prod(dims))
        U = orc.fill_gauge(dims, SEED_U)
        Bh = orc.fill_field(m, V, SEED_B)
        if parity is not None:
            Bh[~_parity_mask(dims, parity)] = 0.0
        o = orc.sbcgrq(U, dims, MASS, Bh, shifts, 0.0, 0.0, max_iterations=iters, trace_limit=iters)
        assert o["iterations"] == iters
        if parity is not None:
            keep = _parity_mask(dims, parity)
            assert np.abs(o["X"][:, ~keep]).max() == 0.0
            Bh, o["X"] = Bh[keep], o["X"][:, keep]
        _ORACLE[key] = (U, Bh, o)
    return _ORACLE[key]


def _solve(bc, env, dims, m, U, Bh, iters, setting, shifts=SHIFTS, parity=None, residues=None, c0=0.0):
    """One fixed-work solve in a fresh context under the environment `setting`; residues: sum mode (SBCGrQ_sum)."""
    for k, v in setting.items():
        env.setenv(k, str(v))
    ctx = bc.Context(dims)
    ctx.profiling(True)
    D = bc.dirac_op(ctx, MASS, U=U)
    B = bc.block_fermion_field(ctx, m, Bh, parity=parity)
    if residues is None:
        X = [bc.block_fermion_field(ctx, m, parity=parity) for _ in shifts]
        info = bc.SBCGrQ(X, B, D, shifts, 0.0, 0.0, max_iterations=iters, trace_limit=iters, return_info=True)
        out = np.stack([x.download() for x in X])
    else:
        Y = bc.block_fermion_field(ctx, m, parity=parity)
        info = bc.SBCGrQ_sum(Y, B, D, shifts, residues, c0, 0.0, 0.0, max_iterations=iters, trace_limit=iters,
                             return_info=True)
        out = Y.download()
    prof = ctx.profile()
    ctx.close()
    assert info["iterations"] == iters
    return out, info, prof


def _check_against_oracle(X, info, o, what, tol_x=1e-11):
    for s in range(len(X)):
        assert rel_err(X[s], o["X"][s]) < tol_x, (what, s, rel_err(X[s], o["X"][s]))
    for key in COEFFS:
        assert rel_err(info["trace"][key], o["trace"][key]) < TOL_COEFF, (what, key)
    assert np.allclose(info["trace"]["residual"], o["trace"]["residual"], rtol=1e-9), what


def _groups(iters, depth):
    return [g for g in [depth] * (iters // depth) + [iters % depth] if g > 0]


def _check_fused_forms(prof, m, iters, setting, summed=False):
    """The profile shows that the fused kernels the setting selects ran (and not the generic path)."""
    assert prof.get("phaseB", {}).get("count", 0) == iters, (setting, sorted(prof))
    assert "block_axpy" not in prof and "block_xpay" not in prof, (setting, sorted(prof))
    pair = int(setting.get("BCG_PAIR_SHIFTS", 4))
    if m == 32 and int(setting.get("BCG_LAZY_Q", 1)) > 1:
        pair = 0  # un-normalised blocks are not grouped at m = 32 (capi_solvers.hip: pair_shifts_depth)
    defer = int(setting.get("BCG_DEFER_X0", 1)) and m != 32
    sfx = "_sum" if summed else ""
    multi = {k: v["count"] for k, v in prof.items() if k.startswith("phaseC_multi")}
    if pair < 2:
        assert not multi and "phaseC_p0" not in prof, (setting, sorted(prof))
        assert prof["phaseC" + sfx]["count"] == iters, (setting, sorted(prof))
    elif m == 32:  # groups of two over the stored blocks; a closing pass of three shifts takes two launches
        assert multi.get("phaseC_multi2" + sfx, 0) == 2 * (iters // 2), (setting, multi)
    else:
        groups = _groups(iters, pair)
        for g in (2, 3, 4):
            assert multi.get(f"phaseC_multi{g}{sfx}", 0) == sum(1 for x in groups if x == g), (setting, multi)
        assert prof.get("phaseC_p0", {}).get("count", 0) == (sum(g - 1 for g in groups if g >= 2) if defer else 0), \
            (setting, sorted(prof))
    if summed:
        assert not any(k in prof for k in ("phaseC", "phaseC_multi2", "phaseC_multi3", "phaseC_multi4")), sorted(prof)


# ---- 1. the fused solver at ragged row counts ---------------------------------------------------------------------------
# (m, dims, iterations): 3V % 16 != 0 throughout (asserted); 1-D, 2-D, 3-D lattices, a 4-D one whose L0 is not a multiple of
# the stencil tile, and one of 708 whole tiles and a partial one (every block of the persistent grids loops over many tiles).
# The iterations keep the block Krylov space well inside 3V (the oracle in its two Gram summation orders agrees to 1e-13).
RAGGED = [
    (8, [37], 7), (8, [10, 6], 7), (8, [5, 3, 7], 7), (8, [9, 5, 3, 3], 7), (8, [18, 10, 7, 3], 7),
    (16, [101], 7), (16, [14, 10], 7), (16, [5, 3, 7], 7), (16, [9, 5, 3, 3], 7), (16, [18, 10, 7, 3], 7),
    (32, [293], 6), (32, [22, 14], 6), (32, [9, 5, 7], 6), (32, [9, 5, 3, 3], 6), (32, [18, 10, 7, 3], 6),
]
RAGGED_IDS = [f"m{m}-{'x'.join(map(str, d))}" for m, d, _ in RAGGED]


def _settings(m):
    """Grouping depth and the deferred X_0 update (BCG_PAIR_SHIFTS, BCG_DEFER_X0); at m = 32 groups of two only, and the
    deferred normalisation of Q (BCG_LAZY_Q=2) with and without them."""
    if m == 32:
        return [dict(BCG_PAIR_SHIFTS=0), dict(BCG_PAIR_SHIFTS=2),
                dict(BCG_PAIR_SHIFTS=0, BCG_LAZY_Q=2), dict(BCG_PAIR_SHIFTS=2, BCG_LAZY_Q=2)]
    return [dict(BCG_PAIR_SHIFTS=0, BCG_DEFER_X0=0)] + [dict(BCG_PAIR_SHIFTS=d, BCG_DEFER_X0=x) for d in (2, 3, 4) for x in (0, 1)]


@pytest.mark.parametrize("m,dims,iters", RAGGED, ids=RAGGED_IDS)
def test_fused_solver_at_ragged_row_counts(bc, orc, env, m, dims, iters):
    """Gap 1 (ragged rows): phase B's tail tile (BCG_ROW_OK, zero-filled loads, skipped stores) inside the fused Gram
    product, deferred Q normalisation, grouped shift updates and the deferred X_0 update, at m = 8, 16, 32 with S = 4 and a
    fixed number of iterations: every X_s and every coefficient of the trace against the oracle."""
    assert _rows(dims) % 16 != 0
    U, Bh, o = _oracle(orc, m, dims, iters)
    lazy_bytes = {}
    for setting in _settings(m):
        X, info, prof = _solve(bc, env, dims, m, U, Bh, iters, setting)
        _check_against_oracle(X, info, o, setting)
        _check_fused_forms(prof, m, iters, setting)
        if m == 32 and setting["BCG_PAIR_SHIFTS"] == 0:
            lazy_bytes[setting.get("BCG_LAZY_Q", 1)] = prof["phaseC"]["bytes"]
    if m == 32:
        # BCG_LAZY_Q=2 ran its own form: phase C leaves Q un-normalised, (1 + 4 S) field passes against (2 + 4 S)
        S = len(SHIFTS)
        assert lazy_bytes[2] * (2 + 4 * S) == pytest.approx(lazy_bytes[1] * (1 + 4 * S), rel=1e-9)


@pytest.mark.parametrize("m,dims,iters", [RAGGED[i] for i in (0, 3, 6, 9, 12, 14)],
                         ids=[RAGGED_IDS[i] for i in (0, 3, 6, 9, 12, 14)])
def test_sum_mode_at_ragged_row_counts(bc, orc, env, m, dims, iters):
    """Gap 1, sum mode (the SUM instantiations of k_phaseC and k_phaseC_multi) at ragged row counts: unit residues give Y
    equal to the ordinary solve's X_k bit for bit, general residues c0 B + sum_s a_s X_s against the oracle's X_s."""
    assert _rows(dims) % 16 != 0
    U, Bh, o = _oracle(orc, m, dims, iters)
    settings = [dict(BCG_PAIR_SHIFTS=0), dict(BCG_PAIR_SHIFTS=2)] if m == 32 else \
        [dict(BCG_PAIR_SHIFTS=0, BCG_DEFER_X0=1), dict(BCG_PAIR_SHIFTS=3, BCG_DEFER_X0=1), dict(BCG_PAIR_SHIFTS=4, BCG_DEFER_X0=0)]
    a, c0 = [0.7, -1.3, 2.5, 0.25], 0.4
    for setting in settings:
        X, info, _ = _solve(bc, env, dims, m, U, Bh, iters, setting)
        for k in range(len(SHIFTS)):
            Y, yi, prof = _solve(bc, env, dims, m, U, Bh, iters, setting, residues=np.eye(len(SHIFTS))[k])
            assert np.array_equal(Y, X[k]), (setting, k, rel_err(Y, X[k]))
            for key in COEFFS:
                assert np.array_equal(yi["trace"][key], info["trace"][key]), (setting, k, key)
        _check_fused_forms(prof, m, iters, setting, summed=True)
        Y, _, _ = _solve(bc, env, dims, m, U, Bh, iters, setting, residues=a, c0=c0)
        ref = c0 * Bh + sum(ak * x for ak, x in zip(a, o["X"]))
        assert rel_err(Y, ref) < 1e-11, setting


# half-volume lattices with even extents whose compact row count 3 V/2 is not a multiple of 16 (asserted)
# (216 and 1080 rows), with iterations that keep the block Krylov space well inside them
HALF = [(8, [6, 6, 2, 2], 6), (16, [6, 6, 2, 2], 5), (32, [6, 6, 2, 2], 3), (8, [10, 6, 6, 2], 6), (16, [10, 6, 6, 2], 6),
        (32, [10, 6, 6, 2], 6)]


@pytest.mark.parametrize("m,dims,iters", HALF, ids=[f"m{m}-{'x'.join(map(str, d))}" for m, d, _ in HALF])
def test_half_volume_solve_at_ragged_compact_row_counts(bc, orc, env, m, dims, iters):
    """Gap 1, half-volume fields: the compact row count 3 V/2 ends in a partial tile (216 and 1080 rows).  Each parity's
    solve against the full-volume oracle with B zero on the other parity (the same Krylov space), default grouping and with
    every shift updated in every iteration."""
    for parity in (0, 1):
        assert _rows(dims, parity) % 16 != 0
        U, Bh, o = _oracle(orc, m, dims, iters, parity=parity)
        for setting in (dict(BCG_PAIR_SHIFTS=4), dict(BCG_PAIR_SHIFTS=0)):
            X, info, prof = _solve(bc, env, dims, m, U, Bh, iters, setting, parity=parity)
            _check_against_oracle(X, info, o, (parity, setting))
            _check_fused_forms(prof, m, iters, setting)


# ---- 2. odd grids for phase B / phase C and the Gram fold ---------------------------------------------------------------
# [16, 8, 8, 6] at m = 16: 18432 rows = 36 whole 512-row chunks, so phase B grids of 8, 11 and 17 blocks take the batched
# kernel with 5 / 4, 4 / 3 and 3 / 2 chunks per block, and 7 the plain one.  At m = 8 and 32, ragged lattices.
GRIDS_B = (1, 3, 7, 8, 11, 17)
GRIDS_C = (1, 5, 11)


@pytest.mark.parametrize("m,dims", [(16, [16, 8, 8, 6]), (8, [18, 10, 7, 3]), (32, [9, 5, 3, 3])],
                         ids=["m16-16x8x8x6", "m8-18x10x7x3", "m32-9x5x3x3"])
def test_phase_B_and_C_on_odd_grids(bc, orc, env, m, dims):
    """Gap 2 (odd grids) and gap 3 (uneven chunks): BCG_ROW_BLOCKS_B in {1, 3, 7, 8, 11, 17} -- one block, fewer blocks than
    the fold's 8 groups, groups of a single block, grids that are not a multiple of 8 -- crossed with BCG_ROW_BLOCKS_C in
    {1, 5, 11}.  Every run against the oracle, and against the default grid to rounding (only the order of the Gram partial
    sums differs)."""
    iters = 7
    rows = _rows(dims)
    if m == 16:
        assert rows % 512 == 0 and all((rows // 512) % b != 0 for b in (8, 11, 17))
    else:
        assert rows % 16 != 0
    U, Bh, o = _oracle(orc, m, dims, iters)
    Xd, infod, _ = _solve(bc, env, dims, m, U, Bh, iters, {})
    _check_against_oracle(Xd, infod, o, "default grid")
    for b in GRIDS_B:
        for c in GRIDS_C:
            setting = dict(BCG_ROW_BLOCKS_B=b, BCG_ROW_BLOCKS_C=c)
            X, info, prof = _solve(bc, env, dims, m, U, Bh, iters, setting)
            _check_against_oracle(X, info, o, setting)
            assert prof["phaseB"]["count"] == iters
            for s in range(len(SHIFTS)):
                assert rel_err(X[s], Xd[s]) < 1e-13, (setting, s)
            for key in COEFFS:
                assert rel_err(info["trace"][key], infod["trace"][key]) < 1e-13, (setting, key)


def test_batched_phase_B_with_more_chunks_than_blocks(bc, orc, env):
    """Gap 3: [32, 16, 16, 12] at m = 16 has 576 chunks of 512 rows, more than the batched kernels' 256 blocks and not a
    multiple of them (blocks 0-63 take three chunks, the others two); a grid of 17 blocks takes 33 or 34.  Against the
    oracle, and against the plain kernels (BCG_ROW_BATCHED=0) to rounding."""
    m, dims, iters, shifts = 16, [32, 16, 16, 12], 5, [0.0, 0.1]
    rows = _rows(dims)
    assert rows % 512 == 0 and rows // 512 == 576
    U, Bh, o = _oracle(orc, m, dims, iters, shifts)
    plain, pinfo, _ = _solve(bc, env, dims, m, U, Bh, iters, dict(BCG_ROW_BATCHED=0), shifts)
    _check_against_oracle(plain, pinfo, o, "plain")
    for setting in (dict(BCG_ROW_BATCHED=1), dict(BCG_ROW_BATCHED=1, BCG_ROW_BLOCKS_B=17, BCG_ROW_BLOCKS_C=17)):
        X, info, _ = _solve(bc, env, dims, m, U, Bh, iters, setting, shifts)
        _check_against_oracle(X, info, o, setting)
        for s in range(len(shifts)):
            assert rel_err(X[s], plain[s]) < 1e-13, (setting, s)


# ---- 3. the Gram product against exact sums --------------------------------------------------------------------------------
# 1-D lattices whose row count 3V is 16 k +- 1 or 512 k +- 16 (asserted): one row past a tile edge, one short of it, half a
# tile past or short of a chunk edge, at small and at many-block sizes.
GRAM_V = [5, 11, 341, 347, 176, 336, 3408, 10928]


def _exact_gram(a, b):
    """a^dagger b of [n, m] complex matrices, the products and sums in extended precision (64-bit significand: the
    reference's own rounding is 2^-11 of the bound below)."""
    assert np.finfo(np.longdouble).nmant >= 63, "needs an extended-precision long double"
    ar, ai = a.real.astype(np.longdouble), a.imag.astype(np.longdouble)
    br, bi = b.real.astype(np.longdouble), b.imag.astype(np.longdouble)
    return ar.T @ br + ai.T @ bi, ar.T @ bi - ai.T @ br


@pytest.mark.parametrize("m", [8, 16, 32])
def test_hermitian_dot_against_exact_sums(bc, m):
    """Gap 1 for the Gram product itself: G = a^dagger b at every row count of GRAM_V, element by element against the
    extended-precision sum, |G - G_exact| <= 2 n u sum_r |a_ri| |b_rj| for the real and imaginary part separately (the
    standard bound of a 2n-term real sum), so that the small off-diagonal entries of Q^dagger Q are held to account too.
    (hermitian_dot forms the lower triangle and mirrors it, inc/fields.hpp:115-120: the upper one must be its exact mirror.)"""
    u = np.finfo(np.float64).eps / 2
    rng = np.random.default_rng(1000 + m)
    low = np.tril_indices(m)
    for V in GRAM_V:
        n = 3 * V
        assert n % 16 in (1, 15) or n % 512 in (16, 496)
        ctx = bc.Context([V])
        a = rng.uniform(-1, 1, (V, m, 3)) + 1j * rng.uniform(-1, 1, (V, m, 3))
        b = rng.uniform(-1, 1, (V, m, 3)) + 1j * rng.uniform(-1, 1, (V, m, 3))
        if n >= m:
            q = np.linalg.qr(a.transpose(0, 2, 1).reshape(n, m))[0]  # orthonormal columns: off-diagonal entries ~ u
            q = np.ascontiguousarray(q.reshape(V, 3, m).transpose(0, 2, 1))
        for x, y in ((a, b), (q, q)) if n >= m else ((a, b),):
            G = bc.block_fermion_field(ctx, m, x).hermitian_dot(bc.block_fermion_field(ctx, m, y))
            assert np.array_equal(np.triu(G, 1), np.conj(np.tril(G, -1)).T)
            xr, yr = x.transpose(0, 2, 1).reshape(n, m), y.transpose(0, 2, 1).reshape(n, m)
            er, ei = _exact_gram(xr, yr)
            bound = (2 * n * u * (np.abs(xr).T @ np.abs(yr)))[low]
            dr = np.abs(G.real[low].astype(np.longdouble) - er[low]).astype(np.float64)
            di = np.abs(G.imag[low].astype(np.longdouble) - ei[low]).astype(np.float64)
            assert (dr <= bound).all() and (di <= bound).all(), (V, m, float((dr / bound).max()), float((di / bound).max()))
        ctx.close()


# ---- 4. the fermion force at partly idle lane groups and in several launches ---------------------------------------------
FORCE_DIMS = [8, 4, 2, 6]


def _force(bc, ctx, D, Xh, a, scale, parity, F0, project, n_work):
    m = Xh[0].shape[1]
    X = [bc.block_fermion_field(ctx, m, x, parity=parity) for x in Xh]
    F = bc.gauge_field(ctx).upload(F0)
    work = [bc.block_fermion_field(ctx, m, parity=parity) for _ in range(n_work)]
    ctx.profile_reset()
    bc.fermion_force(F, X, D, a, scale, project, work)
    return F.download(), ctx.profile()


def _full(half, dims, parity):
    f = np.zeros((int(np.prod(dims)),) + half.shape[1:], dtype=np.complex128)
    f[_parity_mask(dims, parity)] = half
    return f


def _close(got, want, tol=1e-13):
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    assert err <= tol, err


def _rand(rng, shape):
    return rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)


@pytest.mark.parametrize("m", [2, 5, 7, 17, 24, 31])
def test_force_with_idle_lanes(bc, env, m):
    """Gap 5: k_force's lane groups P = 2 (m = 2), P = 8 with idle lanes (m = 5, 7) and P = 32 with idle lanes (m = 17, 24,
    31), full and half fields, with and without the projection, against the numpy force."""
    rng = np.random.default_rng(500 + m)
    dims = FORCE_DIMS
    ctx = bc.Context(dims)
    ctx.profiling(True)
    V, nd = ctx.V, len(dims)
    U = _rand(rng, (V, nd, 3, 3))
    D = bc.dirac_op(ctx, 0.3, U=U)
    for parity in (None, 1):
        n = V if parity is None else V // 2
        S = 3
        Xh = [_rand(rng, (n, m, 3)) for _ in range(S)]
        a, scale = rng.uniform(-2, 2, S), 0.8
        Xfull = Xh if parity is None else [_full(x, dims, parity) for x in Xh]
        for project in (False, True):
            F0 = _rand(rng, (V, nd, 3, 3))
            got, prof = _force(bc, ctx, D, Xh, a, scale, parity, F0, project, n_work=S)
            assert prof["force_project" if project else "force"]["count"] == 1
            _close(got, F0 + numpy_force(U, dims, Xfull, a, scale, project), 1e-13)


@pytest.mark.parametrize("parity", [None, 0])
def test_force_split_into_several_launches(bc, env, parity):
    """Gap 5: ten shifts with ten work fields (launches of 8 + 2 shifts) and with three (3 + 3 + 3 + 1), against the numpy
    force, with and without the projection."""
    rng = np.random.default_rng(600 if parity is None else 601)
    dims, m, S = FORCE_DIMS, 8, 10
    ctx = bc.Context(dims)
    ctx.profiling(True)
    V, nd = ctx.V, len(dims)
    U = _rand(rng, (V, nd, 3, 3))
    D = bc.dirac_op(ctx, 0.3, U=U)
    n = V if parity is None else V // 2
    Xh = [_rand(rng, (n, m, 3)) for _ in range(S)]
    Xfull = Xh if parity is None else [_full(x, dims, parity) for x in Xh]
    a, scale = rng.uniform(-2, 2, S), 1.25
    for project in (False, True):
        want = numpy_force(U, dims, Xfull, a, scale, project)
        for n_work, launches in ((10, 2), (3, 4)):
            F0 = _rand(rng, (V, nd, 3, 3))
            got, prof = _force(bc, ctx, D, Xh, a, scale, parity, F0, project, n_work)
            assert prof["force_project" if project else "force"]["count"] == launches, (n_work, sorted(prof))
            _close(got, F0 + want, 1e-13)
