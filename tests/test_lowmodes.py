"""The in-place basis rotation and the low-mode eigensolver on the device (include/blockcg_hip.h: bcg_basis_rotate,
bcg_spectral_bound, bcg_lowest_modes) against their numpy restatement (tests/lowmodes_ref.py) and numpy's eigh.

Rotation: TOL_KERNEL against einsum on [5,3,2], [37] (111 rows: a ragged last tile), [4,2,4,2] and both half parities of the
latter; every width list of either form; random, upper-triangular, permutation and identity matrices; the form from the
profile counters; the MFMA form against the generic one; the same bits on a second call; bystanders and failed calls.
Eigensolver: basis_ref.deflation_problem() ([4,4,4,2], mass 0.05, n = 384) from the start blocks of the restatement.
Bounds: Ritz values within 10 tol ub of eigh (Hermitian residual bound: |theta - lambda| <= resid <= tol ub, a factor 10
for the rounding of the comparison); |V^dagger V - 1|_F <= 1e-12 (CholQR2 leaves about K eps = 1e-14); reported residuals
within 10 % + 1e-13 ub of those recomputed from the downloaded vectors."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import basis_ref as ref
import lowmodes_ref as lm
from conftest import ROOT, TOL_KERNEL, TOL_SOLUTION, rel_err

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 2
LATTICES = ([5, 3, 2], [37], [4, 2, 4, 2])
MFMA = ([16], [32], [32, 16], [16, 32, 16], [16, 16, 16, 16])
GENERIC = ([5], [1, 7, 12], [8, 8], [32, 3], [16, 5], [31, 32, 1])


@pytest.fixture(scope="module")
def bc():
    import blockcg_amd
    return blockcg_amd


_contexts = {}


def _ctx(bc, dims):
    key = tuple(dims)
    if key not in _contexts:
        _contexts[key] = bc.Context(list(dims))
        _contexts[key].profiling(True)
    return _contexts[key]


def _bits(x):
    return np.ascontiguousarray(x).view(np.float64)


def _forms(ctx):
    p = ctx.profile()
    return p.get("basis_rotate_mfma", {}).get("count", 0), p.get("basis_rotate_generic", {}).get("count", 0)


def _rotated(bc, ctx, V, hosts, Q, expect):
    """upload hosts, rotate by Q with the launch counts asserted, download"""
    for v, h in zip(V, hosts):
        v.upload(h)
    ctx.profile_reset()
    bc.basis_rotate(V, Q)
    assert _forms(ctx) == expect, (ctx.dims, [v.N_rhs for v in V], _forms(ctx))
    return [v.download() for v in V]


def _rotate_case(bc, ctx, widths, parity, mfma, worst):
    what = (ctx.dims, widths, parity)
    K = sum(widths)
    V = [bc.block_fermion_field(ctx, w, parity=parity).setGaussian(300 + k) for k, w in enumerate(widths)]
    bystander = bc.block_fermion_field(ctx, widths[0], parity=parity).setGaussian(77)
    by = bystander.download()
    hosts = [v.download() for v in V]
    rng = np.random.default_rng(1000 * K + len(widths))
    full = rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K))
    upper = np.triu(full)
    perm = np.eye(K)[:, rng.permutation(K)]
    fast, generic = ((1, 0) if mfma else (0, 1)), (0, 1)
    for Q in (full, upper):
        want = lm.rotate(hosts, Q)
        ctx.force_generic(False)
        got = _rotated(bc, ctx, V, hosts, Q, fast)
        e = max(rel_err(g, w) for g, w in zip(got, want))
        worst[0] = max(worst[0], e)
        assert e <= TOL_KERNEL, (what, e)
        again = _rotated(bc, ctx, V, hosts, Q, fast)  # re-uploaded input: the same bits
        assert all(np.array_equal(_bits(a), _bits(g)) for a, g in zip(again, got)), what
        ctx.force_generic(True)
        gen = _rotated(bc, ctx, V, hosts, Q, generic)
        ctx.force_generic(False)
        assert max(rel_err(g, w) for g, w in zip(gen, want)) <= TOL_KERNEL, what
        assert max(rel_err(g, w) for g, w in zip(got, gen)) <= TOL_KERNEL, what
    for force in (False, True):
        ctx.force_generic(force)
        form = generic if force else fast
        moved = _rotated(bc, ctx, V, hosts, perm, form)  # columns cross fields bit for bit
        assert all(np.array_equal(_bits(a), _bits(w)) for a, w in zip(moved, lm.rotate(hosts, perm))), (what, force)
        same = _rotated(bc, ctx, V, hosts, np.eye(K), form)
        assert all(np.array_equal(_bits(a), _bits(h)) for a, h in zip(same, hosts)), (what, force)
    ctx.force_generic(False)
    assert np.array_equal(_bits(bystander.download()), _bits(by)), what


@pytest.mark.parametrize("widths", MFMA + GENERIC, ids=lambda w: "-".join(map(str, w)))
def test_basis_rotate(bc, widths):
    worst = [0.0]
    mfma = widths in MFMA
    for dims in LATTICES:
        _rotate_case(bc, _ctx(bc, dims), widths, None, mfma, worst)
    for parity in (0, 1):
        _rotate_case(bc, _ctx(bc, [4, 2, 4, 2]), widths, parity, mfma, worst)
    print(f"V widths {widths}: rotation {worst[0]:.3e} relative")


def test_basis_rotate_more_than_one_block(bc):
    """[16,16,8,4]: 98304 rows, 6144 tiles on a grid of 1024 blocks; K = 64 as [32,32] (MFMA) and as [31,32,1] (generic)."""
    ctx = _ctx(bc, [16, 16, 8, 4])
    for widths, form in (([32, 32], (1, 0)), ([31, 32, 1], (0, 1))):
        V = [bc.block_fermion_field(ctx, w).setGaussian(40 + k) for k, w in enumerate(widths)]
        hosts = [v.download() for v in V]
        rng = np.random.default_rng(8)
        Q = rng.standard_normal((64, 64)) + 1j * rng.standard_normal((64, 64))
        got = _rotated(bc, ctx, V, hosts, Q, form)
        e = max(rel_err(g, w) for g, w in zip(got, lm.rotate(hosts, Q)))
        print(f"[16,16,8,4] {widths}: {e:.3e}")
        assert e <= TOL_KERNEL


def test_basis_rotate_invalid_calls_leave_V_alone(bc):
    ctx = _ctx(bc, [4, 2, 4, 2])
    other = _ctx(bc, [37])
    lib = ctx.lib
    v16 = bc.block_fermion_field(ctx, 16).setGaussian(1)
    v5 = bc.block_fermion_field(ctx, 5).setGaussian(2)
    v32a = bc.block_fermion_field(ctx, 32).setGaussian(3)
    v32b = bc.block_fermion_field(ctx, 32).setGaussian(4)
    v1 = bc.block_fermion_field(ctx, 1).setGaussian(5)
    vhalf = bc.block_fermion_field(ctx, 16, parity=1).setGaussian(6)
    foreign = bc.block_fermion_field(other, 16).setGaussian(7)
    everything = (v16, v5, v32a, v32b, v1, vhalf)
    before = [f.download() for f in everything]
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731

    def handles(*fields):
        return (ctypes.c_void_p * max(1, len(fields)))(*[f.h if f is not None else None for f in fields])

    def unchanged():
        return all(np.array_equal(_bits(f.download()), _bits(b)) for f, b in zip(everything, before))

    Q = np.ascontiguousarray(np.full((80, 80), 0.5 + 0.25j))
    bad = Q.copy()
    bad.flat[100] = np.nan  # entries 100 and 440 lie inside the 21 x 21 matrix the calls below read
    worse = Q.copy()
    worse.flat[440] = complex(0.0, np.inf)
    for V, nv, q, want in ((None, 2, Q, INVALID), (handles(v16, v5), 0, Q, INVALID), (handles(v16, v5), -1, Q, INVALID),
                           (handles(v16, None), 2, Q, INVALID), (handles(v16, v5), 2, None, INVALID),
                           (handles(v16, v5, v16), 3, Q, INVALID), (handles(v16, foreign), 2, Q, INVALID),
                           (handles(v16, vhalf), 2, Q, INVALID), (handles(v16, v5), 2, bad, INVALID),
                           (handles(v16, v5), 2, worse, INVALID), (handles(v32a, v32b, v1), 3, Q, UNSUPPORTED)):
        rc = lib.bcg_basis_rotate(V, nv, dp(q) if q is not None else None)
        assert rc == want, (nv, rc, want)
        assert unchanged()
    with pytest.raises(bc.BlockCGError):
        bc.basis_rotate([v32a, v32b, v1], np.eye(65))
    with pytest.raises(ValueError):
        bc.basis_rotate([v16, v5], np.eye(20))
    assert unchanged()


# ---- the eigensolver -------------------------------------------------------------------------------------------------------
def _fields(bc, ctx, block, widths, parity=None):
    """an [n, K] block as device fields of the given widths"""
    return [bc.block_fermion_field(ctx, w, host=h, parity=parity) for w, h in zip(widths, ref.split_columns(ref.to_field(block), widths))]


def _block(V):
    return ref.to_vec(ref.concat([v.download() for v in V]))


def _operator(bc):
    ctx = _ctx(bc, ref.DEFLATION_DIMS)
    return ctx, bc.dirac_op(ctx, mass=ref.DEFLATION_MASS, U=lm.lowmodes_problem()["U"])


_stage = {}


def _first_stage(bc):
    """the first stage on the device, run once: (fields, result, downloaded block)"""
    if "first" not in _stage:
        p = lm.lowmodes_problem()
        ctx, D = _operator(bc)
        V = _fields(bc, ctx, p["V0"], lm.LOWMODES_WIDTHS)
        ctx.profile_reset()
        r = bc.lowest_modes(V, D, lm.LOWMODES_WANT, p["ub"], lm.LOWMODES_DEGREE, lm.LOWMODES_TOL, 100)
        _stage["first"] = (V, r, _block(V), _forms(ctx))
    return _stage["first"]


def test_spectral_bound(bc):
    p = lm.lowmodes_problem()
    ctx, D = _operator(bc)
    lmax = p["evals"][-1]
    for steps, seed in ((10, 1), (10, 2), (4, 3), (64, 4)):
        b = bc.spectral_bound(D, steps, seed)
        print(f"{steps}-step bound, seed {seed}: {b:.6f} = {b / lmax:.4f} lambda_max")
        assert lmax <= b <= 1.5 * lmax, (steps, seed, b, lmax)
    assert bc.spectral_bound(D, 10, 1) == bc.spectral_bound(D, 10, 1)
    for steps in (1, 65, 0, -3):
        out = ctypes.c_double(-1.0)
        assert ctx.lib.bcg_spectral_bound(ctx.h, D.h, D.mass, -1, steps, 1, ctypes.byref(out)) == INVALID
        assert out.value == -1.0
    assert ctx.lib.bcg_spectral_bound(ctx.h, D.h, D.mass, 2, 10, 1, ctypes.byref(ctypes.c_double())) == INVALID


def test_lowest_modes_first_stage(bc):
    p, want = lm.lowmodes_problem(), lm.first_stage()
    V, r, W, forms = _first_stage(bc)
    K, nw, ub, tol = sum(lm.LOWMODES_WIDTHS), lm.LOWMODES_WANT, p["ub"], lm.LOWMODES_TOL
    err = np.abs(r["evals"][:nw] - p["evals"][:nw]).max()
    orth = np.linalg.norm(W.conj().T @ W - np.eye(K))
    host_resid = np.linalg.norm(p["A"] @ W - W * r["evals"][None, :], axis=0)
    print(f"{r['iterations']} outer iterations (restatement {want['iterations']}), {r['applications']} block applications, Ritz "
          f"values within {err:.2e} of eigh, |V^dagger V - 1| = {orth:.2e}, worst wanted residual {r['resid'][:nw].max():.2e}")
    assert err <= 10 * tol * ub
    assert abs(r["iterations"] - want["iterations"]) <= 1
    nv, degree = len(lm.LOWMODES_WIDTHS), lm.LOWMODES_DEGREE
    assert r["applications"] == nv * (2 * (r["iterations"] + 1) + degree * r["iterations"])
    assert np.all(np.abs(r["resid"] - host_resid) <= 0.1 * host_resid + 1e-13 * ub), (r["resid"], host_resid)
    assert r["resid"][:nw].max() <= tol * ub
    assert orth <= 1e-12
    assert np.all(np.diff(r["evals"]) >= 0)
    assert forms[0] == 2 * (r["iterations"] + 1) and forms[1] == 0  # two rotations per Ritz step, all in the MFMA form


def test_lowest_modes_locked_second_stage(bc):
    """Lock the 32 converged vectors, ask for 16 more in ONE field of 16 columns (K = n_want = 16): eigenvalues 32..47, cross
    terms.  The caller brings no columns beyond the wanted ones, so the call carries its guard block of 16 (without one the
    last six columns stand at 5.7e-12 .. 7.0e-5 after 20 outer iterations, on the device and in the restatement alike).  The
    guard's noise is the device's, so the iteration count is bounded, not compared: the restatement takes 11 with its own."""
    p = lm.lowmodes_problem()
    ctx, D = _operator(bc)
    V, _, _, _ = _first_stage(bc)
    W = _fields(bc, ctx, p["V1"][:, :16], [16])
    ctx.profile_reset()
    r = bc.lowest_modes(W, D, 16, p["ub"], lm.LOWMODES_DEGREE, lm.LOWMODES_TOL, 100, locked=V[:1])
    forms = _forms(ctx)
    Wh = _block(W)
    err = np.abs(r["evals"] - p["evals"][32:48])
    cross = np.linalg.norm(bc.basis_dot(V[:1], W[0]))
    host_resid = np.linalg.norm(p["A"] @ Wh - Wh * r["evals"][None, :], axis=0)
    print(f"locked stage [16]: {r['iterations']} outer iterations, |theta - lambda| = {err.max():.2e}, |L^dagger V| = {cross:.2e}")
    assert cross <= 1e-12
    assert err.max() <= 10 * lm.LOWMODES_TOL * p["ub"], err
    assert r["iterations"] <= 20
    assert r["applications"] == 2 * (2 * (r["iterations"] + 1) + lm.LOWMODES_DEGREE * r["iterations"])  # V and the guard field
    assert forms == (2 * (r["iterations"] + 1), 0)  # 16 + 16 columns: the MFMA rotation
    assert r["resid"].max() <= lm.LOWMODES_TOL * p["ub"]
    assert np.all(np.abs(r["resid"] - host_resid) <= 0.1 * host_resid + 1e-13 * p["ub"])
    assert np.linalg.norm(Wh.conj().T @ Wh - np.eye(16)) <= 1e-12


def test_lowest_modes_single_column(bc):
    """K = n_want = 1: the lowest eigenpair, one column and the guard block (the generic rotation)."""
    p = lm.lowmodes_problem()
    ctx, D = _operator(bc)
    V = _fields(bc, ctx, p["V0"][:, :1], [1])
    r = bc.lowest_modes(V, D, 1, p["ub"], lm.LOWMODES_DEGREE, lm.LOWMODES_TOL, 100)
    v = _block(V)
    print(f"[1]: {r['iterations']} outer iterations, theta - lambda_0 = {r['evals'][0] - p['evals'][0]:.2e}")
    assert abs(r["evals"][0] - p["evals"][0]) <= 10 * lm.LOWMODES_TOL * p["ub"]
    assert r["resid"][0] <= lm.LOWMODES_TOL * p["ub"]
    assert abs(np.linalg.norm(v) - 1.0) <= 1e-12
    assert np.linalg.norm(p["A"] @ v - r["evals"][0] * v) <= 1.1 * r["resid"][0] + 1e-13 * p["ub"]


def _second_stage(bc):
    """lock the first stage's 32 wanted vectors, K = 32 as [16,16] with 16 wanted; run once: (fields, result)"""
    if "second" not in _stage:
        p = lm.lowmodes_problem()
        ctx, D = _operator(bc)
        V = _first_stage(bc)[0]
        W = _fields(bc, ctx, p["V1"][:, :32], [16, 16])
        _stage["second"] = (W, bc.lowest_modes(W, D, 16, p["ub"], lm.LOWMODES_DEGREE, lm.LOWMODES_TOL, 100, locked=V[:1]))
    return _stage["second"]


def test_lowest_modes_locked_stage_with_spare_columns(bc):
    """Lock 32, K = 32 as [16,16] with 16 wanted: eigenvalues 32..47, the restatement's iteration count, cross terms."""
    p = lm.lowmodes_problem()
    V, _, W1, _ = _first_stage(bc)
    want = lm.chfsi(p["A"], p["V1"][:, :32], 16, lm.LOWMODES_DEGREE, p["ub"], lm.LOWMODES_TOL, 100, L=W1[:, :32], nv=2)
    W, r = _second_stage(bc)
    err = np.abs(r["evals"][:16] - p["evals"][32:48]).max()
    cross = np.linalg.norm(np.concatenate([bc.basis_dot(V[:1], w) for w in W], axis=1))
    print(f"locked stage [16,16]: {r['iterations']} outer iterations (restatement {want['iterations']}), eigenvalues 32..47 "
          f"within {err:.2e}, |L^dagger V| = {cross:.2e}")
    assert err <= 10 * lm.LOWMODES_TOL * p["ub"]
    assert abs(r["iterations"] - want["iterations"]) <= 1
    assert r["applications"] == 2 * (2 * (r["iterations"] + 1) + lm.LOWMODES_DEGREE * r["iterations"])
    assert cross <= 1e-12


def _parity_rows(bc, ctx, parity):
    """rows 3 x + c of the dense operator that a half field of this parity holds, in its order"""
    tag = np.zeros((ctx.V, 1, 3), dtype=np.complex128)
    tag[:, 0, 0] = np.arange(ctx.V)
    half = bc.block_fermion_field(ctx, 1, host=tag).split_parity()[parity].download()
    sites = np.rint(half[:, 0, 0].real).astype(np.int64)
    return (3 * sites[:, None] + np.arange(3)[None, :]).ravel()


@pytest.mark.parametrize("parity", [0, 1])
def test_lowest_modes_half_parity(bc, parity):
    p = lm.lowmodes_problem()
    ctx, D = _operator(bc)
    rows = _parity_rows(bc, ctx, parity)
    Ap = p["A"][np.ix_(rows, rows)]
    lam = np.linalg.eigvalsh(Ap)
    ub = bc.spectral_bound(D, 10, 7, parity=parity)
    assert lam[-1] <= ub <= 1.5 * lam[-1], (ub, lam[-1])
    rng = np.random.default_rng(50 + parity)
    start = rng.standard_normal((len(rows), 48)) + 1j * rng.standard_normal((len(rows), 48))
    V = _fields(bc, ctx, start, [32, 16], parity=parity)
    r = bc.lowest_modes(V, D, 32, ub, lm.LOWMODES_DEGREE, lm.LOWMODES_TOL, 100)
    want = lm.chfsi(Ap, start, 32, lm.LOWMODES_DEGREE, ub, lm.LOWMODES_TOL, 100, nv=2)
    W = _block(V)
    err = np.abs(r["evals"][:32] - lam[:32]).max()
    orth = np.linalg.norm(W.conj().T @ W - np.eye(48))
    print(f"parity {parity}: {r['iterations']} outer iterations (restatement {want['iterations']}), within {err:.2e} of eigh, "
          f"|V^dagger V - 1| = {orth:.2e}")
    assert err <= 10 * lm.LOWMODES_TOL * ub
    assert abs(r["iterations"] - want["iterations"]) <= 1
    assert r["resid"][:32].max() <= lm.LOWMODES_TOL * ub
    assert orth <= 1e-12


def test_lowest_modes_generic_rotation(bc):
    """[12,12] takes the generic rotation (and the generic basis products): 12 wanted of 24."""
    p = lm.lowmodes_problem()
    ctx, D = _operator(bc)
    V = _fields(bc, ctx, p["V0"][:, :24], [12, 12])
    ctx.profile_reset()
    r = bc.lowest_modes(V, D, 12, p["ub"], lm.LOWMODES_DEGREE, lm.LOWMODES_TOL, 100)
    forms = _forms(ctx)
    want = lm.chfsi(p["A"], p["V0"][:, :24], 12, lm.LOWMODES_DEGREE, p["ub"], lm.LOWMODES_TOL, 100, nv=2)
    err = np.abs(r["evals"][:12] - p["evals"][:12]).max()
    print(f"[12,12]: {r['iterations']} outer iterations (restatement {want['iterations']}), within {err:.2e} of eigh")
    assert forms == (0, 2 * (r["iterations"] + 1))
    assert err <= 10 * lm.LOWMODES_TOL * p["ub"]
    assert abs(r["iterations"] - want["iterations"]) <= 1
    assert r["resid"][:12].max() <= lm.LOWMODES_TOL * p["ub"]


def test_lowest_modes_iteration_limit_is_no_error(bc):
    p = lm.lowmodes_problem()
    ctx, D = _operator(bc)
    V = _fields(bc, ctx, p["V0"], lm.LOWMODES_WIDTHS)
    r = bc.lowest_modes(V, D, lm.LOWMODES_WANT, p["ub"], lm.LOWMODES_DEGREE, lm.LOWMODES_TOL, 2)  # BCG_OK: no exception
    W = _block(V)
    assert r["iterations"] == 2
    assert r["resid"][:lm.LOWMODES_WANT].max() > lm.LOWMODES_TOL * p["ub"]
    assert np.linalg.norm(W.conj().T @ W - np.eye(48)) <= 1e-12
    host_resid = np.linalg.norm(p["A"] @ W - W * r["evals"][None, :], axis=0)
    assert np.all(np.abs(r["resid"] - host_resid) <= 0.1 * host_resid + 1e-13 * p["ub"])


def test_lowest_modes_invalid_calls(bc):
    p = lm.lowmodes_problem()
    ctx, D = _operator(bc)
    v32 = bc.block_fermion_field(ctx, 32).setGaussian(1)
    v16 = bc.block_fermion_field(ctx, 16).setGaussian(2)
    w32 = bc.block_fermion_field(ctx, 32).setGaussian(3)
    w1 = bc.block_fermion_field(ctx, 1).setGaussian(4)
    half = bc.block_fermion_field(ctx, 16, parity=0).setGaussian(5)
    everything = (v32, v16, w32, w1, half)
    before = [f.download() for f in everything]
    ub = p["ub"]
    ok = dict(n_want=32, upper_bound=ub, degree=16, tol=1e-10, max_iterations=5)

    def code(V, locked=None, **kw):
        a = dict(ok, **kw)
        try:
            bc.lowest_modes(V, D, a["n_want"], a["upper_bound"], a["degree"], a["tol"], a["max_iterations"], locked=locked)
        except bc.BlockCGError as e:
            return e.code
        return 0

    assert code([v32, v16], n_want=0) == INVALID
    assert code([v32, v16], n_want=49) == INVALID
    assert code([v32, v16], degree=1) == INVALID
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert code([v32, v16], tol=bad) == INVALID
        assert code([v32, v16], upper_bound=bad) == INVALID
    assert code([v32, v16], locked=[v16]) == INVALID
    assert code([v32, v16], locked=[half]) == INVALID
    assert code([v32, half]) == INVALID
    assert code([v32, v32]) == INVALID
    assert code([v32, w32, w1]) == UNSUPPORTED
    for f, b in zip(everything, before):
        assert np.array_equal(_bits(f.download()), _bits(b))


def test_sbcgrq_deflated_with_computed_modes(bc):
    """The input of test_basis.py's deflated solve with the 48 modes computed here -- the first stage's 32 and 16 from the
    locked stage -- in place of uploaded eigenvectors."""
    d = ref.deflation_problem()
    ctx, D = _operator(bc)
    V, r1, _, _ = _first_stage(bc)
    W, r2 = _second_stage(bc)
    basis = [V[0], W[0]]
    evals = np.concatenate([r1["evals"][:32], r2["evals"][:16]])
    B = bc.block_fermion_field(ctx, ref.DEFLATION_M, host=d["B"])
    sigma = list(ref.DEFLATION_SIGMA)
    X = [bc.block_fermion_field(ctx, ref.DEFLATION_M) for _ in sigma]
    Xp = [bc.block_fermion_field(ctx, ref.DEFLATION_M) for _ in sigma]
    eps = ref.DEFLATION_EPS
    it_deflated = bc.SBCGrQ_deflated(X, B, D, sigma, basis, evals, eps, eps)
    it_plain = bc.SBCGrQ(Xp, B, D, sigma, eps, eps)
    Bv = ref.to_vec(d["B"])
    errs = []
    for s, sg in enumerate(sigma):
        exact = ref.to_field(np.linalg.solve(d["A"] + sg * np.eye(Bv.shape[0]), Bv))
        errs.append(rel_err(X[s].download(), exact))
    print(f"operator applications: {it_deflated} deflated against {it_plain} plain; errors against the dense solve {errs}")
    assert max(errs) <= TOL_SOLUTION, errs
    assert it_deflated <= 0.85 * it_plain, (it_deflated, it_plain)


def _run(exe, ok_line):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == ok_line and "FAILED" not in r.stdout, r.stdout + r.stderr


def test_cpp_lowmodes_layer_runs(bc):
    from test_cpp_dropin import _compile
    _run(_compile(os.path.join(ROOT, "tests", "cpp", "lowmodes_run_probe.cpp"), "lowmodes_run_probe"), "LOWMODES_PROBE_OK")


def test_deflated_solve_example(bc):
    from test_cpp_dropin import _compile
    _run(_compile(os.path.join(ROOT, "examples", "deflated_solve.cpp"), "deflated_solve"), "DEFLATED_SOLVE_OK")
