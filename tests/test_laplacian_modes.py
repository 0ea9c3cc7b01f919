"""The per-slice Laplacian eigensolver on the device (include/blockcg_hip.h: bcg_laplacian_modes) against its numpy
restatement (tests/laplacian_modes_ref.py) and numpy's eigh per slice, from the restatement's links and start blocks:
[4,4,4,3] along direction 3 and [3,4,4,4] along direction 0, unitary links with upper_bound 12 and general links with
1.02 lambda_max, degree 16, tol 1e-10.

Bounds, those of tests/test_lowmodes.py slice by slice: Ritz values within 10 tol ub of eigh (Hermitian residual bound:
|theta - lambda| <= resid <= tol ub, a factor 10 for the rounding of the comparison); |V(t)^dagger V(t) - 1|_F <= 1e-12
through basis_slice_dot (CholQR2 leaves about K eps = 1e-14); reported residuals within 10 % + 1e-13 ub of those recomputed
from the downloaded vectors.  Where no guard block is involved (its noise is the device's) the outer-iteration count is the
restatement's."""
import os
import subprocess

import numpy as np
import pytest

import basis_ref as ref
import laplacian_modes_ref as lr
from conftest import ROOT, TOL_KERNEL, rel_err

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 2


@pytest.fixture(scope="module")
def bc():
    import blockcg_amd
    return blockcg_amd


_contexts, _links, _stage = {}, {}, {}


def _ctx(bc, dims):
    key = tuple(dims)
    if key not in _contexts:
        _contexts[key] = bc.Context(list(dims))
        _contexts[key].profiling(True)
    return _contexts[key]


def _gauge(bc, dims, direction, unitary=True):
    key = (tuple(dims), direction, unitary)
    if key not in _links:
        ctx = _ctx(bc, dims)
        _links[key] = (ctx, bc.gauge_field(ctx).upload(lr.problem(tuple(dims), direction, unitary)["U"]))
    return _links[key]


def _fields(bc, ctx, block, widths):
    """an [n, K] block as device fields of the given widths"""
    return [bc.block_fermion_field(ctx, w, host=h) for w, h in zip(widths, ref.split_columns(ref.to_field(block), widths))]


def _block(V):
    return ref.to_vec(ref.concat([v.download() for v in V]))


def _rotations(ctx):
    p = ctx.profile()
    return p.get("basis_slice_rotate_mfma", {}).get("count", 0), p.get("basis_slice_rotate_generic", {}).get("count", 0)


def _check(bc, p, V, r, direction, want, first, nf, what, degree=lr.DEGREE, converged=True):
    """everything a result promises, slice by slice; returns the downloaded block"""
    W = _block(V)
    K = W.shape[1]
    ub, rows = p["ub"], p["rows"]
    assert r["evals"].shape == r["resid"].shape == (len(rows), K)
    err = np.abs(r["evals"][:, :want] - p["evals"][:, first:first + want]).max()
    host_resid = np.stack([np.linalg.norm(p["A"][np.ix_(q, q)] @ W[q] - W[q] * r["evals"][t][None, :], axis=0) for t, q in enumerate(rows)])
    gram = np.concatenate([bc.basis_slice_dot(V, v, direction) for v in V], axis=2)  # [L, K, K] on the device
    orth = max(np.linalg.norm(g - np.eye(K)) for g in gram)
    print(f"{what}: {r['iterations']} outer iterations, {r['applications']} applications, Ritz values within {err:.2e} of eigh, "
          f"|V(t)^dagger V(t) - 1| <= {orth:.2e}, worst wanted residual {r['resid'][:, :want].max():.2e}")
    assert r["applications"] == nf * (2 * (r["iterations"] + 1) + degree * r["iterations"])
    assert np.all(np.abs(r["resid"] - host_resid) <= 0.1 * host_resid + 1e-13 * ub), (r["resid"], host_resid)
    assert orth <= 1e-12
    assert np.all(np.diff(r["evals"], axis=1) >= 0)
    if converged:
        assert err <= 10 * lr.TOL * ub
        assert r["resid"][:, :want].max() <= lr.TOL * ub
    return W


def _first_stage(bc, dims, direction, unitary=True):
    """the first stage on the device, run once per case: (fields, result, rotation launches)"""
    key = (tuple(dims), direction, unitary)
    if key not in _stage:
        p = lr.problem(tuple(dims), direction, unitary)
        ctx, links = _gauge(bc, dims, direction, unitary)
        V = _fields(bc, ctx, p["V0"], lr.WIDTHS)
        ctx.profile_reset()
        r = bc.laplacian_modes(V, links, direction, lr.WANT, p["ub"], lr.DEGREE, lr.TOL, 100)
        _stage[key] = (V, r, _rotations(ctx), ctx.profile())
    return _stage[key]


@pytest.mark.parametrize("dims,direction", lr.CASES, ids=["dir3", "dir0"])
def test_laplacian_modes_first_stage(bc, dims, direction):
    p, want = lr.problem(dims, direction), lr.first_stage(dims, direction)
    V, r, rotations, prof = _first_stage(bc, dims, direction)
    _check(bc, p, V, r, direction, lr.WANT, 0, len(lr.WIDTHS), f"{list(dims)} dir {direction}, {list(lr.WIDTHS)} with {lr.WANT} wanted")
    assert r["iterations"] == want["iterations"]
    assert np.abs(r["evals"] - want["evals"])[:, :lr.WANT].max() <= 10 * lr.TOL * p["ub"]
    assert rotations == (2 * (r["iterations"] + 1), 0)  # two rotations over all slices per Ritz step, all in the MFMA form
    assert prof["shift_sum"]["count"] == r["applications"]
    assert "basis_rotate" not in prof and "basis_dot" not in prof  # nothing of the unsliced solver is called


@pytest.mark.parametrize("dims,direction", lr.CASES, ids=["dir3", "dir0"])
def test_laplacian_modes_guard_block_behind_locked(bc, dims, direction):
    """Lock the 32 converged vectors and ask for 16 more in ONE field of 16 columns (K = n_want = 16): eigenvalues 32..47 of
    every slice.  The call carries its guard block of 16 columns; its noise is the device's, so the iteration count is bounded
    (the restatement takes 4 with its own noise), not compared.  And the same field without locked vectors: eigenvalues 0..15."""
    p = lr.problem(dims, direction)
    ctx, links = _gauge(bc, dims, direction)
    V = _first_stage(bc, dims, direction)[0]
    for locked, first in ((V[:1], 32), (None, 0)):
        W = _fields(bc, ctx, p["V1"][:, :16], [16])
        r = bc.laplacian_modes(W, links, direction, 16, p["ub"], lr.DEGREE, lr.TOL, 100, locked=locked)
        _check(bc, p, W, r, direction, 16, first, 2, f"[16] with 16 wanted, {'32 locked' if locked else 'nothing locked'}")
        assert r["iterations"] <= 10
        if locked:
            cross = np.linalg.norm(bc.basis_slice_dot(locked, W[0], direction))
            print(f"|L(t)^dagger W(t)| over the slices = {cross:.2e}")
            assert cross <= 1e-12


def test_laplacian_modes_locked_stage_with_spare_columns(bc):
    """Lock 32, K = 32 as [16,16] with 16 wanted: no guard block, so the restatement's iteration count."""
    dims, direction = lr.CASES[0]
    p = lr.problem(dims, direction)
    ctx, links = _gauge(bc, dims, direction)
    V = _first_stage(bc, dims, direction)[0]
    L = _block(V[:1])
    want = lr.chfsi(p["A"], p["rows"], p["V1"][:, :32], 16, lr.DEGREE, p["ub"], lr.TOL, 100, L=L, nv=2)
    W = _fields(bc, ctx, p["V1"][:, :32], [16, 16])
    r = bc.laplacian_modes(W, links, direction, 16, p["ub"], lr.DEGREE, lr.TOL, 100, locked=V[:1])
    _check(bc, p, W, r, direction, 16, 32, 2, "[16,16] with 16 wanted behind 32 locked")
    assert r["iterations"] == want["iterations"]


@pytest.mark.parametrize("dims,direction", lr.CASES, ids=["dir3", "dir0"])
def test_laplacian_modes_with_general_links(bc, dims, direction):
    """General complex links: the operator stays Hermitian (the Ritz values hold against eigh of the Hermitian dense matrix,
    and <v, A w> = conj(<w, A v>) on the device), its spectrum leaves [0, 12] and the caller's bound takes over."""
    p, want = lr.problem(dims, direction, False), lr.first_stage(dims, direction, False)
    V, r, _, _ = _first_stage(bc, dims, direction, False)
    _check(bc, p, V, r, direction, lr.WANT, 0, 2, f"{list(dims)} dir {direction}, general links, ub = {p['ub']:.3f}")
    assert r["iterations"] == want["iterations"]
    ctx, links = _gauge(bc, dims, direction, False)
    a = bc.block_fermion_field(ctx, 16).setGaussian(1)
    b = bc.block_fermion_field(ctx, 16).setGaussian(2)
    La, Lb = bc.block_fermion_field(ctx, 16), bc.block_fermion_field(ctx, 16)
    bc.laplacian(La, a, links, direction)
    bc.laplacian(Lb, b, links, direction)
    lhs, rhs = b.hermitian_dot(La), Lb.hermitian_dot(a)
    assert np.linalg.norm(lhs - rhs) <= 1e-13 * np.linalg.norm(lhs)


def test_generic_widths_take_the_generic_rotation(bc):
    """[12,12] with 12 wanted: the generic rotation and the generic per-slice products."""
    dims, direction = lr.CASES[0]
    p = lr.problem(dims, direction)
    ctx, links = _gauge(bc, dims, direction)
    V = _fields(bc, ctx, p["V0"][:, :24], [12, 12])
    ctx.profile_reset()
    r = bc.laplacian_modes(V, links, direction, 12, p["ub"], lr.DEGREE, lr.TOL, 100)
    rotations = _rotations(ctx)
    want = lr.chfsi(p["A"], p["rows"], p["V0"][:, :24], 12, lr.DEGREE, p["ub"], lr.TOL, 100, nv=2)
    _check(bc, p, V, r, direction, 12, 0, 2, "[12,12] with 12 wanted")
    assert rotations == (0, 2 * (r["iterations"] + 1))
    assert r["iterations"] == want["iterations"]


def test_iteration_limit_is_no_error(bc):
    dims, direction = lr.CASES[0]
    p = lr.problem(dims, direction)
    ctx, links = _gauge(bc, dims, direction)
    V = _fields(bc, ctx, p["V0"], lr.WIDTHS)
    r = bc.laplacian_modes(V, links, direction, lr.WANT, p["ub"], lr.DEGREE, lr.TOL, 2)  # BCG_OK: no exception
    assert r["iterations"] == 2
    assert r["resid"][:, :lr.WANT].max() > lr.TOL * p["ub"]
    _check(bc, p, V, r, direction, lr.WANT, 0, 2, "max_iterations = 2", converged=False)


def test_computed_basis_projects_idempotently(bc):
    """The computed basis through basis_slice_axpy(basis_slice_dot): V(t) V(t)^dagger b applied twice against once."""
    dims, direction = lr.CASES[0]
    ctx, _ = _gauge(bc, dims, direction)
    V = _first_stage(bc, dims, direction)[0]
    b = bc.block_fermion_field(ctx, 16).setGaussian(9)
    once, twice = bc.block_fermion_field(ctx, 16), bc.block_fermion_field(ctx, 16)
    bc.basis_slice_axpy(once, V, bc.basis_slice_dot(V, b, direction), direction, None, None, 0.0)
    bc.basis_slice_axpy(twice, V, bc.basis_slice_dot(V, once, direction), direction, None, None, 0.0)
    e = rel_err(twice.download(), once.download())
    print(f"projector on the computed basis: {e:.3e}")
    assert e <= TOL_KERNEL
    assert np.linalg.norm(once.download()) > 0.1 * np.linalg.norm(b.download())  # 48 of a slice's 192 dimensions


def test_invalid_and_unsupported_calls(bc):
    dims, direction = lr.CASES[0]
    p = lr.problem(dims, direction)
    ctx, links = _gauge(bc, dims, direction)
    other = _ctx(bc, [4, 4, 4, 2])
    v32 = bc.block_fermion_field(ctx, 32).setGaussian(1)
    v16 = bc.block_fermion_field(ctx, 16).setGaussian(2)
    w32 = bc.block_fermion_field(ctx, 32).setGaussian(3)
    w1 = bc.block_fermion_field(ctx, 1).setGaussian(4)
    foreign = bc.block_fermion_field(other, 16).setGaussian(5)
    # an even lattice for the half fields
    even_ctx = other
    half = [bc.block_fermion_field(even_ctx, 16, parity=0).setGaussian(6), bc.block_fermion_field(even_ctx, 16, parity=0).setGaussian(7)]
    even_links = bc.gauge_field(even_ctx).setRandom(3)
    everything = (v32, v16, w32, w1, foreign) + tuple(half)
    before = [f.download() for f in everything]
    ok = dict(dir=direction, n_want=32, upper_bound=p["ub"], degree=16, tol=1e-10, max_iterations=5)

    def code(V, locked=None, g=links, **kw):
        a = dict(ok, **kw)
        try:
            bc.laplacian_modes(V, g, a["dir"], a["n_want"], a["upper_bound"], a["degree"], a["tol"], a["max_iterations"], locked=locked)
        except bc.BlockCGError as e:
            return e.code
        return 0

    assert code([v32, v16], n_want=0) == INVALID
    assert code([v32, v16], n_want=49) == INVALID
    assert code([v32, v16], degree=1) == INVALID
    assert code([v32, v16], max_iterations=-1) == INVALID
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert code([v32, v16], tol=bad) == INVALID
        assert code([v32, v16], upper_bound=bad) == INVALID
    assert code([v32, v16], dir=-1) == INVALID
    assert code([v32, v16], dir=4) == INVALID
    lib = ctx.lib
    import ctypes
    hv = (ctypes.c_void_p * 2)(v32.h, v16.h)
    ev, rs = np.zeros((3, 48)), np.zeros((3, 48))
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    assert lib.bcg_laplacian_modes(ctx.h, links.h, 4, hv, 2, None, 0, 32, 16, 12.0, 1e-10, 5, dp(ev), dp(rs), None, None) == INVALID
    assert lib.bcg_laplacian_modes(ctx.h, links.h, 3, hv, 2, None, 0, 32, 16, 12.0, 1e-10, 5, None, dp(rs), None, None) == INVALID
    assert lib.bcg_laplacian_modes(ctx.h, None, 3, hv, 2, None, 0, 32, 16, 12.0, 1e-10, 5, dp(ev), dp(rs), None, None) == INVALID
    assert lib.bcg_laplacian_modes(ctx.h, links.h, 3, hv, 0, None, 0, 32, 16, 12.0, 1e-10, 5, dp(ev), dp(rs), None, None) == INVALID
    assert lib.bcg_laplacian_modes(ctx.h, links.h, 3, hv, 2, None, 1, 32, 16, 12.0, 1e-10, 5, dp(ev), dp(rs), None, None) == INVALID
    assert code([v32, v16], locked=[v16]) == INVALID
    assert code([v32, v16], locked=[foreign]) == INVALID
    assert code([v32, foreign]) == INVALID
    assert code([v32, v32]) == INVALID
    assert code([v32, v16], g=even_links) == INVALID  # the links of another context
    assert code([v32, w32, w1]) == UNSUPPORTED
    assert code(half, g=even_links, n_want=16) == UNSUPPORTED  # half fields: one hop flips the parity
    for f, b in zip(everything, before):
        assert np.array_equal(np.ascontiguousarray(f.download()).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _run(exe, ok_line, args=()):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120)
    print(r.stdout)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == ok_line and "FAILED" not in r.stdout, r.stdout + r.stderr


def test_cpp_layer_runs(bc):
    from test_cpp_dropin import _compile
    _run(_compile(os.path.join(ROOT, "tests", "cpp", "laplacian_modes_run_probe.cpp"), "laplacian_modes_run_probe"), "LAPLACIAN_MODES_PROBE_OK")


def test_laplacian_distillation_example(bc):
    """examples/laplacian_distillation.cpp on 4^4: the Laplacian basis of every time slice, then the chain of
    examples/distillation.cpp on it."""
    from test_cpp_dropin import _compile
    _run(_compile(os.path.join(ROOT, "examples", "laplacian_distillation.cpp"), "laplacian_distillation"), "LAPLACIAN_DISTILLATION_OK",
         ["4", "4", "4", "4"])
