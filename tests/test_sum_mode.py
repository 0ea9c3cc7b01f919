"""Sum mode of SBCGrQ (bcg_sbcgrq_begin_sum / bcg_sbcgrq_solve_sum, SBCGrQ_sum): Y = c0 B + sum_s a_s X_s accumulated in the
phase C kernels instead of keeping the n_shifts solution fields.  The solve itself is the ordinary one, so the trace and the
iteration count are bit-identical; with unit residues Y is X_k bit for bit (the other shifts add exact zeros, in the same
order)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden, rel_err

pytestmark = pytest.mark.gpu

TRACE_KEYS = ("alpha", "rho", "delta", "alpha_s", "beta_s", "residual", "residual_shift")


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


def _ordinary(bc, ctx, D, Bh, m, shifts, eps, eps_s, iters, parity=None, trace=0):
    B = bc.block_fermion_field(ctx, m, Bh, parity=parity)
    X = [bc.block_fermion_field(ctx, m, parity=parity) for _ in shifts]
    info = bc.SBCGrQ(X, B, D, shifts, eps, eps_s, max_iterations=iters, trace_limit=trace, return_info=True)
    return np.stack([x.download() for x in X]), info


def _summed(bc, ctx, D, Bh, m, shifts, a, c0, eps, eps_s, iters, parity=None, trace=0):
    B = bc.block_fermion_field(ctx, m, Bh, parity=parity)
    Y = bc.block_fermion_field(ctx, m, parity=parity)
    info = bc.SBCGrQ_sum(Y, B, D, shifts, a, c0, eps, eps_s, max_iterations=iters, trace_limit=trace, return_info=True)
    return Y.download(), info


def _expected(Bh, X, a, c0):
    ref = c0 * Bh + sum(ak * x for ak, x in zip(a, X))
    scale = abs(c0) * np.linalg.norm(Bh) + sum(abs(ak) * np.linalg.norm(x) for ak, x in zip(a, X))
    return ref, scale


def _host_B(orc, m, V, seed):
    return orc.fill_field(m, V, seed)


# ---- 1. unit residues reproduce each X_s bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize("m", [8, 16, 32])
@pytest.mark.parametrize("S", [4, 1])
@pytest.mark.parametrize("pair,defer", [(0, 0), (0, 1), (2, 0), (2, 1), (4, 0), (4, 1)])
def test_unit_residues_reproduce_each_shift(bc, orc, small, m, S, pair, defer):
    small.setenv("BCG_PAIR_SHIFTS", str(pair))
    small.setenv("BCG_DEFER_X0", str(defer))
    dims, mass, iters = [16, 4, 4, 4], 0.2, 7  # 7 = a group of four and a short one of three
    shifts = [0.0, 1e-3, 0.1, 2.0][:S]
    ctx = bc.Context(dims)
    D = bc.dirac_op(ctx, mass, seed=31)
    Bh = _host_B(orc, m, ctx.V, 32)
    X, info = _ordinary(bc, ctx, D, Bh, m, shifts, 0.0, 0.0, iters)
    assert info["iterations"] == iters
    for k in range(S):
        Y, yi = _summed(bc, ctx, D, Bh, m, shifts, np.eye(S)[k], 0.0, 0.0, 0.0, iters)
        assert yi["iterations"] == iters
        assert np.array_equal(Y, X[k]), (k, rel_err(Y, X[k]))


def test_unit_residues_in_capacity_mode(bc, orc, small):
    """Capacity mode groups in pairs and defers X_0 in the spare-less form (A_1 + M, -M on the host)."""
    dims, m, mass, iters = [32, 4, 4, 12], 16, 0.2, 7
    shifts = [0.0, 1e-3, 0.1, 2.0]
    ctx = bc.Context(dims)
    ctx.capacity_mode(4)
    ctx.profiling(True)
    D = bc.dirac_op(ctx, mass, seed=33)
    Bh = _host_B(orc, m, ctx.V, 34)
    X, _ = _ordinary(bc, ctx, D, Bh, m, shifts, 0.0, 0.0, iters)
    ctx.profile_reset()
    for k in range(len(shifts)):
        Y, _ = _summed(bc, ctx, D, Bh, m, shifts, np.eye(len(shifts))[k], 0.0, 0.0, 0.0, iters)
        assert np.array_equal(Y, X[k]), k
    prof = ctx.profile()
    assert prof["phaseC_multi2_sum"]["count"] >= 4 and "phaseC_multi2" not in prof
    assert prof["phaseC_p0"]["count"] >= 4  # the spare-less X_0 form ran


# ---- 2. general residues: tolerance for Y, bit-identical solve ------------------------------------------------------
def _compare_general(bc, ctx, D, Bh, m, shifts, a, c0, eps, eps_s, iters=100000, parity=None):
    X, info = _ordinary(bc, ctx, D, Bh, m, shifts, eps, eps_s, iters, parity, trace=400)
    Y, yi = _summed(bc, ctx, D, Bh, m, shifts, a, c0, eps, eps_s, iters, parity, trace=400)
    assert yi["iterations"] == info["iterations"]
    for key in TRACE_KEYS:
        assert np.array_equal(yi["trace"][key], info["trace"][key]), key
    ref, scale = _expected(Bh, X, a, c0)
    assert np.linalg.norm(Y - ref) / scale < 1e-12
    return X, Y, info


@pytest.mark.parametrize("m,dims", [(16, [16, 4, 4, 4]), (5, [8, 4, 4, 2])])
def test_general_residues(bc, orc, small, m, dims):
    shifts, a, c0 = [0.0, 1e-3, 0.1, 2.0], [0.7, -1.3, 2.5, 0.25], 0.4
    ctx = bc.Context(dims)
    ctx.profiling(True)
    D = bc.dirac_op(ctx, 0.2, seed=35)
    Bh = _host_B(orc, m, ctx.V, 36)
    _compare_general(bc, ctx, D, Bh, m, shifts, a, c0, 1e-10, 1e-12)
    prof = ctx.profile()
    if m == 16:
        assert prof["phaseC_multi4_sum"]["count"] >= 1  # grouped
        # byte model: ns + 2 n + 2 (+1) rows against ns + 4 n (+1)
        assert prof["phaseC_multi4_sum"]["bytes"] / prof["phaseC_multi4_sum"]["count"] < \
            prof["phaseC_multi4"]["bytes"] / prof["phaseC_multi4"]["count"]


def test_general_residues_nine_shifts_generic_width(bc):
    """m = 12 (generic right-multiplications, K5 launches on Y) with the nine shifts of the reference's benchmark driver."""
    g = load_golden("ref1d_v48_m12.npz")
    ctx = bc.Context([int(d) for d in g["dims"]])
    D = bc.dirac_op(ctx, float(g["mass"]), U=g["U"])
    shifts = list(g["shifts"])
    a = np.linspace(0.1, 0.9, len(shifts))
    _compare_general(bc, ctx, D, g["B"], 12, shifts, a, 0.3, float(g["eps"]), float(g["eps_shifts"]))


# ---- 3. against the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,dims,S", [(16, [8, 8, 8, 8], 4), (32, [4, 4, 4, 4], 8)])
def test_fixed_work_against_oracle(bc, orc, m, dims, S):
    mass = 0.05
    shifts = [0.0, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1.0][:S]
    a = [0.5 + 0.25 * s for s in range(S)]
    c0 = 0.75
    ctx = bc.Context(dims)
    D = bc.dirac_op(ctx, mass, seed=3)
    B = bc.block_fermion_field(ctx, m).setRandom(seed=4)
    Y = bc.block_fermion_field(ctx, m)
    it = bc.SBCGrQ_sum(Y, B, D, shifts, a, c0, 0.0, 0.0, max_iterations=6)
    U = orc.fill_gauge(dims, 3)
    Bh = orc.fill_field(m, ctx.V, 4)
    o = orc.sbcgrq(U, dims, mass, Bh, shifts, 0.0, 0.0, max_iterations=6, trace_limit=6)
    assert it == o["iterations"] == 6
    ref = c0 * Bh + sum(ak * x for ak, x in zip(a, o["X"]))
    assert rel_err(Y.download(), ref) < 1e-11


# ---- 4. reference fixtures -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ref1d_v48_m12.npz", "ref4d_4x4x2x2_m16.npz"])
def test_reference_fixtures(bc, name):
    g = load_golden(name)
    m = g["B"].shape[1]
    shifts, eps, eps_s = list(g["shifts"]), float(g["eps"]), float(g["eps_shifts"])
    a = np.linspace(1.0, 0.2, len(shifts))
    c0 = 0.5
    ctx = bc.Context([int(d) for d in g["dims"]])
    D = bc.dirac_op(ctx, float(g["mass"]), U=g["U"])
    X, info = _ordinary(bc, ctx, D, g["B"], m, shifts, eps, eps_s, 100000)
    Y, yi = _summed(bc, ctx, D, g["B"], m, shifts, a, c0, eps, eps_s, 100000)
    assert yi["iterations"] == info["iterations"] and abs(info["iterations"] - int(g["iterations"])) <= 1
    ref, _ = _expected(g["B"], g["X"], a, c0)
    ordinary_sum = c0 * g["B"] + sum(ak * x for ak, x in zip(a, X))
    assert rel_err(Y, ref) <= 2 * max(rel_err(ordinary_sum, ref), 1e-15)


# ---- 5. retirement ---------------------------------------------------------------------------------------------------
def test_retired_shifts_stop_contributing(bc):
    g = load_golden("extra/ref1d_v96_m4_retire.npz")
    m = g["B"].shape[1]
    shifts = list(g["shifts"])
    ctx = bc.Context([int(d) for d in g["dims"]])
    D = bc.dirac_op(ctx, float(g["mass"]), U=g["U"])
    X, Y, info = _compare_general(bc, ctx, D, g["B"], m, shifts, [1.0, 0.5, 0.25, 0.125], 0.0, float(g["eps"]),
                                  float(g["eps_shifts"]))
    visited = info["trace"]["residual_shift"][:info["iterations"]] >= 0
    assert not visited[-1, 1:].all()  # at least one shift retired before the end


# ---- 6. failure inside a group --------------------------------------------------------------------------------------
def test_error_inside_a_group(bc, orc, small):
    """BCG_DEBUG_FAIL_ITER=3: two iterations of a depth-4 group are pending at the failure; they are flushed into Y."""
    small.setenv("BCG_PAIR_SHIFTS", "4")
    small.setenv("BCG_DEBUG_FAIL_ITER", "3")
    dims, m, mass = [16, 8, 8, 8], 16, 0.2
    shifts, a, c0 = [0.0, 1e-3, 0.1, 2.0], [0.9, 0.6, 0.3, 0.1], 0.2
    ctx = bc.Context(dims)
    D = bc.dirac_op(ctx, mass, seed=91)
    Bh = _host_B(orc, m, ctx.V, 92)
    B = bc.block_fermion_field(ctx, m, Bh)
    X = [bc.block_fermion_field(ctx, m) for _ in shifts]
    st = bc.SBCGrQState(X, B, D, shifts, 0.0, 0.0)
    with pytest.raises(bc.BlockCGError) as e:
        st.iterate(12)
    assert e.value.code == 6
    st.end()
    Xh = np.stack([x.download() for x in X])
    B2 = bc.block_fermion_field(ctx, m, Bh)
    Y = bc.block_fermion_field(ctx, m)
    sst = bc.SBCGrQSumState(Y, B2, D, shifts, a, c0, 0.0, 0.0)
    with pytest.raises(bc.BlockCGError) as e:
        sst.iterate(12)
    assert e.value.code == 6
    with pytest.raises(bc.BlockCGError) as e2:
        sst.iterate(1)
    assert e2.value.code == 1
    sst.end()
    ref, scale = _expected(Bh, Xh, a, c0)
    Yh = Y.download()
    assert np.isfinite(Yh).all() and np.linalg.norm(Yh - ref) / scale < 1e-13
    assert np.abs(Xh[1]).max() > 0


# ---- 7. half-volume ----------------------------------------------------------------------------------------------------
def test_half_volume_fields(bc, orc, small):
    dims, m = [16, 4, 4, 4], 16
    ctx = bc.Context(dims)
    D = bc.dirac_op(ctx, 0.2, seed=37)
    full = bc.block_fermion_field(ctx, m).setRandom(seed=38)
    Bh = full.split_parity()[1].download()
    _compare_general(bc, ctx, D, Bh, m, [0.0, 1e-2, 0.5], [1.5, 0.5, 0.25], 0.1, 1e-10, 1e-12, parity=1)


# ---- 8. arguments --------------------------------------------------------------------------------------------------------
def test_invalid_arguments(bc):
    from blockcg_amd.api import _dp
    ctx = bc.Context([8, 4, 4, 4])
    D = bc.dirac_op(ctx, 0.2, seed=39)
    m = 8
    B = bc.block_fermion_field(ctx, m).setRandom(seed=40)
    Y = bc.block_fermion_field(ctx, m)
    sig = np.array([0.0, 0.1])
    good = np.array([1.0, 0.5])
    it = ctypes.c_int(0)
    res = ctypes.c_double(0.0)

    def call(Yh, res_arr, c0=0.0):
        return ctx.lib.bcg_sbcgrq_solve_sum(ctx.h, D.h, D.mass, Yh, B.h, 2, _dp(sig),
                                            None if res_arr is None else _dp(res_arr), c0, 1e-10, 1e-12, 0, 100,
                                            ctypes.byref(it), ctypes.byref(res), None)

    wide = bc.block_fermion_field(ctx, m + 8)
    half = bc.block_fermion_field(ctx, m, parity=0)
    assert call(Y.h, None) == 1                          # no residues
    assert call(Y.h, np.array([1.0, np.nan])) == 1       # non-finite residue
    assert call(Y.h, np.array([np.inf, 1.0])) == 1
    assert call(Y.h, good, c0=np.nan) == 1               # non-finite c0
    assert call(Y.h, good, c0=-np.inf) == 1
    assert call(B.h, good) == 1                          # Y == B
    assert call(wide.h, good) == 1                       # width differs
    assert call(half.h, good) == 1                       # parity differs
    with pytest.raises(ValueError):
        bc.SBCGrQ_sum(Y, B, D, sig, [1.0])
    # the context still solves
    n = bc.SBCGrQ_sum(Y, B, D, sig, good, 0.5, 1e-10, 1e-12)
    assert 0 < n < 1000
    X = [bc.block_fermion_field(ctx, m) for _ in sig]
    assert bc.SBCGrQ(X, B, D, sig, 1e-10, 1e-12) == n


# ---- 9. the C++ drop-in on the GPU ----------------------------------------------------------------------------------------
def test_cpp_dropin_sum_probe():
    from test_sum_mode_cpu import build_sum_probe
    exe = build_sum_probe()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, BCG_HOP_PATCH="16,2,2", BCG_HOP_BLOCKS="32"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "SUM_OK" in r.stdout, r.stdout
