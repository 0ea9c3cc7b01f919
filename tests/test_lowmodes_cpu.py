"""The low-mode eigensolver without a GPU: the numpy restatement (tests/lowmodes_ref.py) on basis_ref.deflation_problem()
against eigh, the new symbols in the header, the library and the bindings, the drop-in header, and the host
eigen-decomposition (blockcg_amd/csrc/hermitian_eig.hpp) through a stand-alone probe, plain and under
-fsanitize=address,undefined.

Figures of the restatement for the seeds of lowmodes_ref ([4,4,4,2], mass 0.05, n = 384, spectrum [2.67e-3, 14.90]):
10-step bound 18.37 = 1.233 lambda_max; K = 48, 32 wanted, degree 16, tol 1e-10: 14 outer iterations, Ritz values within
1.5e-15 of eigh, |V^dagger V - 1| = 1.1e-14, cond(V^dagger V) <= 1.2e2; locked second stage (K = 48, 32 wanted): 9 outer
iterations, |L^dagger V| = 1.2e-15."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import basis_ref as ref
import lowmodes_ref as lm
from conftest import ROOT

NEW_SYMBOLS = ("bcg_basis_rotate", "bcg_spectral_bound", "bcg_lowest_modes")


def test_rotate_restated_against_a_column_loop():
    rng = np.random.default_rng(3)
    widths = (3, 16, 2)
    V = [ref.random_field(rng, 7, w) for w in widths]
    K = sum(widths)
    Q = rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K))
    got = ref.concat(lm.rotate(V, Q))
    cols = [v[:, k] for v in V for k in range(v.shape[1])]
    for j in range(K):
        want = sum(cols[i] * Q[i, j] for i in range(K))
        assert np.linalg.norm(got[:, j] - want) <= 1e-13 * np.linalg.norm(want)
    assert [g.shape[1] for g in lm.rotate(V, Q)] == list(widths)


def test_bound_brackets_the_spectrum():
    p = lm.lowmodes_problem()
    lmax = p["evals"][-1]
    print(f"10-step bound {p['ub']:.6f} = {p['ub'] / lmax:.4f} lambda_max")
    assert lmax <= p["ub"] <= 1.5 * lmax
    rng = np.random.default_rng(99)
    for _ in range(4):
        v0 = rng.standard_normal(p["A"].shape[0]) + 1j * rng.standard_normal(p["A"].shape[0])
        assert lmax <= lm.lanczos_bound(p["A"], v0, lm.LOWMODES_STEPS) <= 1.5 * lmax


def test_first_stage_restated():
    p, r = lm.lowmodes_problem(), lm.first_stage()
    K = sum(lm.LOWMODES_WIDTHS)
    err = np.abs(r["evals"][:lm.LOWMODES_WANT] - p["evals"][:lm.LOWMODES_WANT]).max()
    orth = np.linalg.norm(r["V"].conj().T @ r["V"] - np.eye(K))
    print(f"{r['iterations']} outer iterations, Ritz values within {err:.2e} of eigh, |V^dagger V - 1| = {orth:.2e}, "
          f"cond(V^dagger V) <= {r['cond']:.2e}")
    assert r["iterations"] <= 20
    assert r["resid"][:lm.LOWMODES_WANT].max() <= lm.LOWMODES_TOL * p["ub"]
    assert err <= 10 * lm.LOWMODES_TOL * p["ub"]
    assert orth <= 1e-12
    assert np.all(np.diff(r["evals"]) >= 0)


def test_locked_second_stage_restated():
    p, r = lm.lowmodes_problem(), lm.first_stage()
    L = r["V"][:, :32]
    r2 = lm.chfsi(p["A"], p["V1"], 32, lm.LOWMODES_DEGREE, p["ub"], lm.LOWMODES_TOL, 100, L=L)
    err = np.abs(r2["evals"][:32] - p["evals"][32:64]).max()
    cross = np.linalg.norm(L.conj().T @ r2["V"])
    print(f"locked stage: {r2['iterations']} outer iterations, eigenvalues 32..63 within {err:.2e}, |L^dagger V| = {cross:.2e}")
    assert r2["iterations"] <= 20
    assert err <= 10 * lm.LOWMODES_TOL * p["ub"]
    assert cross <= 1e-12


def test_all_columns_wanted_restated():
    """n_want == K: without columns beyond the wanted ones the top of the block does not converge (16 locked-stage columns,
    20 iterations: the last at 7.0e-5); with the guard block of 16 columns that such a call carries, it does."""
    p, r = lm.lowmodes_problem(), lm.first_stage()
    L, start = r["V"][:, :32], p["V1"][:, :16]
    assert lm.guard_columns(16, 16) == 16 and lm.guard_columns(60, 60) == 4 and lm.guard_columns(64, 64) == 0
    assert lm.guard_columns(48, 32) == 0
    bare = lm.chfsi(p["A"], start, 15, lm.LOWMODES_DEGREE, p["ub"], lm.LOWMODES_TOL, 20, L=L)  # 15 of 16: no guard block
    assert bare["iterations"] == 20 and np.abs(bare["evals"][:15] - p["evals"][32:47]).max() > 10 * lm.LOWMODES_TOL * p["ub"]
    r2 = lm.chfsi(p["A"], start, 16, lm.LOWMODES_DEGREE, p["ub"], lm.LOWMODES_TOL, 100, L=L, guard=p["V1"][:, 16:32])
    err = np.abs(r2["evals"] - p["evals"][32:48]).max()
    print(f"16 of 16 with a guard block: {r2['iterations']} outer iterations, eigenvalues 32..47 within {err:.2e}")
    assert r2["V"].shape[1] == 16 and r2["iterations"] <= 20
    assert r2["applications"] == 2 * (2 * (r2["iterations"] + 1) + lm.LOWMODES_DEGREE * r2["iterations"])
    assert err <= 10 * lm.LOWMODES_TOL * p["ub"]
    assert np.linalg.norm(L.conj().T @ r2["V"]) <= 1e-12


def test_new_symbols_in_header_library_and_bindings():
    import blockcg_amd
    from blockcg_amd import _lib
    header = open(os.path.join(ROOT, "include", "blockcg_hip.h")).read()
    if not os.path.exists(blockcg_amd.LIB_PATH):
        blockcg_amd.build()
    lib = ctypes.CDLL(blockcg_amd.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    for name in ("basis_rotate", "spectral_bound", "lowest_modes"):
        assert callable(getattr(blockcg_amd, name)), name
    limit = int(re.search(r"#define\s+BCG_BASIS_ROTATE_MAX_COLUMNS\s+(\d+)", header).group(1))
    assert limit == blockcg_amd.BASIS_ROTATE_MAX_COLUMNS == 64


def test_dropin_header_builds():
    inc = os.path.join(ROOT, "blockcg_amd", "include")
    for src in (os.path.join(inc, "blockcg", "lowmodes.hpp"), os.path.join(ROOT, "tests", "cpp", "lowmodes_probe.cpp"),
                os.path.join(ROOT, "tests", "cpp", "lowmodes_run_probe.cpp"), os.path.join(ROOT, "examples", "deflated_solve.cpp")):
        r = subprocess.run(["g++", "-std=c++14", "-O0", "-Wall", "-Wextra", "-fsyntax-only", "-I", inc, src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]


# ---- the host eigen-decomposition ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def eig_probe(request):
    out = os.path.join(ROOT, "examples", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "hermitian_eig_probe_" + request.param)
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-Wextra"] + flags + ["-I", os.path.join(ROOT, "blockcg_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "hermitian_eig_probe.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _decompose(exe, A):
    n = A.shape[0]
    r = subprocess.run([exe, str(n)], input=np.ascontiguousarray(A.T).tobytes(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    d = np.frombuffer(r.stdout, dtype=np.float64)
    assert d.size == n + 2 * n * n
    return d[:n].copy(), d[n:].view(np.complex128).reshape(n, n).T


def _check(A, theta, Z):
    n = A.shape[0]
    scale = max(np.linalg.norm(A), 1e-300)
    assert np.all(np.diff(theta) >= 0)
    assert np.linalg.norm(A @ Z - Z * theta[None, :]) <= 1e-12 * scale
    assert np.linalg.norm(Z.conj().T @ Z - np.eye(n)) <= 1e-12
    assert np.abs(theta - np.linalg.eigvalsh(A)).max() <= 1e-12 * scale


@pytest.mark.parametrize("n", [1, 2, 5, 16, 48, 64])
def test_hermitian_eig_random(eig_probe, n):
    rng = np.random.default_rng(n)
    A = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    A = A + A.conj().T
    _check(A, *_decompose(eig_probe, A))


def test_hermitian_eig_special(eig_probe):
    rng = np.random.default_rng(7)
    n = 12
    Qm, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    lam = np.array([-2.0, -2.0, -2.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 3.0, 3.0, 7.5])  # repeated eigenvalues
    A = (Qm * lam[None, :]) @ Qm.conj().T
    A = 0.5 * (A + A.conj().T)
    _check(A, *_decompose(eig_probe, A))
    # already diagonal, the zero matrix, a real tridiagonal one (the Lanczos matrix) and a graded one
    _check(np.diag(lam[::-1]).astype(complex), *_decompose(eig_probe, np.diag(lam[::-1]).astype(complex)))
    _check(np.zeros((4, 4), complex), *_decompose(eig_probe, np.zeros((4, 4), complex)))
    T = (np.diag(np.arange(1.0, 11.0)) + np.diag(np.full(9, 0.5), 1) + np.diag(np.full(9, 0.5), -1)).astype(complex)
    _check(T, *_decompose(eig_probe, T))
    s = 10.0 ** -np.arange(8.0)
    B = rng.standard_normal((8, 8)) + 1j * rng.standard_normal((8, 8))
    Gd = s[:, None] * (B + B.conj().T) * s[None, :]
    _check(Gd, *_decompose(eig_probe, Gd))


def test_hermitian_eig_refuses_non_finite(eig_probe):
    A = np.eye(3, dtype=complex)
    A[1, 2] = A[2, 1] = np.nan
    r = subprocess.run([eig_probe, "3"], input=np.ascontiguousarray(A.T).tobytes(), capture_output=True)
    assert r.returncode == 1
