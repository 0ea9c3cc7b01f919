"""Products with a basis of another width and the deflated solve, without a GPU: the numpy restatement against a
column-by-column loop, the new symbols in the header, the library and the bindings, the drop-in header, and the deflated
solve restated in numpy (tests/basis_ref.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np

import basis_ref as ref
from conftest import ROOT

NEW_SYMBOLS = ("bcg_basis_dot", "bcg_basis_axpy", "bcg_field_copy_columns")


def test_reference_against_a_column_loop():
    rng = np.random.default_rng(11)
    V, m, widths = 7, 5, (1, 7, 12)
    Vs = [ref.random_field(rng, V, w) for w in widths]
    b = ref.random_field(rng, V, m)
    C = ref.basis_dot(Vs, b)
    cols = [v[:, k] for v in Vs for k in range(v.shape[1])]  # [V, 3] each
    assert C.shape == (sum(widths), m)
    for i, vi in enumerate(cols):
        for j in range(m):
            assert abs(C[i, j] - np.vdot(vi.ravel(), b[:, j].ravel())) <= 1e-13 * np.linalg.norm(vi) * np.linalg.norm(b[:, j])
    y = ref.random_field(rng, V, m)
    Cm = rng.standard_normal((sum(widths), m)) + 1j * rng.standard_normal((sum(widths), m))
    for beta in (0.0, 1.0, -0.5):
        want = beta * y if beta != 0 else np.zeros_like(y)
        for i, vi in enumerate(cols):
            for j in range(m):
                want[:, j] += vi * Cm[i, j]
        got = ref.basis_axpy(y, Vs, Cm, beta)
        assert np.linalg.norm(got - want) <= 1e-13 * np.linalg.norm(want)
    ynan = np.full_like(y, np.nan)
    assert np.isfinite(ref.basis_axpy(ynan, Vs, Cm, 0.0)).all()
    # the Gram matrix of one field against itself is what hermitian_dot mirrors; the rectangular product is not Hermitian
    G = ref.basis_dot([b], b)
    assert np.allclose(G, G.conj().T)


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
    for name in ("basis_dot", "basis_axpy", "deflate", "low_mode_solution", "SBCGrQ_deflated"):
        assert callable(getattr(blockcg_amd, name)), name
    assert hasattr(blockcg_amd.block_fermion_field, "copy_columns")


def test_dropin_header_builds(tmp_path):
    inc = os.path.join(ROOT, "blockcg_amd", "include")
    r = subprocess.run(["g++", "-std=c++14", "-O0", "-Wall", "-Wextra", "-fsyntax-only", "-I", inc,
                        os.path.join(inc, "blockcg", "basis.hpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["g++", "-std=c++14", "-O0", "-Wall", "-Wextra", "-fsyntax-only", "-I", inc,
                        os.path.join(ROOT, "tests", "cpp", "basis_probe.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_deflated_solve_restated():
    """[4,4,4,2], m = 8, K = 48 lowest eigenvectors of the dense operator (conftest.hop_by_lines, numpy eigh), mass 0.05,
    eps 1e-10, BCGrQ with numpy's QR.  Operator applications, deflated against plain, for the seed of basis_ref:
        sigma = 0:     48 against 69
        sigma = 0.05:  48 against 63
    The condition tests/test_basis.py puts on the device solve -- deflated <= 0.85 x plain at the lowest shift -- holds for the
    restatement on that test's own input, and the solutions agree with the dense solve."""
    p = ref.deflation_problem()
    A, W, evals = p["A"], p["W"], p["evals"]
    n = A.shape[0]
    assert np.linalg.norm(W.conj().T @ W - np.eye(W.shape[1])) <= 1e-12
    assert np.linalg.norm(A @ W - W * evals) <= 1e-12 * np.linalg.norm(A)
    Bv = ref.to_vec(p["B"])
    assert np.array_equal(ref.to_field(Bv), p["B"])
    for sigma in ref.DEFLATION_SIGMA[:2]:
        As = A + sigma * np.eye(n)
        Xd, it_deflated = ref.deflated_bcgrq(A, Bv, W, evals, sigma, ref.DEFLATION_EPS)
        Xp, it_plain = ref.bcgrq(As, Bv, ref.DEFLATION_EPS)
        exact = np.linalg.solve(As, Bv)
        print(f"sigma = {sigma}: {it_deflated} deflated against {it_plain} plain")
        assert it_deflated <= 0.85 * it_plain, (sigma, it_deflated, it_plain)
        assert np.linalg.norm(Xd - exact) <= 1e-11 * np.linalg.norm(exact)
        assert np.linalg.norm(Xp - exact) <= 1e-11 * np.linalg.norm(exact)
