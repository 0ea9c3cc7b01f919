"""CPU checks of the fermion force (bcg_force_accumulate, bcg_gauge_download, bcg_gauge_set_zero; blockcg::fermion_force):
the C header compiles as C99 with the new declarations, the library exports and binds them, the C++ probe compiles against
the drop-in headers (tests/test_force.py runs it on the GPU) -- and the derivative formula of the header itself, checked in
numpy against a finite difference of the action on a 2-D toy lattice, so a sign or convention error in the contract shows up
without a GPU.  The numpy force below is the reference tests/test_force.py compares the kernel with."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, hop_by_lines

INC = os.path.join(ROOT, "blockcg_amd", "include")
LIBDIR = os.path.join(ROOT, "blockcg_amd", "_build")
OUT = os.path.join(ROOT, "examples", "_build")

C99_SRC = r"""
#include "blockcg_hip.h"
#include <stddef.h>
int main(void) {
  int (*force)(bcg_context*, const bcg_gauge*, bcg_field* const*, int, const double*, double, int, bcg_field* const*, int,
               bcg_gauge*) = bcg_force_accumulate;
  int (*down)(const bcg_gauge*, double*) = bcg_gauge_download;
  int (*zero)(bcg_gauge*) = bcg_gauge_set_zero;
  return (force != NULL && down != NULL && zero != NULL) ? 0 : 1;
}
"""


# ---- the numpy force: the header's formula, term for term ------------------------------------------------------------------
def lattice_coords(dims):
    """[V, ndim] coordinates of the lexicographic sites (x0 fastest)."""
    c = np.array(list(itertools.product(*[range(d) for d in reversed(dims)])))[:, ::-1]
    return c.reshape(-1, len(dims))


def plus_neighbours(dims):
    """[ndim, V]: index of x + mu (periodic)."""
    c = lattice_coords(dims)
    strides = np.cumprod([1] + list(dims[:-1]))
    out = []
    for mu in range(len(dims)):
        cp = c.copy()
        cp[:, mu] = (cp[:, mu] + 1) % dims[mu]
        out.append(cp @ strides)
    return np.array(out)


def etas(dims):
    """[ndim, V]: eta_mu(x) = (-1)^(x_0 + ... + x_{mu-1})."""
    c = lattice_coords(dims)
    return np.array([(-1.0) ** (c[:, :mu].sum(axis=1) % 2) for mu in range(len(dims))])


def force_matrices(dims, X, Y, residues, scale=1.0):
    """G[x, mu] as 3 x 3 matrices (row r, column c): scale sum_s a_s eta_mu(x) sum_j [Y(x+mu) X(x)^dag - X(x+mu) Y(x)^dag].
    X, Y: lists of full fields [V, m, 3] (host layout [x, j, c])."""
    V, nd = int(np.prod(dims)), len(dims)
    nb, eta = plus_neighbours(dims), etas(dims)
    G = np.zeros((V, nd, 3, 3), dtype=np.complex128)
    for a, x, y in zip(residues, X, Y):
        for mu in range(nd):
            t = np.einsum("vjr,vjc->vrc", y[nb[mu]], x.conj()) - np.einsum("vjr,vjc->vrc", x[nb[mu]], y.conj())
            G[:, mu] += scale * a * eta[mu][:, None, None] * t
    return G


def to_host(M):
    """3 x 3 matrices -> the link layout of the host arrays ([.., k, r] = M(r, k)), and back."""
    return np.ascontiguousarray(np.swapaxes(M, -1, -2))


def ta(M):
    """TA(M) = (M - M^dag)/2 - tr(M - M^dag)/6 per 3 x 3 matrix."""
    A = 0.5 * (M - np.conj(np.swapaxes(M, -1, -2)))
    tr = np.trace(A, axis1=-2, axis2=-1)
    return A - (tr / 3.0)[..., None, None] * np.eye(3)


def numpy_force(U, dims, X, residues, scale=1.0, project=False):
    """The force in the host link layout [V, ndim, 3, 3]; Y_s = D X_s by conftest.hop_by_lines."""
    Y = [hop_by_lines(U, dims, x) for x in X]
    G = force_matrices(dims, X, Y, residues, scale)
    if project:
        G = ta(to_host(U) @ G)
    return to_host(G)


def dense_D(U, dims):
    """D as a dense (3V x 3V) matrix on vectors indexed 3 x + c, from hop_by_lines on identity columns."""
    V = int(np.prod(dims))
    eye = np.eye(3 * V, dtype=np.complex128).reshape(V, 3, 3 * V).transpose(0, 2, 1)
    out = hop_by_lines(U, dims, np.ascontiguousarray(eye))  # out[x, n, c] = D[3x + c, n]
    return out.transpose(0, 2, 1).reshape(3 * V, 3 * V)


def to_vec(f):
    """field [V, m, 3] -> (3V x m) columns."""
    return f.transpose(0, 2, 1).reshape(-1, f.shape[1])


def from_vec(v, V):
    return np.ascontiguousarray(v.reshape(V, 3, -1).transpose(0, 2, 1))


def action(D, mass, Bv, sigma, residues):
    """S = sum_s a_s sum_j B_j^dag (mass^2 - D^2 + sigma_s)^-1 B_j (real for anti-Hermitian D)."""
    n = D.shape[0]
    A = mass * mass * np.eye(n) - D @ D
    return sum(a * np.trace(Bv.conj().T @ np.linalg.solve(A + s * np.eye(n), Bv)).real for s, a in zip(sigma, residues))


def derivative(G, dU):
    """sum_{x,mu} Re tr(dU G), both as 3 x 3 matrices."""
    return np.einsum("xmrc,xmcr->", dU, G).real


def _rand(rng, shape):
    return rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)


def test_derivative_formula_by_finite_difference():
    """The contract on a 4 x 6 lattice (6: an extent whose eta pattern differs from 4's), m = 2, three shifts: X_s by dense
    solve, G by the formula, dS against (S(U + e dU) - S(U - e dU)) / 2e for a random complex dU."""
    rng = np.random.default_rng(11)
    dims, m, mass = [4, 6], 2, 1.5
    sigma, a = [0.0, 0.3, 1.1], [0.8, -0.4, 1.7]
    V = int(np.prod(dims))
    U = _rand(rng, (V, 2, 3, 3))
    dU = _rand(rng, (V, 2, 3, 3))
    B = _rand(rng, (V, m, 3))
    D0, Dd = dense_D(U, dims), dense_D(dU, dims)
    A = mass * mass * np.eye(3 * V) - D0 @ D0
    X = [from_vec(np.linalg.solve(A + s * np.eye(3 * V), to_vec(B)), V) for s in sigma]
    G = force_matrices(dims, X, [hop_by_lines(U, dims, x) for x in X], a)
    eps = 1e-6
    fd = (action(D0 + eps * Dd, mass, to_vec(B), sigma, a) - action(D0 - eps * Dd, mass, to_vec(B), sigma, a)) / (2 * eps)
    dS = derivative(G, to_host(dU))
    assert abs(fd - dS) <= 1e-7 * abs(dS), (fd, dS)
    # the projected form: U -> exp(e P) U, P traceless anti-Hermitian, dS/de = sum Re tr(P TA(U G))
    P = ta(_rand(rng, (V, 2, 3, 3)))
    Um = to_host(U)
    dUp = to_host(P @ Um)  # first order of exp(e P) U - U
    Dp = dense_D(dUp, dims)
    fdp = (action(D0 + eps * Dp, mass, to_vec(B), sigma, a) - action(D0 - eps * Dp, mass, to_vec(B), sigma, a)) / (2 * eps)
    dSp = np.einsum("xmrc,xmcr->", P, ta(Um @ G)).real
    assert abs(fdp - dSp) <= 1e-7 * abs(dSp), (fdp, dSp)


def _lib():
    import blockcg_amd
    if not os.path.exists(blockcg_amd.LIB_PATH):
        blockcg_amd.build()
    return blockcg_amd.load()


def build_force_probe():
    """g++ on tests/cpp/force_probe.cpp against the drop-in headers (test_cpp_dropin.py's recipe); returns the executable."""
    _lib()
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "force_probe")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I", INC, os.path.join(ROOT, "tests", "cpp", "force_probe.cpp"),
           "-o", exe, "-L", LIBDIR, "-lblockcg_hip", f"-Wl,-rpath,{LIBDIR}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "force_c99.c"
    src.write_text(C99_SRC)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-c", str(src), "-o", str(tmp_path / "force_c99.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_exports_and_binds_the_force_entry_points():
    from blockcg_amd import _lib as L
    lib = _lib()
    for name in ("bcg_force_accumulate", "bcg_gauge_download", "bcg_gauge_set_zero"):
        assert name in L.SIGNATURES
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]


def test_python_interface_present():
    import blockcg_amd
    assert callable(blockcg_amd.fermion_force) and isinstance(blockcg_amd.gauge_field, type)


def test_cpp_program_compiles_against_dropin_headers():
    assert os.path.exists(build_force_probe())


@pytest.mark.parametrize("dims", [[6], [4, 3], [2, 4, 3]])
def test_numpy_force_layout_is_consistent(dims):
    """The numpy force agrees with the derivative read off the dense operator: dS = 2 Re X^dag dD Y summed over shifts, for
    one random X (no solve), on lattices with an extent 2 and odd extents."""
    rng = np.random.default_rng(3)
    V, nd, m = int(np.prod(dims)), len(dims), 2
    U, dU, X = _rand(rng, (V, nd, 3, 3)), _rand(rng, (V, nd, 3, 3)), _rand(rng, (V, m, 3))
    F = numpy_force(U, dims, [X], [1.0])
    Dd = dense_D(dU, dims)
    Yv = to_vec(hop_by_lines(U, dims, X))
    want = 2 * np.trace(to_vec(X).conj().T @ Dd @ Yv).real
    assert abs(derivative(to_host(F), to_host(dU)) - want) <= 1e-12 * abs(want)
