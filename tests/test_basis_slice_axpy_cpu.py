"""What bcg_basis_slice_axpy (include/blockcg_hip.h) needs that runs without a GPU: the numpy restatement
(tests/basis_slice_axpy_ref.py) against a plain loop over sites, the adjoint identity between it and the restatement of
bcg_basis_slice_dot, the symbol in the header, the built library and the bindings, and the C++ layer and its example through
the host compiler."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import basis_ref
import basis_slice_axpy_ref as ref
import basis_slice_ref
from conftest import ROOT


def _momentum(n, direction):
    q = list(n) + [0] * (4 - len(n))
    q[direction] = 0
    return q


@pytest.mark.parametrize("dims,widths,m,momentum", [([4, 2, 4, 2], (1, 7, 4), 5, [-1, 1, 3, 5]), ([5, 3, 2], (6, 3), 4, [2, -1, 1])],
                         ids=["4x2x4x2", "5x3x2"])
def test_restatement_against_a_loop_over_sites(dims, widths, m, momentum):
    rng = np.random.default_rng(11)
    parities = (None, 0, 1) if all(d % 2 == 0 for d in dims) else (None,)
    K = sum(widths)
    for parity in parities:
        sites = int(np.prod(dims)) // (1 if parity is None else 2)
        V = [basis_ref.random_field(rng, sites, w) for w in widths]
        y = basis_ref.random_field(rng, sites, m)
        for direction in range(len(dims)):
            L = dims[direction]
            for slices in (None, [L - 1], [L - 1, 0]):
                S = L if slices is None else len(slices)
                C = rng.standard_normal((S, K, m)) + 1j * rng.standard_normal((S, K, m))
                for mom in (None, _momentum(momentum, direction)):
                    for beta in (0.0, 1.0, -0.5):
                        got = ref.basis_slice_axpy(y, V, C, dims, direction, slices, mom, beta, parity)
                        want = ref.by_sites(y, V, C, dims, direction, slices, mom, beta, parity)
                        assert got.shape == want.shape == y.shape
                        assert np.linalg.norm(got - want) <= 1e-13 * np.linalg.norm(want)
                        listed = np.isin(ref.slice_of_sites(dims, direction, parity), range(L) if slices is None else slices)
                        if beta == 1.0:
                            assert np.array_equal(got[~listed], y[~listed])
                        if beta == 0.0:
                            assert np.all(got[~listed] == 0)


@pytest.mark.parametrize("dims", [[4, 2, 4, 2], [5, 3, 2]], ids=["4x2x4x2", "5x3x2"])
def test_adjoint_of_the_slice_dot(dims):
    """sum_x conj(y) b = sum_t sum_ij conj(C_t(i, j)) tau_p(t; i, j) for y = basis_slice_axpy(0, V, C, p, beta = 0)."""
    rng = np.random.default_rng(13)
    widths, m = (3, 5), 4
    K = sum(widths)
    parities = (None, 0, 1) if all(d % 2 == 0 for d in dims) else (None,)
    for parity in parities:
        sites = int(np.prod(dims)) // (1 if parity is None else 2)
        V = [basis_ref.random_field(rng, sites, w) for w in widths]
        b = basis_ref.random_field(rng, sites, m)
        for direction in range(len(dims)):
            L = dims[direction]
            p = _momentum([3, -1, 2, 1][:len(dims)], direction)
            C = rng.standard_normal((L, K, m)) + 1j * rng.standard_normal((L, K, m))
            for mom in (None, p):
                y = ref.basis_slice_axpy(None, V, C, dims, direction, None, mom, 0.0, parity)
                tau, _ = basis_slice_ref.basis_slice_dot(V, b, dims, direction, None if mom is None else [mom], parity)
                lhs = np.vdot(y, b)
                rhs = np.vdot(C, tau[0])
                assert abs(lhs - rhs) <= 1e-13 * np.linalg.norm(y) * np.linalg.norm(b), (parity, direction, mom)


def test_symbol_in_header_library_and_bindings():
    import blockcg_amd
    from blockcg_amd import _lib
    header = open(os.path.join(ROOT, "include", "blockcg_hip.h")).read()
    if not os.path.exists(blockcg_amd.LIB_PATH):
        blockcg_amd.build()
    lib = ctypes.CDLL(blockcg_amd.LIB_PATH)
    assert re.search(r"\bint\s+bcg_basis_slice_axpy\s*\(", header)
    assert "bcg_basis_slice_axpy" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["bcg_basis_slice_axpy"][1]) == 9
    assert hasattr(lib, "bcg_basis_slice_axpy")
    assert callable(blockcg_amd.basis_slice_axpy)


def test_dropin_header_and_example_build():
    inc = os.path.join(ROOT, "blockcg_amd", "include")
    for src in (os.path.join(inc, "blockcg", "basis.hpp"), os.path.join(ROOT, "examples", "distillation.cpp")):
        r = subprocess.run(["g++", "-std=c++14", "-O0", "-Wall", "-Wextra", "-fsyntax-only", "-I", inc, src], capture_output=True,
                           text=True)
        assert r.returncode == 0, (src, r.stderr[-3000:])
