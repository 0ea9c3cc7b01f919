"""The distillation basis without a GPU: the numpy restatements of bcg_basis_slice_rotate (tests/basis_slice_rotate_ref.py)
and bcg_laplacian_modes (tests/laplacian_modes_ref.py), the new symbols in the header, the library and the bindings, and the
drop-in header with its probe and its example under g++ -fsyntax-only.

Figures of the restatement for the seeds of laplacian_modes_ref (degree 16, tol 1e-10; unitary links, upper_bound 12, the
spectrum of a slice within [1.51, 10.49]; general links, upper_bound 1.02 lambda_max = 13.1):
    [4,4,4,3] dir 3 and [3,4,4,4] dir 0: [32, 16] with 32 wanted, [16] with 16 wanted (guard block), 16 behind 32 locked,
    general links: 4 outer iterations each, with one interval for all slices as with an interval per slice;
    Ritz values within 5e-14 of eigh per slice."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import basis_ref
import basis_slice_rotate_ref as rot
import laplacian_modes_ref as lr
from basis_slice_axpy_ref import slice_of_sites
from conftest import ROOT
from sources_ref import parity_mask

NEW_SYMBOLS = ("bcg_basis_slice_rotate", "bcg_laplacian_modes")


@pytest.mark.parametrize("dims,parities", [([4, 2, 4, 2], (None, 0, 1)), ([5, 3, 2], (None,))])
def test_rotation_restated_against_a_loop_over_sites(dims, parities):
    rng = np.random.default_rng(5)
    widths = (3, 16, 2)
    K = sum(widths)
    for parity in parities:
        sites = int(parity_mask(dims, parity).sum())
        V = [basis_ref.random_field(rng, sites, w) for w in widths]
        for direction in range(len(dims)):
            L = dims[direction]
            for slices in (None, [L - 1], [L - 1, 0]):
                S = L if slices is None else len(slices)
                Q = rng.standard_normal((S, K, K)) + 1j * rng.standard_normal((S, K, K))
                got = rot.basis_slice_rotate(V, Q, dims, direction, slices, parity)
                want = rot.by_sites(V, Q, dims, direction, slices, parity)
                assert [g.shape[1] for g in got] == list(widths)
                assert np.linalg.norm(basis_ref.concat(got) - basis_ref.concat(want)) <= 1e-13 * np.linalg.norm(basis_ref.concat(want))
                listed = np.isin(slice_of_sites(dims, direction, parity), range(L) if slices is None else slices)
                assert np.array_equal(basis_ref.concat(got)[~listed], basis_ref.concat(V)[~listed])


@pytest.mark.parametrize("dims,direction", lr.CASES)
@pytest.mark.parametrize("unitary", [True, False], ids=["unitary", "general"])
def test_dense_operator_is_hermitian_and_block_diagonal(dims, direction, unitary):
    p = lr.problem(dims, direction, unitary)
    A, rows = p["A"], p["rows"]
    assert np.abs(A - A.conj().T).max() <= 1e-14 * np.abs(A).max()
    assert sorted(np.concatenate(rows)) == list(range(A.shape[0]))
    for s, r in enumerate(rows):
        for t, q in enumerate(rows):
            if s != t:
                assert not A[np.ix_(r, q)].any()  # exactly zero between different slices
    assert p["evals"].max() < p["ub"]
    if unitary:  # -Lap_dir of unitary links is positive and 4 (ndim - 1) bounds it; general links have neither property
        assert p["ub"] == 12.0 and p["evals"].min() > 0.0


def _check(p, r, want, first, what):
    """Ritz values of the wanted columns within 10 tol ub of eigh per slice; V orthonormal per slice"""
    err = np.abs(r["evals"][:, :want] - p["evals"][:, first:first + want]).max()
    orth = max(np.linalg.norm(r["V"][q].conj().T @ r["V"][q] - np.eye(r["V"].shape[1])) for q in p["rows"])
    print(f"{what}: {r['iterations']} outer iterations, Ritz values within {err:.2e} of eigh, |V(t)^dagger V(t) - 1| <= {orth:.2e}")
    assert r["iterations"] <= 10
    assert r["resid"][:, :want].max() <= lr.TOL * p["ub"]
    assert err <= 10 * lr.TOL * p["ub"]
    assert orth <= 1e-12
    assert np.all(np.diff(r["evals"], axis=1) >= 0)
    return err


@pytest.mark.parametrize("dims,direction", lr.CASES)
def test_solver_restated(dims, direction):
    p = lr.problem(dims, direction)
    K = sum(lr.WIDTHS)
    # [32, 16] with 32 wanted: one interval for all slices needs exactly the outer iterations of an interval per slice
    r = lr.first_stage(dims, direction)
    _check(p, r, lr.WANT, 0, f"{dims} dir {direction}, {list(lr.WIDTHS)} with {lr.WANT} wanted")
    assert r["applications"] == 2 * (2 * (r["iterations"] + 1) + lr.DEGREE * r["iterations"])
    own = lr.chfsi(p["A"], p["rows"], p["V0"], lr.WANT, lr.DEGREE, p["ub"], lr.TOL, 100, nv=2, per_slice_intervals=True)
    assert own["iterations"] == r["iterations"]
    assert r["V"].shape[1] == K
    # [16] with 16 wanted: the guard block
    g = lr.chfsi(p["A"], p["rows"], p["V1"][:, :16], 16, lr.DEGREE, p["ub"], lr.TOL, 100, guard=p["V1"][:, 16:32])
    _check(p, g, 16, 0, "[16] with 16 wanted and the guard block")
    assert g["V"].shape[1] == 16 and g["applications"] == 2 * (2 * (g["iterations"] + 1) + lr.DEGREE * g["iterations"])
    # 16 behind 32 locked
    L = r["V"][:, :32]
    k = lr.chfsi(p["A"], p["rows"], p["V1"][:, :16], 16, lr.DEGREE, p["ub"], lr.TOL, 100, L=L, guard=p["V1"][:, 16:32])
    _check(p, k, 16, 32, "16 behind 32 locked")
    assert max(np.linalg.norm(L[q].conj().T @ k["V"][q]) for q in p["rows"]) <= 1e-12


@pytest.mark.parametrize("dims,direction", lr.CASES)
def test_solver_restated_with_general_links(dims, direction):
    p = lr.problem(dims, direction, False)
    assert p["ub"] > 12.0  # the bound of unitary links does not hold here
    _check(p, lr.first_stage(dims, direction, False), lr.WANT, 0, f"{dims} dir {direction}, general links, ub = {p['ub']:.3f}")


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
    for name in ("basis_slice_rotate", "laplacian_modes"):
        assert callable(getattr(blockcg_amd, name)), name


def test_dropin_header_builds():
    inc = os.path.join(ROOT, "blockcg_amd", "include")
    for src in (os.path.join(inc, "blockcg", "lowmodes.hpp"), os.path.join(ROOT, "tests", "cpp", "laplacian_modes_run_probe.cpp"),
                os.path.join(ROOT, "examples", "laplacian_distillation.cpp")):
        r = subprocess.run(["g++", "-std=c++14", "-O0", "-Wall", "-Wextra", "-fsyntax-only", "-I", inc, src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
