"""Stout smearing and the plaquette without a GPU: the numpy restatement (tests/stout_ref.py) against itself -- three
formulations of the step that differ in the exponential (eigendecomposition, scaled Taylor series, Cayley-Hamilton) -- its
invariants (unit links, SU(3), gauge covariance, the plaquette), the Cayley-Hamilton form at tiny and degenerate Q, and the
bindings, headers and example of the device calls.  The spread of the three formulations (<= 2.5e-14 asserted, a few 1e-15
measured) is what the 1e-13 bound of the GPU tests is measured against."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import stout_ref as ref

DIMS = [4, 4, 2, 6]
V = int(np.prod(DIMS))
TABLE = np.array([[0.12 + 0.01 * mu + 0.003 * nu for nu in range(4)] for mu in range(4)])


@pytest.fixture(scope="module")
def fields():
    rng = np.random.default_rng(11)
    return {"random": ref.random_links((V, 4), rng), "su3": ref.random_su3((V, 4), 0.4, rng)}


@pytest.mark.parametrize("kind", ["random", "su3"])
def test_three_formulations_agree(fields, kind):
    U = fields[kind]
    outs = [ref.stout_smear(U, TABLE, DIMS, 3, exp=e) for e in (ref.exp_eigh, ref.exp_taylor, ref.exp_ch)]
    spread = max(ref.rel_err(outs[i], outs[j]) for i, j in ((0, 1), (0, 2), (1, 2)))
    print(kind, "spread of the three formulations after 3 steps: %.2e" % spread)
    assert spread <= 2.5e-14


def test_unit_links_are_a_fixed_point():
    U = np.broadcast_to(np.eye(3, dtype=np.complex128), (V, 4, 3, 3)).copy()
    for e in (ref.exp_taylor, ref.exp_ch):  # Q = 0 exactly, and both forms give exp(0) = 1 exactly
        assert np.array_equal(ref.stout_smear(U, TABLE, DIMS, 2, exp=e), U)
    assert np.abs(ref.stout_smear(U, TABLE, DIMS, 2, exp=ref.exp_eigh) - U).max() <= 1e-15


def test_su3_stays_su3(fields):
    out = ref.stout_smear(fields["su3"], 0.1, DIMS, 3, dir=3, exp=ref.exp_ch)
    unit = np.abs(ref.dagger(out) @ out - np.eye(3)).max()
    det = np.abs(np.linalg.det(out) - 1.0).max()
    print("U^dagger U - 1: %.2e, det - 1: %.2e" % (unit, det))
    assert unit <= 1e-13 and det <= 1e-13


@pytest.mark.parametrize("kind", ["random", "su3"])
def test_gauge_covariance_of_the_reference(fields, kind):
    rng = np.random.default_rng(5)
    g = ref.random_su3((V,), 1.0, rng)
    U = fields[kind]
    a = ref.stout_smear(ref.gauge_transform(U, g, DIMS), TABLE, DIMS, 2, exp=ref.exp_ch)
    b = ref.gauge_transform(ref.stout_smear(U, TABLE, DIMS, 2, exp=ref.exp_ch), g, DIMS)
    assert ref.rel_err(a, b) <= 1e-13


def test_plaquette(fields):
    rng = np.random.default_rng(6)
    U = fields["su3"]
    g = ref.random_su3((V,), 1.0, rng)
    P = ref.plaquette(U, DIMS)
    assert np.abs(ref.plaquette(ref.gauge_transform(U, g, DIMS), DIMS) - P).max() <= 1e-13
    assert np.array_equal(P, P.T) and np.all(np.diag(P) == 0.0)
    # spatial smearing: higher in every plane (every plane holds a smeared direction)
    P3 = ref.plaquette(ref.stout_smear(U, 0.1, DIMS, 3, dir=3), DIMS)
    off = ~np.eye(4, dtype=bool)
    print("mean plaquette %.3f -> %.3f" % (P[off].mean(), P3[off].mean()))
    assert np.all(P3[off] > P[off])
    # only the pair (0, 1) smeared: the plane (2, 3) holds no smeared direction and keeps its plaquette to rounding
    pair = np.zeros((4, 4))
    pair[0, 1] = pair[1, 0] = 0.1
    Pp = ref.plaquette(ref.stout_smear(U, pair, DIMS, 3), DIMS)
    assert Pp[0, 1] > P[0, 1] and abs(Pp[2, 3] - P[2, 3]) <= 1e-14


def test_cayley_hamilton_at_tiny_and_degenerate_q():
    rng = np.random.default_rng(7)
    H = ref.random_hermitian_traceless((64,), rng)
    for eps in (1.0, 1e-3, 1e-6, 1e-9, 1e-12, 0.0):
        E = ref.exp_ch(eps * H)
        assert np.all(np.isfinite(E))
        assert np.abs(E - ref.exp_taylor(eps * H)).max() <= 1e-14, eps
    g = ref.random_su3((8,), 1.0, rng)
    for a in (1.0, -1.0, 0.3, -0.3, 1e-4, -1e-4):
        D = np.diag([a, a, -2.0 * a]).astype(np.complex128)
        for Q in (D[None], g @ D @ ref.dagger(g)):
            Q = 0.5 * (Q + ref.dagger(Q))
            E = ref.exp_ch(Q)
            assert np.all(np.isfinite(E))
            assert np.abs(E - ref.exp_taylor(Q)).max() <= 1e-14, a


def test_bindings_name_the_new_calls():
    import blockcg_amd
    from blockcg_amd import _lib
    header = open(os.path.join(ROOT, "include", "blockcg_hip.h")).read()
    for name, nargs in (("bcg_gauge_stout_smear", 6), ("bcg_gauge_plaquette", 3)):
        assert re.search(r"\bint\s+%s\s*\(" % name, header)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    assert callable(blockcg_amd.stout_smear) and callable(blockcg_amd.plaquette)


def test_headers_and_example_pass_the_host_compiler():
    inc = os.path.join(ROOT, "blockcg_amd", "include")
    for src in (os.path.join(inc, "blockcg", "gauge.hpp"), os.path.join(inc, "blockcg", "dirac_op.hpp"),
                os.path.join(ROOT, "examples", "stout_distillation.cpp")):
        r = subprocess.run(["g++", "-std=c++14", "-O0", "-Wall", "-Wextra", "-fsyntax-only", "-x", "c++", "-I", inc, src],
                           capture_output=True, text=True)
        assert r.returncode == 0, (src, r.stderr[-3000:])
