"""The covariant nearest-neighbour sum, the part that needs no GPU: the numpy reference (tests/shift_sum_ref.py) against
conftest.hop_by_lines, its adjoint identity and gauge covariance; the entry points bound and exported; the drop-in header."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, hop_by_lines, rel_err
import shift_sum_ref as ref

SHAPES = ([4, 2, 4, 2], [3, 5, 2], [7], [2, 2, 2, 2])  # extents >= 2: hop_by_lines skips directions of extent 1


def _random_coefficients(rng, nd):
    c0 = complex(rng.normal(), rng.normal())
    f = rng.normal(size=nd) + 1j * rng.normal(size=nd)
    b = rng.normal(size=nd) + 1j * rng.normal(size=nd)
    return c0, f, b


@pytest.mark.parametrize("dims", SHAPES, ids=str)
def test_reference_is_the_hop(dims):
    """(0, 1/2, -1/2, eta) is the operator D of conftest.hop_by_lines (which shares no gather with the reference here)."""
    rng = np.random.default_rng(1)
    V = int(np.prod(dims))
    U, psi = ref.random_links(rng, dims), ref.random_field(rng, V, 3)
    got = ref.shift_sum(U, dims, psi, 0.0, 0.5, -0.5, eta=True)
    err = rel_err(got, hop_by_lines(U, dims, psi))
    print(f"{dims}: reference vs hop_by_lines {err:.2e}")
    assert err <= 1e-15 * 4


@pytest.mark.parametrize("eta", [False, True])
@pytest.mark.parametrize("dims", SHAPES + ([1, 4, 2, 3],), ids=str)
def test_adjoint_identity(dims, eta):
    """<phi, S(c0, f, b) psi> = <S(conj c0, conj b, conj f) phi, psi> for arbitrary complex links."""
    rng = np.random.default_rng(2)
    V = int(np.prod(dims))
    U, psi, phi = ref.random_links(rng, dims), ref.random_field(rng, V, 2), ref.random_field(rng, V, 2)
    c0, f, b = _random_coefficients(rng, len(dims))
    lhs = np.vdot(phi, ref.shift_sum(U, dims, psi, c0, f, b, eta))
    rhs = np.vdot(ref.shift_sum(U, dims, phi, np.conj(c0), np.conj(b), np.conj(f), eta), psi)
    scale = np.linalg.norm(phi) * np.linalg.norm(ref.shift_sum(U, dims, psi, c0, f, b, eta))
    assert abs(lhs - rhs) <= 1e-14 * scale


@pytest.mark.parametrize("dims", ([4, 2, 4, 2], [3, 5, 2]), ids=str)
def test_gauge_covariance(dims):
    """U'_mu(x) = g(x) U_mu(x) g(x+mu)^dagger and psi' = g psi give S' psi' = g S psi (unitary g from a numpy QR)."""
    rng = np.random.default_rng(3)
    nd, V = len(dims), int(np.prod(dims))
    U, psi = ref.unitary_links(rng, dims), ref.random_field(rng, V, 2)
    g, _ = np.linalg.qr(rng.normal(size=(V, 3, 3)) + 1j * rng.normal(size=(V, 3, 3)))  # g[x] = g(x)(r, k), ordinary row/col
    Ug = np.empty_like(U)
    for mu in range(nd):
        xf = ref.neighbours(dims, mu, +1)
        M = np.swapaxes(U[:, mu], 1, 2)  # M[x](r, k)
        Mg = g @ M @ np.conj(np.swapaxes(g[xf], 1, 2))
        Ug[:, mu] = np.swapaxes(Mg, 1, 2)
    rot = lambda f: np.einsum("xrk,xjk->xjr", g, f)  # noqa: E731
    c0, f, b = _random_coefficients(rng, nd)
    for eta in (False, True):
        assert rel_err(ref.shift_sum(Ug, dims, rot(psi), c0, f, b, eta), rot(ref.shift_sum(U, dims, psi, c0, f, b, eta))) <= 1e-14


def test_zero_coefficients_skip_their_links():
    """The reference itself never touches the links of a direction whose two coefficients are 0: NaN there stays out."""
    rng = np.random.default_rng(4)
    dims = [4, 2, 4, 2]
    U, psi = ref.random_links(rng, dims), ref.random_field(rng, int(np.prod(dims)), 2)
    Un = U.copy()
    Un[:, 3] = np.nan
    assert np.array_equal(ref.laplacian(Un, dims, psi, 3), ref.laplacian(U, dims, psi, 3))
    assert not np.all(np.isfinite(ref.laplacian(Un, dims, psi, -1)))


def test_entry_points_are_bound_and_exported():
    import blockcg_amd
    from blockcg_amd import _lib
    if not os.path.exists(blockcg_amd.LIB_PATH):
        blockcg_amd.build()
    lib = ctypes.CDLL(blockcg_amd.LIB_PATH)
    for name in ("bcg_dirac_shift_sum", "bcg_covariant_smear"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for name in ("shift_sum", "covariant_shift", "laplacian", "smear"):
        assert callable(getattr(blockcg_amd, name)), name


def test_dropin_header_has_the_new_functions():
    inc = os.path.join(ROOT, "blockcg_amd", "include")
    r = subprocess.run(["g++", "-std=c++14", "-O0", "-Wall", "-Wextra", "-fsyntax-only", "-I", inc,
                        os.path.join(ROOT, "tests", "cpp", "shift_sum_probe.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
