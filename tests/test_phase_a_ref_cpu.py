"""The reference of tests/test_phase_a_operator.py (tests/phase_a_ref.py) against the CPU oracle, at every shape that file runs.

What is held, and why at these bounds:
  * T_ref(sigma_0 = 0) against oracle.dirac_apply, the oracle's double-precision m^2 - D^2 with its own neighbour
    arithmetic: the two share no code, the reference rounds once from extended precision, so the difference is the
    oracle's own rounding -- a few ulp of |T|.  Bound: TOL_KERNEL / 10 = 1e-14, so that the GPU test's TOL_KERNEL keeps a
    tenfold margin over the reference's share at least.  Measured (x86 long double): 1.58e-16 .. 1.59e-16 in the norm at
    every shape, 3.2e-16 at worst per site relative to max |T|.
  * G_ref against numpy's complex128 P^dagger T_ref: the rounding of a complex128 sum of 3 V terms; bound as above.
    Measured: 1.2e-16 .. 7.1e-16.
  * The reference contains no factored form: with sigma_0 != 0 it equals T_ref(0) + sigma_0 P, and G_ref is Hermitian to rounding
    (it is never symmetrised)."""
import functools

import numpy as np
import pytest

from conftest import TOL_KERNEL, rel_err
import phase_a_ref as ref

MASS = 0.2


@functools.lru_cache(maxsize=None)
def _case(name):
    import oracle
    orc = oracle.Oracle()
    dims = ref.ALL_SHAPES[name][0]
    U = orc.fill_gauge(dims, ref.SEED_U)
    P = np.random.default_rng(ref.SEED_P).normal(size=(int(np.prod(dims)), ref.M, 3, 2)).view(np.complex128)[..., 0]
    T, G = ref.phase_a(U, dims, MASS, 0.0, P)
    return dims, U, P, T, G, orc.dirac_apply(U, dims, MASS, P)


@pytest.mark.parametrize("name", sorted(ref.ALL_SHAPES))
def test_reference_against_the_oracle(name):
    dims, U, P, T, G, want = _case(name)
    e = rel_err(T, want)
    e_site = np.abs(T - want).max() / np.abs(want).max()
    eg = rel_err(ref.gram_double(P, T), G)
    print(f"{name} [{ref.PRECISION}]: T_ref vs oracle {e:.3e} (per site {e_site:.3e}), numpy P^dagger T vs G_ref {eg:.3e}")
    assert e < TOL_KERNEL / 10 and e_site < TOL_KERNEL / 10
    assert eg < TOL_KERNEL / 10
    assert rel_err(G, G.conj().T) < TOL_KERNEL / 10 and np.any(G != G.conj().T)  # Hermitian by the operator, not by a mirror


def test_reference_shift_is_additive_and_unfactored():
    dims, U, P, T0, G0, _ = _case("16x4x8x3")
    for mass, sigma0 in ((MASS, 0.05), (MASS, -0.04 - 1e-3), (0.0, 0.0), (30.0, 100.0)):
        T, G = ref.phase_a(U, dims, mass, sigma0, P)
        want = T0 + (mass * mass + sigma0 - MASS * MASS) * P
        e = rel_err(T, want)
        print(f"mass {mass} sigma0 {sigma0}: T_ref vs T_ref(0) + shift P {e:.3e}")
        assert e < TOL_KERNEL / 10
        assert rel_err(G, ref.gram_double(P, T)) < TOL_KERNEL / 10


def test_every_geometry_is_legal_for_the_bundle_sweep():
    """plan_hop4 / bundle_ok (hop_plan.cpp) at m = 16, restated: the table in phase_a_ref.py row by row."""
    for name, (dims, patch, blocks) in ref.ALL_SHAPES.items():
        p0, p1, p2 = (int(v) for v in patch.split(",")) if patch else (16, 8, 8)
        nb = int(blocks) if blocks else 512
        L0, L1, L2, L3 = dims
        tiles = L0 * L1 * L2 * L3 // 16
        assert L0 % 16 == 0 and p0 % 16 == 0 and L0 % p0 == 0 and L1 % p1 == 0 and L2 % p2 == 0, name
        assert p1 % 2 == 0 and p2 % 2 == 0 and tiles % 8 == 0 and nb % 8 == 0 and tiles >= nb, name
        assert ((L0 // p0) * (L1 // p1) * (L2 // p2)) % 8 == 0, name
        assert nb // 8 == (p0 // 16) * p1 * p2 == (p0 // 4) * (p1 // 2) * (p2 // 2), name
