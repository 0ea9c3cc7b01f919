"""Complex right-multiplications of the MFMA row kernels (mfma_common.hpp: rmul_acc, rmul_acc2) on coefficient matrices
that stress the three-product (Gauss) form at m = 16: purely real, purely imaginary, |Re| >> |Im| and the reverse, the
identity and an ill-conditioned upper-triangular inverse, besides a dense random one.  K5 (y += x C) and K6
(y = y C + b x) run through the plain kernel on a ragged row count and through the batched one on rows that are a
multiple of 512; a short seeded solve runs phase B, phase C, k_phaseC_p0 and the closing pass k_phaseC_multi, in the
ordinary and in the sum mode.  Everything against the oracle."""
import numpy as np
import pytest

from conftest import TOL_COEFF, TOL_KERNEL, rel_err

pytestmark = pytest.mark.gpu

KINDS = ("random", "real", "imag", "re_dominant", "im_dominant", "identity", "upper_inverse")


@pytest.fixture(scope="module")
def bc():
    import blockcg_amd
    return blockcg_amd


def _coefficients(kind, m, seed):
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(-1, 1, (m, m)), rng.uniform(-1, 1, (m, m))
    if kind == "random":
        return a + 1j * b
    if kind == "real":
        return a + 0j
    if kind == "imag":
        return 1j * b
    if kind == "re_dominant":
        return a + 1e-7j * b
    if kind == "im_dominant":
        return 1e-7 * a + 1j * b
    if kind == "identity":
        return np.eye(m, dtype=np.complex128)
    # rho^-1 of an ill-conditioned upper-triangular rho (condition number ~1e8), as phase C and thinQR apply it
    d = np.logspace(0, -8, m) * np.exp(2j * np.pi * rng.uniform(size=m))
    R = np.diag(d) @ (np.eye(m) + 0.3 * np.triu(a + 1j * b, 1))
    assert np.linalg.cond(R) > 1e7
    return np.triu(np.linalg.inv(R))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", [16, 32])
@pytest.mark.parametrize("dims", [[16, 8, 8, 8], [5, 3, 7]], ids=["batched", "ragged"])
def test_right_multiplications_against_the_oracle(bc, orc, monkeypatch, kind, m, dims):
    monkeypatch.setenv("BCG_HOP_PATCH", "16,2,2")
    V = int(np.prod(dims))
    Xh = orc.fill_field(m, V, 61)
    Yh = orc.fill_field(m, V, 62)
    # a field whose imaginary parts are a million times its real parts: x_re + x_im keeps only the leading digits of x_re
    Zh = Xh.real * 1e-6 + 1j * Xh.imag
    C = _coefficients(kind, m, 63)
    ctx = bc.Context(dims)
    F = lambda a: bc.block_fermion_field(ctx, m, a)  # noqa: E731
    zero = np.zeros_like(Yh)
    for x in (Xh, Zh):
        assert rel_err(F(zero).add(F(x), C).download(), orc.add_matrix(zero, x, C)) < TOL_KERNEL, "x C"
        assert rel_err(F(Yh).add(F(x), C).download(), orc.add_matrix(Yh, x, C)) < TOL_KERNEL, "K5"
        assert rel_err(F(Yh).rescale_add(C, F(x), 0.7).download(), orc.rescale_add_matrix(Yh, C, x, 0.7)) < TOL_KERNEL, "K6"
        assert rel_err(F(x).rescale_add(C, F(zero), 1.0).download(), orc.rescale_add_matrix(x, C, zero, 1.0)) < TOL_KERNEL, "x C"
    ctx.close()


@pytest.mark.parametrize("summed", [False, True], ids=["plain", "sum"])
def test_short_seeded_solve_against_the_oracle(bc, orc, monkeypatch, summed):
    """m = 16, four shifts, nine iterations: the shift updates are grouped over four iterations (the closing pass
    k_phaseC_multi at depth 4) and the iterations after the last full group go to the other kernels."""
    monkeypatch.setenv("BCG_HOP_PATCH", "16,2,2")
    m, dims, mass = 16, [8, 8, 8, 8], 0.05
    shifts = [0.0, 1e-4, 1e-2, 0.5]
    residues = [0.3, -1.25, 2.0, 0.7]
    iters = 9
    ctx = bc.Context(dims)
    ctx.profiling(True)
    D = bc.dirac_op(ctx, mass, seed=3)
    B = bc.block_fermion_field(ctx, m).setRandom(seed=4)
    if summed:
        Y = bc.block_fermion_field(ctx, m)
        info = bc.SBCGrQ_sum(Y, B, D, shifts, residues, 0.0, 0.0, 0.0, max_iterations=iters, trace_limit=iters,
                             return_info=True)
    else:
        X = [bc.block_fermion_field(ctx, m) for _ in shifts]
        info = bc.SBCGrQ(X, B, D, shifts, 0.0, 0.0, max_iterations=iters, trace_limit=iters, return_info=True)
    prof = ctx.profile()
    U = orc.fill_gauge(dims, 3)
    Bh = orc.fill_field(m, ctx.V, 4)
    o = orc.sbcgrq(U, dims, mass, Bh, shifts, 0.0, 0.0, max_iterations=iters, trace_limit=iters)
    assert info["iterations"] == o["iterations"] == iters
    if summed:
        assert prof["phaseC_multi4_sum"]["count"] >= 1
        want = sum(a * x for a, x in zip(residues, o["X"]))
        assert rel_err(Y.download(), want) < 1e-11
    else:
        assert prof["phaseC_multi4"]["count"] >= 1
        assert rel_err(np.stack([x.download() for x in X]), o["X"]) < 1e-11
    for key in ("alpha", "rho", "delta", "alpha_s", "beta_s"):
        assert rel_err(info["trace"][key], o["trace"][key]) < TOL_COEFF, key
    ctx.close()
