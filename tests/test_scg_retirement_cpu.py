"""SCG's retirement counter on the CPU (no GPU needed): why bcg_scg_solve gives it a floor of 1.

src/standard_solvers.cpp:90-92 decrements the number of active shifts whenever |r| zeta_last < eps_shifts, with no floor.  There
it is harmless: x_0 and p_0 are updated outside the shift loop (:73-75).  In bcg_scg_solve shift 0 is entry 0 of the `active`
entries handed to the fused update, so a counter of 0 stops the base system (and indexes coefficient vectors of length 0).
This file replays the solver's HOST arithmetic -- the scalar recurrences :65-81 and the retirement line -- over residual norms
computed with the oracle's operator, and shows that on the inputs tests/test_standard_solvers.py uses the unguarded counter
reaches 0 while the loop still has most of its iterations to run; the guarded one stops at 1.  It also checks the oracle's
guarded SCG: same results as CG for the base system, bit for bit."""
import numpy as np

DIMS, MASS, EPS, EPS_SHIFTS = [12, 6, 4], 0.05, 1e-10, 1e-4


def _inputs(orc):
    V = int(np.prod(DIMS))
    return orc.fill_gauge(DIMS, 81), orc.fill_field(1, V, 82)


def _replay_counter(orc, U, b, sigma, eps, eps_shifts, floor):
    """CG on the base system with numpy sums, the zeta / theta recurrences and the retirement line as the library's host
    code has them.  Returns (iterations run, iteration at which the counter first fell below 1 or None, final counter)."""
    n = len(sigma)
    rdot = lambda u, v: float(np.vdot(u, v).real)  # noqa: E731
    x = np.zeros_like(b)
    p, r = b.copy(), b.copy()
    rr = rdot(r, r)
    stop = eps * np.sqrt(rr)
    alpha, beta = 1.0, 0.0
    zeta, theta = np.ones(n), np.ones(n)
    active, it, first_zero, ratio = n, 0, None, None
    while np.sqrt(rr) > stop and it < 5000:
        t = orc.dirac_apply(U, DIMS, MASS, p) + sigma[0] * p
        it += 1
        alpha_old = alpha
        alpha = rr / rdot(p, t)
        r = r - alpha * t
        rr_old, beta_old = rr, beta
        rr = rdot(r, r)
        beta = rr / rr_old
        x = x + alpha * p
        p = beta * p + r
        for s in range(active - 1, 0, -1):
            inv_theta = 1.0 + (sigma[s] - sigma[0]) * alpha + beta_old * (alpha / alpha_old) * (1.0 - theta[s])
            theta[s] = 1.0 / inv_theta
            zeta[s] *= theta[s]
        # (at 0 the unguarded library would go on to read zeta[-1]; the replay stops counting there)
        if active > (1 if floor else 0) and np.sqrt(rr) * zeta[active - 1] < eps_shifts:
            active -= 1
            if active == 0:
                first_zero, ratio = it, np.sqrt(rr) / stop
    return it, first_zero, ratio, active


def test_unguarded_counter_reaches_zero_long_before_convergence(orc):
    U, b = _inputs(orc)
    for sigma in ([0.0, 0.3, 2.0, 9.0], [0.0]):
        it, first_zero, ratio, _ = _replay_counter(orc, U, b, sigma, EPS, EPS_SHIFTS, floor=False)
        # the counter is 0 with the base system's residual still orders above its stopping criterion (eps_shifts / (eps |b|)
        # = 4e4 at most) and many iterations from it
        assert first_zero is not None and first_zero < it - 100 and ratio > 100, (sigma, first_zero, it, ratio)
        it_g, zero_g, _, active = _replay_counter(orc, U, b, sigma, EPS, EPS_SHIFTS, floor=True)
        assert zero_g is None and active == 1 and it_g == it, (sigma, it_g, it, active)


def test_oracle_scg_base_system_is_cg_bit_for_bit(orc):
    """The guarded oracle gives what the reference gives: x_0 is CG's solution whatever retires (same statements on the same
    values), and one shift alone with a loose eps_shifts is CG."""
    U, b = _inputs(orc)
    x_cg, it_cg = orc.cg(U, DIMS, MASS, b, EPS)
    for sigma in ([0.0, 0.3, 2.0, 9.0], [0.0]):
        x, it = orc.scg(U, DIMS, MASS, b, sigma, EPS, EPS_SHIFTS)
        assert it == it_cg and np.array_equal(x[0], x_cg), sigma
        res = orc.true_residuals(U, DIMS, MASS, b, sigma, x)
        assert res[0].max() < 2 * EPS and (len(sigma) == 1 or res[1:].min() > 100 * EPS), res
