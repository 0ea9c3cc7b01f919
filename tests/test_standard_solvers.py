"""CG, SCG, BCG and BCGrQ (capi_solvers.hip: bcg_cg_solve, bcg_scg_solve, bcg_bcg_solve, bcg_bcgrq_solve -- what the drop-in
standard_solvers.hpp and block_solvers.hpp call) against the CPU oracle on seeded inputs:
  * a fixed number of iterations, where convergence cannot smooth over a kernel error: every width class, 4-D, 3-D and 1-D;
  * the fused SCG update (k_scg_update) against the plain axpys of CG, bit for bit;
  * its grid-stride wrap and ragged tail (more elements than one grid pass, not a multiple of the block);
  * shifts that retire while the base system goes on, one shift alone, more shifts than one launch holds;
  * half-volume fields;  * refused arguments.
Every solve that runs to convergence is capped at the oracle's iteration count + 2, so that a wrong library stops."""
import numpy as np
import pytest

from conftest import TOL_SOLUTION, rel_err

pytestmark = pytest.mark.gpu

MASS = 0.2
SHIFTS3 = [0.0, 1e-3, 0.5]
FIXED_DIMS = [[6, 4, 2, 3], [5, 3, 7], [37]]
WIDTHS = [1, 2, 5, 8, 16, 17, 32]
ITERS = 4
TOL_FIXED = 1e-11      # X after four fixed iterations (the figure of test_gpu_parity.py::test_every_block_width)
TOL_RESIDUAL = 1e-9    # true residuals of unconverged iterates, O(1) values


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, list) else str(v)


@pytest.fixture(scope="module")
def bc():
    import blockcg_amd
    return blockcg_amd


# seeded host inputs, computed once per module and never written to
_GAUGE, _FIELD = {}, {}


def _gauge(orc, dims, seed):
    key = (tuple(dims), seed)
    if key not in _GAUGE:
        _GAUGE[key] = orc.fill_gauge(dims, seed)
        _GAUGE[key].setflags(write=False)
    return _GAUGE[key]


def _field(orc, m, V, seed):
    key = (m, V, seed)
    if key not in _FIELD:
        _FIELD[key] = orc.fill_field(m, V, seed)
        _FIELD[key].setflags(write=False)
    return _FIELD[key]


def _device(bc, dims, mass, U):
    ctx = bc.Context(dims)
    return ctx, bc.dirac_op(ctx, mass, U=U)


def _stack(xs):
    return np.stack([x.download() for x in xs])


def _check_residuals(bc, orc, xs, b, D, U, dims, mass, bh, shifts):
    """bcg_true_residuals on the device against the oracle's, on the very fields the device holds."""
    got = bc.true_residuals(xs, b, D, shifts)
    want = orc.true_residuals(U, dims, mass, bh, shifts, _stack(xs))
    assert rel_err(got, want) < TOL_RESIDUAL, (got, want)


# ---- fixed work --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", FIXED_DIMS, ids=_ids)
def test_cg_and_scg_fixed_iterations_match_oracle(bc, orc, dims):
    V = int(np.prod(dims))
    U, bh = _gauge(orc, dims, 5), _field(orc, 1, V, 6)
    ctx, D = _device(bc, dims, MASS, U)
    b = bc.block_fermion_field(ctx, 1, bh)
    x = bc.block_fermion_field(ctx, 1)
    it = bc.CG(x, b, D, 0.0, max_iterations=ITERS)
    xo, ito = orc.cg(U, dims, MASS, bh, 0.0, ITERS)
    assert it == ito == ITERS
    assert rel_err(x.download(), xo) < TOL_FIXED
    _check_residuals(bc, orc, [x], b, D, U, dims, MASS, bh, [0.0])
    xs = [bc.block_fermion_field(ctx, 1) for _ in SHIFTS3]
    it = bc.SCG(xs, b, D, SHIFTS3, 0.0, 0.0, max_iterations=ITERS)
    xo, ito = orc.scg(U, dims, MASS, bh, SHIFTS3, 0.0, 0.0, ITERS)
    assert it == ito == ITERS
    for s in range(len(SHIFTS3)):
        assert rel_err(xs[s].download(), xo[s]) < TOL_FIXED, s
    _check_residuals(bc, orc, xs, b, D, U, dims, MASS, bh, SHIFTS3)


@pytest.mark.parametrize("m", WIDTHS)
@pytest.mark.parametrize("dims", FIXED_DIMS, ids=_ids)
def test_bcg_and_bcgrq_fixed_iterations_match_oracle(bc, orc, dims, m):
    """Four fixed iterations -- but no more than the field has room for.  k iterations span a block Krylov space of m k of the
    field's 3 V directions, and the residual block after them is orthogonal to it.  BCG inverts P^dagger A P, m new
    directions per iteration: k m <= 3 V.  BCGrQ also orthonormalises the residual block (thinQR) in the same iteration, m
    further directions: (k + 1) m <= 3 V; past that the block's Gram matrix is singular and the library reports the
    breakdown (BCG_ERR_NUMERIC), as it should.  One step further either solver is undefined: the oracle with sequential
    and with tree-shaped sums then differs from itself by 1.0 (BCG) or returns NaN (BCGrQ).
    That bites at one case only: 37 sites, m = 32, 3 V = 111 -- three iterations of BCG, two of BCGrQ (the oracle's own
    spread there is 9e-15 and 1e-15; at most 2e-15 in every other case)."""
    V = int(np.prod(dims))
    room = {False: min(ITERS, 3 * V // m), True: min(ITERS, 3 * V // m - 1)}
    assert room == {False: ITERS, True: ITERS} or (dims, m, room) == ([37], 32, {False: 3, True: 2})
    U, Bh = _gauge(orc, dims, 5), _field(orc, m, V, 6)
    ctx, D = _device(bc, dims, MASS, U)
    B = bc.block_fermion_field(ctx, m, Bh)
    X = bc.block_fermion_field(ctx, m)
    for with_qr, solver in ((False, bc.BCG), (True, bc.BCGrQ)):
        iters = room[with_qr]
        it = solver(X, B, D, 0.0, max_iterations=iters)
        Xo, ito = orc.bcg(U, dims, MASS, Bh, 0.0, iters, with_qr=with_qr)
        assert it == ito == iters, with_qr
        assert rel_err(X.download(), Xo) < TOL_FIXED, with_qr
        _check_residuals(bc, orc, [X], B, D, U, dims, MASS, Bh, [0.0])


# ---- the fused SCG update against the plain axpys ----------------------------------------------------------------------
RET_DIMS, RET_MASS, RET_EPS = [12, 6, 4], 0.05, 1e-10   # 288 sites; gauge seed 81, source seed 82


def _retirement_inputs(bc, orc, dims=RET_DIMS):
    V = int(np.prod(dims))
    U, bh = _gauge(orc, dims, 81), _field(orc, 1, V, 82)
    ctx, D = _device(bc, dims, RET_MASS, U)
    return U, bh, ctx, D, bc.block_fermion_field(ctx, 1, bh)


def _cg_on_device(bc, orc, ctx, D, b, U, bh, dims=RET_DIMS):
    xo, ito = orc.cg(U, dims, RET_MASS, bh, RET_EPS)
    x = bc.block_fermion_field(ctx, 1)
    it = bc.CG(x, b, D, RET_EPS, max_iterations=ito + 2)
    assert abs(it - ito) <= 1 and rel_err(x.download(), xo) < TOL_SOLUTION
    return x.download(), it, xo


def test_scg_with_the_single_shift_zero_is_cg_bit_for_bit(bc, orc):
    """k_scg_update promises the iterates of the unfused axpys; with the one shift 0 those are CG's (the oracle shows the same
    on the CPU: tests/test_scg_retirement_cpu.py).  Converged: every coefficient of ~700 iterations comes from those iterates."""
    U, bh, ctx, D, b = _retirement_inputs(bc, orc)
    x_cg, it_cg, _ = _cg_on_device(bc, orc, ctx, D, b, U, bh)
    xs = [bc.block_fermion_field(ctx, 1)]
    it = bc.SCG(xs, b, D, [0.0], RET_EPS, max_iterations=it_cg + 2)
    assert it == it_cg
    assert np.array_equal(xs[0].download(), x_cg)


# ---- grid-stride wrap and ragged tail of k_scg_update ------------------------------------------------------------------
LONG_V = 700003   # m = 1: 2 100 009 elements > 8192 blocks x 256 threads of one grid pass, and no multiple of 256


@pytest.fixture(scope="module")
def long_lattice(bc, orc):
    dims = [LONG_V]
    ctx = bc.Context(dims)
    D = bc.dirac_op(ctx, MASS, seed=91)            # links seeded on the device; the oracle's from the same generator
    bh = orc.fill_field(1, LONG_V, 92)
    return dict(dims=dims, ctx=ctx, D=D, b=bc.block_fermion_field(ctx, 1, bh), bh=bh, U=orc.fill_gauge(dims, 91))


def test_scg_update_wraps_the_grid_and_handles_the_ragged_tail(bc, orc, long_lattice):
    L = long_lattice
    assert 3 * LONG_V > 8192 * 256 and (3 * LONG_V) % 256 != 0
    xs = [bc.block_fermion_field(L["ctx"], 1) for _ in SHIFTS3]
    it = bc.SCG(xs, L["b"], L["D"], SHIFTS3, 0.0, 0.0, max_iterations=ITERS)
    xo, ito = orc.scg(L["U"], L["dims"], MASS, L["bh"], SHIFTS3, 0.0, 0.0, ITERS)
    assert it == ito == ITERS
    for s in range(len(SHIFTS3)):
        got = xs[s].download()
        assert rel_err(got, xo[s]) < TOL_FIXED, s
        # on their own: the sites whose elements come after the first grid pass (second trip of the grid-stride loop), and
        # those of the last, partly filled block (2 100 009 = 8203 x 256 + 41 elements: the last 14 sites)
        assert rel_err(got[8192 * 256 // 3:], xo[s][8192 * 256 // 3:]) < TOL_FIXED, s
        assert rel_err(got[-14:], xo[s][-14:]) < TOL_FIXED, s


def test_scg_single_shift_is_cg_bit_for_bit_on_the_long_lattice(bc, long_lattice):
    L = long_lattice
    x = bc.block_fermion_field(L["ctx"], 1)
    xs = [bc.block_fermion_field(L["ctx"], 1)]
    assert bc.CG(x, L["b"], L["D"], 0.0, max_iterations=6) == 6
    assert bc.SCG(xs, L["b"], L["D"], [0.0], 0.0, 0.0, max_iterations=6) == 6
    assert np.array_equal(xs[0].download(), x.download())


# ---- retirement --------------------------------------------------------------------------------------------------------
def test_scg_shifts_retire_and_the_base_system_goes_on(bc, orc):
    """eps_shifts is compared with the unnormalised residual times zeta (src/standard_solvers.cpp:90), eps is scaled by |b|
    (:57): with eps_shifts = 1e-4 > eps |b| = 2.4e-9 the counter of active shifts would pass 1 long before the base system
    has converged.  The reference updates x_0, p_0 outside its shift loop, so its base system runs to eps whatever the
    counter says; here shift 0 is an entry of the fused launch and must never retire.  (A library without that floor
    stops updating x_0: its true residual stays near eps_shifts / |b|, four orders above 2 eps.)"""
    shifts, eps_s = [0.0, 0.3, 2.0, 9.0], 1e-4
    U, bh, ctx, D, b = _retirement_inputs(bc, orc)
    xo, ito = orc.scg(U, RET_DIMS, RET_MASS, bh, shifts, RET_EPS, eps_s)
    xs = [bc.block_fermion_field(ctx, 1) for _ in shifts]
    it = bc.SCG(xs, b, D, shifts, RET_EPS, eps_s, max_iterations=ito + 2)
    assert abs(it - ito) <= 1, (it, ito)
    got = _stack(xs)
    # the shifted systems did retire before the end (else this test checks nothing): their residuals stay far above eps
    ro = orc.true_residuals(U, RET_DIMS, RET_MASS, bh, shifts, xo)
    assert ro[1:].min() > 100 * RET_EPS, ro
    assert rel_err(got[1:], xo[1:]) < 1e-9      # frozen at the same iterations
    x_cg, _, xo_cg = _cg_on_device(bc, orc, ctx, D, b, U, bh)
    assert rel_err(got[0], xo_cg) < TOL_SOLUTION and rel_err(got[0], x_cg) < TOL_SOLUTION
    res = bc.true_residuals(xs, b, D, shifts)
    assert res[0].max() < 2 * RET_EPS, res


def test_scg_one_shift_with_a_loose_eps_shifts_is_cg_bit_for_bit(bc, orc):
    """n_shifts = 1: zeta_0 stays 1, so the retirement line compares |r| itself with eps_shifts -- true from |r| < 1e-4 on,
    with the solve needing |r| < 2.4e-9.  Shift 0 does not retire: same count and solution as CG."""
    U, bh, ctx, D, b = _retirement_inputs(bc, orc)
    x_cg, it_cg, _ = _cg_on_device(bc, orc, ctx, D, b, U, bh)
    xs = [bc.block_fermion_field(ctx, 1)]
    it = bc.SCG(xs, b, D, [0.0], RET_EPS, 1e-4, max_iterations=it_cg + 2)
    assert it == it_cg
    assert np.array_equal(xs[0].download(), x_cg)
    assert bc.true_residuals(xs, b, D, [0.0]).max() < 2 * RET_EPS


MANY_DIMS = [8, 4, 4, 2]
MANY_SHIFTS = [0.05 * k for k in range(20)]


def _oracle_spread_of_retired_solutions(orc, U, dims, bh, shifts, eps, eps_s, x_ref):
    """How far the ORACLE's own solutions move, per shift, when one element of the source changes by one ulp (12 samples,
    the largest kept).  A retired solution is frozen at the iteration |r| zeta_s first falls below eps_shifts; after
    hundreds of CG iterations |r| has drifted by far more than an ulp between any two roundings of the same arithmetic, so
    a shift that retires late is frozen an iteration earlier or later, or at a slightly different iterate."""
    worst = np.zeros(len(shifts))
    for k in range(12):
        bp = bh.copy()
        v = bp.view(np.float64).reshape(-1)
        v[17 * k + 3] = np.nextafter(v[17 * k + 3], np.inf)
        x, _ = orc.scg(U, dims, RET_MASS, bp, shifts, eps, eps_s)
        worst = np.maximum(worst, [rel_err(x[s], x_ref[s]) for s in range(len(shifts))])
    return worst


def test_scg_more_shifts_than_one_launch_holds(bc, orc):
    """20 shifts: two launches of k_scg_update per iteration (16 + 4) until the counter of active shifts has fallen to 16,
    one from there on; it falls through 16 while the solve runs.
    Bound per shift: 1e-9, or ten times the oracle's own spread under a one-ulp change of the source where that is larger.
    (The oracle's sums in SCG do not depend on set_gram_arith -- sequential and tree-shaped runs are bit-identical -- so the
    spread is taken over perturbed inputs.)  Measured: shift 1 (sigma = 0.05, the last to retire, some 300 iterations in)
    moves by 2e-7 .. 4.4e-6 in the oracle, shift 2 by 1e-10, shift 0 by 7e-13, every other shift by less than 1e-13; the
    library differs from the oracle by 4.0e-6 at shift 1."""
    eps_s = 1e-3
    U, bh, ctx, D, b = _retirement_inputs(bc, orc, MANY_DIMS)
    xo, ito = orc.scg(U, MANY_DIMS, RET_MASS, bh, MANY_SHIFTS, RET_EPS, eps_s)
    # shift 15 did retire (its solution differs from the one it converges to without retirement): at most 15 were active at the end
    x_all, _ = orc.scg(U, MANY_DIMS, RET_MASS, bh, MANY_SHIFTS, RET_EPS, 0.0)
    assert not np.array_equal(xo[15], x_all[15])
    xs = [bc.block_fermion_field(ctx, 1) for _ in MANY_SHIFTS]
    it = bc.SCG(xs, b, D, MANY_SHIFTS, RET_EPS, eps_s, max_iterations=ito + 2)
    assert abs(it - ito) <= 1, (it, ito)
    got = _stack(xs)
    spread = _oracle_spread_of_retired_solutions(orc, U, MANY_DIMS, bh, MANY_SHIFTS, RET_EPS, eps_s, xo)
    assert spread[2:].max() < 1e-9 and spread[0] < 1e-10, spread   # the bound is wider than 1e-9 at shift 1 at most
    for s in range(len(MANY_SHIFTS)):
        assert rel_err(got[s], xo[s]) < max(1e-9, 10 * spread[s]), (s, spread[s])
    assert bc.true_residuals(xs[:1], b, D, [0.0]).max() < 2 * RET_EPS
    # fixed work, nothing retires: both launches of every iteration against the oracle
    it = bc.SCG(xs, b, D, MANY_SHIFTS, 0.0, 0.0, max_iterations=ITERS)
    xo4, ito4 = orc.scg(U, MANY_DIMS, RET_MASS, bh, MANY_SHIFTS, 0.0, 0.0, ITERS)
    assert it == ito4 == ITERS
    for s in range(len(MANY_SHIFTS)):
        assert rel_err(xs[s].download(), xo4[s]) < TOL_FIXED, s


# ---- half-volume fields ------------------------------------------------------------------------------------------------
def _parity_masks(dims):
    V = int(np.prod(dims))
    idx = np.arange(V)
    par = np.zeros(V, dtype=np.int64)
    for L in dims:           # x0 fastest
        par += idx % L
        idx = idx // L
    return [(par % 2) == p for p in (0, 1)]


@pytest.mark.parametrize("dims", [[8, 4, 4, 6], [4, 6, 2, 4]], ids=_ids)
def test_solvers_on_half_volume_fields(bc, orc, dims):
    """The operator does not mix site parities (tests/test_half_volume.py), so a solve on the half field of parity q is the
    full-volume solve of the source with its other parity zeroed: the zero sites add exact zeros to every sum, the
    coefficients are the half solve's.  (The full-volume solve of the WHOLE source is another iteration: its scalar and
    m x m coefficients mix the two parities' sums, so after a fixed number of iterations it is not the two half solves.)
    Four fixed iterations, every solver, both parities, merged and compared on the full lattice."""
    V = int(np.prod(dims))
    U = _gauge(orc, dims, 5)
    masks = _parity_masks(dims)
    ctx, D = _device(bc, dims, MASS, U)

    def masked(a, q):
        out = a.copy()
        out[~masks[q]] = 0.0
        return out

    def run(m, device_solve, oracle_solve, shifts):
        Bh = _field(orc, m, V, 6)
        B = bc.block_fermion_field(ctx, m, Bh)
        halves = B.split_parity()
        want = np.zeros((len(shifts), V, m, 3), dtype=np.complex128)
        parts = []
        for q in (0, 1):
            Xq = [bc.block_fermion_field(ctx, m, parity=q) for _ in shifts]
            assert device_solve(Xq, halves[q]) == ITERS
            Bq = masked(Bh, q)
            Xo = oracle_solve(Bq)
            assert not Xo[:, ~masks[q]].any()        # the oracle's solution stays on parity q
            want += Xo
            # true residuals of the half fields: the oracle's full-lattice ones of the same fields, zero elsewhere
            full = np.zeros_like(want)
            full[:, masks[q]] = _stack(Xq)
            got_res = bc.true_residuals(Xq, halves[q], D, shifts)
            assert rel_err(got_res, orc.true_residuals(U, dims, MASS, Bq, shifts, full)) < TOL_RESIDUAL, (m, q)
            parts.append(Xq)
        for s in range(len(shifts)):
            merged = bc.block_fermion_field(ctx, m).merge_parity(parts[0][s], parts[1][s])
            assert rel_err(merged.download(), want[s]) < TOL_FIXED, (m, s)

    run(1, lambda X, B: bc.CG(X[0], B, D, 0.0, max_iterations=ITERS),
        lambda Bq: orc.cg(U, dims, MASS, Bq, 0.0, ITERS)[0][None], [0.0])
    run(1, lambda X, B: bc.SCG(X, B, D, SHIFTS3, 0.0, 0.0, max_iterations=ITERS),
        lambda Bq: orc.scg(U, dims, MASS, Bq, SHIFTS3, 0.0, 0.0, ITERS)[0], SHIFTS3)
    run(5, lambda X, B: bc.BCG(X[0], B, D, 0.0, max_iterations=ITERS),
        lambda Bq: orc.bcg(U, dims, MASS, Bq, 0.0, ITERS)[0][None], [0.0])
    run(16, lambda X, B: bc.BCGrQ(X[0], B, D, 0.0, max_iterations=ITERS),
        lambda Bq: orc.bcg(U, dims, MASS, Bq, 0.0, ITERS, with_qr=True)[0][None], [0.0])


# ---- refused arguments -------------------------------------------------------------------------------------------------
def test_refused_arguments_return_invalid_and_leave_x_untouched(bc):
    dims = [8, 4]
    ctx, other = bc.Context(dims), bc.Context(dims)
    D = bc.dirac_op(ctx, 0.5, seed=1)
    new = lambda c, m, seed, parity=None: bc.block_fermion_field(c, m, parity=parity).setRandom(seed=seed)  # noqa: E731
    b1, b3 = new(ctx, 1, 2), new(ctx, 3, 3)
    x1, x1b, x3 = new(ctx, 1, 4), new(ctx, 1, 5), new(ctx, 3, 6)
    b_even, x_odd = new(ctx, 1, 7, 0), new(ctx, 1, 8, 1)
    x_far, b_far = new(other, 1, 9), new(other, 1, 10)
    X_even5, B_odd5 = new(ctx, 5, 11, 0), new(ctx, 5, 12, 1)
    X_far5, B5 = new(other, 5, 13), new(ctx, 5, 14)
    cases = [
        ("CG on width 3", lambda: bc.CG(x3, b3, D, 1e-10), [x3, b3]),
        ("SCG on width 3", lambda: bc.SCG([x3], b3, D, [0.0], 1e-10), [x3, b3]),
        ("SCG: one x_s of width 3", lambda: bc.SCG([x1, x3], b1, D, [0.0, 0.1], 1e-10), [x1, x3]),
        ("CG: x is b", lambda: bc.CG(b1, b1, D, 1e-10), [b1]),
        ("SCG: x_1 is b", lambda: bc.SCG([x1, b1], b1, D, [0.0, 0.1], 1e-10), [x1, b1]),
        ("BCG: X is B", lambda: bc.BCG(b3, b3, D, 1e-10), [b3]),
        ("BCGrQ: X is B", lambda: bc.BCGrQ(b3, b3, D, 1e-10), [b3]),
        ("SCG: negative first shift", lambda: bc.SCG([x1, x1b], b1, D, [-0.1, 0.0], 1e-10), [x1, x1b]),
        ("SCG: unsorted shifts", lambda: bc.SCG([x1, x1b], b1, D, [0.1, 0.0], 1e-10), [x1, x1b]),
        ("CG: parities differ", lambda: bc.CG(x_odd, b_even, D, 1e-10), [x_odd]),
        ("SCG: parities differ", lambda: bc.SCG([x_odd], b_even, D, [0.0], 1e-10), [x_odd]),
        ("CG: half x, full b", lambda: bc.CG(x_odd, b1, D, 1e-10), [x_odd]),
        ("BCG: parities differ", lambda: bc.BCG(X_even5, B_odd5, D, 1e-10), [X_even5]),
        ("BCGrQ: parities differ", lambda: bc.BCGrQ(X_even5, B_odd5, D, 1e-10), [X_even5]),
        ("CG: x of another context", lambda: bc.CG(x_far, b1, D, 1e-10), [x_far]),
        ("CG: b of another context", lambda: bc.CG(x1, b_far, D, 1e-10), [x1]),
        ("SCG: x of another context", lambda: bc.SCG([x_far], b1, D, [0.0], 1e-10), [x_far]),
        ("SCG: b of another context", lambda: bc.SCG([x1], b_far, D, [0.0], 1e-10), [x1]),
        ("BCG: X of another context", lambda: bc.BCG(X_far5, B5, D, 1e-10), [X_far5]),
        ("BCGrQ: X of another context", lambda: bc.BCGrQ(X_far5, B5, D, 1e-10), [X_far5]),
        ("SCG: no shifts", lambda: bc.SCG([], b1, D, [], 1e-10), [x1, b1]),
    ]
    for name, call, fields in cases:
        before = [f.download() for f in fields]
        with pytest.raises(bc.BlockCGError) as e:
            call()
        assert e.value.code == 1, name          # BCG_ERR_INVALID
        for f, a in zip(fields, before):
            assert np.array_equal(f.download(), a), name
    # the same fields in a call that is in order: it runs
    assert bc.SCG([x1, x1b], b1, D, [0.0, 0.1], 1e-10, max_iterations=3) == 3
