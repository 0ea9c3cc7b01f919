"""The factored stencil pair as an OPERATOR (capi_operator.hip: plan_pair; kernels_stencil.hip: k_hop4b<16, HOP_FACT1>,
k_hop4b<16, HOP_FACT2>): one phase A of a solver, T = (A + sigma_0) P and G = P^dagger T, run once by the test aid
bcg_debug_phase_a and held field by field against tests/phase_a_ref.py -- the unfactored T = (m^2 + sigma_0) P - D (D P) in
extended precision with its own neighbour table, no mu anywhere -- over launch geometries, tuning, parameters of the
factorisation, against the other form (BCG_HOP_FACTORED=0), against the solver's own launch and interleaved with the other
users of tmp, partials, dev_gram and the fold tickets in one context.

Every case asserts from the profile which form ran (stencil_form_factored_pair once per call with two k_hop4b launches and
no k_hop4c; or the key absent where the pair must decline) and prints every error it measured with the form's name.

Bounds, all the project's constants: rel_err(T) < TOL_KERNEL and per site |T - T_ref| < 1e-13 max |T_ref| (the form of
tests/test_fullsize_parity.py), rel_err(G) <= TOL_KERNEL, on against off within FORM_BOUND of tests/test_factored_stencil.py.
The reference's own share (tests/test_phase_a_ref_cpu.py, on the CPU): T_ref against the oracle's double-precision
dirac_apply 1.58e-16 .. 1.59e-16 in the norm and at most 3.2e-16 per site at every shape here (held below TOL_KERNEL / 10
there: a margin of 600 under TOL_KERNEL), G_ref against numpy's complex128 product 1.2e-16 .. 7.1e-16.

The x3 pipeline of k_hop4b at L3 = 1, 2, 3 (whole-field window x3_lo = 0, x3_n = L3, direction 3 undivided, no ring; the
software-pipelined step, which m = 16 takes).  Slots and link images alternate by x3 & 1; "slice s" is the row
in + (col + s S3) RB of the wave's column, col < S3, so slice s is inside the field exactly when 0 <= s < L3:
  L3 = 1  prologue: centre slice_of(0) = slice 0, -x3 row slice_of(-1) = slice L3 - 1 = 0, links of slice 0 with U_3(x - 3)
          from slice L3 - 1 = 0.  The one step has more = false: no link DMA, no next rows, no park_u3; its +x3 row is the wrap
          row iw_* = slice_of(L3) = slice 0 (x3 + 1 < L3 is false).  The INCR pointers set up for slice 1 (ik_*, ir_*) are
          past the end and never dereferenced: every use is under `more` or `x3 + 1 < L3`.
  L3 = 2  prologue: slot 0 <- slice 0, slot 1 <- slice 1 (= L3 - 1).  Step 0 reads slot 1 as -x3 (slice 1: the wrap), DMAs
          slice 1 (ir_*) into slot 1 and the links of slice 1 into image 1, next rows from slice 1; step 1 reads slot 0 as
          -x3 (slice 0), has more = false and takes the wrap row slice 0 into slot 0, which no wave reads as a centre in that
          step (centres are slot 1) and which the next column's prologue rewrites behind its barrier.
  L3 = 3  prologue: slot 0 <- slice 0, slot 1 <- slice 2.  Steps 0, 1 DMA slices 1, 2 (ir_* advanced once each, never to slice
          3: the advance is under x3 + 1 < L3 at use), step 2 the wrap row slice 0; -x3 rows read back are slices 2, 0, 1.
          Link rows are fetched for slices 1 and 2 only (under `more`), U_3(x - 3) carried from the previous image.
  In all three p is not read (factored pair) or is slice x3 (other form), out is slice x3, 0 <= x3 < L3; the rows that leave the
  bundle in x1 / x2 are rows of the same slice.  All three extents ran and passed; nothing declines them.

Measured on the GPU (largest over each group; factored pair unless said):
  geometries   T 1.73e-16 in the norm, 2.8e-16 per site, G 1.5e-16 (L3 = 1, 2, 3: T 1.73e-16, 1.72e-16, 1.73e-16); the other
               form T 1.68e-16, G 1.4e-16; on against off T 1.80e-16 .. 1.82e-16, G 1.1e-16 .. 1.6e-16
  tuning       T 1.72e-16 / 2.8e-16 per site, G 1.2e-16; T bit-identical across pacing and tile order; G bit-identical under
               pacing, 1.5e-16 between the tile orders at 32x8x8x6
  parameters   pair: T 1.72e-16 / 2.5e-16 per site, G 1.4e-16; c0 <= 0 (other form, bundle sweep) T 1.69e-16, G 1.4e-16;
               BCG_HOP_BUNDLE=0 (other form, row sweep) T 1.67e-16, G 1.2e-16
  solver       raw G of the aid on thinQR(B) equals the raw G of the solver's first phase A bit for bit
  one context  T 1.72e-16, G 1.5e-16; D.op 2.1e-16, true_residuals 2.4e-15, D.D 1.9e-16 in between; calls 3 .. 6 equal
               call 1 bit for bit"""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest

from conftest import TOL_KERNEL, rel_err
import phase_a_ref as ref
from test_factored_stencil import FORM_BOUND, _count

pytestmark = pytest.mark.gpu

M = ref.M
MASS, SIGMA0 = 0.2, 0.05


@functools.lru_cache(maxsize=None)
def _inputs(name):
    import oracle
    dims = ref.ALL_SHAPES[name][0]
    U = oracle.Oracle().fill_gauge(dims, ref.SEED_U)
    P = np.random.default_rng(ref.SEED_P).normal(size=(int(np.prod(dims)), M, 3, 2)).view(np.complex128)[..., 0]
    P = np.ascontiguousarray(P)
    for a in (U, P):
        a.setflags(write=False)
    return dims, U, P


@functools.lru_cache(maxsize=None)
def _hop_twice(name):
    dims, U, P = _inputs(name)
    return ref.hop_twice(U, dims, P)


@functools.lru_cache(maxsize=None)
def _reference(name, mass, sigma0):
    """(T_ref, G_ref) of the shape's P, computed once and shared read-only."""
    dims, U, P = _inputs(name)
    T, G = ref.phase_a(U, dims, mass, sigma0, P, _hop_twice(name))
    for a in (T, G):
        a.setflags(write=False)
    return T, G


@contextlib.contextmanager
def _tuning(kv):
    """The environment a context is created under (every BCG_HOP_* is read there): None removes a variable."""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class _Run:
    """A context of the shape's tuning with the links and P on the device."""

    def __init__(self, name, factored=True, **env):
        import blockcg_amd as bc
        self.bc, self.name = bc, name
        self.dims, U, P = _inputs(name)
        _, patch, blocks = ref.ALL_SHAPES[name]
        # (patch None: the default-tuning row, which must see no override)
        tuning = {"BCG_HOP_FACTORED": int(factored), "BCG_HOP_PATCH": patch, "BCG_HOP_BLOCKS": blocks}
        tuning.update(env)
        with _tuning(tuning):
            self.ctx = bc.Context(self.dims)
        self.ctx.profiling(True)
        self.D = bc.dirac_op(self.ctx, MASS, U=U)
        self.P = bc.block_fermion_field(self.ctx, M, P)
        self.T = bc.block_fermion_field(self.ctx, M)
        self.calls = 0
        lib = self.ctx.lib
        lib.bcg_debug_phase_a.restype = ctypes.c_int
        lib.bcg_debug_phase_a.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_void_p,
                                          ctypes.c_void_p]
        for fn in (lib.bcg_debug_phase_a_gram, lib.bcg_debug_phase_a_gram_raw):
            fn.restype = ctypes.c_int
            fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]

    def _gram(self, fn):
        G = np.zeros((M, M), dtype=np.complex128)  # column-major from the library
        return G.T.copy() if fn(self.ctx.h, M, G.ctypes.data_as(ctypes.c_void_p)) == 0 else None

    def phase_a(self, mass=MASS, sigma0=SIGMA0, P=None):
        """One call of the aid into a T full of NaN: (T, G as the host used it, G as the device summed it)."""
        self.T.upload(np.full((self.ctx.V, M, 3), complex(np.nan, np.nan)))
        self.ctx.check(self.ctx.lib.bcg_debug_phase_a(self.ctx.h, self.D.h, mass, sigma0, self.T.h, (P or self.P).h))
        self.calls += 1
        lib = self.ctx.lib
        return self.T.download(), self._gram(lib.bcg_debug_phase_a_gram), self._gram(lib.bcg_debug_phase_a_gram_raw)

    def assert_form(self, form):
        """From the profile, for the `calls` calls of the aid so far and nothing else on this context."""
        prof, n = self.ctx.profile(), self.calls
        if form == "factored pair":
            assert _count(prof, "stencil_form_factored_pair") == n, sorted(prof)
        else:
            assert "stencil_form_factored_pair" not in prof, sorted(prof)
        if form == "other form, row sweep":
            assert _count(prof, "stencil_form_k_hop4c") == 2 * n and "stencil_form_k_hop4b" not in prof, sorted(prof)
        else:
            assert _count(prof, "stencil_form_k_hop4b") == 2 * n and "stencil_form_k_hop4c" not in prof, sorted(prof)
        assert _count(prof, "hop") == n and _count(prof, "hop_shifted_gram") == n, sorted(prof)


def _hold(tag, form, T, G, T_ref, G_ref):
    """T and G of one call against the reference at the bounds of the module docstring; prints what it measured."""
    assert np.isfinite(T).all(), f"{tag}: T keeps NaN or holds Inf"
    e = rel_err(T, T_ref)
    e_site = np.abs(T - T_ref).max() / np.abs(T_ref).max()
    eg = rel_err(G, G_ref)
    print(f"{tag} [{form}; reference in {ref.PRECISION}]: T {e:.3e} (per site {e_site:.3e}), G {eg:.3e}")
    assert e < TOL_KERNEL
    assert np.abs(T - T_ref).max() < 1e-13 * np.abs(T_ref).max()
    assert eg <= TOL_KERNEL
    return e, e_site, eg


def _hold_raw(tag, G, G_raw):
    """The factored pair's G as the device summed it: exactly Hermitian, real diagonal, and what the host used."""
    assert G_raw is not None, tag
    assert np.all(np.diagonal(G_raw).imag == 0.0), tag
    assert np.array_equal(G_raw, G_raw.conj().T), tag
    assert np.array_equal(G_raw, G), tag


@functools.lru_cache(maxsize=None)
def _on(name, mass=MASS, sigma0=SIGMA0):
    run = _Run(name)
    out = run.phase_a(mass, sigma0)
    run.assert_form("factored pair")
    return out


@functools.lru_cache(maxsize=None)
def _off(name, mass=MASS, sigma0=SIGMA0):
    run = _Run(name, factored=False)
    out = run.phase_a(mass, sigma0)
    run.assert_form("other form, bundle sweep")
    return out


@pytest.mark.parametrize("name", list(ref.GEOMETRIES))
def test_geometry_against_the_reference(name):
    T, G, G_raw = _on(name)
    _hold(name, "factored pair", T, G_raw, *_reference(name, MASS, SIGMA0))
    _hold_raw(name, G, G_raw)


@pytest.mark.parametrize("name", list(ref.GEOMETRIES))
def test_geometry_against_the_other_form(name):
    (T, G, _), (T_off, G_off, _) = _on(name), _off(name)
    _hold(name, "other form, bundle sweep", T_off, G_off, *_reference(name, MASS, SIGMA0))
    e, eg = rel_err(T, T_off), rel_err(G, G_off)
    print(f"{name} factored pair vs other form: T {e:.3e}, G {eg:.3e}")
    assert 0.0 < e < FORM_BOUND  # (not bit-identical: another rounding of the same operator)
    assert 0.0 < eg < FORM_BOUND


@pytest.mark.parametrize("name", list(ref.TUNING_SHAPES))
def test_pacing_changes_no_bit_of_t(name):
    """BCG_HOP_SYNC / BCG_HOP_BUNDLE_SYNC 0/0 (unpaced), 1/-1 and 4/-4 (a negative window forces pacing on sweeps this short,
    as in test_column_sweep_stencil): pacing changes when a block runs, not what it computes."""
    outs = []
    for sync, bundle_sync in (("0", "0"), ("1", "-1"), ("4", "-4")):
        run = _Run(name, BCG_HOP_SYNC=sync, BCG_HOP_BUNDLE_SYNC=bundle_sync)
        T, G, G_raw = run.phase_a()
        run.assert_form("factored pair")
        _hold(f"{name} sync {sync}/{bundle_sync}", "factored pair", T, G_raw, *_reference(name, MASS, SIGMA0))
        _hold_raw(name, G, G_raw)
        outs.append((T, G_raw))
    for T, G in outs[1:]:
        assert np.array_equal(T, outs[0][0])
        e = rel_err(G, outs[0][1])
        print(f"{name}: G paced vs unpaced {e:.3e}")
        assert e <= FORM_BOUND


@pytest.mark.parametrize("name", list(ref.TUNING_SHAPES))
def test_super_patch_order_changes_no_bit_of_t(name):
    """BCG_HOP_SUPER: tile order only (at 16x8x8x8 with patches of 16 there is one patch in x0, so plan_hop4 keeps the plain
    order either way; 32x8x8x6 has 2 x 4 x 4 patches and takes the 2 x 2 x 2 super-patches).  G sums the same block partials
    in another order."""
    outs = []
    for sup in ("0", "1"):
        run = _Run(name, BCG_HOP_SUPER=sup)
        T, G, G_raw = run.phase_a()
        run.assert_form("factored pair")
        _hold(f"{name} super {sup}", "factored pair", T, G_raw, *_reference(name, MASS, SIGMA0))
        _hold_raw(name, G, G_raw)
        outs.append((T, G_raw))
    assert np.array_equal(outs[1][0], outs[0][0])
    e = rel_err(outs[1][1], outs[0][1])
    print(f"{name}: G super-patch order vs plain order {e:.3e}")
    assert e <= FORM_BOUND


@pytest.mark.parametrize("mass,sigma0", [(1e-3, 0.0), (0.2, 0.0), (0.5, -0.2), (0.0, 1e-12), (30.0, 100.0)])
def test_parameters_of_the_factorisation(mass, sigma0):
    """c0 = mass^2 + sigma_0 > 0 from 1e-12 to 1e3: mu = sqrt(c0) from 1e-6 to 32."""
    name = "16x8x8x8"
    T, G, G_raw = _on(name, mass, sigma0)
    _hold(f"{name} mass {mass} sigma0 {sigma0}", "factored pair", T, G_raw, *_reference(name, mass, sigma0))
    _hold_raw(name, G, G_raw)


@pytest.mark.parametrize("mass,sigma0", [(0.0, 0.0), (0.2, -0.04 - 1e-3)])
def test_pair_declines_without_a_positive_c0(mass, sigma0):
    """c0 <= 0 has no real mu: plan_pair() declines, and the other form's kernels give the same T and G."""
    name = "16x8x8x8"
    assert not mass * mass + sigma0 > 0.0
    run = _Run(name)
    T, G, _ = run.phase_a(mass, sigma0)
    run.assert_form("other form, bundle sweep")
    _hold(f"{name} mass {mass} sigma0 {sigma0}", "other form, bundle sweep", T, G, *_reference(name, mass, sigma0))


def test_pair_declines_on_the_row_sweep():
    """BCG_HOP_BUNDLE=0: the column sweep over rows (k_hop4c) has no factored modes."""
    name = "16x8x8x8"
    run = _Run(name, BCG_HOP_BUNDLE="0")
    T, G, _ = run.phase_a()
    run.assert_form("other form, row sweep")
    _hold(f"{name} BCG_HOP_BUNDLE=0", "other form, row sweep", T, G, *_reference(name, MASS, SIGMA0))


def test_aid_validates_its_arguments_like_dirac_apply():
    """Same context, same shape, T != P, otherwise BCG_ERR_INVALID (1) and nothing runs."""
    a, b = _Run("16x4x8x1"), _Run("16x4x8x2")
    aid = a.ctx.lib.bcg_debug_phase_a
    narrow = a.bc.block_fermion_field(a.ctx, 8)
    assert aid(a.ctx.h, a.D.h, MASS, SIGMA0, a.P.h, a.P.h) == 1          # T is P
    assert aid(a.ctx.h, a.D.h, MASS, SIGMA0, narrow.h, a.P.h) == 1       # another width
    assert aid(a.ctx.h, a.D.h, MASS, SIGMA0, b.T.h, a.P.h) == 1          # a field of another context
    assert aid(a.ctx.h, b.D.h, MASS, SIGMA0, a.T.h, a.P.h) == 1          # links of another context
    assert aid(a.ctx.h, None, MASS, SIGMA0, a.T.h, a.P.h) == 1 and aid(None, a.D.h, MASS, SIGMA0, a.T.h, a.P.h) == 1
    assert "hop" not in a.ctx.profile() and "hop" not in b.ctx.profile()
    assert aid(a.ctx.h, a.D.h, MASS, SIGMA0, a.T.h, a.P.h) == 0


def test_aid_runs_the_launch_of_the_solver():
    """One iteration of SBCGrQ, then the aid on P = thinQR(B) in a fresh context of the same settings.  The solver forms its
    first P_0 with the function behind bcg_field_thin_qr (capi_solvers.hip: sbcgrq_begin calls thin_qr on its copy of B and
    copies the result into P_0), whose kernels sum in a fixed order: the same bits reach the same launch, so the raw G of
    the two is equal bit for bit."""
    name = "16x8x8x8"
    bc = __import__("blockcg_amd")
    shifts = (SIGMA0, 0.3)
    solver = _Run(name)
    X = [bc.block_fermion_field(solver.ctx, M) for _ in shifts]
    bc.SBCGrQ(X, solver.P, solver.D, list(shifts), 0.0, 0.0, max_iterations=1)
    prof = solver.ctx.profile()
    assert _count(prof, "stencil_form_factored_pair") == 1 and _count(prof, "hop_shifted_gram") == 1, sorted(prof)
    G_solver = solver._gram(solver.ctx.lib.bcg_debug_phase_a_gram_raw)
    aid = _Run(name)
    aid.P.thinQR()
    T, G, G_raw = aid.phase_a(MASS, shifts[0])
    aid.assert_form("factored pair")
    _hold_raw(name, G, G_raw)
    assert np.isfinite(T).all()
    print(f"{name} [factored pair]: raw G of the aid vs the solver's first phase A {rel_err(G_raw, G_solver):.3e}")
    assert np.array_equal(G_raw, G_solver)
    # and it is the Gram matrix of A + sigma_0 = c0 - D^2 on an orthonormal block: no eigenvalue below c0 (to rounding)
    assert np.linalg.eigvalsh(G_raw).min() >= (MASS * MASS + shifts[0]) * (1.0 - 1e-10)


def test_one_context_shares_its_buffers():
    """tmp, partials, dev_gram and the fold tickets serve the unfactored hop and the fused residual besides: the pair
    alternated with D.op, D.D and true_residuals in ONE context gives the same bits before and after, every intermediate
    result matches its own reference, and the fold tickets come back to zero call after call."""
    import oracle
    orc = oracle.Oracle()
    name = "32x8x8x6"
    dims, U, P = _inputs(name)
    run = _Run(name)
    bc, ctx = run.bc, run.ctx
    out = bc.block_fermion_field(ctx, M)
    Xh = 0.25 * np.random.default_rng(ref.SEED_P + 1).normal(size=(ctx.V, M, 3, 2)).view(np.complex128)[..., 0]
    X = [bc.block_fermion_field(ctx, M, Xh)]
    T1, G1, R1 = run.phase_a(MASS, SIGMA0)
    _hold(f"{name} call 1", "factored pair", T1, R1, *_reference(name, MASS, SIGMA0))
    _hold_raw(name, G1, R1)
    run.D.op(out, run.P)
    e = rel_err(out.download(), orc.dirac_apply(U, dims, MASS, P))
    print(f"{name} D.op between the calls [other form]: {e:.3e}")
    assert e < TOL_KERNEL
    Tm, Gm, Rm = run.phase_a(MASS, 0.3)
    _hold(f"{name} call 2, sigma0 0.3", "factored pair", Tm, Rm, *_reference(name, MASS, 0.3))
    _hold_raw(name, Gm, Rm)
    res = bc.true_residuals(X, run.P, run.D, [0.0])
    want = orc.true_residuals(U, dims, MASS, P, [0.0], np.stack([Xh]))
    e = rel_err(res, want)
    print(f"{name} true_residuals between the calls [fused HOP_RESID]: {e:.3e}")
    assert e < 1e-11 and want.min() > 1e-3  # (the bound test_fused_true_residual_check holds it to)
    run.D.D(out, run.P)
    e = rel_err(out.download(), orc.hop(U, dims, P))
    print(f"{name} D.D between the calls [plain hop]: {e:.3e}")
    assert e < TOL_KERNEL
    prof = ctx.profile()
    assert _count(prof, "hop_residual") == 1 and "stencil_form_k_hop4c" not in prof, sorted(prof)
    for k in range(4):  # the last call, then three more: the fold tickets are reused
        T2, G2, R2 = run.phase_a(MASS, SIGMA0)
        assert np.array_equal(T2, T1) and np.array_equal(R2, R1) and np.array_equal(G2, G1), k
    assert _count(ctx.profile(), "stencil_form_factored_pair") == run.calls == 6
    print(f"{name} [factored pair]: calls 3 .. 6 equal call 1 bit for bit")
