"""SBCGrQ at m = 16 with phase B inside the second stencil factor (capi_operator.hip: plan_pair with phase B inside and
its two launchers, pair_first_factor and pair_second_factor; kernels_stencil.hip: k_hop4b<16, HOP_FACT1, GRAM> and
k_hop4b_fusedB).  BCG_HOP_FUSED_B=0 keeps the pair's operator form and the phase B kernel.

The first factor W = (mu - D) P_0 sums G = W^dagger W = P_0^dagger (A + sigma_0) P_0 from its own output, so alpha = G^-1 is on
the host before the second factor starts; that launch forms T = (mu + D) W per site, applies Q' = Q rho_prev^-1 - T alpha on
chip and sums Q'^dagger Q'.  T is never written.

Shapes: 16 x 8 x 8 x 8 and 32 x 8 x 8 x 6 with patches of 16 x 2 x 2 and 32 blocks, the smallest lattices on which both
launches are bundle plans (tests/test_factored_stencil.py), and 32 x 4 x 4 x 3: two tiles in x0, an odd number of slices, the
fewest patches the walk takes (8), so that every block's last column ends on the last rows of the field.  A shape whose row
count 3V is no multiple of 16 does not exist on this path: the bundle sweep needs L0 a multiple of the 16-site tile and
(L0 / 16)(L1 / 2)(L2 / 2) a multiple of 8, so V is a multiple of 512 -- the wave's 12 rows never straddle the end of a field,
and phase B's batched form (chunks of 512 rows) always applies to the comparison.

Bounds.  Q' of the fused launch against k_phaseB on T of the unfused second factor: bit for bit -- the matrix instructions
take the same products in the same order with the operands' roles exchanged (rows as A, coefficients as B).  The Gram
matrices (first reduction against hermitian_dot(P_0, dirac_apply P_0); second against k_phaseB's): 1e-13, the project's bound
for one primitive (TOL_KERNEL).  Solves on against off: FORM_BOUND = 9e-14 of test_factored_stencil.py; against the oracle:
that file's bounds (TOL_COEFF for the traces, 1e-10 for X_s).  Off against the parent commit's build: the SHA-256 of every X_s
recorded from that build (tests/golden/fused_phase_b_parent.json).  On, and the two test aids, against the build before the
pair's two renditions in host code became one: SHA-256 again (tests/golden/factored_pair_parent.json)."""
import contextlib
import ctypes
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import TOL_COEFF, TOL_KERNEL, rel_err
from test_factored_stencil import FORM_BOUND, ITERS, KEYS, SHIFTS, _count, _oracle

pytestmark = pytest.mark.gpu

M = 16
SHAPES = {"16x8x8x8": [16, 8, 8, 8], "32x8x8x6": [32, 8, 8, 6], "32x4x4x3": [32, 4, 4, 3]}
SEED_U, SEED_B = 171, 172  # (test_factored_stencil.py's: its oracle solves are shared)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_phase_b_parent.json")
GOLDEN_PAIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "factored_pair_parent.json")


@contextlib.contextmanager
def _env(**kv):
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


def _context(dims, fused=True, **extra):
    import blockcg_amd as bc
    with _env(BCG_HOP_FUSED_B=int(fused), BCG_HOP_PATCH="16,2,2", BCG_HOP_BLOCKS="32", **extra):
        return bc.Context(dims)


@functools.lru_cache(maxsize=None)
def _inputs(shape, m=M):
    import oracle
    orc = oracle.Oracle()
    dims = SHAPES.get(shape) or [int(d) for d in shape.split("x")]
    U = orc.fill_gauge(dims, SEED_U)
    Bh = orc.fill_field(m, int(np.prod(dims)), SEED_B)
    for a in (U, Bh):
        a.setflags(write=False)
    return dims, U, Bh


def _random_field(V, seed):
    a = np.random.default_rng(seed).normal(size=(V, M, 3, 2)).view(np.complex128)[..., 0]
    return np.ascontiguousarray(a)


def _mat(ctx, name, m=M):
    G = np.zeros((m, m), dtype=np.complex128)  # column-major from the library
    fn = getattr(ctx.lib, name)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    assert fn(ctx.h, m, G.ctypes.data_as(ctypes.c_void_p)) == 0
    return G.T.copy()


def _first_factor(ctx, D, sigma0, W, P):
    fn = ctx.lib.bcg_debug_fused_first_factor
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    ctx.check(fn(ctx.h, D.h, D.mass, sigma0, W.h, P.h))


def _phase_b(ctx, D, sigma0, W, T, Q, Qout, alpha, rinv, fused):
    """Q' into Qout and G2 = Q'^dagger Q' (as the host uses it) by the fused launch or by FACT2 + k_phaseB."""
    fn = ctx.lib.bcg_debug_phase_b_from_w
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double] + [ctypes.c_void_p] * 6 + [ctypes.c_int, ctypes.c_void_p]
    a = np.ascontiguousarray(alpha.T)  # column-major
    r = None if rinv is None else np.ascontiguousarray(rinv.T)
    G2 = np.zeros((M, M), dtype=np.complex128)
    ctx.check(fn(ctx.h, D.h, D.mass, sigma0, W.h, T.h, Q.h, Qout.h, a.ctypes.data_as(ctypes.c_void_p),
                 None if r is None else r.ctypes.data_as(ctypes.c_void_p), int(fused), G2.ctypes.data_as(ctypes.c_void_p)))
    return G2.T.copy()


# ---- the first reduction: G from the first factor ---------------------------------------------------------------------
@pytest.mark.parametrize("mass", [0.2, 1e-3])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_first_reduction_from_the_first_factor(shape, mass):
    import blockcg_amd as bc
    dims, U, _ = _inputs(shape)
    ctx = _context(dims)
    ctx.profiling(True)
    D = bc.dirac_op(ctx, mass, U=U)
    P = bc.block_fermion_field(ctx, M, _random_field(ctx.V, 7))
    W = bc.block_fermion_field(ctx, M)
    _first_factor(ctx, D, 0.0, W, P)
    prof = ctx.profile()
    assert _count(prof, "stencil_form_k_hop4b") == 1 and _count(prof, "hop") == 1, sorted(prof)
    G = _mat(ctx, "bcg_debug_phase_a_gram_raw")
    assert np.all(np.diagonal(G).imag == 0.0)
    assert np.array_equal(G, G.conj().T)
    AP = bc.block_fermion_field(ctx, M)
    D.op(AP, P)
    G_ref = P.hermitian_dot(AP)
    e = rel_err(G, G_ref)
    print(f"{shape} mass {mass}: G of the first factor vs P^dagger (A P): {e:.3e}")
    assert e < TOL_KERNEL
    # and it is W^dagger W of the W the launch wrote
    e = rel_err(G, W.hermitian_dot(W))
    print(f"{shape} mass {mass}: G of the first factor vs W^dagger W: {e:.3e}")
    assert e < TOL_KERNEL


# ---- the fused update against FACT2 + k_phaseB from the same operands ---------------------------------------------------
@pytest.mark.parametrize("normalise", [True, False], ids=["rinv", "no-rinv"])
@pytest.mark.parametrize("mass", [0.2, 1e-3])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_fused_update_is_phase_b_bit_for_bit(shape, mass, normalise):
    import blockcg_amd as bc
    dims, U, _ = _inputs(shape)
    ctx = _context(dims)
    D = bc.dirac_op(ctx, mass, U=U)
    P = bc.block_fermion_field(ctx, M, _random_field(ctx.V, 7))
    W = bc.block_fermion_field(ctx, M)
    _first_factor(ctx, D, 0.0, W, P)
    Qh = _random_field(ctx.V, 8)
    Q = bc.block_fermion_field(ctx, M, Qh)
    rng = np.random.default_rng(9)
    alpha = np.linalg.inv(_mat(ctx, "bcg_debug_phase_a_gram"))  # what the solver would use
    rinv = None
    if normalise:  # an upper triangular matrix with a diagonal near one, full otherwise
        rinv = np.triu(rng.normal(size=(M, M)) + 1j * rng.normal(size=(M, M))) * 0.1 + np.diag(1.0 + 0.1 * rng.random(M))
    T = bc.block_fermion_field(ctx, M)
    out_f, out_u = bc.block_fermion_field(ctx, M), bc.block_fermion_field(ctx, M)
    G2_u = _phase_b(ctx, D, 0.0, W, T, Q, out_u, alpha, rinv, fused=False)
    G2_f = _phase_b(ctx, D, 0.0, W, T, Q, out_f, alpha, rinv, fused=True)
    assert np.array_equal(Q.download(), Qh)  # a separate output leaves Q as it was
    Qu, Qf = out_u.download(), out_f.download()
    assert np.isfinite(Qu).all() and np.linalg.norm(Qu) > 0
    diff = np.abs(Qf - Qu).max()
    print(f"{shape} mass {mass} {'rinv' if normalise else 'no rinv'}: max |Q'_fused - Q'_phaseB| = {diff:.3e}")
    assert np.array_equal(Qf, Qu)
    e = rel_err(G2_f, G2_u)
    print(f"{shape} mass {mass}: second Gram matrix fused vs k_phaseB: {e:.3e}")
    assert e < TOL_KERNEL
    assert np.array_equal(G2_f, G2_f.conj().T) and np.all(np.diagonal(G2_f).imag == 0.0)
    # in place: the same bits
    G2_i = _phase_b(ctx, D, 0.0, W, T, Q, Q, alpha, rinv, fused=True)
    assert np.array_equal(Q.download(), Qf) and np.array_equal(G2_i, G2_f)


# ---- solves ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _solve(shape, mass, fused, depth, m=M, ring=0, half=False, bundle=None, repeat=0):
    """ITERS iterations with the switch as given: (X_s, trace, profile).  repeat: a cache key for a second, identical solve."""
    import blockcg_amd as bc
    dims, U, Bh = _inputs(shape, m)
    ctx = _context(dims, fused, BCG_PAIR_SHIFTS=depth, BCG_HOP_BUNDLE=bundle)
    ctx.capacity_mode(ring)
    ctx.profiling(True)
    D = bc.dirac_op(ctx, mass, U=U)
    B = bc.block_fermion_field(ctx, m, Bh)
    X = [bc.block_fermion_field(ctx, m) for _ in SHIFTS]
    if half:
        bc.SBCGrQ_half_volume(X, B, D, list(SHIFTS), 0.0, 0.0, max_iterations=ITERS)
        return [x.download() for x in X], None, ctx.profile()
    info = bc.SBCGrQ(X, B, D, list(SHIFTS), 0.0, 0.0, max_iterations=ITERS, trace_limit=ITERS, return_info=True)
    return [x.download() for x in X], info["trace"], ctx.profile()


@pytest.mark.parametrize("depth", [4, 1], ids=["groups-of-4", "no-groups"])
@pytest.mark.parametrize("mass", [0.2, 1e-3])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_solve_on_against_off_and_the_oracle(shape, mass, depth):
    Xon, ton, pon = _solve(shape, mass, True, depth)
    Xoff, toff, poff = _solve(shape, mass, False, depth)
    # the profile: one fused launch per iteration when on, none when off; the classes keep their counts and bytes
    assert _count(pon, "stencil_form_fused_phaseB") == ITERS and "stencil_form_fused_phaseB" not in poff
    for prof in (pon, poff):
        n = _count(prof, "hop")
        assert n >= ITERS and _count(prof, "hop_shifted_gram") == n and _count(prof, "phaseB") == ITERS, sorted(prof)
        assert _count(prof, "stencil_form_k_hop4b") == 2 * n and _count(prof, "stencil_form_factored_pair") == n
        assert prof["hop_shifted_gram"]["bytes"] == prof["hop"]["bytes"]
    V = int(np.prod(SHAPES[shape]))
    assert poff["phaseB"]["bytes"] - pon["phaseB"]["bytes"] == pytest.approx(ITERS * V * 48.0 * M, rel=1e-12)
    assert pon["phaseB"]["ms"] == 0.0 and poff["phaseB"]["ms"] > 0.0
    worst = 0.0
    for key in KEYS:
        e = rel_err(ton[key], toff[key])
        print(f"{shape} mass {mass} depth {depth} on vs off {key}: {e:.3e}")
        worst = max(worst, e)
    for s in range(len(SHIFTS)):
        e = rel_err(Xon[s], Xoff[s])
        print(f"{shape} mass {mass} depth {depth} on vs off X[{s}]: {e:.3e}")
        worst = max(worst, e)
    assert worst < FORM_BOUND
    if shape in ("16x8x8x8", "32x8x8x6"):
        o = _oracle(shape, mass, SHIFTS)
    else:
        import oracle
        dims, U, Bh = _inputs(shape)
        o = oracle.Oracle().sbcgrq(U, dims, mass, Bh, list(SHIFTS), 0.0, 0.0, max_iterations=ITERS, trace_limit=ITERS)
    for key in KEYS:
        e = rel_err(ton[key], o["trace"][key])
        print(f"{shape} mass {mass} depth {depth} fused vs oracle {key}: {e:.3e}")
        assert e < TOL_COEFF, key
    for s in range(len(SHIFTS)):
        e = rel_err(Xon[s], o["X"][s])
        print(f"{shape} mass {mass} depth {depth} fused vs oracle X[{s}]: {e:.3e}")
        assert e < 1e-10, s


@pytest.mark.parametrize("depth", [4, 1], ids=["groups-of-4", "no-groups"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_two_identical_solves_are_bit_identical(shape, depth):
    a, b = _solve(shape, 1e-3, True, depth), _solve(shape, 1e-3, True, depth, repeat=1)
    for s in range(len(SHIFTS)):
        assert np.array_equal(a[0][s], b[0][s]), s
    for key in KEYS:
        assert np.array_equal(a[1][key], b[1][key]), key


def _digest(X):
    return [hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest() for x in X]


@pytest.mark.parametrize("depth", [4, 1], ids=["groups-of-4", "no-groups"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_off_is_the_parent_build_bit_for_bit(shape, depth):
    """The X_s of BCG_HOP_FUSED_B=0 against the digests recorded from the parent commit's library (mass 1e-3, same inputs)."""
    want = json.load(open(GOLDEN))[f"{shape} depth {depth}"]
    assert _digest(_solve(shape, 1e-3, False, depth)[0]) == want


# ---- the switch on: the pair's host code against the build before it became one pair ---------------------------------------
# tests/golden/factored_pair_parent.json: SHA-256 digests recorded from the library of the commit before the two renditions
# of the pair were merged into one (capi_operator.hip: plan_pair, pair_first_factor, pair_second_factor), same inputs.  The
# Gram reductions sum in a fixed order (test_two_identical_solves_are_bit_identical), so equality is the bound.
def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _solve_on_digests(shape, depth):
    X, trace, _ = _solve(shape, 1e-3, True, depth)
    return {"X": _digest(X), **{key: _sha(trace[key]) for key in KEYS}}


def _operator_form_digests(mass):
    """One bcg_debug_phase_a on 16 x 8 x 8 x 8 -- the operator form of the pair, T = (mu + D)(mu - D) P and the partials of
    W^dagger W: T and the Gram matrix as the device summed it."""
    import blockcg_amd as bc
    dims, U, _ = _inputs("16x8x8x8")
    ctx = _context(dims)
    ctx.profiling(True)
    D = bc.dirac_op(ctx, mass, U=U)
    P = bc.block_fermion_field(ctx, M, _random_field(ctx.V, 7))
    T = bc.block_fermion_field(ctx, M)
    fn = ctx.lib.bcg_debug_phase_a
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    ctx.check(fn(ctx.h, D.h, mass, 0.0, T.h, P.h))
    prof = ctx.profile()
    assert _count(prof, "stencil_form_factored_pair") == 1 and "stencil_form_fused_phaseB" not in prof, sorted(prof)
    return {"T": _sha(T.download()), "G_raw": _sha(_mat(ctx, "bcg_debug_phase_a_gram_raw"))}


def _phase_b_aid_digests(fused, normalise):
    """bcg_debug_phase_b_from_w on 16 x 8 x 8 x 8 at mass 1e-3 from operands that no launch of the library made: Q' and G2."""
    import blockcg_amd as bc
    dims, U, _ = _inputs("16x8x8x8")
    ctx = _context(dims)
    D = bc.dirac_op(ctx, 1e-3, U=U)
    W = bc.block_fermion_field(ctx, M, _random_field(ctx.V, 11))
    Q = bc.block_fermion_field(ctx, M, _random_field(ctx.V, 12))
    T, out = bc.block_fermion_field(ctx, M), bc.block_fermion_field(ctx, M)
    rng = np.random.default_rng(13)
    alpha = 0.1 * (rng.normal(size=(M, M)) + 1j * rng.normal(size=(M, M))) + np.eye(M)
    rinv = np.triu(rng.normal(size=(M, M)) + 1j * rng.normal(size=(M, M))) * 0.1 + np.diag(1.0 + 0.1 * rng.random(M))
    G2 = _phase_b(ctx, D, 0.0, W, T, Q, out, alpha, rinv if normalise else None, fused=fused)
    return {"Q": _sha(out.download()), "G2": _sha(G2)}


@pytest.mark.parametrize("depth", [4, 1], ids=["groups-of-4", "no-groups"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_on_is_the_parent_build_bit_for_bit(shape, depth):
    """Every X_s and every trace array of BCG_HOP_FUSED_B=1 against the digests recorded from the parent commit's library."""
    assert _solve_on_digests(shape, depth) == json.load(open(GOLDEN_PAIR))[f"solve {shape} depth {depth}"]


@pytest.mark.parametrize("mass", [0.2, 1e-3])
def test_operator_form_is_the_parent_build_bit_for_bit(mass):
    assert _operator_form_digests(mass) == json.load(open(GOLDEN_PAIR))[f"phase_a 16x8x8x8 mass {mass}"]


@pytest.mark.parametrize("normalise", [True, False], ids=["rinv", "no-rinv"])
@pytest.mark.parametrize("fused", [0, 1], ids=["fact2-phaseB", "fused"])
def test_phase_b_aid_is_the_parent_build_bit_for_bit(fused, normalise):
    want = json.load(open(GOLDEN_PAIR))[f"phase_b 16x8x8x8 fused {fused} {'rinv' if normalise else 'no-rinv'}"]
    assert _phase_b_aid_digests(fused, normalise) == want


# ---- where the path must not be taken ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["m8", "m32", "ring", "half", "bundle0"])
def test_no_fused_launch_elsewhere(case):
    kw = {"m8": dict(shape="16x8x4x8", m=8), "m32": dict(shape="16x8x8x8", m=32), "ring": dict(shape="16x8x8x8", ring=4),
          "half": dict(shape="16x8x8x8", half=True), "bundle0": dict(shape="16x8x8x8", bundle=0)}[case]
    shape = kw.pop("shape")
    prof = _solve(shape, 0.2, True, 4, **kw)[2]
    assert "stencil_form_fused_phaseB" not in prof, sorted(prof)
    if "phaseB" in prof:  # (phase B is then a launch of its own, with its time)
        assert prof["phaseB"]["ms"] > 0.0
