"""The fused second factor (kernels_stencil.hip: k_hop4b_fusedB) with its Q rows loaded a step ahead and the product
Q rho_prev^-1 formed in front of the step's next-row loads instead of in the tail, against the build
before that change: SHA-256 digests recorded from the parent commit's library into tests/golden/fused_b_q_ahead_parent.json,
same inputs.  The chain is the tail's first call of rmul_rows operation for operation, and the Gram reductions sum in a fixed
order (tests/test_fused_phase_b.py: test_two_identical_solves_are_bit_identical), so equality is the bound.

What is compared: every X_s and every coefficient trace of 6 iterations of SBCGrQ (the solver updates Q in place; its first
iteration has no rho_prev^-1, the others have), at group depths 4 and 1; Q' and the Gram matrix of bcg_debug_phase_b_from_w
from operands no launch made, with and without rho_prev^-1, into a separate field and in place.

Shapes, all with patches of 16 x 2 x 2 and 32 blocks (the bundle sweep; a block then sweeps (L0 / 16)(L1 / 2)(L2 / 2) / 8
columns):
  32 x 4 x 4 x 3    the shortest column: one column per block, three steps -- the first, one in the middle, the last;
  16 x 8 x 8 x 8    two columns per block;
  16 x 8 x 12 x 4   three columns per block: the per-column first load of Q on a column that is neither the first nor the last.
A window of a single step does not exist for this launch: hop_plan_pair hands both factors the whole column (x3_n = L3)."""
import ctypes
import functools
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M = 16
ITERS = 6
SHIFTS = (0.0, 1e-3, 0.1)
KEYS = ("alpha", "rho", "delta", "alpha_s", "beta_s")
MASS = 1e-3
SHAPES = {"32x4x4x3": [32, 4, 4, 3], "16x8x8x8": [16, 8, 8, 8], "16x8x12x4": [16, 8, 12, 4]}
COLUMNS = {"32x4x4x3": 1, "16x8x8x8": 2, "16x8x12x4": 3}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_b_q_ahead_parent.json")
_TUNING = {"BCG_HOP_FUSED_B": "1", "BCG_HOP_PATCH": "16,2,2", "BCG_HOP_BLOCKS": "32"}


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _context(dims, **extra):
    import blockcg_amd as bc
    env = dict(_TUNING, **{k: str(v) for k, v in extra.items()})
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return bc.Context(dims)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _field(V, seed):
    a = np.random.default_rng(seed).normal(size=(V, M, 3, 2)).view(np.complex128)[..., 0]
    return np.ascontiguousarray(a)


def _count(prof, key):
    return prof.get(key, {}).get("count", 0)


def solve_digests(shape, depth):
    """ITERS iterations of SBCGrQ on the fused path: digests of every X_s and of every trace array."""
    import blockcg_amd as bc
    dims = SHAPES[shape]
    assert (dims[0] // 16) * (dims[1] // 2) * (dims[2] // 2) == 8 * COLUMNS[shape]
    ctx = _context(dims, BCG_PAIR_SHIFTS=depth)
    ctx.profiling(True)
    D = bc.dirac_op(ctx, MASS, seed=21)
    B = bc.block_fermion_field(ctx, M, _field(ctx.V, 22))
    X = [bc.block_fermion_field(ctx, M) for _ in SHIFTS]
    info = bc.SBCGrQ(X, B, D, list(SHIFTS), 0.0, 0.0, max_iterations=ITERS, trace_limit=ITERS, return_info=True)
    assert _count(ctx.profile(), "stencil_form_fused_phaseB") == ITERS, sorted(ctx.profile())
    Xh = [x.download() for x in X]
    assert all(np.isfinite(x).all() and np.linalg.norm(x) > 0 for x in Xh)
    return {"X": [_sha(x) for x in Xh], **{key: _sha(info["trace"][key]) for key in KEYS}}


def phase_b_digests(shape, normalise):
    """bcg_debug_phase_b_from_w, fused, from operands that no launch of the library made: Q' and the Gram matrix, written to
    a separate field (Q must stay as it was) and then in place."""
    import blockcg_amd as bc
    ctx = _context(SHAPES[shape])
    D = bc.dirac_op(ctx, MASS, seed=21)
    W = bc.block_fermion_field(ctx, M, _field(ctx.V, 31))
    Qh = _field(ctx.V, 32)
    Q = bc.block_fermion_field(ctx, M, Qh)
    T, out = bc.block_fermion_field(ctx, M), bc.block_fermion_field(ctx, M)
    rng = np.random.default_rng(33)
    alpha = 0.1 * (rng.normal(size=(M, M)) + 1j * rng.normal(size=(M, M))) + np.eye(M)
    rinv = np.triu(rng.normal(size=(M, M)) + 1j * rng.normal(size=(M, M))) * 0.1 + np.diag(1.0 + 0.1 * rng.random(M))
    fn = ctx.lib.bcg_debug_phase_b_from_w
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double] + [ctypes.c_void_p] * 6 + [ctypes.c_int, ctypes.c_void_p]
    a = np.ascontiguousarray(alpha.T)  # column-major
    r = np.ascontiguousarray(rinv.T) if normalise else None

    def run(dst):
        G2 = np.zeros((M, M), dtype=np.complex128)
        ctx.check(fn(ctx.h, D.h, D.mass, 0.0, W.h, T.h, Q.h, dst.h, a.ctypes.data_as(ctypes.c_void_p),
                     None if r is None else r.ctypes.data_as(ctypes.c_void_p), 1, G2.ctypes.data_as(ctypes.c_void_p)))
        return G2

    G_apart = run(out)
    assert np.array_equal(Q.download(), Qh)  # a separate output leaves Q as it was
    Q_apart = out.download()
    assert np.isfinite(Q_apart).all() and np.linalg.norm(Q_apart) > 0
    G_in_place = run(Q)
    return {"Q": _sha(Q_apart), "G2": _sha(G_apart), "Q in place": _sha(Q.download()), "G2 in place": _sha(G_in_place)}


def all_digests():
    """Every case of this file by its key in the golden file (the recorder runs this against the parent commit's library)."""
    d = {}
    for shape in sorted(SHAPES):
        for depth in (4, 1):
            d[f"solve {shape} depth {depth}"] = solve_digests(shape, depth)
        for normalise in (True, False):
            d[f"phase_b {shape} {'rinv' if normalise else 'no-rinv'}"] = phase_b_digests(shape, normalise)
    return d


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("depth", [4, 1], ids=["groups-of-4", "no-groups"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_solve_is_the_parent_build_bit_for_bit(shape, depth):
    assert solve_digests(shape, depth) == _golden()[f"solve {shape} depth {depth}"]


@pytest.mark.parametrize("normalise", [True, False], ids=["rinv", "no-rinv"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_phase_b_is_the_parent_build_bit_for_bit(shape, normalise):
    got = phase_b_digests(shape, normalise)
    assert got["Q in place"] == got["Q"] and got["G2 in place"] == got["G2"]
    assert got == _golden()[f"phase_b {shape} {'rinv' if normalise else 'no-rinv'}"]
