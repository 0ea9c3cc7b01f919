"""Reference of phase A of a solver iteration as ONE operation (capi_solvers.hip: phase_A):

    T = (mass^2 + sigma_0) P - D (D P),      G = P^dagger T

D is shift_sum_ref.shift_sum(U, dims, psi, 0, 0.5, -0.5, eta=True) -- the identity tests/test_shift_sum.py holds against
bcg_dirac_hop -- so neighbours come from that module's coordinate-tuple table and no site stride is shared with the kernels.
The unfactored form on purpose: there is no mu = sqrt(mass^2 + sigma_0) anywhere in this file, so an algebra error in the
factored stencil pair (W = (mu - D) P, T = (mu + D) W, G = W^dagger W) cannot cancel against the same error here.

Arithmetic: np.clongdouble where the platform's long double carries more than 52 mantissa bits (x86: 63), complex128
elsewhere; PRECISION names which, and the tests print it.  Results are rounded to complex128 once, at the end.

Host layouts as everywhere in tests/: P, T [V, m, 3]; U [V, ndim, 3, 3]; G[i, j] = sum over sites and colours of
conj(P[x, i, c]) T[x, j, c]."""
import numpy as np

import shift_sum_ref

EXTENDED = np.finfo(np.longdouble).nmant > 52
CTYPE = np.clongdouble if EXTENDED else np.complex128
RTYPE = np.longdouble if EXTENDED else np.float64
PRECISION = f"{np.dtype(CTYPE).name} ({np.finfo(RTYPE).nmant} mantissa bits)"

# The launch geometries of tests/test_phase_a_operator.py: name -> (dims, BCG_HOP_PATCH or None, BCG_HOP_BLOCKS or None).
# Legal for the bundle sweep at m = 16 by plan_hop4 / bundle_ok (hop_plan.cpp), tiles of 16 x0 sites, re-derived row by row:
# whole patches (p0 | L0, 16 | p0, p1 | L1, p2 | L2, p1 and p2 even), tiles = V / 16 a multiple of 8 and >= blocks, patches
# (L0/p0)(L1/p1)(L2/p2) a multiple of 8, blocks / 8 = (p0/16) p1 p2 [column form] = (p0/4)(p1/2)(p2/2) [bundles]:
#   16x4x8xL3    16,2,2 / 32   tiles 32 L3    patches 1*2*4 = 8     32/8 = 4 = 1*2*2 = 4*1*1
#   16x2x16x4    16,2,2 / 32   tiles 128      patches 1*1*8 = 8     (p1 = L1: x1 - 1 and x1 + 1 are the same row)
#   16x16x2x4    16,2,2 / 32   tiles 128      patches 1*8*1 = 8     (p2 = L2)
#   48x4x8x4     16,2,2 / 32   tiles 384      patches 3*2*4 = 24
#   32x8x8x6     32,2,2 / 64   tiles 768      patches 1*4*4 = 16    64/8 = 8 = 2*2*2 = 8*1*1
#   16x8x16x4    16,4,4 / 128  tiles 512      patches 1*2*4 = 8     128/8 = 16 = 1*4*4 = 4*2*2
#   16x4x16x4    16,2,4 / 64   tiles 256      patches 1*2*4 = 8     64/8 = 8 = 1*2*4 = 4*1*2
#   32x16x16x4   default: patch (16),8,8, 512 blocks: tiles 2048, patches 2*2*2 = 8, 512/8 = 64 = 1*8*8 = 4*4*4
#   16x8x8x8, 32x8x8x6 with 16,2,2 / 32: the shapes of tests/test_factored_stencil.py (patches 1*4*4 and 2*4*4)
GEOMETRIES = {
    "16x4x8x1": ([16, 4, 8, 1], "16,2,2", "32"),
    "16x4x8x2": ([16, 4, 8, 2], "16,2,2", "32"),
    "16x4x8x3": ([16, 4, 8, 3], "16,2,2", "32"),
    "16x4x8x5": ([16, 4, 8, 5], "16,2,2", "32"),
    "16x2x16x4": ([16, 2, 16, 4], "16,2,2", "32"),
    "16x16x2x4": ([16, 16, 2, 4], "16,2,2", "32"),
    "48x4x8x4": ([48, 4, 8, 4], "16,2,2", "32"),
    "32x8x8x6-p32": ([32, 8, 8, 6], "32,2,2", "64"),
    "16x8x16x4": ([16, 8, 16, 4], "16,4,4", "128"),
    "16x4x16x4": ([16, 4, 16, 4], "16,2,4", "64"),
    "32x16x16x4-default": ([32, 16, 16, 4], None, None),
}
TUNING_SHAPES = {  # the tuning, parameter, solver and shared-buffer groups
    "16x8x8x8": ([16, 8, 8, 8], "16,2,2", "32"),
    "32x8x8x6": ([32, 8, 8, 6], "16,2,2", "32"),
}
ALL_SHAPES = dict(GEOMETRIES, **TUNING_SHAPES)
SEED_U, SEED_P = 271, 272
M = 16


def dirac_hop(U, dims, psi):
    """D psi, in the precision of its arguments."""
    return shift_sum_ref.shift_sum(U, dims, psi, 0, 0.5, -0.5, eta=True)


def hop_twice(U, dims, P):
    """D (D P) in CTYPE, not rounded: the part of T_ref that does not depend on mass and sigma_0."""
    Ux = np.asarray(U, dtype=CTYPE)
    return dirac_hop(Ux, dims, dirac_hop(Ux, dims, np.asarray(P, dtype=CTYPE)))


def phase_a(U, dims, mass, sigma0, P, DDP=None):
    """(T_ref, G_ref) in complex128, computed in CTYPE.  DDP: hop_twice(U, dims, P) where the caller keeps it."""
    Px = np.asarray(P, dtype=CTYPE)
    c0 = RTYPE(mass) * RTYPE(mass) + RTYPE(sigma0)
    Tx = c0 * Px - (hop_twice(U, dims, P) if DDP is None else DDP)
    m = Px.shape[1]
    rows = lambda f: f.transpose(0, 2, 1).reshape(-1, m)  # noqa: E731  [(site, colour), column]
    Gx = rows(Px).conj().T @ rows(Tx)
    return Tx.astype(np.complex128), Gx.astype(np.complex128)


def gram_double(P, T):
    """numpy's own P^dagger T in complex128."""
    m = P.shape[1]
    return P.transpose(0, 2, 1).reshape(-1, m).conj().T @ T.transpose(0, 2, 1).reshape(-1, m)
